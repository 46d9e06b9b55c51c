// pick_params.h - the parameter structs of the pick and logits-process kernels (decode.hip), and PickCall: the one host-side description
// of a pick that every aki_greedy_pick* / aki_sample_pick* entry point (api.hip) fills, pick_call_check validates and pick_call_launch
// turns into one launch.
#pragma once
#include "aki_device.h"

namespace aki {

struct PickParams {
  const bf16_t* logits; int B, V, ld;
  const int64_t* eos; int n_eos; int64_t pad;
  unsigned char* done; int64_t* ids; int64_t* tokens; int tokens_ld;
  int* cache_len; const int* start_len; int advance; int* done_at;
  // optional: the NEXT decode step's input row, gathered here (DecoupledEmbedding, src/helpers.py:350-492: ids above max_original_id index the
  // additional table) so that a greedy token needs no embedding launch
  const bf16_t* emb_main; const bf16_t* emb_extra; int64_t max_original_id; int d; bf16_t* emb_out;
  int step;   // added to t (the sampler's eager loop passes the token index here when it has no cache_len); 0 for the greedy picks
};

// Constrained decoding (aki_amd/constraint.py): a deterministic automaton over token ids.  table[s, v] is the state behind token v in state
// s, negative = v is not allowed in s; states[b, n] is the state in which row b picks its generated token n (column 0: the start state).
// The state is addressed by the token index, like the processors' history, never carried in a counter: a replayed graph, a rewind of
// cache_len after a chain give-up and a repeated step then read and write the right column with nothing to reset.
// The per-row form (row_base and row_states set, both or neither): `table` is a POOL of n_states rows holding several automata one behind
// the other, each with its own state numbers from 0; row b's automaton is the row_states[b] pool rows from row_base[b] on.  Both arrays
// are read by the launch, so a captured step serves a row whose automaton is replaced in place between replays (generate_many's admit).
struct ConstraintParams {
  const int16_t* table; int table_ld, n_states;
  int* states; int states_ld;
  const int* row_base; const int* row_states;
};

struct ProcParams {
  const void* in; int in_f32, ld_in;
  float* out; int ld_out;
  int V;
  const int64_t* tokens; int tokens_ld;
  const int* cache_len; const int* start_len; int step;
  const unsigned char* done;
  float penalty; int ngram, min_len;
  const int64_t* eos; int n_eos;
  const int64_t* suppress; int n_suppress;
  const int64_t* begin_suppress; int n_begin;
  const int64_t* bad_ids; const int* bad_off; int n_bad, n_bad_ids;
  ConstraintParams c;                 // c.table == nullptr: no constraint
  // stage 1b, optional: the OpenAI frequency / presence penalties, one float per row (device arrays of B entries; nullptr = 0 for every
  // row).  A value that is not finite reads as 0.  Every thread of row b reads the same entry: workgroup-uniform.
  const float* freq; const float* pres;
};

struct SampleParams {
  float temperature; int top_k; float top_p;
  unsigned seed_lo, seed_hi, off_lo, off_hi;
  float* probs; int ld_probs;
  int processed;                                            // the processors ran: x is the f32 scratch row, not the bf16 logits
  const float* min_p;                                       // optional, one float per row (B entries): keep iff exp(y - ymax) >= min_p[b]
};

// The per-row form (aki_sample_pick_rows): row b reads its own temperature[b], top_k[b], top_p[b] and Philox key seed[b] from device
// arrays of B entries, and draws with the counter (n, 0, 0, 0) - the stream belongs to the row's seed, not to the row index, so it is the
// draw row 0 of a batch-1 scalar call with that seed and offset 0 makes.  One workgroup per row: the values are workgroup-uniform.
// Nothing validates the arrays on the device; bad bits stay inside the row: a temperature that is not > 0 (zero, negative, NaN) takes
// the greedy pick, top_k[b] <= 0 or >= V is no top-k filter, top_p[b] >= 1 is no top-p filter (and a top_p that is not > 0 keeps the
// maximum only).  top_k[b] == 1 is the greedy branch, as in the scalar form.  min_p (nullable, as in SampleParams): a value outside
// (0, 1] is no filter.
struct SampleRowParams {
  const float* temperature; const int* top_k; const float* top_p; const unsigned long long* seed;
  float* probs; int ld_probs;
  int processed;
  const float* min_p;
};

constexpr int PROC_SET_WORDS = 9;
struct ProcSetParams {
  const int* sets; int n_sets; const int* row_set;
  const int64_t* ids; int n_ids; const int* bad_off; int n_words;
};

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// How an entry point takes its token constraint.  WIDE allows at most 32767 states (one automaton for every row); the two ROWS kinds take
// a pool of any positive size with row_base / row_states, and ROWS_OR_NONE reads a NULL table as "no constraint" (the other six arguments
// are then not looked at); WIDE_OR_NONE is WIDE with the same reading of a NULL table.
enum ConstraintKind { CON_NONE = 0, CON_WIDE, CON_ROWS, CON_ROWS_OR_NONE, CON_WIDE_OR_NONE };
enum SamplerKind { SAMPLER_NONE = 0, SAMPLER_SCALAR, SAMPLER_ROWS };

// One pick, as its entry point was called.  The kernel structs hold the narrowed values; the strides and counts the C ABI takes as 64-bit
// are kept beside them as passed, so that pick_call_check sees what the caller wrote.
struct PickCall {
  PickParams p;
  ProcParams q;            // the processors and the f32 scratch (q.out / q.ld_out); q.step is the launcher's to set
  ProcSetParams ps;        // sets: one processor set per row, in the place of q's scalar processor values
  SampleParams sp;         // sampler == SAMPLER_SCALAR
  SampleRowParams sr;      // sampler == SAMPLER_ROWS
  int sampler;
  bool processed;          // the entry point takes a scratch and processors: every form but aki_greedy_pick / aki_greedy_pick_embed
  bool sets;
  bool embed_required;     // aki_greedy_pick_embed: the tables are not optional
  int constraint;          // a ConstraintKind
  int64_t ld, ld_scores, ld_probs, table_ld, num_additional;
};

}  // namespace aki
