"""Scripted beam-search cases and their float64 reference (no model, no GPU): what tests/test_beam_cases_cpu.py checks on the CPU and
tests/test_beam_gpu.py runs through ops.beam_logprob / ops.beam_step.

The reference is HF's beam search with a BeamSearchScorer as AKI._beam_search (aki_amd/aki.py) states it, in float64 numpy: log-softmax,
the 2K best of logp + running score ranked by score (exactly equal scores: the lower flat index k*V + v first - the project's rule,
torch.topk promises none), EOS candidates of rank < K become hypotheses, at most K hypotheses per sample (a better one evicts the
worst; among equal worst scores the lowest slot), the three early-stopping modes, the closing step.  It is driven by scripted logits
[T, B*K, V]: the logits of slot row r at step t do not depend on the tokens chosen, and parents are applied to the reference's own
sequences.  A frozen (done) sample keeps its state, takes pad tokens and identity parents, as include/aki_mi355x.h states for aki_beam_step.

THE ERROR BOUND of the kernels' f32 arithmetic, derived from beam.hip (first order, u = 2^-24, M = max |logit|, A = 2M + ln V >= |logp|):
  logprob  d = x - m: u * 2M.  expf(d): relative 2M u (the argument's error) + 4u (2 ulp).  The sum of the V positive terms: a thread adds
           ceil(V / 1024) of them in turn, then 6 butterfly levels and 15 wave sums: relative (ceil(V / 1024) + 21) u.  logf: the sum's
           relative error + 4u ln V (2 ulp of a value <= ln V).  m + log s: u (M + ln V).  x - lse: u A.  Together
             E_lp(M, V) = u * (5 M + 6 ln V + ceil(V / 1024) + 26)                                   (one unit of slack for second order)
  score    a running score after step t is t + 1 log-probabilities added in f32, one rounding u |sum| <= u (s + 1) A at step s:
             E_score(M, V, t) = (t + 1) E_lp + u A (t + 1)(t + 2) / 2
  hyp      sum / (t + 1) ** length_penalty: the sum's error (the divisor is >= 1 for length_penalty >= 0) + a division (0.5 ulp), a powf
           (2 ulp) and slack on |sum| <= (t + 1) A:  E_hyp(M, V, t) = E_score(M, V, t) + 4 u (t + 1) A
A case's `bound` is E_hyp at its last step, the largest of them.  The reference reports the smallest margin of every decision it takes
(adjacent ranked candidates that are not exact ties, up to rank 2K against rank 2K + 1; a new hypothesis against the worst held; the worst
against the second worst when one is evicted; the worst against the best running score); the CPU test asserts margin >= 4 * bound for every
case, so f32 arithmetic within the bound takes the same decisions.  Exact ties in float64 must be ties of one beam's equal logits: those
are exactly equal in f32 too (same row constant, same running score).

`python tests/beam_cases.py` searches the seed of every case again (the first seed whose margins and events hold)."""
import functools
import math

import numpy as np

U = 2.0 ** -24
KERNEL_THREADS = 1024          # beam.hip: BEAM_THREADS, a thread owns the columns v = tid (mod 1024) of all K beams of a sample


def logprob_bound(M, V):
    return U * (5.0 * M + 6.0 * math.log(V) + math.ceil(V / KERNEL_THREADS) + 26.0)


def score_bound(M, V, t):
    A = 2.0 * M + math.log(V)
    return (t + 1) * logprob_bound(M, V) + U * A * (t + 1) * (t + 2) / 2.0


def hyp_bound(M, V, t):
    return score_bound(M, V, t) + 4.0 * U * (t + 1) * (2.0 * M + math.log(V))


def round_bf16(x):
    """float32 array rounded to the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def logprob_ref(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


class RefSearch:
    """The float64 search.  step(logits_t) advances every sample by one token and appends to `steps` what the kernel must reproduce."""

    def __init__(self, B, K, T, eos, pad, length_penalty, early_stopping):
        self.B, self.K, self.T = B, K, T
        self.eos, self.pad, self.lp, self.es = set(int(e) for e in eos), int(pad), float(length_penalty), early_stopping
        self.scores = np.zeros((B, K), dtype=np.float64)
        self.scores[:, 1:] = -1e9
        self.seqs = [[] for _ in range(B * K)]
        self.hyps = [[] for _ in range(B)]            # per sample: slots of [score, tokens]
        self.done = [False] * B
        self.t = 0
        self.min_margin = math.inf
        self.events = set()
        self.steps = []

    def _margin(self, a, b):
        self.min_margin = min(self.min_margin, abs(a - b))

    def rank(self, logits_t, b, n):
        """The n best candidates of sample b: (score, beam, token) by score descending, exactly equal scores by flat index ascending."""
        K = self.K
        rows = np.asarray(logits_t[b * K:(b + 1) * K], dtype=np.float64)
        V = rows.shape[1]
        cand = (logprob_ref(rows) + self.scores[b][:, None]).reshape(-1)
        n = min(n, cand.size)
        kth = np.partition(cand, cand.size - n)[cand.size - n]
        idx = np.flatnonzero(cand >= kth)
        idx = idx[np.lexsort((idx, -cand[idx]))][:n]
        return [(float(cand[i]), int(i // V), int(i % V)) for i in idx]

    def _worst(self, b):
        h = self.hyps[b]
        return min(range(len(h)), key=lambda i: (h[i][0], i))

    def _add(self, b, score_sum, toks):
        sc = score_sum / (max(len(toks), 1) ** self.lp)
        h = self.hyps[b]
        if len(h) < self.K:
            h.append([sc, toks])
            return
        w = self._worst(b)
        self._margin(sc, h[w][0])
        if sc > h[w][0]:
            others = [x[0] for i, x in enumerate(h) if i != w]
            if others:
                self._margin(h[w][0], min(others))
            h[w] = [sc, toks]
            self.events.add("evicted")

    def step(self, logits_t):
        B, K, t = self.B, self.K, self.t
        last = t + 1 == self.T
        nxt_tok = np.full((B, K), self.pad, dtype=np.int64)
        nxt_beam = np.zeros((B, K), dtype=np.int64)
        nxt_score = np.full((B, K), -1e9, dtype=np.float64)
        rows_logits = np.asarray(logits_t, dtype=np.float64)
        for b in range(B):
            if self.done[b]:
                nxt_beam[b] = np.arange(K)
                nxt_score[b] = self.scores[b]
                continue
            ranked = self.rank(logits_t, b, 2 * K + 1)
            for r in range(min(2 * K, len(ranked) - 1)):
                (s0, k0, v0), (s1, k1, v1) = ranked[r], ranked[r + 1]
                if s0 == s1:                      # an exact tie: the index decides - it must be a tie in f32 too
                    assert k0 == k1 and rows_logits[b * K + k0, v0] == rows_logits[b * K + k1, v1], "an exact float64 tie across beams"
                    self.events.add("tie_in" if r + 1 < 2 * K else "tie_2k")
                    if r + 1 == K:
                        self.events.add("tie_k")
                else:
                    self._margin(s0, s1)
            if any(tok in self.eos for _, _, tok in ranked[K:2 * K]):
                self.events.add("eos_ignored")       # whether the walk below reaches it or not: it never becomes a hypothesis
            n = 0
            for r, (sc, beam, tok) in enumerate(ranked[:2 * K]):
                if tok in self.eos:
                    if r < K:
                        self._add(b, sc, self.seqs[b * K + beam] + [tok])
                        self.events.add("eos_hyp")
                    continue
                nxt_tok[b, n], nxt_beam[b, n], nxt_score[b, n] = tok, beam, sc
                n += 1
                if n == K:
                    break
            if n < K:
                self.events.add("slots_unfilled")
            if len(self.hyps[b]) >= K:
                best_running = nxt_score[b].max() / ((t + 1) ** self.lp)
                worst = self.hyps[b][self._worst(b)][0]
                if self.es is False:
                    self._margin(worst, best_running)
                if self.es is True or (self.es is False and worst >= best_running):
                    self.done[b] = True
                    self.events.add(f"done_at_{t}")
            if last and not self.done[b]:
                for i in range(K):
                    if nxt_score[b, i] > -1e8:
                        self._add(b, nxt_score[b, i], self.seqs[b * K + int(nxt_beam[b, i])] + [int(nxt_tok[b, i])])
                        self.events.add("closing")
        parent = (np.arange(B)[:, None] * K + nxt_beam).reshape(-1)
        self.seqs = [self.seqs[int(p)] + [int(tk)] for p, tk in zip(parent, nxt_tok.reshape(-1))]
        self.scores = nxt_score
        self.t = t + 1
        self.steps.append(dict(parent=parent.astype(np.int32), next_ids=nxt_tok.reshape(-1).copy(), seqs=np.array(self.seqs, dtype=np.int64),
                               beam_scores=nxt_score.copy(), done=np.array(self.done, dtype=np.uint8)))


# name, K, B, V, T, length_penalty, early_stopping, eos ids, plants, events that must occur, seed.
# plants: ("eos", t, b, rank) swaps an eos column with the column of sample b's candidate of that rank at step t (same row: the row's
# log-sum-exp is unchanged); ("tie", t, b, rank) copies that candidate's logit to another column of its row, which makes ranks `rank` and
# `rank + 1` an exact tie of one beam.
SPECS = [
    dict(name="k1_b1_v64", K=1, B=1, V=64, T=3, lp=1.0, es=False, eos=[5], plants=[("eos", 1, 0, 1), ("eos", 2, 0, 0)],
         expect={"eos_ignored", "eos_hyp"}, seed=0),
    dict(name="k2_b3_v64_done_at_2", K=2, B=3, V=64, T=5, lp=1.0, es=True, eos=[3], plants=[("eos", 1, 0, 0), ("eos", 2, 0, 0)],
         expect={"eos_hyp", "done_at_2", "closing"}, seed=0),
    dict(name="k2_b1_v1000_evict", K=2, B=1, V=1000, T=5, lp=2.0, es="never", eos=[10],
         plants=[("eos", 0, 0, 0), ("eos", 1, 0, 0), ("eos", 2, 0, 0), ("eos", 3, 0, 1)], expect={"eos_hyp", "evicted", "closing"}, seed=0),
    dict(name="k3_b3_v1000", K=3, B=3, V=1000, T=6, lp=0.0, es=False, eos=[1, 2],
         plants=[("eos", 1, 0, 1), ("eos", 2, 1, 4), ("tie", 1, 1, 1), ("tie", 3, 2, 0), ("eos", 3, 0, 0)],
         expect={"eos_hyp", "eos_ignored", "tie_in", "closing"}, seed=115),
    dict(name="k4_b1_real_v_unfilled", K=4, B=1, V=32064 + 6, T=4, lp=1.0, es=False, eos=[32007, 32001],
         plants=[("eos", 2, 0, r) for r in range(6)], expect={"eos_hyp", "eos_ignored", "slots_unfilled"}, seed=0),
    dict(name="k4_b3_real_v_ties", K=4, B=3, V=32064 + 6, T=3, lp=1.0, es="never", eos=[32000],
         plants=[("tie", 1, 0, 3), ("tie", 1, 1, 7), ("tie", 2, 2, 2), ("eos", 2, 1, 1)], expect={"tie_k", "tie_2k", "tie_in", "eos_hyp"}, seed=0),
    dict(name="k8_b1_v1000", K=8, B=1, V=1000, T=6, lp=2.0, es=False, eos=[0],
         plants=[("eos", 1, 0, 2), ("eos", 2, 0, 12), ("eos", 3, 0, 0), ("tie", 4, 0, 7)], expect={"eos_hyp", "eos_ignored", "tie_k"}, seed=1),
    dict(name="k8_b3_v64", K=8, B=3, V=64, T=4, lp=0.0, es=True, eos=[1, 2], plants=[("eos", 1, 1, 3), ("eos", 2, 2, 9)],
         expect={"eos_hyp", "eos_ignored", "closing"}, seed=3),
    dict(name="k16_b1_real_v", K=16, B=1, V=32064 + 6, T=3, lp=1.0, es=False, eos=[32000],
         plants=[("eos", 1, 0, 3), ("eos", 2, 0, 20), ("tie", 1, 0, 15), ("tie", 2, 0, 31)],
         expect={"eos_hyp", "eos_ignored", "tie_k", "tie_2k"}, seed=1),
    dict(name="k16_b3_v64", K=16, B=3, V=64, T=3, lp=1.0, es="never", eos=[9], plants=[("eos", 1, 1, 5)], expect={"eos_hyp", "closing"}, seed=2),
    dict(name="k16_b3_v1000", K=16, B=3, V=1000, T=3, lp=2.0, es=False, eos=[7, 8], plants=[("eos", 1, 0, 0), ("eos", 2, 2, 17)],
         expect={"eos_hyp", "eos_ignored", "closing"}, seed=343),
    dict(name="k3_b1_real_v_no_eos", K=3, B=1, V=32064 + 6, T=6, lp=0.0, es=False, eos=[], plants=[], expect={"closing"}, seed=0),
]
PAD = 0


class Case:
    pass


def build(spec, seed=None):
    """The case of a spec: logits float32 [T, B*K, V] (bf16 values), the finished reference, the bound, the smallest margin, the events."""
    K, B, V, T = spec["K"], spec["B"], spec["V"], spec["T"]
    rng = np.random.default_rng(spec["seed"] if seed is None else seed)
    logits = round_bf16(4.0 * rng.standard_normal((T, B * K, V), dtype=np.float32))
    ref = RefSearch(B, K, T, spec["eos"], PAD, spec["lp"], spec["es"])
    for t in range(T):
        for kind, pt, b, r in spec["plants"]:
            if pt != t or ref.done[b]:
                continue
            ranked = ref.rank(logits[t], b, 2 * K + 1)
            _, beam, tok = ranked[r]
            row = logits[t, b * K + beam]
            top = {v for _, k, v in ranked if k == beam}
            if kind == "eos":
                free = [e for e in spec["eos"] if e not in top]
                if tok in spec["eos"] or not free:
                    continue
                row[tok], row[free[0]] = row[free[0]], row[tok]
            else:
                other = next(v for v in rng.permutation(V) if v not in top and v not in spec["eos"])
                row[other] = row[tok]
        ref.step(logits[t])
    c = Case()
    c.spec, c.logits, c.ref = spec, logits, ref
    c.M = float(np.abs(logits).max())
    c.logprob_bound = logprob_bound(c.M, V)
    c.bound = hyp_bound(c.M, V, T - 1)
    c.min_margin, c.events = ref.min_margin, ref.events
    return c


def holds(c):
    return c.min_margin >= 4.0 * c.bound and c.spec["expect"] <= c.events


@functools.lru_cache(maxsize=None)
def case(name):
    return build(next(s for s in SPECS if s["name"] == name))


NAMES = [s["name"] for s in SPECS]


if __name__ == "__main__":
    for s in SPECS:
        for seed in range(2000):
            c = build(s, seed)
            if holds(c):
                print(f"{s['name']}: seed {seed} (margin {c.min_margin:.3g}, 4 * bound {4 * c.bound:.3g}, events {sorted(c.events)})")
                break
        else:
            print(f"{s['name']}: no seed found")
