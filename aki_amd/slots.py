"""In-flight batching for generate: the host-side bookkeeping of `AkiMethods.generate_many` (aki_amd/aki.py).

A decode batch is a fixed number of rows ("slots") over one KV cache and one captured step.  A row that has finished - its EOS, or its
token budget (ops.slot_tick) - is parked on the device; at the host's next look it is retired and the next pending request is admitted
into it (a batch-1 prefill + ops.kv_slot_admit) while the other rows stay mid-sequence.  Nothing in this module touches a device: the
scheduler is driven through three callbacks, so a fake token source exercises the very loop generate_many runs."""
from __future__ import annotations

import struct
from collections import deque
from dataclasses import dataclass
from typing import TYPE_CHECKING, Callable, List, Optional, Sequence, Tuple

if TYPE_CHECKING:
    from .constraint import TokenConstraint


# The logits-processor settings a request may own (HF GenerationMixin._get_logits_processor's keywords), with their neutral values
PROCESSOR_FIELDS = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "bad_words_ids": (), "min_length": 0, "min_new_tokens": 0,
                    "suppress_tokens": (), "begin_suppress_tokens": ()}


MAX_PENALTY = 3.0e38                # what the C entry points accept (below FLT_MAX)

# The additive penalties a request may own (the OpenAI / vLLM definition; ops.LogitsProcessors states the arithmetic), with their neutral
# values.  They travel BESIDE the processor sets, as one float per slot, never inside a set's record.
PENALTY_FIELDS = {"frequency_penalty": 0.0, "presence_penalty": 0.0}
MAX_ADDITIVE_PENALTY = 2.0


def check_additive_penalty(who: str, name: str, value) -> float:
    """frequency_penalty / presence_penalty: a finite float in [-2, 2] -> the float32 the device reads.  ValueError beginning with `who`."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not -MAX_ADDITIVE_PENALTY <= v <= MAX_ADDITIVE_PENALTY:
        raise ValueError(f"{who}: {name} has to be a finite float in [-{MAX_ADDITIVE_PENALTY:g}, {MAX_ADDITIVE_PENALTY:g}], got {value}")
    return struct.unpack("<f", struct.pack("<f", v))[0]


def check_min_p(who: str, value) -> float:
    """min_p: a float in [0, 1] -> the float32 the device reads.  ValueError beginning with `who`."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{who}: min_p has to be a float in [0, 1], got {value}")
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _is_int(x) -> bool:
    """An integer, or a float / a one-element array or tensor whose value is a whole number (nothing is truncated silently)."""
    if isinstance(x, bool):
        return False
    if isinstance(x, int):
        return True
    try:
        return float(x) == int(x)
    except (TypeError, ValueError, OverflowError):
        return False


def check_processor_value(who: str, name: str, value, V: Optional[int] = None):
    """One processor setting, checked by the rules of ops.LogitsProcessors -> its normal form (float, int, tuple of ints, tuple of tuples).
    ValueError beginning with `who`.  V (the logits' width) bounds the ids when it is known."""
    def ids(x, what):
        if isinstance(x, (str, bytes)) or not hasattr(x, "__iter__"):
            raise ValueError(f"{who}: {what} is a list of token ids, got {x!r}")
        out = []
        for i in x:
            if not _is_int(i):
                raise ValueError(f"{who}: {what}: a token id is an integer, got {i!r}")
            i = int(i)
            if i < 0 or (V is not None and i >= int(V)):
                raise ValueError(f"{who}: {what}: every id has to be in [0, {'V' if V is None else int(V)}), got {i}")
            out.append(i)
        return tuple(out)

    if name == "repetition_penalty":
        try:
            pen = float(value)
        except (TypeError, ValueError):
            pen = float("nan")
        if not (pen > 0.0 and pen <= MAX_PENALTY):
            raise ValueError(f"{who}: repetition_penalty has to be a strictly positive float (at most {MAX_PENALTY:g}: it is a float32 on "
                             f"the device), got {value}")
        return struct.unpack("<f", struct.pack("<f", pen))[0]          # the float32 the device reads: 1.2 and np.float32(1.2) are one set
    if name in ("no_repeat_ngram_size", "min_length", "min_new_tokens"):
        if not _is_int(value) or not 0 <= int(value) < 1 << 31:
            raise ValueError(f"{who}: {name} is a non-negative integer, got {value!r}")
        return int(value)
    if name in ("suppress_tokens", "begin_suppress_tokens"):
        return ids(value, name)
    if name == "bad_words_ids":
        if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
            raise ValueError(f"{who}: bad_words_ids has to be a list of non-empty lists of token ids, got {value!r}")
        words = []
        for w in value:
            if isinstance(w, (str, bytes)) or not hasattr(w, "__iter__") or len(w) == 0:
                raise ValueError(f"{who}: bad_words_ids has to be a list of non-empty lists of token ids, got {value!r}")
            words.append(ids(w, "bad_words_ids"))
        return tuple(words)
    raise KeyError(name)


@dataclass(frozen=True)
class RequestParams:
    """What one request of generate_many asks for beyond its budget.  do_sample with temperature / top_k / top_p: the device sampler
    (ops.sample_pick_rows) with these values in the request's row; seed: the request's own 64-bit Philox key (None: derived, see
    request_seed) - its draws depend on (seed, generated-token index) only, never on the slot or the neighbours.  logprobs: return the
    log-probability of every returned token under the raw model distribution, with the top_logprobs most likely alternatives.
    constraint: an aki_amd.TokenConstraint with one start state, or None - the request's tokens walk that automaton (the same object may
    serve several requests: its table is stored once); it composes with sampling and log-probabilities.
    The logits processors (PROCESSOR_FIELDS: repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens,
    suppress_tokens, begin_suppress_tokens): None = the request takes the call's value (params=, else the call-wide keyword); any other
    value, the neutral ones 1.0 / 0 / () included, belongs to the request alone (resolve_processors).
    stop_sequences: None = the request takes the call's stop set (params=, else the call-wide stop_sequences= keyword); a list of token-id
    sequences is the request's own set (aki_amd/stops.py states the rule), () means this request has none.
    min_p (HF MinPLogitsWarper, behind top-p; a float in [0, 1], 0 = no filter) is request-owned like temperature, and like top_p it is
    ignored for a greedy request.  frequency_penalty / presence_penalty (PENALTY_FIELDS; finite floats in [-2, 2]): None = the call's
    value (params=, else the call-wide keyword); any other value, 0.0 included, belongs to the request alone (resolve_penalties)."""
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: Optional[int] = None
    logprobs: bool = False
    top_logprobs: int = 0
    constraint: Optional["TokenConstraint"] = None
    repetition_penalty: Optional[float] = None
    no_repeat_ngram_size: Optional[int] = None
    bad_words_ids: Optional[Sequence[Sequence[int]]] = None
    min_length: Optional[int] = None
    min_new_tokens: Optional[int] = None
    suppress_tokens: Optional[Sequence[int]] = None
    begin_suppress_tokens: Optional[Sequence[int]] = None
    stop_sequences: Optional[Sequence[Sequence[int]]] = None
    min_p: float = 0.0
    frequency_penalty: Optional[float] = None
    presence_penalty: Optional[float] = None

    def check(self, index, max_top: int) -> "RequestParams":
        """ValueError naming request `index` (a number, or a word such as "default") for a value the device sampler or ops.token_logprob
        does not take; max_top: ops.LOGPROB_MAX_TOP."""
        who = f"request {index}"
        if not float(self.temperature) > 0.0:
            raise ValueError(f"{who}: temperature must be positive, got {self.temperature}")
        if not 0.0 < float(self.top_p) <= 1.0:
            raise ValueError(f"{who}: 0 < top_p <= 1 is expected, got {self.top_p}")
        if int(self.top_k) != self.top_k or int(self.top_k) < 0:
            raise ValueError(f"{who}: top_k is an integer >= 0, got {self.top_k}")
        if int(self.top_logprobs) != self.top_logprobs or not 0 <= int(self.top_logprobs) <= int(max_top):
            raise ValueError(f"{who}: top_logprobs must be in 0..{max_top}, got {self.top_logprobs}")
        if self.top_logprobs and not self.logprobs:
            raise ValueError(f"{who}: top_logprobs needs logprobs=True")
        if self.seed is not None and (int(self.seed) != self.seed or not 0 <= int(self.seed) < 1 << 64):
            raise ValueError(f"{who}: seed is an integer in [0, 2^64), got {self.seed}")
        if self.constraint is not None:
            from .constraint import TokenConstraint
            if not isinstance(self.constraint, TokenConstraint):
                raise ValueError(f"{who}: constraint is an aki_amd.TokenConstraint or None, got {type(self.constraint).__name__}")
            if len(self.constraint.starts) != 1:
                raise ValueError(f"{who}: a constraint with {len(self.constraint.starts)} start states; a request is one row, so exactly one "
                                 "start state is expected")
        for name in PROCESSOR_FIELDS:                   # the ids' upper bound needs the logits' width: processor_set_key
            if getattr(self, name) is not None:
                check_processor_value(who, name, getattr(self, name))
        check_min_p(who, self.min_p)
        for name in PENALTY_FIELDS:
            if getattr(self, name) is not None:
                check_additive_penalty(who, name, getattr(self, name))
        if self.stop_sequences is not None:             # likewise: stops.check_stop_sequences again with the width
            from .stops import check_stop_sequences
            check_stop_sequences(who, self.stop_sequences)
        return self


def resolve_processors(own: Optional[RequestParams], default: Optional[RequestParams], call: dict) -> dict:
    """One request's processor settings {field: value}: its own RequestParams' value, else that of `default` (generate_many's params=),
    else the call-wide keyword's (`call`: every field of PROCESSOR_FIELDS, None read as neutral).  Only None passes a level on: an explicit
    neutral value overrides."""
    out = {}
    for name, neutral in PROCESSOR_FIELDS.items():
        v = None if own is None else getattr(own, name)
        if v is None and default is not None:
            v = getattr(default, name)
        if v is None:
            v = call.get(name)
        out[name] = neutral if v is None else v
    return out


def resolve_penalties(own: Optional[RequestParams], default: Optional[RequestParams], call: Optional[dict]) -> dict:
    """One request's {frequency_penalty, presence_penalty}, by resolve_processors' rule: its own RequestParams' value, else that of
    `default` (generate_many's params=), else the call-wide keyword's (`call`), else 0.  Only None passes a level on: an explicit 0.0
    overrides.  The values as the float32 the device reads."""
    out = {}
    for name, neutral in PENALTY_FIELDS.items():
        v = None if own is None else getattr(own, name)
        if v is None and default is not None:
            v = getattr(default, name)
        if v is None and call is not None:
            v = call.get(name)
        out[name] = struct.unpack("<f", struct.pack("<f", float(neutral if v is None else v)))[0]
    return out


def processor_set_key(who: str, resolved: dict, eos_ids: Sequence[int], V: int) -> tuple:
    """A request's resolved settings as one hashable value, equal for equal behaviour: (penalty, ngram, min_len, suppress ids, begin-suppress
    ids, bad words) with min_len = max(min_length, min_new_tokens) (no prompt counts here), every id checked against [0, V) and a one-token
    bad word that is an eos id dropped, as HF's NoBadWordsLogitsProcessor does.  ValueError beginning with `who`."""
    v = {name: check_processor_value(who, name, resolved[name], V) for name in PROCESSOR_FIELDS}
    eos = {int(e) for e in eos_ids}
    words = tuple(w for w in v["bad_words_ids"] if not (len(w) == 1 and w[0] in eos))
    min_len = max(v["min_length"], v["min_new_tokens"]) if eos else 0          # without an eos id there is nothing to ban
    return (v["repetition_penalty"], v["no_repeat_ngram_size"], min_len, v["suppress_tokens"], v["begin_suppress_tokens"], words)


NEUTRAL_SET_KEY = (1.0, 0, 0, (), (), ())


def banning_keywords(who: str, resolved: dict, eos_ids: Sequence[int], V: int) -> List[str]:
    """The keywords among a request's resolved settings that ban a token, judged on the NORMAL form processor_set_key builds: a minimum
    length without an eos id and a bad word that is dropped ban nothing; lists may be arrays or tensors."""
    v = {name: check_processor_value(who, name, resolved[name], V) for name in PROCESSOR_FIELDS}
    eos = {int(e) for e in eos_ids}
    on = {"no_repeat_ngram_size": v["no_repeat_ngram_size"] > 0,
          "bad_words_ids": any(not (len(w) == 1 and w[0] in eos) for w in v["bad_words_ids"]),
          "min_length": bool(eos) and v["min_length"] > 0, "min_new_tokens": bool(eos) and v["min_new_tokens"] > 0,
          "suppress_tokens": len(v["suppress_tokens"]) > 0, "begin_suppress_tokens": len(v["begin_suppress_tokens"]) > 0}
    return [k for k in PROCESSOR_FIELDS if on.get(k)]


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """Philox4x32-10 on Python integers: counter (c0, c1, c2, c3) and key (k0, k1) as 32-bit words -> the four output words."""
    m = 0xFFFFFFFF
    c0, c1, c2, c3 = (int(c) & m for c in counter)
    k0, k1 = (int(k) & m for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def request_seed(seed: int, offset: int, r: int) -> int:
    """The 64-bit Philox key of request r (its position in `requests`) of the generate_many call that took `offset` from a
    DeviceGenerator(seed): words 0 and 1 of Philox4x32-10(key = seed, counter = (r, 0, offset lo, offset hi)) as word0 | word1 << 32.
    Host only, Python integers.  A request's draws then use this key with the counter (generated-token index, 0, 0, 0)."""
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((int(r), 0, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return w[0] | (w[1] << 32)


def expanded_length(ids: Sequence[int], media_token_id: int, n_vis_tokens: int) -> int:
    """The length of a prompt in the language stream: every `<image>` placeholder among `ids` is replaced by the n_vis_tokens vision tokens of
    its image (the splice of VLMWithLanguageStream._prepare_inputs_for_forward), so T ids become T + (n_vis_tokens - 1) * n_images rows."""
    ids = list(ids)
    return len(ids) + (int(n_vis_tokens) - 1) * sum(1 for i in ids if int(i) == int(media_token_id))


def slot_capacity(prompts: Sequence[Sequence[int]], budgets: Sequence[int], media_token_id: int, n_vis_tokens: int) -> int:
    """Rows of the slot cache: the largest (expanded prompt length + token budget) over the requests - computed from the ids on the host."""
    if len(prompts) != len(budgets):
        raise ValueError("slot_capacity: one budget per prompt")
    return max((expanded_length(p, media_token_id, n_vis_tokens) + int(b) for p, b in zip(prompts, budgets)), default=0)


class SlotScheduler:
    """Which request sits in which slot, which pending request goes where, and the counters of a run.  Pure bookkeeping.

    `run(admit, step, look, retire)` is the whole loop:
      admit(request, slot) -> bool   put the request into the slot (its token 0 included); True when it may have finished at once
                                     (a budget of one token), which makes the scheduler look before it steps
      step(n)                        n decode steps of all slots, no synchronisation
      look() -> (done, done_at)      the only synchronisation: per slot, whether its row has finished and the index of its last token
      retire(request, slot, n)       the row's first n = done_at + 1 tokens are the request's result: copy them out now
      room() -> int (optional)       decode steps that still fit before the next look must happen (the cache's capacity)
    The host looks every `period` steps.  A finished slot is retired at the first look after it finished and refilled then, lowest free
    slot first, requests in their order; with nothing pending it stays done and parked.  The run ends at the first look after the last
    row finished.  Counters: steps (decode steps replayed), total_row_steps = slots * steps, live_row_steps (steps that produced a returned
    token: a request of n tokens costs n - 1, token 0 comes from its prefill), admits, looks."""

    def __init__(self, n_requests: int, slots: int, period: int = 8):
        n_requests, slots, period = int(n_requests), int(slots), int(period)
        if n_requests < 0 or slots < 1 or period < 1:
            raise ValueError("SlotScheduler: n_requests >= 0, slots >= 1 and period >= 1 are expected")
        self.n_requests, self.slots, self.period = n_requests, slots, period
        self.slot_request: List[Optional[int]] = [None] * slots
        self.pending = deque(range(n_requests))
        self.lengths: List[Optional[int]] = [None] * n_requests      # tokens returned per request, once retired
        self.served_in: List[Optional[int]] = [None] * n_requests    # the slot that served it
        self.steps = self.live_row_steps = self.total_row_steps = self.admits = self.looks = 0

    def busy(self) -> bool:
        return any(r is not None for r in self.slot_request)

    def admissions(self) -> List[Tuple[int, int]]:
        """(slot, request) for every free slot that gets a pending request now; the slots are marked taken."""
        out = []
        for slot in range(self.slots):
            if not self.pending:
                break
            if self.slot_request[slot] is None:
                req = self.pending.popleft()
                self.slot_request[slot] = req
                out.append((slot, req))
        self.admits += len(out)
        return out

    def stepped(self, n: int) -> None:
        self.steps += n
        self.total_row_steps += self.slots * n

    def retirements(self, done, done_at) -> List[Tuple[int, int, int]]:
        """One look's result -> (slot, request, tokens) of every occupied slot whose row has finished; the slots are freed."""
        self.looks += 1
        out = []
        for slot, req in enumerate(self.slot_request):
            if req is not None and done[slot]:
                n = int(done_at[slot]) + 1
                if n < 1:
                    raise RuntimeError(f"slot {slot} is done without a last-token index")
                self.slot_request[slot] = None
                self.lengths[req], self.served_in[req] = n, slot
                self.live_row_steps += n - 1
                out.append((slot, req, n))
        return out

    def run(self, admit: Callable[[int, int], bool], step: Callable[[int], None], look: Callable[[], tuple],
            retire: Callable[[int, int, int], None], room: Optional[Callable[[], int]] = None) -> None:
        while True:
            quick = False
            for slot, req in self.admissions():
                quick = bool(admit(req, slot)) or quick
            if not self.busy():
                return
            if not quick:
                n = self.period if room is None else min(self.period, int(room()))
                if n < 1:
                    raise RuntimeError("SlotScheduler: no room for a decode step although a slot is live")
                step(n)
                self.stepped(n)
            done, done_at = look()
            for slot, req, n in self.retirements(done, done_at):
                retire(req, slot, n)

    def in_request_order(self, results: dict) -> list:
        """{request: result} -> the results as a list in request order (every request must have been served)."""
        missing = [r for r in range(self.n_requests) if r not in results]
        if missing:
            raise RuntimeError(f"requests {missing} were never served")
        return [results[r] for r in range(self.n_requests)]

    def stats(self) -> dict:
        return {"slots": self.slots, "period": self.period, "requests": self.n_requests, "steps": self.steps,
                "live_row_steps": self.live_row_steps, "total_row_steps": self.total_row_steps, "admits": self.admits, "looks": self.looks}
