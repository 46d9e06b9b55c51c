"""AKI model class: host-side mirror of src/aki.py (train-time AKI) with the same constructor and
forward signature; see also src/modeling_aki.py:83-151 (HF-Hub twin, same forward).

Reference: /root/reference/codes/open_flamingo/src/aki.py  (__init__ :10-50, set_trainable :52-57, forward :65-134)
"""
from __future__ import annotations

import itertools
from collections import namedtuple
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import torch
from torch import nn

try:  # the HF container generate's structured outputs subclass
    from transformers.utils import ModelOutput
except Exception:  # pragma: no cover - transformers is present in this image
    ModelOutput = object

from . import ops
from .helpers import PerceiverResampler
from .phi3 import AkiKVCache, DecodeGraph
from .pick_stage import PickStage
from .slots import (PENALTY_FIELDS, RequestParams, SlotScheduler, banning_keywords, check_additive_penalty, check_min_p, processor_set_key,
                    request_seed, resolve_penalties, resolve_processors, slot_capacity)
from .stops import check_stop_sequences, first_finish, resolve_stop_sequences
from .vlm import VLMWithLanguageStream


def sample_next(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, generator=None,
                min_p: float = 0.0) -> torch.Tensor:
    """One sampling step on [B, V] logits, in HF's processor order: temperature, top-k, top-p (nucleus), min-p, multinomial."""
    x = logits.float() / temperature
    V = x.shape[-1]
    if 0 < top_k < V:
        kth = x.topk(top_k, dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sx, si = x.sort(dim=-1, descending=True)
        cum = sx.softmax(dim=-1).cumsum(dim=-1)
        drop = cum - sx.softmax(dim=-1) >= top_p            # keep the smallest prefix whose mass reaches top_p (always >= 1 token)
        sx = sx.masked_fill(drop, float("-inf"))
        x = torch.full_like(x, float("-inf")).scatter(-1, si, sx)
    if min_p > 0.0:                                         # HF MinPLogitsWarper: drop what lies below min_p times the largest probability
        probs = x.softmax(dim=-1)
        x = x.masked_fill(probs < min_p * probs.amax(dim=-1, keepdim=True), float("-inf"))
    return torch.multinomial(x.softmax(dim=-1), 1, generator=generator).squeeze(-1)


# HF generation keywords that select a logits processor (transformers GenerationMixin._get_logits_processor), with their neutral values
PROCESSOR_KWARGS = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "bad_words_ids": None, "min_length": 0, "min_new_tokens": 0,
                    "suppress_tokens": None, "begin_suppress_tokens": None}


def _pop_processor_kwargs(kwargs: dict) -> dict:
    """The logits-processor keywords of `generate` (popped), with None read as the neutral value, as HF's GenerationConfig does."""
    out = {}
    for k, neutral in PROCESSOR_KWARGS.items():
        v = kwargs.pop(k, None)
        out[k] = neutral if v is None else v
    return out


def _pop_penalty_kwargs(who: str, kwargs: dict) -> dict:
    """frequency_penalty= / presence_penalty= (popped, None read as 0), checked: finite floats in [-2, 2], as the float32 the device reads."""
    out = {}
    for k, neutral in PENALTY_FIELDS.items():
        v = kwargs.pop(k, None)
        out[k] = check_additive_penalty(who, k, neutral if v is None else v)
    return out


def _reject_unused_kwargs(kwargs: dict) -> None:
    """What HF's `_validate_model_kwargs` does with keywords generate() does not use: a ValueError naming them, never a silent drop."""
    if kwargs:
        raise ValueError(f"generate() cannot honour the keyword argument(s) {sorted(kwargs)}: the supported ones are the greedy / sampling / "
                         f"beam-search controls, the logits processors {sorted(PROCESSOR_KWARGS)}, min_p, {sorted(PENALTY_FIELDS)} and stop_sequences (lists of token ids, "
                         "matched on the device: what stopping_criteria / stop_strings would be asked for)")


def _embedding_tables(emb: nn.Module, logits: torch.Tensor):
    """(weight, additional weight or None, max_original_id) when ops.greedy_pick can gather the picked token's embedding row itself
    (bf16 tables that hold a row for every logit column), else None: the module's own forward is used."""
    w = getattr(emb, "weight", None)
    if w is None or w.dtype != torch.bfloat16 or not w.is_contiguous() or w.device != logits.device or w.shape[1] % 8:
        return None
    n_add = int(getattr(emb, "num_additional_embeddings", 0) or 0)
    if n_add > 0:
        extra, max_orig = emb.additional_embedding.weight, int(emb.max_original_id)
        if extra.dtype != torch.bfloat16 or not extra.is_contiguous() or extra.device != w.device or w.shape[0] <= max_orig:
            return None
        rows = max_orig + 1 + extra.shape[0]
    elif type(emb) is nn.Embedding or hasattr(emb, "max_original_id"):
        extra, max_orig, rows = None, w.shape[0] - 1, w.shape[0]
    else:
        return None
    return (w, extra, max_orig) if logits.shape[-1] <= rows else None


# The keyword arguments of `generate`, resolved and validated by _parse_generate_kwargs.  rng: None or a torch.Generator (sample_next) or an
# ops.DeviceGenerator, which device_rng repeats (else None: no device sampler); n_ret: num_return_sequences; eos_ids: a set; processors:
# the logits-processor keywords (PROCESSOR_KWARGS) with None read as the neutral value; output_logprobs / top_logprobs: the per-token
# log-probabilities of the returned tokens and that many alternatives (ops.token_logprob).
# constraint: None, a constraint.TokenConstraint or a list of one per sample (constrained decoding; bound to the device in generate).
# stops: the call's stop set in its normal form (stops.check_stop_sequences; () = none), one set for every row.
# min_p: the sampler's min-p filter (0 = none; ignored without do_sample, as top_p is); penalties: {frequency_penalty, presence_penalty},
# the additive penalties beside the processors (PENALTY_FIELDS; 0 = neutral).
GenerateOptions = namedtuple("GenerateOptions", "num_beams do_sample temperature top_k top_p rng device_rng length_penalty early_stopping "
                                                "n_ret max_new_tokens eos_ids pad_id use_graph processors output_logprobs top_logprobs "
                                                "constraint stops min_p penalties", defaults=(0.0, None))

# the processors that ban tokens outright: together with a constraint they could leave a row with nothing allowed
BANNING_KWARGS = ("no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens")


@dataclass
class AkiGenerateOutput(ModelOutput):
    """What `generate(..., output_logprobs=True)` returns.  sequences: what generate returns without the keyword, int64 [rows, steps];
    logprobs f32 [rows, steps]: the log-probability of every returned token under the raw model distribution of its step; top_token_ids
    int64 [rows, steps, k] and top_logprobs f32 [rows, steps, k]: the k most likely tokens of each step and theirs (None for k = 0).
    Positions behind a row's EOS hold 0.0, -1 and 0.0.  All on the device."""
    sequences: Optional[torch.Tensor] = None
    logprobs: Optional[torch.Tensor] = None
    top_token_ids: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None


@dataclass
class AkiScoreOutput(ModelOutput):
    """What `score` returns.  logprobs f32 [B, N, T]: the teacher-forced log-probability of every continuation token, zero behind each
    length; sum_logprobs f32 [B, N]; lengths int64 [B, N]; top_token_ids int64 [B, N, T, k] and top_logprobs f32 [B, N, T, k] as in
    AkiGenerateOutput (None for k = 0; -1 and 0.0 behind each length).  All on the device."""
    logprobs: Optional[torch.Tensor] = None
    sum_logprobs: Optional[torch.Tensor] = None
    lengths: Optional[torch.Tensor] = None
    top_token_ids: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None


@dataclass
class AkiRequestOutput(ModelOutput):
    """One request's result from `generate_many` when any request asked for log-probabilities.  tokens: what generate_many returns
    without them, 1-D int64; logprobs f32 [n], top_token_ids int64 [n, k] and top_logprobs f32 [n, k] for the request's own
    k = top_logprobs (None for k = 0), as in AkiGenerateOutput; all three None for a request that did not ask.  All on the device."""
    tokens: Optional[torch.Tensor] = None
    logprobs: Optional[torch.Tensor] = None
    top_token_ids: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None


class _LogprobBuffers:
    """The outputs of ops.token_logprob for one decode loop, pre-filled with the skipped values: lp f32 [rows, steps], and for k > 0
    top_ids int64 [rows, steps, k] and top_lp f32 [rows, steps, k] (else None)."""

    def __init__(self, rows: int, steps: int, k: int, device):
        self.k = k
        self.lp = torch.zeros((rows, steps), dtype=torch.float32, device=device)
        self.top_ids = torch.full((rows, steps, k), -1, dtype=torch.int64, device=device) if k else None
        self.top_lp = torch.zeros((rows, steps, k), dtype=torch.float32, device=device) if k else None

    def args(self) -> dict:
        return dict(top_k=self.k, out_logprob=self.lp, out_top_ids=self.top_ids, out_top_logprobs=self.top_lp)

    def reset_from(self, t: int):
        self.lp[:, t:] = 0.0
        if self.k:
            self.top_ids[:, t:] = -1
            self.top_lp[:, t:] = 0.0

    def cut(self, n: int):
        return self.lp[:, :n], (self.top_ids[:, :n] if self.k else None), (self.top_lp[:, :n] if self.k else None)


def _parse_generate_kwargs(kwargs: dict, default_pad_id, default_eos_ids, from_cache: bool, batch: Optional[int] = None) -> GenerateOptions:
    """Every keyword of `generate` popped from `kwargs`, checked and given its default, before any device work.  default_eos_ids: a callable,
    asked only when the caller passes no `eos_token_id`; from_cache: generate(past_key_values=...); batch: the number of samples, which a
    list of constraints has to match.  A keyword that is left over (`logits_processor`, `stopping_criteria`, `output_scores`,
    `generation_config`, `prefix_allowed_tokens_fn`, ...) raises ValueError instead of being ignored."""
    num_beams = int(kwargs.pop("num_beams", 1))
    do_sample = bool(kwargs.pop("do_sample", False))
    temperature = float(kwargs.pop("temperature", 1.0))
    top_k = int(kwargs.pop("top_k", 0) or 0)
    top_p = float(kwargs.pop("top_p", 1.0))
    min_p = check_min_p("generate", kwargs.pop("min_p", None) or 0.0)
    penalties = _pop_penalty_kwargs("generate", kwargs)
    rng = kwargs.pop("generator", None)
    length_penalty = float(kwargs.pop("length_penalty", 1.0))
    early_stopping = kwargs.pop("early_stopping", False)
    device_rng = rng if isinstance(rng, ops.DeviceGenerator) else None
    if device_rng is not None:
        if not do_sample or num_beams > 1:
            raise ValueError("generator=DeviceGenerator(...) selects the device sampler: it needs do_sample=True and num_beams=1")
        if not 0.0 < top_p <= 1.0 or top_k < 0:
            raise ValueError("the device sampler takes 0 < top_p <= 1 and top_k >= 0")
    n_ret = int(kwargs.pop("num_return_sequences", 1))
    if n_ret < 1:
        raise ValueError("num_return_sequences must be at least 1")
    if n_ret > 1 and num_beams > 1:
        raise NotImplementedError("num_return_sequences > 1 with beam search")
    if num_beams < 1 or (num_beams > 1 and do_sample):
        raise NotImplementedError("beam-sample decoding (num_beams > 1 with do_sample=True)")
    for name, v in (("min_p", min_p), *penalties.items()):
        if num_beams > 1 and v != 0.0:
            raise NotImplementedError(f"{name} with num_beams > 1: beam search under min_p or the frequency / presence penalties")
    if n_ret > 1 and not do_sample:
        raise ValueError("num_return_sequences > 1 needs do_sample=True: greedy decoding returns one sequence per sample")
    if do_sample and temperature <= 0:
        raise ValueError("temperature must be positive")
    if from_cache and (num_beams > 1 or n_ret > 1):
        raise NotImplementedError("generate(past_key_values=...) continues one sequence per cached row: beam search and "
                                  "num_return_sequences > 1 start from a fresh prefill")
    max_new_tokens = int(kwargs.pop("max_new_tokens", kwargs.pop("max_length", 20)))
    # HF `generate` stops on generation_config.eos_token_id when the caller passes none (the reference's callers pass only
    # max_new_tokens / do_sample: local_demo.py:76-87, eval_cv_bench/eval.py:99-104); `eos_token_id=[]` switches it off.
    eos = kwargs.pop("eos_token_id", None)
    if eos is None:
        eos = default_eos_ids()
    eos_ids = set([eos] if isinstance(eos, int) else (eos or []))
    pad_id = kwargs.pop("pad_token_id", default_pad_id)
    use_graph = kwargs.pop("use_graph", None)
    if use_graph is None:
        use_graph = max_new_tokens >= 8          # capture costs about two eager steps
    processors = _pop_processor_kwargs(kwargs)
    output_logprobs = bool(kwargs.pop("output_logprobs", False))
    top_logprobs = int(kwargs.pop("top_logprobs", 0) or 0)
    if top_logprobs and not output_logprobs:
        raise ValueError("top_logprobs needs output_logprobs=True")
    if not 0 <= top_logprobs <= ops.LOGPROB_MAX_TOP:
        raise ValueError(f"top_logprobs must be in 0..{ops.LOGPROB_MAX_TOP}")
    if output_logprobs and num_beams > 1:
        raise NotImplementedError("output_logprobs with num_beams > 1: beam search keeps last_beam_scores")
    constraint = kwargs.pop("constraint", None)
    if constraint is not None:
        from .constraint import TokenConstraint
        if num_beams > 1:
            raise NotImplementedError("constraint with num_beams > 1: beam search under a token constraint")
        banning = [k for k in BANNING_KWARGS if processors[k]]
        if banning:
            raise ValueError(f"constraint together with {banning}: a processor that bans tokens can leave a constrained row with nothing "
                             "allowed; only repetition_penalty composes with a constraint")
        if not isinstance(constraint, TokenConstraint):
            constraint = list(constraint) if isinstance(constraint, (list, tuple)) else [constraint]
            if not constraint or any(not isinstance(c, TokenConstraint) for c in constraint):
                raise ValueError("constraint is an aki_amd.TokenConstraint or a list of one per sample")
            if batch is not None and len(constraint) != batch:
                raise ValueError(f"constraint lists {len(constraint)} constraints for a batch of {batch} samples")
    stops = kwargs.pop("stop_sequences", None)
    stops = () if stops is None else check_stop_sequences("generate", stops)       # the ids' upper bound needs the logits' width: generate
    if stops and num_beams > 1:
        raise NotImplementedError("stop_sequences with num_beams > 1: beam search under stop sequences")
    _reject_unused_kwargs(kwargs)
    return GenerateOptions(num_beams=num_beams, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, rng=rng,
                           device_rng=device_rng, length_penalty=length_penalty, early_stopping=early_stopping, n_ret=n_ret,
                           max_new_tokens=max_new_tokens, eos_ids=eos_ids, pad_id=pad_id, use_graph=use_graph, processors=processors,
                           output_logprobs=output_logprobs, top_logprobs=top_logprobs, constraint=constraint, stops=stops, min_p=min_p,
                           penalties=penalties)


# The keyword arguments of `generate_many`, resolved by _parse_many_kwargs: max_new_tokens is the default budget of a request, params the
# RequestParams of a request that brings none, generator None or the ops.DeviceGenerator the sampled requests' seeds are derived from,
# stops the call-wide stop_sequences= keyword in its normal form or None: the default of every request whose RequestParams leave it None;
# penalties the call-wide frequency_penalty= / presence_penalty= keywords (PENALTY_FIELDS), the default of the same kind.
ManyOptions = namedtuple("ManyOptions", "max_new_tokens eos_ids pad_id use_graph processors params generator stops penalties",
                         defaults=(None,))


@dataclass
class _ManyPlan:
    """What AkiMethods._plan_many hands to generate_many's two paths.  reqs: _many_requests' (vision_x, lang_x, budget, RequestParams);
    seeds: _many_seeds' value per request; eos_list: the call's eos ids, sorted.  For a queue that is not empty also, per request:
    resolved (its processor keywords), set_keys (their slots.processor_set_key), stop_keys (its stop set, normal form); mixed: the
    requests resolve to more than one processor set, else pk is the one they share; pool: the constraint.ConstraintPool of a call with a
    constrained request; dev / dtype / on_device (bf16 on the GPU: the device picks) and width, the logits' columns; extras: per request
    {frequency_penalty, presence_penalty, min_p} (slots.resolve_penalties; min_p 0 for a greedy request, which ignores it)."""
    opt: ManyOptions
    slots: int
    reqs: list
    seeds: list
    eos_list: list
    resolved: Optional[list] = None
    set_keys: Optional[list] = None
    stop_keys: Optional[list] = None
    extras: Optional[list] = None
    mixed: bool = False
    pk: Optional[dict] = None
    pool: object = None
    dev: Optional[torch.device] = None
    dtype: Optional[torch.dtype] = None
    on_device: bool = False
    width: int = 0

    @property
    def sampled(self) -> bool:
        return any(rp.do_sample for *_, rp in self.reqs)

    def uses(self, name: str) -> bool:
        """Some request of the call carries a value of `name` (frequency_penalty, presence_penalty, min_p) that is not neutral."""
        return any(e[name] != 0.0 for e in self.extras or ())

    @property
    def penalized(self) -> bool:
        return any(self.uses(k) for k in ("frequency_penalty", "presence_penalty", "min_p"))

    @property
    def constrained(self) -> bool:
        return any(rp.constraint is not None for *_, rp in self.reqs)

    @property
    def want_lp(self) -> bool:
        return any(rp.logprobs for *_, rp in self.reqs)

    @property
    def top(self) -> int:
        return max(int(rp.top_logprobs) for *_, rp in self.reqs)

    @property
    def any_stops(self) -> bool:
        return any(self.stop_keys)

    def result(self, tok, rp, lp=None, top_ids=None, top_lp=None):
        """One request's return value: the tokens, or an AkiRequestOutput when any request of the call asked for log-probabilities."""
        if not self.want_lp:
            return tok
        if not rp.logprobs:
            return AkiRequestOutput(tokens=tok)
        k = int(rp.top_logprobs)
        return AkiRequestOutput(tokens=tok, logprobs=lp, top_token_ids=top_ids[:, :k].clone() if k else None,
                                top_logprobs=top_lp[:, :k].clone() if k else None)

# what generate_many refuses, with the reason: (keyword, the test that it is in force, why)
MANY_REFUSED = (
    ("do_sample", lambda v: bool(v), "sampling belongs to a request, not to the call: pass RequestParams(do_sample=True, ...) in the request "
                                     "tuple or as params="),
    ("num_beams", lambda v: v is not None and int(v) > 1, "beam search re-orders the rows of its cache; a slot is one row"),
    ("num_return_sequences", lambda v: v is not None and int(v) > 1, "it needs sampling; pass the prompt as several requests instead"),
    ("output_logprobs", lambda v: bool(v), "log-probabilities belong to a request, not to the call: pass RequestParams(logprobs=True, ...) in "
                                           "the request tuple or as params="),
    ("constraint", lambda v: v is not None, "a token constraint belongs to a request, not to the call: pass RequestParams(constraint=...) in the "
                                            "request tuple or as params="),
    ("past_key_values", lambda v: v is not None, "every request is prefilled into its slot; continue a cache with generate()"),
)


def _parse_many_kwargs(kwargs: dict, default_pad_id, default_eos_ids) -> ManyOptions:
    """Every keyword of `generate_many` popped from `kwargs` and checked, before any device work.  The keywords of MANY_REFUSED raise
    NotImplementedError naming the keyword and the reason; whatever is left over raises ValueError (_reject_unused_kwargs)."""
    for name, in_force, why in MANY_REFUSED:
        if name in kwargs and in_force(kwargs[name]):
            raise NotImplementedError(f"generate_many does not take {name}: {why}")
        kwargs.pop(name, None)
    max_new_tokens = int(kwargs.pop("max_new_tokens", kwargs.pop("max_length", 20)))
    if max_new_tokens < 1:
        raise ValueError("generate_many: max_new_tokens must be at least 1")
    eos = kwargs.pop("eos_token_id", None)
    if eos is None:
        eos = default_eos_ids()
    eos_ids = set([eos] if isinstance(eos, int) else (eos or []))
    pad_id = kwargs.pop("pad_token_id", default_pad_id)
    use_graph = kwargs.pop("use_graph", None)
    processors = _pop_processor_kwargs(kwargs)
    penalties = _pop_penalty_kwargs("generate_many: the call-wide keyword", kwargs)
    params = kwargs.pop("params", None)
    if params is None:
        params = RequestParams()
    if not isinstance(params, RequestParams):
        raise ValueError("generate_many: params is an aki_amd.RequestParams, the default of the requests that bring none")
    params.check("default (params=)", ops.LOGPROB_MAX_TOP)
    generator = kwargs.pop("generator", None)
    if generator is not None and not isinstance(generator, ops.DeviceGenerator):
        raise ValueError("generate_many: generator is an aki_amd.DeviceGenerator (the sampled requests' seeds are derived from it on the "
                         "host) or None; a torch.Generator cannot seed the device sampler")
    stops = kwargs.pop("stop_sequences", None)
    if stops is not None:
        stops = check_stop_sequences("generate_many: the call-wide keyword", stops)
    _reject_unused_kwargs(kwargs)
    return ManyOptions(max_new_tokens=max_new_tokens, eos_ids=eos_ids, pad_id=pad_id, use_graph=True if use_graph is None else bool(use_graph),
                       processors=processors, params=params, generator=generator, stops=stops, penalties=penalties)


def _many_requests(requests, default_budget: int, default_params: Optional[RequestParams] = None):
    """`generate_many`'s requests -> a list of (vision_x or None, lang_x [1, T], budget, RequestParams), shapes, budgets and parameters
    checked on the host."""
    out = []
    default_params = RequestParams() if default_params is None else default_params
    for i, r in enumerate(requests):
        if not isinstance(r, (tuple, list)) or len(r) not in (2, 3, 4):
            raise ValueError(f"request {i}: (vision_x, lang_x), (vision_x, lang_x, max_new_tokens) or (vision_x, lang_x, max_new_tokens or "
                             "None, RequestParams) is expected")
        vx, lx = r[0], r[1]
        rp = default_params if len(r) < 4 or r[3] is None else r[3]
        if not isinstance(rp, RequestParams):
            raise ValueError(f"request {i}: its fourth entry is an aki_amd.RequestParams")
        rp.check(i, ops.LOGPROB_MAX_TOP)
        budget = int(default_budget if len(r) == 2 or r[2] is None else r[2])
        if not torch.is_tensor(lx) or lx.dim() != 2 or lx.shape[0] != 1 or lx.shape[1] < 1 or lx.dtype != torch.long:
            raise ValueError(f"request {i}: lang_x is an int64 tensor [1, T] without padding, T >= 1")
        if vx is not None and (not torch.is_tensor(vx) or vx.dim() != 6 or vx.shape[0] != 1):
            raise ValueError(f"request {i}: vision_x is [1, T_img, 1, C, H, W] or None")
        if budget < 1:
            raise ValueError(f"request {i}: a budget of {budget} tokens; at least 1 is expected")
        out.append((vx, lx, budget, rp))
    return out


def _many_seeds(reqs, generator) -> List[Optional[int]]:
    """The 64-bit Philox key of every sampled request (None for the others), on the host.  A request's own `seed` is used as it is; the
    others get slots.request_seed(S, offset, r) with r the request's position: (S, offset) = (generator.seed, generator.next_offset()) -
    the offset is taken ONCE per generate_many call, whether or not anything samples - or, without a generator, S = 64 bits from torch's
    CPU default generator (so torch.manual_seed reproduces a call and successive calls differ; drawn only when a request needs it) and
    offset 0.  No device work."""
    offset = generator.next_offset() if generator is not None else 0
    base = generator.seed if generator is not None else None
    seeds = []
    for r, (_, _, _, rp) in enumerate(reqs):
        if not rp.do_sample:
            seeds.append(None)
        elif rp.seed is not None:
            seeds.append(int(rp.seed))
        else:
            if base is None:
                hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
                base = (hi << 32) | lo
            seeds.append(request_seed(base, offset, r))
    return seeds


def _logits_processors(V: int, device, pk: dict, eos_ids, **kw):
    """The ops.LogitsProcessors of a processor-keyword dict (PROCESSOR_KWARGS' keys; kw: constraint=, slot_constraints= or the additive
    penalties frequency_penalty= / presence_penalty=), or None when
    nothing in it is active: the picks then launch exactly what they launch without processors."""
    p = ops.LogitsProcessors(V, device, pk["repetition_penalty"], pk["no_repeat_ngram_size"], max(int(pk["min_length"]), int(pk["min_new_tokens"])),
                             eos_ids, pk["suppress_tokens"], pk["begin_suppress_tokens"], pk["bad_words_ids"], **kw)
    return p if p.active else None


def _device_sampler_args(opt: GenerateOptions):
    """ops.sample_pick's own arguments when a DeviceGenerator selected the device sampler, else None: one offset per generate call."""
    g = opt.device_rng
    if g is None:
        return None
    args = dict(temperature=opt.temperature, top_k=opt.top_k, top_p=opt.top_p, seed=g.seed, offset=g.next_offset())
    if opt.min_p:                               # without it the pick takes the entry point it always took
        args["min_p"] = opt.min_p
    return args


def _first_end(tokens: torch.Tensor, eos_t, stops=()):
    """tokens [B, n], eos_t [E] or None, the call's stop set `stops` (normal form, one set for every row) -> stops.first_finish's
    (finished [B] bool: an EOS or a stop sequence ends the row; index [B] int64 of the token that ends it, 0 where nothing does;
    stop_hit [B] int32)."""
    return first_finish(tokens, eos_t, [stops], [0] * tokens.shape[0])


def _many_stop_sets(reqs, opt: "ManyOptions", V: Optional[int] = None):
    """Every request's resolved stop set in its normal form (stops.resolve_stop_sequences: its own, else params=, else the call-wide
    keyword; none of them: ()), the ids checked against V where it is known.  ValueError naming the request."""
    out = []
    for i, (*_, rp) in enumerate(reqs):
        v = resolve_stop_sequences(rp.stop_sequences, opt.params.stop_sequences, opt.stops)
        out.append(() if v is None else check_stop_sequences(f"request {i}", v, V))
    return out


def _pad_rows(rows, pad_id: int, device) -> torch.Tensor:
    """A list of 1-D int64 token rows of any lengths -> [B, longest] on `device`, the shorter rows filled up with pad_id."""
    out = torch.full((len(rows), max(x.numel() for x in rows)), pad_id, dtype=torch.long)
    for b, x in enumerate(rows):
        out[b, : x.numel()] = x
    return out.to(device)


def _logits_width(lm) -> int:
    """V', the columns of a language model's logits: DecoupledLinear's output is the original ids followed by the added ones (helpers.py),
    a plain head's its rows."""
    head = lm.get_output_embeddings()
    return int(head.max_original_id) + 1 + int(head.additional_out_features) if hasattr(head, "max_original_id") else int(head.out_features)


def _plan_many(model, requests, slots, kwargs) -> "_ManyPlan":
    """generate_many's host half (model: the AkiMethods object, of which it reads pad_token_id, default_eos_token_ids and lang_model): the
    keywords, the requests, their seeds, and every request's resolved processor settings, stop set and
    constraint, checked against the logits' width.  Every ValueError / NotImplementedError the arguments can cause is raised here,
    before any device work.  An empty queue: the plan holds no more than the (checked) slots."""
    opt = _parse_many_kwargs(kwargs, model.pad_token_id, model.default_eos_token_ids)
    slots = int(slots)
    if slots < 1 or slots > ops.SLOT_MAX_ROWS:
        raise ValueError(f"generate_many: 1 <= slots <= {ops.SLOT_MAX_ROWS} (the rows the skinny decode GEMMs take) is expected, got {slots}")
    reqs = _many_requests(requests, opt.max_new_tokens, opt.params)
    plan = _ManyPlan(opt, slots, reqs, _many_seeds(reqs, opt.generator), sorted(opt.eos_ids))
    model.last_many_stats = None
    model.last_stop_hits = None
    if not reqs:
        return plan
    plan.dev = reqs[0][1].device
    plan.dtype = model.lang_model.get_input_embeddings().weight.dtype
    plan.on_device = plan.dev.type == "cuda" and plan.dtype == torch.bfloat16
    if plan.sampled and not plan.on_device:
        raise ValueError("generate_many: a sampled request needs the device sampler, which needs bf16 logits on the GPU")
    eos_list, width = plan.eos_list, _logits_width(model.lang_model)
    plan.width = width
    # every request's stop set: its own, else params=, else the call-wide keyword, its ids checked against the logits' width
    plan.stop_keys = _many_stop_sets(reqs, opt, width)
    # every request's processor settings: its own, else params=, else the call-wide keyword - checked on the host against the logits'
    # width and reduced to one value per distinct behaviour.  A call whose requests all resolve to one set runs the call-wide path.
    plan.resolved = [resolve_processors(rp, opt.params, opt.processors) for *_, rp in reqs]
    plan.set_keys = [processor_set_key(f"request {i}", r, eos_list, width) for i, r in enumerate(plan.resolved)]
    # the additive penalties resolve the same way; min_p is the request's own (a greedy request's is ignored, as its top_p is)
    plan.extras = [dict(resolve_penalties(rp, opt.params, opt.penalties), min_p=check_min_p(f"request {i}", rp.min_p) if rp.do_sample else 0.0)
                   for i, (*_, rp) in enumerate(reqs)]
    plan.mixed = len(set(plan.set_keys)) > 1
    plan.pk = opt.processors if plan.mixed else plan.resolved[0]
    if plan.constrained:                            # the host half: every table with its eos columns, checked before any device work
        from .constraint import ConstraintPool
        plan.pool = ConstraintPool(eos_list, [rp.constraint for *_, rp in reqs], width)
        for i, ((*_, rp), r) in enumerate(zip(reqs, plan.resolved)):
            banning = banning_keywords(f"request {i}", r, eos_list, width) if rp.constraint is not None else []
            for k in PROCESSOR_KWARGS:              # what bans nothing after normalisation goes to generate() as the neutral value
                if rp.constraint is not None and k in BANNING_KWARGS and k not in banning:
                    r[k] = PROCESSOR_KWARGS[k]
            if banning:
                raise ValueError(f"request {i}: a constraint together with {banning}: a processor that bans tokens can leave a constrained "
                                 "row with nothing allowed; only repetition_penalty composes with a constraint (a request overrides a "
                                 "call-wide keyword with the neutral value in its RequestParams)")
        if not plan.on_device:
            first = next(i for i, (*_, rp) in enumerate(reqs) if rp.constraint is not None)
            raise ValueError(f"request {first}: a constrained request needs the device pick, which needs bf16 logits on the GPU")
    return plan

def _many_one_by_one(model, plan: "_ManyPlan"):
    """generate_many with one slot or one request: generate() per request, in order."""
    opt, eos_list = plan.opt, plan.eos_list
    outs, sched, hits = [], SlotScheduler(len(plan.reqs), 1), []
    for (vx, lx, budget, rp), seed, own, stop_key, extra in zip(plan.reqs, plan.seeds, plan.resolved, plan.stop_keys, plan.extras):
        kw_r = dict(own, eos_token_id=eos_list, pad_token_id=opt.pad_id, max_new_tokens=budget)
        kw_r.update({k: v for k, v in extra.items() if v != 0.0})
        if stop_key:
            kw_r.update(stop_sequences=stop_key)
        if rp.do_sample:                        # the same stream: key seed, counter (token index, row 0, offset 0)
            kw_r.update(do_sample=True, temperature=float(rp.temperature), top_k=int(rp.top_k), top_p=float(rp.top_p),
                        generator=ops.DeviceGenerator(seed))
        if rp.logprobs:
            kw_r.update(output_logprobs=True, top_logprobs=int(rp.top_logprobs))
        if rp.constraint is not None:
            kw_r.update(constraint=rp.constraint)
        out = model._generate_one(vx, lx, **kw_r)
        row = out.sequences if rp.logprobs else out
        eos_t = torch.tensor(eos_list, dtype=torch.long, device=row.device) if eos_list else None
        tok = model._cut_behind_eos(row, eos_t, stop_key).clone()
        hits.append(int(model.last_stop_hits[0]) if stop_key else -1)
        n = tok.numel()
        if rp.logprobs:
            cut = lambda x: None if x is None else x[:n].clone()
            outs.append(AkiRequestOutput(tokens=tok, logprobs=cut(out.logprobs), top_token_ids=cut(out.top_token_ids),
                                         top_logprobs=cut(out.top_logprobs)))
        else:
            outs.append(plan.result(tok, rp))
    model.last_many_stats = dict(sched.stats(), per_request_generate=True)
    model.last_stop_hits = hits if plan.any_stops else None
    return outs

def _many_on_slots(model, plan: "_ManyPlan"):
    """generate_many's loop over slots: the slot cache and the per-row buffers allocated once, ONE PickStage over them (what the
    captured step, the eager step and - on one-row views - the admit all run), and the scheduler's four callbacks."""
    opt, reqs, lm, dev, on_device = plan.opt, plan.reqs, model.lang_model, plan.dev, plan.on_device
    eos_list, width = plan.eos_list, plan.width
    slots = min(plan.slots, len(reqs))
    flat = torch.cat([r[1][0] for r in reqs]).tolist()       # one copy for all prompts, ahead of any launch
    ends = list(itertools.accumulate(r[1].shape[1] for r in reqs))
    ids_host = [flat[e - r[1].shape[1]:e] for e, r in zip(ends, reqs)]
    capacity = slot_capacity(ids_host, [r[2] for r in reqs], model.media_token_id, model.num_tokens_per_vis)
    rot = lm.model.rotary_emb
    if rot.short is not None and capacity > rot.orig_max:
        raise NotImplementedError(f"generate_many on a LongRoPE model with a slot capacity of {capacity} rows above "
                                  f"original_max_position_embeddings = {rot.orig_max}: HF picks the factor set per batch, not per row")
    cfg = lm.config
    H = cfg.num_attention_heads
    Dh = getattr(cfg, "head_dim", None) or cfg.hidden_size // H
    cache = AkiKVCache(len(lm.model.layers), slots, H, Dh, capacity, plan.dtype, dev, lm.kv_cache_dtype)    # valid_bits None: a lone prompt has no padding
    max_budget = max(r[2] for r in reqs)
    tokens = torch.full((slots, max_budget), opt.pad_id, dtype=torch.long, device=dev)
    done = torch.ones(slots, dtype=torch.uint8, device=dev)
    done_at = torch.zeros(slots, dtype=torch.int32, device=dev)
    start_len = torch.zeros(slots, dtype=torch.int32, device=dev)
    limit = torch.ones(slots, dtype=torch.int32, device=dev)
    eos_t = torch.tensor(eos_list, dtype=torch.long, device=dev) if eos_list else None
    pick = dict(pad_token_id=opt.pad_id, eos_ids=eos_t, done=done, tokens=tokens, start_len=start_len, done_at=done_at)
    # the processed pick keeps a score scratch per batch size, whose address the captured step holds: the admit's one-row pick gets its own.
    # Requests with different settings: the pool of distinct sets (uploaded once) and one set index per slot, allocated ahead of the
    # capture and rewritten in place at admit (ops.ProcessorSets) - it stands in the place of the one LogitsProcessors.
    # A call in which a request carries min_p or a frequency / presence penalty takes the per-row form too (those values travel beside the
    # sets, one float per slot), whether or not its processor settings differ.
    by_sets = plan.mixed or plan.penalized
    processors = lambda: None if by_sets else _logits_processors(width, dev, plan.pk, eos_list, slot_constraints=plan.constrained)
    proc, proc1 = processors(), processors()
    psets = ops.ProcessorSets(width, dev, eos_list, plan.set_keys, slots) if by_sets else None
    if proc is not None:
        pick["processors"] = proc
    if psets is not None:
        pick["processor_sets"] = psets
    owner = proc if proc is not None else psets
    if on_device and owner is not None:
        owner.scores(slots, dev)                    # allocated ahead of the capture
    # a call with a constrained request: the pool of tables (uploaded once), and per slot the place of its request's table and its state
    # history, allocated ahead of the capture and rewritten in place at admit.  An unconstrained request is a state -1 row.
    slot_con = None
    if plan.constrained:
        slot_con = pick["slot_constraints"] = ops.SlotConstraints(plan.pool.bind(dev), slots, max_budget)
    # a call with stops: the pool of distinct stop sets (uploaded once), and per slot the place of its request's set and its hit,
    # allocated ahead of the capture and rewritten in place at admit.  The check rides in the tick's launch (ops.slot_tick(stops=...)).
    stop_sets = ops.StopSets(dev, plan.stop_keys, slots) if plan.any_stops else None
    # a call with a sampled request: every row's sampler parameters and Philox key live in device arrays the captured pick reads
    # (ops.sample_pick_rows).  A parked row and a greedy request are top_k = 1 rows, the greedy pick's token.
    rows = None
    if plan.sampled:
        rows = dict(temperature=torch.ones(slots, dtype=torch.float32, device=dev), top_k=torch.ones(slots, dtype=torch.int32, device=dev),
                    top_p=torch.ones(slots, dtype=torch.float32, device=dev), seed=torch.zeros(slots, dtype=torch.int64, device=dev))
    # min_p and the two penalties: per-slot f32 arrays beside the sampler's four, allocated only when some request uses one, written in
    # place at admit ahead of the pick of token 0, read by the one captured step.  (min_p belongs to the sampler: without a sampled
    # request nothing uses it.)
    extra = {k: torch.zeros(slots, dtype=torch.float32, device=dev) for k in ("frequency_penalty", "presence_penalty", "min_p") if plan.uses(k)}
    for k, x in extra.items():
        (rows if k == "min_p" else pick)[k] = x
    # log-probabilities: one ops.token_logprob behind each pick, per slot; a request's columns are [0, its tokens)
    lpb = _LogprobBuffers(slots, max_budget, plan.top, dev) if plan.want_lp else None
    stage = PickStage(pick, rows=rows, processors_row=proc1, logprob=None if lpb is None else lpb.args(), stops=stop_sets, limit=limit,
                      torch_pick=not on_device)
    stepper = None if not opt.use_graph else DecodeGraph(lm, cache, greedy=stage) if on_device else DecodeGraph(lm, cache)
    ids = stepper.ids if stepper is not None else torch.zeros(slots, dtype=torch.long, device=dev)
    sched = SlotScheduler(len(reqs), slots, period=8)
    results, hits, seen = {}, {}, {}

    def admit(req, slot):
        vx, lx, budget, rp = reqs[req]
        src, logits = model._prefill_request(vx, lx)
        ops.kv_slot_admit(src, cache, slot)
        cache.host_len = max(cache.host_len, src.host_len)
        cache.cache_len[slot:slot + 1].copy_(src.cache_len)
        start_len[slot:slot + 1].copy_(src.cache_len)
        done[slot] = 0
        done_at[slot] = -1
        limit[slot] = budget
        tokens[slot] = opt.pad_id
        if rows is not None:                        # the slot's sampler parameters, in place: tensor fills, nothing copied from the host
            seed = plan.seeds[req]
            rows["temperature"][slot] = float(rp.temperature) if rp.do_sample else 1.0
            rows["top_k"][slot] = int(rp.top_k) if rp.do_sample else 1
            rows["top_p"][slot] = float(rp.top_p) if rp.do_sample else 1.0
            rows["seed"][slot] = 0 if seed is None else (seed - (1 << 64) if seed >= 1 << 63 else seed)     # the key's bits as int64
        for k, x in extra.items():                  # the slot's min_p and penalties, in place
            x[slot] = plan.extras[req][k]
        if slot_con is not None:                    # the slot's automaton: where its table begins, its start state in column 0
            slot_con.admit(slot, plan.pool.base[req], plan.pool.n_states[req], plan.pool.start[req])
        if psets is not None:                       # the slot's processor set, ahead of the pick of token 0
            psets.admit(slot, plan.set_keys[req])
        if stop_sets is not None:                   # the slot's stop set, its hit back to -1
            stop_sets.admit(slot, plan.stop_keys[req])
        # token 0, from the prefill: the stage at B = 1 on row views.  The stops are checked behind the pick and AHEAD of the tick: a
        # one-token stop ends a request here
        stage.row(slot).run(logits.contiguous(), ids[slot:slot + 1], cache.cache_len[slot:slot + 1], advance=False, fuse_stops=False)
        return budget == 1

    def step(n):
        for _ in range(n):
            if stepper is not None and on_device:
                stepper.step_greedy()
                continue
            if stepper is not None:
                lg = stepper.step(ids)
            elif on_device:                         # the pick advances cache_len; the torch pick leaves that to the decode step
                lg = lm.decode_step(input_ids=ids, past_key_values=cache, advance=False)
            else:
                lg = lm.decode_step(input_ids=ids, past_key_values=cache)
            stage.run(lg, ids, cache.cache_len, advance=True)

    def look():
        state = [done.to(torch.int32), done_at, cache.cache_len] + ([] if stop_sets is None else [stop_sets.stop_hit])
        state = torch.stack(state).tolist()         # the one synchronisation
        d, at, ln = state[:3]
        seen["hit"] = state[3] if stop_sets is not None else None
        # host_len bounds the row the next step appends at.  A parked row stays on its one dead cache row (ops.slot_tick), so under the
        # captured step, whose grid is sized by the capacity, only the live rows count; eager steps size their grid by host_len and
        # need every row's keys inside it.
        live = [n for n, dd in zip(ln, d) if not dd]
        cache.host_len = max(live, default=0) if stepper is not None else max(ln)
        return d, at

    def retire(req, slot, n):
        rp = reqs[req][3]
        hits[req] = -1 if stop_sets is None else int(seen["hit"][slot])
        tok = tokens[slot, :n].clone()
        if rp.logprobs:                             # the columns behind n may hold what the slot's previous request left: never returned
            results[req] = plan.result(tok, rp, lpb.lp[slot, :n].clone(), None if lpb.top_ids is None else lpb.top_ids[slot, :n],
                                       None if lpb.top_lp is None else lpb.top_lp[slot, :n])
        else:
            results[req] = plan.result(tok, rp)

    sched.run(admit, step, look, retire, room=lambda: capacity - cache.host_len)
    model.last_many_stats = sched.stats()
    model.last_stop_hits = sched.in_request_order(hits) if stop_sets is not None else None
    model._post_forward_hook()
    return sched.in_request_order(results)


class AkiMethods:
    """Everything the train-time class below and its HF-Hub twin (modeling_aki.AKI) share: the two differ in their constructors only, so
    each is this class in front of VLMWithLanguageStream plus an __init__."""

    last_beam_scores = None     # after a device beam search (_beam_search_device): the returned rows' scores, HF's sequences_scores

    def set_trainable(self):
        """Unfreeze everything except the vision_encoder (src/aki.py:52-57)."""
        self.requires_grad_(True)
        self.vision_encoder.requires_grad_(False)

    def _should_apply_weight_decay(self, parameter_name):
        return True

    def default_eos_token_ids(self):
        """What `lang_model.generate` would stop on by default: generation_config.eos_token_id (Phi-3.5-mini-instruct ships
        [32007, 32001, 32000]) when the checkpoint carried one, else config.eos_token_id."""
        for holder in (getattr(self.lang_model, "generation_config", None), getattr(self.lang_model, "config", None)):
            eos = getattr(holder, "eos_token_id", None) if holder is not None else None
            if eos is not None:
                return [int(eos)] if isinstance(eos, int) else [int(e) for e in eos]
        return []

    def forward(self, vision_x: Optional[torch.Tensor], lang_x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None, image_size: Optional[Tuple] = None,
                past_key_values: Optional[List[Union[torch.Tensor, Tuple[torch.Tensor]]]] = None,
                past_media_locations: Optional[torch.Tensor] = None, past_vision_tokens: Optional[torch.Tensor] = None,
                use_cache: Optional[bool] = False, **kwargs):
        """vision_x (B, T_img, F=1, C, H, W); lang_x (B, T_txt) with <image> placeholders -> CausalLMOutputWithPast
        whose logits cover the EXPANDED stream length L (src/aki.py:65-134)."""
        assert not (past_vision_tokens is None) ^ (past_media_locations is None), \
            "past_vision_tokens and past_media_locations must both be None or both be not None"
        if vision_x is not None:
            plan = self._start_splice_plan(lang_x) if past_key_values is None else None   # ahead of the vision side's launches
            vision_tokens = self.vision_tokenizer(self._encode_vision_x(vision_x=vision_x))
        else:
            vision_tokens, plan = None, None
        new_inputs = self._prepare_inputs_for_forward(
            vision_tokens=vision_tokens, lang_x=lang_x, attention_mask=attention_mask, vision_attention_mask=None,
            labels=labels, past_key_values=past_key_values, past_media_locations=past_media_locations,
            padding_side="right", past_vision_tokens=past_vision_tokens, splice_plan=plan)
        output = self.lang_model(**new_inputs, use_cache=use_cache, past_key_values=past_key_values, **kwargs)
        self._post_forward_hook()
        return output

    def _beam_search(self, cache, logits, K: int, max_new_tokens: int, eos_ids, pad_id: int, length_penalty: float, early_stopping,
                     proc=None):
        """Beam search over the decode path (the algorithm of HF `GenerationMixin` beam search with a `BeamSearchScorer`:
        2K candidates per step, hypotheses normalised by generated_length ** length_penalty, one sequence returned per sample).
        The prompt's cache rows are expanded to K beams and re-ordered in place every step (AkiKVCache.select_rows)."""
        dev = logits.device
        B = logits.shape[0]
        if max_new_tokens <= 0:                        # nothing to generate: the greedy path returns an empty tensor too
            return torch.zeros((B, 0), dtype=torch.long, device=dev)
        cache.select_rows(torch.arange(B, device=dev).repeat_interleave(K))
        logp = torch.log_softmax(logits.float(), dim=-1).repeat_interleave(K, dim=0)             # [B*K, V]
        V = logp.shape[-1]
        scores = torch.zeros((B, K), dtype=torch.float32, device=dev)
        scores[:, 1:] = -1e9                                                                      # all beams start identical: keep one
        seqs = torch.zeros((B * K, 0), dtype=torch.long, device=dev)
        hyps = [[] for _ in range(B)]                                                             # per sample: (score, tokens)
        done = [False] * B
        eos_set = set(int(e) for e in eos_ids)

        def worst(b):
            return min(h[0] for h in hyps[b]) if len(hyps[b]) >= K else -float("inf")

        def add(b, score_sum, toks, gen_len):
            sc = score_sum / (max(gen_len, 1) ** length_penalty)
            if len(hyps[b]) < K or sc > worst(b):
                hyps[b].append((sc, toks))
                if len(hyps[b]) > K:
                    hyps[b].remove(min(hyps[b], key=lambda h: h[0]))

        for t in range(max_new_tokens):
            if proc is not None:                       # HF: the processors see each beam's log-softmax scores and its own tokens
                proc.apply(logp, out=logp, tokens=seqs, step=seqs.shape[1])
            cand = (logp.view(B, K, V) + scores[:, :, None]).view(B, K * V)
            top_s, top_i = cand.topk(2 * K, dim=-1)
            top_s_h, top_i_h = top_s.tolist(), top_i.tolist()
            nxt_tok = torch.full((B, K), pad_id, dtype=torch.long)
            nxt_beam = torch.zeros((B, K), dtype=torch.long)
            nxt_score = torch.full((B, K), -1e9, dtype=torch.float32)
            seqs_h = seqs.tolist() if eos_set else None
            for b in range(B):
                if done[b]:
                    nxt_beam[b] = torch.arange(K)
                    continue
                n = 0
                for rank, (sc, idx) in enumerate(zip(top_s_h[b], top_i_h[b])):
                    beam, tok = divmod(idx, V)
                    if tok in eos_set:
                        if rank < K:                                                              # HF: EOS beyond the K best is ignored
                            add(b, sc, seqs_h[b * K + beam] + [tok], t + 1)
                        continue
                    nxt_tok[b, n], nxt_beam[b, n], nxt_score[b, n] = tok, beam, sc
                    n += 1
                    if n == K:
                        break
                if len(hyps[b]) >= K:
                    best_running = float(nxt_score[b].max()) / ((t + 1) ** length_penalty)
                    if early_stopping is True or (early_stopping is False and worst(b) >= best_running):
                        done[b] = True
            if all(done) or t + 1 == max_new_tokens:
                # close the books: running beams become hypotheses (with the token chosen at this step)
                for b in range(B):
                    if done[b]:
                        continue
                    for n in range(K):
                        if float(nxt_score[b, n]) > -1e8:
                            base = seqs[b * K + int(nxt_beam[b, n])].tolist()
                            add(b, float(nxt_score[b, n]), base + [int(nxt_tok[b, n])], t + 1)
                break
            gather = (torch.arange(B)[:, None] * K + nxt_beam).view(-1).to(dev)
            seqs = torch.cat([seqs.index_select(0, gather), nxt_tok.view(-1, 1).to(dev)], dim=1)
            scores = nxt_score.to(dev)
            cache.select_rows(gather)
            step_logits = self.lang_model.decode_step(input_ids=nxt_tok.view(-1).to(dev), past_key_values=cache)
            logp = torch.log_softmax(step_logits.float(), dim=-1)
        return _pad_rows([torch.tensor(max(h, key=lambda x: x[0])[1], dtype=torch.long) for h in hyps], pad_id, dev)

    def _device_beam_search_ok(self, cache, logits, K: int, eos_ids) -> bool:
        """The device path (ops.beam_step / ops.kv_beam_reorder) is opt-in (`lang_model.device_beam_search = True`) and serves bf16 / f32
        logits on the GPU over an ungrouped cache whose K and V are contiguous tensors in the model's dtype; anything else keeps the
        host loop."""
        if not getattr(self.lang_model, "device_beam_search", False):
            return False
        if not logits.is_cuda or logits.dtype not in (torch.bfloat16, torch.float32):
            return False
        if K > ops.BEAM_MAX_K or len(eos_ids) > ops.BEAM_MAX_EOS or logits.shape[-1] < 2:
            return False
        if getattr(cache, "kv_dtype", None) != "bf16" or getattr(cache, "group", 1) != 1:
            return False
        return all(t_.is_cuda and t_.is_contiguous() and t_.dtype in (torch.bfloat16, torch.float32) for t_ in list(cache.k) + list(cache.v))

    def _beam_search_device(self, cache, logits, K: int, max_new_tokens: int, eos_ids, pad_id: int, length_penalty: float, early_stopping,
                            proc=None, use_graph: bool = False):
        """_beam_search with the per-token work on the device: ops.beam_logprob (f32 log-softmax), the processors, ops.beam_step (the
        2K candidates, ranked - exactly equal scores by the lower beam * V + token - and all of the BeamSearchScorer bookkeeping), and
        ops.kv_beam_reorder, which moves only the cache rows written since the prefill, in place: the cache tensors keep their
        addresses, so the decode step at B*K rows is replayed from a DecodeGraph.  The host looks at the done flags every 8th token."""
        dev = logits.device
        B = logits.shape[0]
        self.last_beam_scores = []
        if max_new_tokens <= 0:
            return torch.zeros((B, 0), dtype=torch.long, device=dev)
        if cache.host_len + max_new_tokens - 1 > cache.capacity:                   # before any launch
            raise ops.AkiError(f"KV cache is full: {cache.host_len} of {cache.capacity} rows used, beam search needs {max_new_tokens - 1} more; "
                               "size it with lang_model(..., use_cache=True, cache_capacity=...)")
        lm = self.lang_model
        cache.select_rows(torch.arange(B, device=dev).repeat_interleave(K))        # the one copy of the prompt rows: B -> B*K
        table = ops.KVBeamTable(list(cache.k) + list(cache.v))
        start_len, host_len0 = cache.cache_len.clone(), cache.host_len
        pos_lo = int(start_len.min())                  # once per call: a ragged batch's short prompts write below the longest prompt's end
        st = ops.BeamState(B, K, max_new_tokens, dev, eos_ids, pad_id, length_penalty, early_stopping)
        logp = torch.empty((B * K, logits.shape[-1]), dtype=torch.float32, device=dev)

        def select(step_logits, t):
            ops.beam_logprob(step_logits, out=logp)
            if proc is not None:                       # HF: the processors see each beam's log-softmax scores and its own tokens
                proc.apply(logp, out=logp, tokens=st.seqs, step=t)
            ops.beam_step(logp, st, t, last=t + 1 == max_new_tokens)

        select(logits.repeat_interleave(K, dim=0).contiguous(), 0)
        stepper = DecodeGraph(lm, cache) if use_graph else None
        for t in range(1, max_new_tokens):
            if t % 8 == 0 and bool(st.done.all()):     # frozen samples make the late look harmless
                break
            if cache.host_len > host_len0:
                ops.kv_beam_reorder(table, st.parent, start_len, cache.cache_len, K, pos_lo, cache.host_len)
            if stepper is not None:
                step_logits = stepper.step(st.next_ids)
            else:
                step_logits = lm.decode_step(input_ids=st.next_ids, past_key_values=cache)
            select(step_logits, t)
        count = st.hyp_count.tolist()
        score, length, toks = st.hyp_score.tolist(), st.hyp_len.tolist(), st.hyp_tokens.cpu()
        best = []                                      # last_beam_scores: HF's sequences_scores of the returned rows (f32, length-normalised)
        for b in range(B):                             # the best hypothesis; among equal scores the lowest slot
            i = max(range(count[b]), key=lambda j: (score[b][j], -j))
            best.append(toks[b, i, :length[b][i]])
            self.last_beam_scores.append(score[b][i])
        return _pad_rows(best, pad_id, dev)

    def _continue_from_cache(self, vision_x, lang_x, attention_mask, cache, max_new_tokens):
        """The prefill of generate(past_key_values=cache) - the reference's continuation call (src/aki.py:193-200): the new ids `lang_x`
        [B, T] are appended to the cache (Phi3ForCausalLM._continue: one chunked pass with lang_model.chunked_continue, T decode steps
        without); then the same greedy / sampling loops run as behind a prefill.  Returns (cache, each sample's logits row n_new[b] - 1,
        (cache_len clone, host_len) behind the new ids - what _trim_cache_to_returned counts from).  attention_mask, if given, spans the
        cached tokens and the new ids (width past length + T, else ValueError); its last T columns are ones followed by zeros per row (a
        right-padded chunk, else ValueError), which gives n_new; ragged rows need `lang_model.chunked_continue = True`."""
        if vision_x is not None:
            raise NotImplementedError("new images on top of an existing KV cache: the reference cannot do it either "
                                      "(its mask for the new chunk would not cover the cached columns); start a new prefill")
        if not isinstance(cache, AkiKVCache):
            raise ops.AkiError("past_key_values must be the AkiKVCache returned by a use_cache=True forward of this model")
        if lang_x is None or lang_x.dim() != 2 or lang_x.shape[1] < 1:
            raise ValueError("generate(past_key_values=...) takes the new token ids as lang_x [B, T], T >= 1")
        B, T_new = lang_x.shape
        if cache.cache_len.shape[0] != B:
            raise ValueError(f"the KV cache holds {cache.cache_len.shape[0]} rows, lang_x brings {B}")
        n_new = None
        if attention_mask is not None:
            past_len = cache.get_seq_length()
            if attention_mask.dim() != 2 or attention_mask.shape[0] != B or attention_mask.shape[1] != past_len + T_new:
                raise ValueError(f"attention_mask must be [B, past length + new ids] = [{B}, {past_len} + {T_new}] (the entire past, image "
                                 f"tokens included, and the current input ids); got {tuple(attention_mask.shape)}")
            tail = attention_mask[:, past_len:].ne(0)
            counts = tail.sum(1)
            prefix = torch.arange(T_new, device=tail.device)[None, :] < counts[:, None]
            if not bool((tail == prefix).all()) or int(counts.min()) < 1:
                raise ValueError("the mask over the new ids must be ones followed by zeros in every row (a right-padded chunk), "
                                 "with at least one real token per sample")
            if int(counts.min()) < T_new:
                n_new = counts.to(torch.int32)
        if cache.host_len + T_new + max_new_tokens - 1 > cache.capacity:           # before any launch
            raise ops.AkiError(f"KV cache is full: {cache.host_len} of {cache.capacity} rows used, the continuation needs {T_new} + "
                               f"{max_new_tokens - 1} more; size it with lang_model(..., use_cache=True, cache_capacity=...)")
        self._prepare_inputs_for_forward(vision_tokens=None, lang_x=lang_x, attention_mask=attention_mask, past_key_values=cache)
        logits = self.lang_model._continue(lang_x, None, cache, n_new=n_new).logits           # [B, T, V']
        last = logits[:, -1] if n_new is None else logits[torch.arange(B, device=logits.device), n_new.long() - 1]
        return cache, last, (cache.cache_len.clone(), cache.host_len)           # the caller's cache: the state behind the new ids

    @staticmethod
    def _trim_cache_to_returned(cache, start_len, host_len0, out, eos_t, stops=()):
        """The end of generate(past_key_values=...): every row's cache ends right before its last returned token.  start_len / host_len0:
        the cache's lengths behind the new ids; out [B, steps]: the returned tokens; a row's last token is its first finish (its first EOS
        or the end of its first stop sequence of `stops`), or column steps - 1.
        The decode loops themselves run past that point: the graph / device loop looks at the finished flags only every 8th token,
        and until then ops.greedy_pick / ops.sample_pick feed a finished row pad tokens and advance its cache_len like any other (the host
        loop does the same to the finished rows of a batch), so pad-token rows land behind the EOS.  They are cut off here by rewinding
        cache_len, at B = 1 and per row in a batch: the rows behind are dead and the next append overwrites them."""
        steps = out.shape[1]
        kept = torch.full_like(start_len, steps - 1)
        if eos_t is not None or stops:
            finished, first, _ = _first_end(out, eos_t, stops)
            kept = torch.where(finished, first.to(kept.dtype), kept)
        cache.cache_len.copy_(start_len + kept)
        cache.host_len = host_len0 + steps - 1

    def _prefill_prompt(self, vision_x, lang_x, attention_mask, max_new_tokens):
        """The prompt stage of a generate() without a cache: splice plan, vision side, MMA prefill into a KV cache with room for the new
        tokens.  Returns (cache, logits [B, V'] of each sample's last real token, None) - the triple of _continue_from_cache, whose third
        item is None because no caller's cache was appended to."""
        plan = self._start_splice_plan(lang_x)
        vision_tokens = self.vision_tokenizer(self._encode_vision_x(vision_x=vision_x))
        new_inputs = self._prepare_inputs_for_forward(vision_tokens=vision_tokens, lang_x=lang_x, attention_mask=attention_mask,
                                                      padding_side="right", splice_plan=plan)
        L = new_inputs["inputs_embeds"].shape[1]
        out = self.lang_model(inputs_embeds=new_inputs["inputs_embeds"], attention_mask=new_inputs["attention_mask"], use_cache=True,
                              cache_capacity=L + max_new_tokens, last_token_logits=True)
        return out.past_key_values, out.logits[:, 0], None

    def _expand_rows(self, cache, logits, n_ret: int, max_new_tokens: int):
        """num_return_sequences = N continuations per sample behind one prefill: row b * N + j continues sample b (HF order), so the device
        sampler's row index is b * N + j.  Returns the logits at B * N rows: token 0 of every row is drawn from its sample's prefill logits.
        The prompt's K/V rows are replicated N times (select_rows) unless `lang_model.share_prompt_kv = True`, with which the N rows of a
        sample read ONE copy of them (AkiKVCache.share_prefix + ops.decode_attn_group) where a grouped cache is possible: a bf16 model and
        cache, head_dim 96, more than one new token - anything else stays replicated."""
        B = logits.shape[0]
        logits = logits.repeat_interleave(n_ret, dim=0)
        if getattr(self.lang_model, "share_prompt_kv", False) and max_new_tokens > 1 and AkiKVCache.can_share_prefix(cache):
            cache.share_prefix(n_ret)
        else:
            cache.select_rows(torch.arange(B, device=logits.device).repeat_interleave(n_ret))
        return logits

    # The one-launch decode chain (one sequence, decode_chain.hip) bounds every dependency wait; a wait that gives up leaves garbage in that
    # step's output and a sticky error word.  Both decode loops below read the word wherever they synchronise anyway (every 8th token) and once
    # at the end; on an error the tokens after the last verified point are decoded again on the five-launch-per-layer path: nothing unverified
    # is ever returned (lm.decode_verified switches the chain off for this cache and warns).

    def _decode_on_device(self, opt: GenerateOptions, cache, logits, proc, eos_t):
        """The pick loop on the device: greedy, or sampling on the device (ops.sample_pick in the pick's place: the same loop, the same three
        launches per token; draws that depend on (seed, call, token index, row) and not on the batch).  The pick (argmax, pad for finished
        rows, append, eos check, cache_len advance, the next step's embedding row) is one launch behind the decode step (inside the replayed
        graph where there is one); the host looks at the finished flags every 8th token instead of syncing per token.  Until that look
        ops.greedy_pick / ops.sample_pick feed a finished row pad tokens and advance its cache_len like any other, so pad-token rows land
        behind the EOS in the cache (_trim_cache_to_returned cuts them off for a caller who keeps the cache).
        logits [B, V'] bf16 on the GPU: the prompt stage's; proc: the active ops.LogitsProcessors or None; eos_t: the eos ids as an int64
        tensor or None.  Returns (the new tokens [B, <= max_new_tokens], cut behind the last row's EOS where every row hit one; the
        _LogprobBuffers of opt.output_logprobs, uncut, else None).
        opt.stops: one ops.stop_check behind the pick (and the log-probability launch) of token 0, of every eager step and inside the
        graph; a row it ends is a done row like one the pick's EOS check ended, so the host looks every 8th token whenever there are
        stops, also without an EOS id.  last_stop_hits is the StopSets' stop_hit afterwards."""
        lm, dev, B, max_new_tokens, pad_id = self.lang_model, logits.device, logits.shape[0], opt.max_new_tokens, opt.pad_id
        tokens = torch.full((B, max_new_tokens), pad_id, dtype=torch.long, device=dev)
        chained = lambda: getattr(cache, "chain", None) is not None
        stepper = None
        done8 = torch.zeros(B, dtype=torch.uint8, device=dev)
        done_at = torch.full((B,), -1, dtype=torch.int32, device=dev)
        start_len, host_len0 = cache.cache_len.clone(), cache.host_len
        pick = dict(pad_token_id=pad_id, eos_ids=eos_t, done=done8, tokens=tokens, start_len=start_len, done_at=done_at)
        if proc is not None:                    # the processors read tokens[:, :t] and t from cache_len: replays and rewinds stay right
            pick["processors"] = proc
        ids = torch.zeros(B, dtype=torch.long, device=dev)
        emb_mod = lm.get_input_embeddings()
        embed = _embedding_tables(emb_mod, logits)
        nxt_emb = None if embed is None else torch.empty((B, emb_mod.weight.shape[1]), dtype=torch.bfloat16, device=dev)
        # output_logprobs: one ops.token_logprob behind each pick (in-loop form: it reads the index the pick just wrote from cache_len)
        lpb = _LogprobBuffers(B, max_new_tokens, opt.top_logprobs, dev) if opt.output_logprobs else None
        stops = None
        if opt.stops and max_new_tokens >= 1:           # one set for every row; row_set / stop_hit allocated ahead of any capture
            stops = ops.StopSets(dev, [opt.stops], B)
            stops.row_set.fill_(stops.index[opt.stops])
            self.last_stop_hits = stops.stop_hit
        stage = PickStage(pick, embed=embed, next_embeds=nxt_emb, sampler=_device_sampler_args(opt),
                          logprob=None if lpb is None or max_new_tokens < 1 else lpb.args(), stops=stops)
        ends = eos_t is not None or stops is not None   # a row can finish ahead of its budget
        logits = logits.contiguous()
        stage.run(logits, ids, cache.cache_len, advance=False)      # token 0, from the prefill
        t, t_ok = 1, 1                                  # tokens[:, :t_ok] are verified (token 0 comes from the prefill, not from the chain)
        period = 8 if ends else 32                      # host synchronisations: the finished flags need them often, the chain's verification alone does not
        while True:
            ok = True
            while t < max_new_tokens:
                if t % period == 0 and (ends or chained()):
                    if chained() and not lm.decode_verified(cache):
                        ok = False
                        break
                    t_ok = t
                    if ends and bool(done8.all()):
                        break
                if stepper is not None:
                    stepper.step_greedy()
                else:
                    # One sequence on the one-launch decode chain is three launches per token (chain, head, pick + embedding):
                    # the host runs far ahead of them and a hipGraph would only add its capture (about 12 ms per call, 7 tokens' worth).
                    # Anything else - batches, the five-launch-per-layer path - is ~165 launches per token and is captured after its first
                    # eager step.
                    if nxt_emb is not None:
                        lg = lm.decode_step(inputs_embeds=nxt_emb, past_key_values=cache, advance=False)
                    else:
                        lg = lm.decode_step(input_ids=ids, past_key_values=cache, advance=False)
                    stage.run(lg, ids, cache.cache_len, advance=True)
                    if not chained():
                        stepper = DecodeGraph(lm, cache, greedy=stage)
                        stepper.ids.copy_(ids)
                t += 1
            if ok and chained() and not lm.decode_verified(cache):
                ok = False
            if ok:
                break
            # recovery: back to the last verified token, then on without the chain.  The finished flags are rebuilt from the verified tokens
            # (a batch can hold rows that finished before that point; one sequence would have ended the loop there)
            t = t_ok
            cache.cache_len.copy_(start_len + (t_ok - 1))
            cache.host_len = host_len0 + (t_ok - 1)
            tokens[:, t_ok:] = pad_id
            if lpb is not None:
                lpb.reset_from(t_ok)
            done8.zero_()
            done_at.fill_(-1)
            if ends:
                finished, first, hit = _first_end(tokens[:, :t_ok], eos_t, opt.stops)
                done8.copy_(finished.to(torch.uint8))
                done_at.copy_(torch.where(finished, first.to(torch.int32), torch.full_like(done_at, -1)))
                if stops is not None:
                    stops.stop_hit.copy_(hit)
            ids.copy_(tokens[:, t_ok - 1])
            if nxt_emb is not None:
                nxt_emb.copy_(emb_mod(ids))
        if ends and bool(done8.all()):
            return tokens[:, :int(done_at.max()) + 1], lpb
        return tokens[:, :t], lpb

    def _decode_on_host(self, opt: GenerateOptions, cache, logits, proc, eos_t):
        """The loop that picks on the host, one synchronisation per token where there is an EOS id: `sample_next` sampling (generator None or
        a torch.Generator), the device sampler outside a graph, and greedy where the device loop does not apply (f32, use_graph=False).  The
        decode step is replayed from a DecodeGraph with use_graph.  A finished row of a batch is stepped on with pad tokens until every row
        has finished.  Arguments and return value as _decode_on_device; the tokens [B, <= max_new_tokens] are cut where every row has finished.
        opt.stops: a row is also finished when stops.first_finish over tokens[:, :t] says so - the same synchronisation per token."""
        lm, B, max_new_tokens, pad_id = self.lang_model, logits.shape[0], opt.max_new_tokens, opt.pad_id
        do_sample, temperature, top_k, top_p, rng = opt.do_sample, opt.temperature, opt.top_k, opt.top_p, opt.rng
        tokens = torch.full((B, max_new_tokens), pad_id, dtype=torch.long, device=logits.device)
        done = torch.zeros(B, dtype=torch.bool, device=logits.device)
        chained = lambda: getattr(cache, "chain", None) is not None
        sampler = _device_sampler_args(opt)
        min_p = {"min_p": opt.min_p} if opt.min_p else {}       # sample_next's; without it the call is the one it always was
        stepper = DecodeGraph(lm, cache) if opt.use_graph else None
        lpb = _LogprobBuffers(B, max_new_tokens, opt.top_logprobs, logits.device) if opt.output_logprobs else None
        t, n_out = 0, max_new_tokens
        ck = None                                           # the state at the last verified point of a chained decode
        while True:
            ok = True
            while t < max_new_tokens:
                if t % 8 == 0 and (t == 0 or chained()):
                    if chained() and not lm.decode_verified(cache):
                        ok = False
                        break
                    ck = (t, logits.clone(), done.clone(), cache.cache_len.clone(), cache.host_len)
                if sampler is not None:             # the device sampler outside a graph: one launch, the draw of token t (no cache_len: n = step)
                    nxt = ops.sample_pick(logits.contiguous(), torch.empty(B, dtype=torch.long, device=logits.device), processors=proc,
                                          tokens=tokens, step=t, **sampler)
                else:
                    x = logits if proc is None else proc.apply(logits, tokens=tokens, step=t)
                    nxt = sample_next(x, temperature, top_k, top_p, rng, **min_p) if do_sample else x.float().argmax(dim=-1)
                nxt = torch.where(done, torch.full_like(nxt, pad_id), nxt)
                tokens[:, t] = nxt
                if proc is not None and sampler is None:        # a constraint's next state (ops.sample_pick stores it itself)
                    proc.advance_states(nxt, t, done)
                if lpb is not None:                 # the raw logits of this step, at the token returned; rows finished before it are skipped
                    ops.token_logprob(logits, ids=nxt, skip=done.to(torch.uint8), step=t, **lpb.args())
                t += 1
                if eos_t is not None or opt.stops:
                    if opt.stops:
                        done = done | _first_end(tokens[:, :t], eos_t, opt.stops)[0]
                    else:
                        done = done | (nxt[:, None] == eos_t[None, :]).any(-1)
                    if bool(done.all()):
                        n_out = t
                        break
                if t < max_new_tokens:
                    logits = stepper.step(nxt) if stepper is not None else lm.decode_step(input_ids=nxt, past_key_values=cache)
            if ok and chained() and not lm.decode_verified(cache):
                ok = False
            if ok:
                break
            t, logits, done, cl, cache.host_len = ck
            cache.cache_len.copy_(cl)
            tokens[:, t:] = pad_id
            if lpb is not None:
                lpb.reset_from(t)
            n_out, stepper = max_new_tokens, None           # a graph captured around the chain is gone with it
            if opt.use_graph:
                stepper = DecodeGraph(lm, cache)
        if opt.stops:
            self.last_stop_hits = _first_end(tokens[:, :n_out], eos_t, opt.stops)[2]
        return tokens[:, :n_out], lpb

    @torch.no_grad()
    def score(self, vision_x, lang_x, continuations, attention_mask=None, continuation_lengths=None, top_logprobs: int = 0,
              use_graph: Optional[bool] = None):
        """The teacher-forced log-likelihood of N given continuations per prompt behind ONE prefill - the counterpart of
        `num_return_sequences`, and what a multiple-choice eval ranks its answers by.  vision_x / lang_x / attention_mask: the prompt batch,
        as for generate; continuations int64 [B, N, T]; continuation_lengths [B, N] with values in 1..T (default: all T);
        top_logprobs = k <= ops.LOGPROB_MAX_TOP alternatives per position; use_graph: replay the decode steps from a hipGraph (default:
        from T = 8 on, generate's rule).  Returns an AkiScoreOutput: logprobs [B, N, T] with logprobs[b, n, t] = log p(continuations[b, n, t]
        | prompt b, continuations[b, n, :t]) under the raw model distribution (the f32 log-softmax of the step's logits, as
        generate(output_logprobs=True) reports it), zero behind each length; sum_logprobs [B, N]; lengths; the top-k pair.
        Column 0 is scored from the prefill's logits; step t = 1 .. T - 1 feeds continuations[..., t - 1] to one decode step over the
        B * N rows (_expand_rows: replicated prompt rows, or one shared copy under lang_model.share_prompt_kv) and its logits score
        continuations[..., t].  A row past its length is fed pad_token_id and writes zeros, the way the decode loops treat finished rows.
        Shapes and lengths are checked before any launch."""
        k = int(top_logprobs)
        if not 0 <= k <= ops.LOGPROB_MAX_TOP:
            raise ValueError(f"top_logprobs must be in 0..{ops.LOGPROB_MAX_TOP}")
        if not torch.is_tensor(continuations) or continuations.dtype != torch.long or continuations.dim() != 3:
            raise ValueError("score takes continuations as an int64 tensor [B, N, T]")
        B, N, T = continuations.shape
        if lang_x is None or lang_x.dim() != 2 or lang_x.shape[0] != B or N < 1 or T < 1:
            raise ValueError(f"score: continuations [B, N, T] with N, T >= 1 and B = the prompt batch are expected, got {tuple(continuations.shape)} "
                             f"for lang_x {None if lang_x is None else tuple(lang_x.shape)}")
        if continuation_lengths is None:
            lengths = torch.full((B, N), T, dtype=torch.long)
        else:
            lengths = torch.as_tensor(continuation_lengths)
            if tuple(lengths.shape) != (B, N) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError(f"continuation_lengths is an integer tensor [B, N] = [{B}, {N}]")
            lengths = lengths.long()
            if int(lengths.min()) < 1 or int(lengths.max()) > T:
                raise ValueError(f"continuation_lengths must lie in 1..T = 1..{T}")
        if vision_x is None:
            raise NotImplementedError("text-only generation is outside the AKI hot path")
        cache, logits, _ = self._prefill_prompt(vision_x, lang_x, attention_mask, T)
        if N > 1:
            logits = self._expand_rows(cache, logits, N, T)
        lm, dev, rows = self.lang_model, logits.device, B * N
        lengths = lengths.to(dev)
        live = torch.arange(T, device=dev)[:, None] < lengths.reshape(1, rows)                 # [T, rows]: step-major, a step's row is contiguous
        ids = continuations.to(dev).reshape(rows, T).t().contiguous()
        fed = torch.where(live, ids, torch.full_like(ids, self.pad_token_id))
        skip = (~live).to(torch.uint8)
        buf = _LogprobBuffers(rows, T, k, dev)
        ops.token_logprob(logits, ids=ids[0], skip=skip[0], step=0, **buf.args())

        def steps(graph: bool):
            stepper = DecodeGraph(lm, cache) if graph else None
            for t in range(1, T):
                lg = stepper.step(fed[t - 1]) if stepper is not None else lm.decode_step(input_ids=fed[t - 1], past_key_values=cache)
                ops.token_logprob(lg, ids=ids[t], skip=skip[t], step=t, **buf.args())

        if T > 1:
            len0, host_len0 = cache.cache_len.clone(), cache.host_len
            graph = T >= 8 if use_graph is None else bool(use_graph)
            steps(graph)
            if not lm.decode_verified(cache):      # a chained step (one row) failed its check: the same steps again on the per-layer path
                cache.cache_len.copy_(len0)
                cache.host_len = host_len0
                steps(graph)
        self._post_forward_hook()
        shape = lambda x: None if x is None else x.reshape(B, N, T, k)
        return AkiScoreOutput(logprobs=buf.lp.reshape(B, N, T), sum_logprobs=buf.lp.sum(1).reshape(B, N), lengths=lengths,
                              top_token_ids=shape(buf.top_ids), top_logprobs=shape(buf.top_lp))

    last_many_stats = None      # after generate_many: the SlotScheduler's counters (slots.SlotScheduler.stats) as a dict
    # after a generate() with stop_sequences: int32 device tensor [rows], rows = B * num_return_sequences - per row the index within the stop
    # set of the sequence that ended it, -1 for a row that ended otherwise; after generate_many with stops: a list of ints in request
    # order; after a call without stops: None
    last_stop_hits = None

    def _logits_width(self) -> int:
        return _logits_width(self.lang_model)

    def _prefill_request(self, vision_x, lang_x):
        """One request of generate_many, prefilled at batch 1 into a cache of exactly its length: (cache, logits [1, V']).  Without an image
        the ids go to the language model as they are (what forward does with vision_x=None)."""
        if vision_x is not None:
            cache, logits, _ = self._prefill_prompt(vision_x, lang_x, None, 0)
            return cache, logits
        out = self.lang_model(input_ids=lang_x, use_cache=True, cache_capacity=lang_x.shape[1], last_token_logits=True)
        return out.past_key_values, out.logits[:, 0]

    def _generate_one(self, vision_x, lang_x, **kwargs):
        """generate() for one request of generate_many, as a 1-D tensor - with output_logprobs an AkiGenerateOutput of the one row's fields.
        A request without an image is continued from a cache of its first T - 1 ids (generate itself prefills image prompts only)."""
        def row0(out):
            if not isinstance(out, AkiGenerateOutput):
                return out[0]
            first = lambda x: None if x is None else x[0]
            return AkiGenerateOutput(sequences=out.sequences[0], logprobs=first(out.logprobs), top_token_ids=first(out.top_token_ids),
                                     top_logprobs=first(out.top_logprobs))

        if vision_x is not None:
            return row0(self.generate(vision_x, lang_x, **kwargs))
        if lang_x.shape[1] < 2:
            raise ValueError("a request without an image needs at least 2 prompt ids")
        budget = int(kwargs.get("max_new_tokens", 20))
        cache = self.lang_model(input_ids=lang_x[:, :-1], use_cache=True, cache_capacity=lang_x.shape[1] + budget,
                                last_token_logits=True).past_key_values
        return row0(self.generate(None, lang_x[:, -1:], past_key_values=cache, **kwargs))

    @staticmethod
    def _cut_behind_eos(row: torch.Tensor, eos_t, stops=()):
        """A 1-D token row cut behind its first finish: its first EOS or the end of its first stop sequence (both included)."""
        if (eos_t is None and not stops) or row.numel() == 0:
            return row
        finished, first, _ = _first_end(row[None], eos_t, stops)
        return row[: int(first[0]) + 1] if bool(finished[0]) else row

    @torch.no_grad()
    def generate_many(self, requests, slots: int = 8, **kwargs):
        """In-flight batching: a queue of requests served over a fixed number of decode rows ("slots").  A static batch steps a finished row
        on with pad tokens until its longest row has finished; here a finished row is retired and refilled from the queue while the others
        stay mid-sequence, so answers of very different lengths keep the batch occupied.

        requests: a sequence of (vision_x, lang_x), (vision_x, lang_x, max_new_tokens) or (vision_x, lang_x, max_new_tokens or None,
        RequestParams); vision_x [1, T_img, 1, C, H, W] or None, lang_x int64 [1, T] without padding.  Returns a list of 1-D int64 device
        tensors in request order, each cut behind its first EOS (EOS included) or at its budget.  `last_many_stats` holds the scheduler's
        counters afterwards.
        Keywords: max_new_tokens (the default budget), eos_token_id, pad_token_id, use_graph, the logits processors of PROCESSOR_KWARGS
        (the default of every request: one ops.LogitsProcessors for all rows when no request overrides them - it reads each row's own history
        and index, and a refilled row starts with an empty one),
        params (the RequestParams of the requests that bring none) and generator (an aki_amd.DeviceGenerator or None).
        Sampling, log-probabilities and token constraints belong to the REQUEST (aki_amd.RequestParams), never to the call:
          * do_sample=True with temperature, top_k, top_p: the device sampler with that row's own values (ops.sample_pick_rows: the four
            per-slot arrays are written in place at admit and read by the captured step).  bf16 on the GPU only; on an f32 model a sampled
            request is a ValueError before any device work.  A greedy request in such a call is a top_k = 1 row: the greedy pick's token.
            A call in which nothing samples runs exactly the greedy launches.
          * the seed rule: a request's draws are Philox4x32-10(key = its seed, counter = (generated-token index, 0, 0, 0)) - they depend
            on the request's seed and nothing else, not on its slot, the schedule or its neighbours, and they are the draws of
            generate(..., do_sample=True, generator=DeviceGenerator(seed)) for that request alone (which is what slots == 1 runs).
            seed=None: slots.request_seed(S, offset, r), r the request's position in `requests`, with (S, offset) taken from
            `generator` - its offset is bumped ONCE per generate_many call, whether or not anything samples - or, with generator=None,
            S = 64 bits drawn on the host from torch's CPU default generator (torch.manual_seed reproduces a call; successive calls
            differ) and offset 0.  A torch.Generator as generator: ValueError.
          * logprobs=True with top_logprobs=k <= ops.LOGPROB_MAX_TOP: the raw-distribution values generate(output_logprobs=True) reports
            (before processors, temperature and filters), one ops.token_logprob behind each pick, launched only when a request asks.
            The call then returns a list of AkiRequestOutput(tokens, logprobs [n], top_token_ids [n, k], top_logprobs [n, k]), the
            three extra fields None for the requests that did not ask (and the top fields for k = 0).
          * constraint=an aki_amd.TokenConstraint with one start state: the request's tokens walk that automaton (an eos id only behind an
            accepting state).  The distinct constraints of a call (by identity) are checked against the call's eos ids and the logits'
            width and uploaded once as one pool of tables, states not renumbered (constraint.ConstraintPool: 32767 states per
            constraint, DEFAULT_MAX_TABLE_BYTES for the pool); each slot holds its request's place in the pool and its own state
            history (ops.SlotConstraints), rewritten in place at admit and read by the captured pick, which masks inside the launch.
            An unconstrained request in such a call is a row without a state: the plain token.  A call in which no request is
            constrained launches exactly what it launched before.  Composes with do_sample (the draw is made inside the allowed set)
            and logprobs (the raw distribution).  bf16 on the GPU only; another V, an eos id used as a transition or a reachable state
            that allows nothing: ValueError naming the request, before any device work.  The banning rule is per request: a request that,
            after resolution, carries a constraint AND a banning processor (BANNING_KWARGS) is a ValueError naming it and the keyword; a
            constrained request next to an unconstrained one with bans is legal, and a constrained request may override a call-wide
            banning keyword with the neutral value.  Only repetition_penalty composes with a constraint.
          * the logits processors of PROCESSOR_KWARGS as RequestParams fields, None by default: None takes the call's value (params=, else
            the call-wide keyword); any other value, the neutral 1.0 / 0 / () included, is the request's alone.  The distinct resolved
            settings of a call form a pool deduplicated by value and uploaded once (ops.ProcessorSets); each slot holds one int32 set
            index, filled at admit ahead of the pick of token 0 and read by the captured pick (aki_greedy_pick_rows /
            aki_sample_pick_rows_processed; an f32 model's torch pick takes aki_logits_process_rows' scores).  A call whose requests all
            resolve to ONE set launches exactly what it launched before.  Log-probabilities stay the raw distribution's.
          * stop_sequences (the rule and the limits: generate's docstring, aki_amd/stops.py), None by default: None takes the call's
            value - params=, else the call-wide `stop_sequences=` keyword, which is every request's default; () means this request has
            none.  The ids are checked against the logits' width; a bad value is a ValueError naming the request, before any device
            work.  The distinct resolved sets of a call form one pool, deduplicated by value and uploaded once (ops.StopSets); each slot
            holds the place of its request's set and its hit, filled at admit.  The admit checks the row behind the pick of token 0 and
            ahead of the tick (a one-token stop can end a request at its prefill); the captured step takes the tick that checks the
            stops in the same launch (ops.slot_tick(stops=...)), so a queue with stops costs no launch more than one without, and the
            hits ride in the look's one copy.  A request is cut behind its matched sequence.  `last_stop_hits` is a list of ints in
            request order afterwards (None after a call without stops).  A call in which no request resolves to a non-empty set
            launches exactly what it launched before.
          * min_p (a float in [0, 1], 0 = no filter; generate's docstring states the rule): request-owned like temperature, ignored for a
            greedy request as its top_p is; a call-wide `min_p=` keyword is a ValueError.  frequency_penalty / presence_penalty (finite
            floats in [-2, 2]), None by default: None takes the call's value - params=, else the call-wide keyword; an explicit 0.0 is
            the request's alone.  The three values are per-slot f32 device arrays beside the sampler's four, allocated only when some
            request of the call uses one, written in place at admit ahead of the pick of token 0 and read by the captured pick
            (aki_greedy_pick_rows_penalized / aki_sample_pick_rows_penalized; such a call takes the per-row processor form whether or
            not its processor settings differ).  The counts are taken from the slot's own generated tokens on every step, so a refilled
            slot starts from nothing.  A call in which no request uses them launches exactly what it launched before.
          Bad values (temperature <= 0, min_p outside [0, 1], a penalty outside [-2, 2], top_p outside (0, 1], top_k < 0, top_logprobs outside the limit or without logprobs, a seed outside
          [0, 2^64)): ValueError naming the request, before any device work.
        Refused with NotImplementedError (MANY_REFUSED): num_beams > 1, num_return_sequences > 1, past_key_values, and the
        CALL-WIDE do_sample / output_logprobs / constraint keywords (use RequestParams); a LongRoPE model whose slot capacity exceeds
        original_max_position_embeddings (HF picks the factor set per batch, not per row).  Any other keyword (temperature, top_k, top_p,
        top_logprobs among them): ValueError.  slots above ops.SLOT_MAX_ROWS: ValueError.
        The loop (aki_amd/slots.py holds its bookkeeping):
          * one AkiKVCache of `slots` rows and capacity max(expanded prompt length + budget), computed from the ids on the host; the per-row
            tokens / done / done_at / start_len / limit / ids buffers are allocated once - the captured step holds their addresses;
          * admit: a batch-1 prefill, ops.kv_slot_admit into the slot's rows, the slot's state (and sampler parameters) reset in place,
            token 0 picked from the prefill's logits on row views (advance=False; scored there too when log-probabilities are on), one
            ops.slot_tick - a budget of 1 or an EOS as token 0 retires the row at once;
          * decode: ONE DecodeGraph over the slot cache with the pick and ops.slot_tick inside, captured once per call; the host looks
            every 8th replay (its only synchronisation), retires finished slots and admits pending requests into them.  A slot with
            nothing pending stays done and parked (slot_tick keeps it on one dead cache row).
        f32 models (logits the pick kernel does not take) replay the plain step and pick with torch operations on the device, still without
        a synchronisation per token.  slots == 1 or a single request: generate() per request (the one-launch chain is the batch-1 path)."""
        plan = _plan_many(self, requests, slots, kwargs)
        if not plan.reqs:
            self.last_many_stats = SlotScheduler(0, plan.slots).stats()
            return []
        if plan.slots == 1 or len(plan.reqs) == 1:
            return _many_one_by_one(self, plan)
        return _many_on_slots(self, plan)

    @torch.no_grad()
    def generate(self, vision_x, lang_x, image_size=None, attention_mask=None, past_key_values=None,
                 past_media_locations=None, past_vision_tokens=None, **kwargs):
        """Generation (src/aki.py:136-209 + src/aki_generation.py:36-86; local_demo.py / eval.py call it with do_sample=False): MMA prefill
        into a KV cache, then one HIP decode step per token.

        Arguments: `vision_x` (B, T_img, F=1, C, H, W) and `lang_x` [B, T_txt] with <image> placeholders, `attention_mask` [B, T_txt], as
        for forward; the HF keyword arguments the reference forwards (`**kwargs`, src/aki.py:160-207): `max_new_tokens` (or `max_length`;
        20), `eos_token_id` (default: default_eos_token_ids(); [] switches stopping off), `pad_token_id`, `use_graph` (replay the decode step
        from a hipGraph; default: from 8 new tokens on) and the ones below.  Any other keyword raises ValueError (_parse_generate_kwargs).
        Modes:
          * greedy (default).
          * sampling: `do_sample=True` with `temperature`, `top_k`, `top_p` and an optional `generator`.  An `aki_amd.DeviceGenerator(seed)`
            there selects the device sampler (ops.sample_pick; bf16 on the GPU), None or a `torch.Generator` the `sample_next` path.
          * `num_return_sequences=N` with sampling: N continuations per sample, [B*N, <= max_new_tokens] in HF order (row b*N + j is
            continuation j of sample b) behind one prefill (_expand_rows).  ValueError without sampling, NotImplementedError with beams.
          * beam search: `num_beams=K`, `length_penalty`, `early_stopping`; one returned sequence per sample.  `lang_model.device_beam_search
            = True` runs the search on the device (_beam_search_device) where it can; the host loop (_beam_search) is used otherwise and by
            default: the device path's step time has not been measured yet.
          * logits processors, in every mode, on the device and in HF's order (ops.LogitsProcessors): `repetition_penalty`,
            `no_repeat_ngram_size`, `bad_words_ids`, `min_length` / `min_new_tokens` (eos ids banned until that many tokens are generated),
            `suppress_tokens`, `begin_suppress_tokens`.  As in HF `generate` with inputs_embeds only, they see the generated tokens, never
            the prompt; beam search applies them to each beam's log-softmax scores.
          * `frequency_penalty`, `presence_penalty` (the OpenAI definition in vLLM's order; finite floats in [-2, 2], 0 = neutral): stage
            1b of the processors, directly behind the repetition penalty and before every ban.  For every distinct GENERATED token (never
            the prompt's) with c occurrences: score - fl(frequency_penalty * c), then score - presence_penalty, each one rounded f32
            operation; the counts are recomputed from the row's tokens on every step.  They ban nothing, so they compose with a
            constraint.  In every mode but beam search (NotImplementedError).
          * `min_p` (HF MinPLogitsWarper; a float in [0, 1], 0 = no filter) with sampling: behind temperature, top-k and top-p, a kept
            token stays iff exp(y - max y) >= min_p, i.e. its probability is at least min_p times the largest.  The maximum always
            stays; top-p's mass is decided before it.  Both samplers (the device sampler inside its one launch, `sample_next` in torch).
            Without `do_sample` it is ignored, as `top_p` is (its range is still checked); with beams NotImplementedError.
          * `constraint=` an `aki_amd.TokenConstraint` (aki_amd/constraint.py), or a list of one per sample: constrained decoding.  The
            automaton's table lives on the device, the mask is the last stage of the logits processors and the pick stores each row's
            next state, so the launches per token and the host's look every 8th token stay as they are.  Every returned row is a walk of
            its automaton; an eos id can be emitted only in an accepting state (`TokenConstraint.from_choices(choices, V)` + `eos_token_id`
            gives "one of the choices, then EOS").  Greedy, sampling (both samplers), `num_return_sequences` (row b*N + j starts in
            sample b's start state), from a cache, with `output_logprobs` (still the RAW distribution) and with `repetition_penalty`.
            Refused before any device work: `num_beams > 1` (NotImplementedError); a processor that bans tokens
            (`no_repeat_ngram_size`, `bad_words_ids`, `min_length` / `min_new_tokens`, `suppress_tokens`, `begin_suppress_tokens`: the
            pair could leave a row with nothing allowed), a list whose length is not B, a constraint built for another V than the
            logits' width V', an eos id used as a transition, a reachable state that allows nothing (ValueError).  HF's
            `prefix_allowed_tokens_fn` callback stays refused: a Python call per row per step cannot ride the device loop.
            Greedy decoding inside a trie takes the locally best allowed token: it does NOT return the most likely choice as a whole;
            `score` ranks a closed set of answers by likelihood.
          * `past_key_values=cache` (the AkiKVCache of a use_cache=True forward or of an earlier turn; `vision_x` must be None) continues
            from the cache instead of a prefill: `lang_x` [B, T] holds the NEW ids only and `attention_mask`, if given, spans past + new ids
            (_continue_from_cache).  Greedy and sampling only: beam search and N > 1 from a cache raise NotImplementedError.
          * `output_logprobs=True` (with `top_logprobs=k`, k <= ops.LOGPROB_MAX_TOP = 8): the call returns an AkiGenerateOutput whose
            `sequences` are the tokens described below, with `logprobs` f32 [rows, steps] and, for k > 0, `top_token_ids` int64 /
            `top_logprobs` f32 [rows, steps, k], all on the device and cut with the tokens.  The log-probabilities come from the RAW model
            distribution - the f32 log-softmax of each step's logits before logits processors, temperature, top-k or top-p - read at the
            token that was returned: HF's compute_transition_scores(sequences, logits, normalize_logits=True).  One ops.token_logprob
            launch behind each pick (inside the replayed graph where there is one).  Positions behind a row's EOS hold 0.0, -1 and 0.0.
            Greedy, sampling, N continuations and from a cache; with num_beams > 1 NotImplementedError (beam search keeps
            last_beam_scores).  `top_logprobs` without `output_logprobs`, or above the limit: ValueError.  `score` is the counterpart
            for continuations the caller supplies.
          * `stop_sequences=[[id, ...], ...]`: one stop set for every row of the call - at most ops.STOP_MAX_SEQS = 64 token-id sequences
            of 1 to ops.STOP_MAX_LEN = 32 ids in [0, V') (ValueError otherwise, before any device work); None, [] and () mean none, and
            the call launches exactly what it launches without the keyword.  A live row finishes at the first generated-token index t
            at which a sequence s of the set matches: with n = len(s), n <= t + 1 and tokens[t - n + 1 .. t] == s.  Only generated tokens
            count, never the prompt.  The matched sequence STAYS in the returned tokens, as an EOS does and as HF's `stop_strings`
            does; what follows it is pad.  `last_stop_hits` (int32 device tensor [rows], rows = B * num_return_sequences; None after a
            call without stops) holds per row the index within the set of the LOWEST-numbered sequence that matched at that t, -1
            for a row that ended otherwise; a row its EOS ended at the same t keeps -1 (EOS wins a tie), a stop at the last token of the
            budget is a stop.  Stops change WHEN a row ends, never WHAT it picks: they apply behind the pick, so they ignore
            `min_length` / `min_new_tokens`, as HF's stopping criteria do.  Matched on the device: one ops.stop_check launch behind
            each pick (inside the replayed graph where there is one), and the host looks at the finished flags every 8th token as it
            does for an EOS, also with `eos_token_id=[]`; the host loops (f32, `torch.Generator` sampling, `use_graph=False`) apply
            the same rule in torch (stops.first_finish).  Composes with the processors, both samplers, `output_logprobs`,
            `num_return_sequences`, `past_key_values` and `constraint` (a constrained row may end outside an accepting state, as it may
            at its budget).  With `num_beams > 1`: NotImplementedError.  HF's `stopping_criteria` and `stop_strings` stay refused
            (ValueError): pass the tokenised strings as `stop_sequences`.
        Returns, like HF `generate` called with `inputs_embeds` only, just the NEW tokens [B, <= max_new_tokens]; finished rows are padded
        with pad_token_id.
        After a call from a cache the LAST returned token of a row - its EOS or the end of its stop sequence where it hit one, else the
        last column - is not in the cache,
        so the next turn's `lang_x` must begin with it: on return cache_len[b] = its value before the call + n_new[b] + (tokens returned
        for row b) - 1, at B = 1 and per row in a batch - there the next turn's chunk is ragged (chunked_continue).  The cache must have
        room for T + max_new_tokens - 1 more rows (AkiError before any launch otherwise).
        Differences from the reference, both only visible for B > 1 (where the reference is inconsistent): the
        prompt batch is right-padded and every sample continues from its own length."""
        opt = _parse_generate_kwargs(kwargs, self.pad_token_id, self.default_eos_token_ids, past_key_values is not None,
                                     batch=None if lang_x is None else lang_x.shape[0])
        self.last_stop_hits = None
        if opt.stops:                              # the ids against the logits' width, before any device work
            check_stop_sequences("generate", opt.stops, self._logits_width())
        con = None
        if opt.constraint is not None:             # the host half of binding: the table with its eos columns, checked before any launch
            from .constraint import constraint_for_rows
            if lang_x is None:
                raise ValueError("generate(constraint=...) needs lang_x")
            con, rows_start = constraint_for_rows(opt.constraint, lang_x.shape[0], opt.n_ret)
            width = self._logits_width()
            if con.V != width:
                raise ValueError(f"the constraint was built for V = {con.V}, the logits have {width} columns")
            con.with_eos(sorted(opt.eos_ids))
        if past_key_values is not None:
            cache, logits, appended = self._continue_from_cache(vision_x, lang_x, attention_mask, past_key_values, opt.max_new_tokens)
        elif vision_x is None:
            raise NotImplementedError("text-only generation is outside the AKI hot path")
        else:
            cache, logits, appended = self._prefill_prompt(vision_x, lang_x, attention_mask, opt.max_new_tokens)
        bound = None if con is None else con.bind(sorted(opt.eos_ids), logits.device, rows_start)
        proc = _logits_processors(logits.shape[-1], logits.device, opt.processors, sorted(opt.eos_ids), constraint=bound,
                                  **(opt.penalties or {}))
        if opt.num_beams > 1:
            beam = (opt.num_beams, opt.max_new_tokens, opt.eos_ids, opt.pad_id, opt.length_penalty, opt.early_stopping, proc)
            if self._device_beam_search_ok(cache, logits, opt.num_beams, opt.eos_ids):
                tokens = self._beam_search_device(cache, logits, *beam, opt.use_graph)
            else:
                tokens = self._beam_search(cache, logits, *beam)
        else:
            if opt.n_ret > 1:
                logits = self._expand_rows(cache, logits, opt.n_ret, opt.max_new_tokens)
            eos_t = torch.tensor(sorted(opt.eos_ids), dtype=torch.long, device=logits.device) if opt.eos_ids else None
            on_device = logits.is_cuda and logits.dtype == torch.bfloat16
            if opt.device_rng is not None and not on_device:
                raise ValueError("the device sampler needs bf16 logits on the GPU")
            if opt.use_graph and (not opt.do_sample or opt.device_rng is not None) and on_device:
                tokens, lpb = self._decode_on_device(opt, cache, logits, proc, eos_t)
            else:
                tokens, lpb = self._decode_on_host(opt, cache, logits, proc, eos_t)
            if appended is not None:               # the caller's cache: every row ends right before its last returned token
                self._trim_cache_to_returned(cache, *appended, tokens, eos_t, opt.stops)
            if opt.stops and self.last_stop_hits is None:          # nothing was generated
                self.last_stop_hits = torch.full((tokens.shape[0],), -1, dtype=torch.int32, device=tokens.device)
        self._post_forward_hook()
        if opt.output_logprobs:                    # never with beams (_parse_generate_kwargs)
            lp, top_ids, top_lp = lpb.cut(tokens.shape[1])
            return AkiGenerateOutput(sequences=tokens, logprobs=lp, top_token_ids=top_ids, top_logprobs=top_lp)
        return tokens


class AKI(AkiMethods, VLMWithLanguageStream):
    def __init__(self, vision_encoder: nn.Module, lang_model: nn.Module, vis_feature_dim: int, initial_tokenizer_len: int,
                 pad_token_id: int, decoder_layers_attr_name: str = None, gradient_checkpointing: bool = False,
                 base_img_size: Optional[int] = None, num_vision_tokens: int = 144):
        self._special_tokens = {"media_token": "<image>", "end_of_trunk_token": "<|endofchunk|>"}
        lang_embedding_dim = lang_model.get_input_embeddings().weight.shape[1]
        super().__init__(
            vision_encoder=vision_encoder,
            vision_tokenizer=PerceiverResampler(dim=vis_feature_dim, dim_inner=lang_embedding_dim, num_latents=num_vision_tokens),
            lang_model=lang_model, initial_tokenizer_len=initial_tokenizer_len, gradient_checkpointing=gradient_checkpointing,
            base_img_size=base_img_size, decoder_layers_attr_name=decoder_layers_attr_name, pad_token_id=pad_token_id)
