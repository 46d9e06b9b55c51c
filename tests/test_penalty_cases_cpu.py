"""min_p and the frequency / presence penalties, the parts that need no GPU: the case table of tests/penalty_cases.py against its
conditions, every reference mutation caught, min_p's kept set against the installed transformers, every host-side refusal, the
resolution of a request's values, which C entry point a call reaches, and the new entry points' own argument checks."""
import types

import numpy as np
import pytest
import torch

import penalty_cases as P
import sampling_cases as S
from test_many_processors_cpu import V_STUB, _requests, _stub as _many_stub

NEW_ENTRIES = ("aki_logits_process_penalized", "aki_greedy_pick_penalized", "aki_sample_pick_penalized",
               "aki_logits_process_rows_penalized", "aki_greedy_pick_rows_penalized", "aki_sample_pick_rows_penalized")


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_should():
    cs = P.cases()
    assert len({c.name for c in cs}) == len(cs)
    main = {(c.sigma, c.T, c.k, c.p, c.min_p) for c in cs if c.V == S.V_MAIN and c.kind == "normal" and not c.processed and c.min_p > 0}
    assert main == {(s, T, k, p, m) for s in (2.0, 4.0) for T in (0.7, 1.0, 1.3) for k, p in ((0, 1.0), (50, 0.9), (1000, 0.5))
                    for m in (0.02, 0.1, 0.5)}
    small = [c for c in cs if c.V == S.V_SMALL and c.min_p > 0 and not c.processed]
    assert S.V_SMALL % 8 == 3 and {(c.k, c.p, c.min_p) for c in small if c.kind == "normal"} == \
        {(k, p, m) for k, p in ((0, 1.0), (50, 0.9), (1000, 0.5)) for m in (0.02, 0.1, 0.5)}
    assert S.ROWS == 8 and S.STEPS == 25 and len(S.OFFSETS) == 10
    ties = [c for c in cs if c.kind == "max_ties"]
    assert ties and all(c.min_p == 1.0 for c in ties)
    for c in ties:                                          # tied maxima all stay, and nothing else does
        r = P.reference(c)
        assert r.kept.sum() == (r.y == r.y.max()).sum() >= 6
    assert any(c.min_p == 0.0 and not c.penalized for c in cs) and any(c.kind == "neg_inf" and c.min_p > 0 for c in cs)
    assert any(c.min_p > 0 and c.penalty != 1.0 and c.suppress and not c.penalized for c in cs)
    pen = P.penalty_cases()
    assert {len(c.history) for c in pen} >= {0, 1, 37} and any(c.full for c in pen) and any(c.done for c in pen)
    h37 = [c for c in pen if len(c.history) == 37][0]
    counts = np.unique(np.asarray(h37.history), return_counts=True)
    assert {1, 2} <= set(counts[1].tolist()) and counts[1].max() >= 5
    assert any(g < 0 for g in h37.history) and any(g >= h37.V for g in h37.history)
    assert any(c.frequency < 0 and c.presence < 0 for c in pen)
    assert any(c.frequency != 0 and c.presence == 0 and c.penalty == 1.0 for c in pen)
    assert any(c.presence != 0 and c.frequency == 0 and c.penalty == 1.0 for c in pen)
    assert any(c.frequency != 0 and c.presence != 0 and c.penalty == 1.3 for c in pen)
    sup = [c for c in pen if c.suppress]
    assert sup and all(set(c.suppress) & set(c.history) for c in sup)
    for c in sup:                                           # a penalised token that is also suppressed ends at -inf
        assert np.isneginf(P.scores(c)[list(set(c.suppress) & set(c.history))]).all()


@pytest.mark.parametrize("c", P.cases(), ids=lambda c: c.name)
def test_conditions_on_the_inputs(c):
    ok, f = P.conditions_hold(c)
    assert ok, f
    if not c.penalized and c.kind != "max_ties":            # the restated base rule is S's own, where S can see the whole row
        assert P.base_conditions_hold(c) == S.conditions_hold(c)[0]
    if c.min_p > 0:
        assert f.minp_gap > P.MINP_MARGIN and f.multi <= P.MINP_MULTI_LIMIT, f
    r = P.reference(c)
    assert r.kept[np.argmax(r.y)] and abs(r.probs.sum() - 1.0) < 1e-12
    u = S.uniform(*S.draws(c))
    assert S.accepted(r, S.reference_tokens(r, u), u).all()
    if c.min_p > 0:                                         # min_p never changes top-p's mass: it only drops tokens top-p kept
        base = S.reference(c, P.scores(c))
        assert not (r.kept & ~base.kept).any() and r.boundary_gap == base.boundary_gap


def test_min_p_zero_filters_nothing_and_the_f32_threshold_is_the_devices():
    c = next(k for k in P.cases() if k.name == "minp-zero")
    assert np.array_equal(P.reference(c).kept, S.reference(c, P.scores(c)).kept)
    assert np.float64(np.float32(0.1)) != 0.1               # the reference compares with the float32 the device reads


# ---- the mutations --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", P.MINP_MUTATIONS)
def test_every_min_p_mutation_is_caught(mutation):
    """A reference with the defect keeps another set than the reference on at least one case - the GPU test compares the support of
    probs_out with the reference's kept set on every case.  minp_strict differs exactly where a weight EQUALS min_p: the tie cases."""
    caught = [c.name for c in P.minp_cases() if c.min_p > 0 and not np.array_equal(P.reference(c, mutation=mutation).kept, P.reference(c).kept)]
    assert caught, mutation
    if mutation == "minp_strict":
        assert all("ties" in n for n in caught)
    else:
        assert len(caught) >= 10, caught


@pytest.mark.parametrize("mutation", P.PENALTY_MUTATIONS)
def test_every_penalty_mutation_is_caught(mutation):
    """A restatement with the defect gives other bits than the reference on at least one penalty case."""
    caught = [c.name for c in P.penalty_cases() if not np.array_equal(P.scores(c, mutation=mutation).view(np.uint32), P.scores(c).view(np.uint32))]
    assert caught, mutation


# ---- transformers ----------------------------------------------------------------------------------------------------------------------------
def _hf_support(c, x):
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    sc = torch.from_numpy(x)[None].clone()
    ids = torch.zeros((1, 1), dtype=torch.long)
    if c.T != 1.0:
        sc = TemperatureLogitsWarper(float(c.T))(ids, sc)
    if c.k > 0:
        sc = TopKLogitsWarper(min(c.k, c.V))(ids, sc)
    if c.p < 1.0:
        sc = TopPLogitsWarper(float(c.p))(ids, sc)
    if c.min_p > 0.0:
        sc = MinPLogitsWarper(float(c.min_p))(ids, sc)
    return torch.isfinite(sc[0]).numpy()


def test_kept_set_is_transformers_support():
    """Temperature -> top-k -> top-p -> MinPLogitsWarper on every min_p case whose top-p boundary class holds one token (HF's top-p
    sorts: it splits a class of equal values arbitrarily).  The margin MINP_MARGIN is far above HF's f32 softmax error."""
    exact = 0
    for c in P.minp_cases():
        x = P.scores(c)
        r = P.reference(c, x)
        if c.p < 1.0 and r.boundary_multiplicity > 1:
            continue
        assert np.array_equal(_hf_support(c, x), r.kept & np.isfinite(r.y)), c.name
        exact += 1
    assert exact >= 30, exact


def test_sample_next_is_the_same_warper():
    """The torch.Generator loop's restatement (aki.sample_next): its support is the reference's kept set."""
    from aki_amd.aki import sample_next
    for name in ("minp-s2-T0.7-k50-p0.9-m0.1", "minp-small-k0-p1-m0.5", "minp-one-ties"):
        c = next(k for k in P.cases() if k.name == name)
        x = torch.from_numpy(P.scores(c))[None].repeat(64, 1)
        g = torch.Generator().manual_seed(3)
        r = P.reference(c)
        if c.p < 1.0 and r.boundary_multiplicity > 1:
            continue
        for _ in range(8):
            tok = sample_next(x, c.T, c.k, c.p, g, float(np.float32(c.min_p)))
            assert r.kept[tok.numpy()].all(), name


# ---- host-side refusals ---------------------------------------------------------------------------------------------------------------------
def _gen_stub():
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: [])


BAD = [("min_p", -0.1), ("min_p", 1.5), ("min_p", float("nan")), ("min_p", "x"), ("frequency_penalty", 2.5), ("frequency_penalty", -2.01),
       ("frequency_penalty", float("inf")), ("frequency_penalty", float("nan")), ("frequency_penalty", "x"), ("presence_penalty", 3.0),
       ("presence_penalty", float("-inf")), ("presence_penalty", float("nan"))]


@pytest.mark.parametrize("name, value", BAD, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BAD)])
def test_generate_refuses_bad_values_before_device_work(name, value):
    from aki_amd.aki import AKI
    kw = {name: value}
    with pytest.raises(ValueError, match=name):
        AKI.generate(_gen_stub(), None, None, max_new_tokens=4, do_sample=True, **kw)


def test_generate_takes_the_keywords_and_refuses_them_under_beams():
    from aki_amd.aki import AKI, PROCESSOR_KWARGS, _parse_generate_kwargs
    from aki_amd.slots import PROCESSOR_FIELDS
    kw = dict(min_p=0.1, frequency_penalty=0.5, presence_penalty=-0.5)
    lang_x = torch.zeros((1, 3), dtype=torch.long)
    with pytest.raises(NotImplementedError, match="text-only"):                # past the parser: the text-only check needs no device
        AKI.generate(_gen_stub(), None, lang_x, max_new_tokens=4, do_sample=True, **kw)
    greedy = {"min_p": 0.3}
    with pytest.raises(NotImplementedError, match="text-only"):                # min_p without do_sample is ignored, as top_p is
        AKI.generate(_gen_stub(), None, lang_x, max_new_tokens=4, **greedy)
    for name, v in kw.items():
        one = {name: v}
        with pytest.raises(NotImplementedError, match=name):
            AKI.generate(_gen_stub(), None, None, max_new_tokens=4, num_beams=2, **one)
    for name in kw:                                                            # None and the neutral value are no request for it
        for neutral in ({name: None}, {name: 0.0}):
            with pytest.raises(NotImplementedError, match="text-only"):
                AKI.generate(_gen_stub(), None, lang_x, max_new_tokens=4, num_beams=2, **neutral)
    opt = _parse_generate_kwargs(dict(kw, do_sample=True), 0, lambda: [], False)
    assert opt.min_p == float(np.float32(0.1)) and opt.penalties == dict(frequency_penalty=0.5, presence_penalty=-0.5)
    assert set(opt.processors) == set(PROCESSOR_KWARGS) and not set(kw) & (set(PROCESSOR_KWARGS) | set(PROCESSOR_FIELDS))


def test_processor_object_takes_and_checks_the_penalties():
    from aki_amd import ops
    for kw in (dict(frequency_penalty=2.5), dict(frequency_penalty=float("nan")), dict(presence_penalty=-2.5), dict(presence_penalty=float("inf")),
               dict(presence_penalty="x")):
        with pytest.raises(ValueError):
            ops.LogitsProcessors(100, "cpu", **kw)
    assert not ops.LogitsProcessors(100, "cpu", frequency_penalty=0.0, presence_penalty=0.0).active
    for kw in (dict(frequency_penalty=0.5), dict(presence_penalty=-2.0), dict(frequency_penalty=2.0, presence_penalty=0.1)):
        p = ops.LogitsProcessors(100, "cpu", **kw)
        assert p.active and p.penalized
    with pytest.raises(ValueError):
        ops.LogitsProcessors(200_000, "cpu", presence_penalty=0.5)             # active: the kernel's V limit applies
    p = ops.LogitsProcessors(100, "cpu", frequency_penalty=0.1)
    fq, pr = p.penalty_rows(3, "cpu")
    assert pr is None and fq.dtype == torch.float32 and fq.tolist() == [float(np.float32(0.1))] * 3 and p.penalty_rows(3, "cpu")[0] is fq


# ---- RequestParams and generate_many's host half ---------------------------------------------------------------------------------------------
MANY_BAD = [(dict(min_p=-0.5), "min_p"), (dict(min_p=1.01), "min_p"), (dict(min_p=float("nan")), "min_p"), (dict(frequency_penalty=2.1), "frequency_penalty"),
            (dict(frequency_penalty=float("nan")), "frequency_penalty"), (dict(presence_penalty=-3), "presence_penalty"),
            (dict(presence_penalty=float("inf")), "presence_penalty"), (dict(presence_penalty="x"), "presence_penalty")]


@pytest.mark.parametrize("slots", [3, 1])
def test_generate_many_validates_on_the_host_and_names_the_request(slots):
    from aki_amd import RequestParams
    from aki_amd.aki import AKI
    plain = RequestParams()
    many = lambda per_request, **kw: AKI.generate_many(_many_stub(), _requests(per_request), slots=slots, **kw)
    for kw, what in MANY_BAD:
        with pytest.raises(ValueError, match=f"request 3.*{what}"):
            RequestParams(**kw).check(3, 5)
        with pytest.raises(ValueError, match=f"request 1.*{what}"):
            many([plain, RequestParams(**kw)])
        with pytest.raises(ValueError, match=f"params=.*{what}"):
            many([plain, plain], params=RequestParams(**kw))
    for name in ("frequency_penalty", "presence_penalty"):
        with pytest.raises(ValueError, match=name):
            many([plain, plain], **{name: 2.5})
    with pytest.raises(ValueError, match="min_p"):                             # request-owned, like temperature
        many([plain, plain], **{"min_p": 0.1})
    with pytest.raises(ValueError, match="temperature"):
        many([plain, plain], temperature=0.7)


def test_request_values_resolve_own_then_params_then_call():
    from aki_amd import RequestParams
    from aki_amd.aki import AKI
    from aki_amd.slots import resolve_penalties
    f = lambda v: float(np.float32(v))
    call = dict(frequency_penalty=0.3, presence_penalty=0.4)
    default = RequestParams(frequency_penalty=0.7)
    assert resolve_penalties(RequestParams(frequency_penalty=1.1, presence_penalty=0.0), default, call) == dict(frequency_penalty=f(1.1), presence_penalty=0.0)
    assert resolve_penalties(RequestParams(), default, call) == dict(frequency_penalty=f(0.7), presence_penalty=f(0.4))
    assert resolve_penalties(RequestParams(), RequestParams(), call) == dict(frequency_penalty=f(0.3), presence_penalty=f(0.4))
    assert resolve_penalties(RequestParams(frequency_penalty=0.0), default, call)["frequency_penalty"] == 0.0        # an explicit 0.0 overrides
    assert resolve_penalties(None, None, None) == dict(frequency_penalty=0.0, presence_penalty=0.0)
    assert RequestParams().min_p == 0.0 and RequestParams().frequency_penalty is None and RequestParams().presence_penalty is None
    # the slots == 1 path: what generate() is handed per request
    seen = []
    params = [RequestParams(), RequestParams(frequency_penalty=0.0, presence_penalty=1.5), RequestParams(min_p=0.25, presence_penalty=0.0)]
    AKI.generate_many(_many_stub(seen=seen), _requests(params), slots=1, params=RequestParams(presence_penalty=0.5), **dict(call))
    pick = lambda kw: {k: kw.get(k) for k in ("frequency_penalty", "presence_penalty", "min_p")}
    assert [pick(kw) for kw in seen] == [
        dict(frequency_penalty=f(0.3), presence_penalty=0.5, min_p=None),      # nothing of its own: params=, else the call-wide keyword
        dict(frequency_penalty=None, presence_penalty=1.5, min_p=None),        # its explicit 0.0 overrides both: nothing is handed on
        dict(frequency_penalty=f(0.3), presence_penalty=None, min_p=None)]     # a greedy request's min_p is ignored, as its top_p is


# ---- which entry point a call reaches --------------------------------------------------------------------------------------------------------
class _Recorder:
    """A stand-in for the loaded library: every aki_* call is recorded with its argument count and answers AKI_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("aki_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, len(a))) or 0


@pytest.fixture
def rec(monkeypatch):
    from aki_amd import _lib as L, ops
    r = _Recorder()
    monkeypatch.setattr(L, "load", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_dev", lambda *ts: next(t.device for t in ts if t is not None))
    return r


def _pick_buffers(B=3, V=64):
    return (torch.zeros((B, V), dtype=torch.bfloat16), torch.zeros(B, dtype=torch.long),
            dict(tokens=torch.zeros((B, 6), dtype=torch.long), cache_len=torch.zeros(B, dtype=torch.int32), start_len=torch.zeros(B, dtype=torch.int32)))


def _sets(V=64, B=3):
    from aki_amd import ops
    from aki_amd.slots import NEUTRAL_SET_KEY
    return ops.ProcessorSets(V, "cpu", [], [NEUTRAL_SET_KEY], B)


def _rows(B=3):
    return dict(temperature=torch.ones(B), top_k=torch.zeros(B, dtype=torch.int32), top_p=torch.ones(B), seed=torch.zeros(B, dtype=torch.int64))


def test_a_call_without_the_new_values_reaches_no_new_entry_point(rec):
    from aki_amd import _lib as L, ops
    x, ids, kw = _pick_buffers()
    proc = ops.LogitsProcessors(64, "cpu", repetition_penalty=1.3)
    ops.greedy_pick(x, ids, **kw)
    ops.greedy_pick(x, ids, processors=proc, **kw)
    ops.greedy_pick(x, ids, processor_sets=_sets(), **kw)
    ops.sample_pick(x, ids, temperature=0.7, top_k=5, top_p=0.9, **kw)
    ops.sample_pick(x, ids, processors=proc, min_p=0.0, **kw)
    ops.sample_pick_rows(x, ids, **_rows(), **kw)
    ops.sample_pick_rows(x, ids, processor_sets=_sets(), **_rows(), **kw)
    proc.apply(x, tokens=kw["tokens"])
    _sets().apply(x, tokens=kw["tokens"])
    names = [n for n, _ in rec.calls]
    assert names == ["aki_greedy_pick", "aki_greedy_pick_processed", "aki_greedy_pick_rows", "aki_sample_pick", "aki_sample_pick",
                     "aki_sample_pick_rows", "aki_sample_pick_rows_processed", "aki_logits_process", "aki_logits_process_rows"]
    assert not set(names) & set(NEW_ENTRIES)
    for n, count in rec.calls:
        assert count == len(L.SIGNATURES[n][1]), n


def test_a_call_with_a_new_value_reaches_its_penalized_entry_point(rec):
    from aki_amd import _lib as L, ops
    x, ids, kw = _pick_buffers()
    pen = ops.LogitsProcessors(64, "cpu", frequency_penalty=0.5)
    fq = torch.full((3,), 0.5)
    ops.greedy_pick(x, ids, processors=pen, **kw)
    ops.greedy_pick(x, ids, processor_sets=_sets(), presence_penalty=fq, **kw)
    ops.sample_pick(x, ids, min_p=0.1, **kw)
    ops.sample_pick(x, ids, processors=pen, **kw)
    ops.sample_pick_rows(x, ids, processor_sets=_sets(), min_p=fq, **_rows(), **kw)
    ops.sample_pick_rows(x, ids, processor_sets=_sets(), frequency_penalty=fq, **_rows(), **kw)
    pen.apply(x, tokens=kw["tokens"])
    _sets().apply(x, tokens=kw["tokens"], frequency_penalty=fq)
    assert [n for n, _ in rec.calls] == ["aki_greedy_pick_penalized", "aki_greedy_pick_rows_penalized", "aki_sample_pick_penalized",
                                         "aki_sample_pick_penalized", "aki_sample_pick_rows_penalized", "aki_sample_pick_rows_penalized",
                                         "aki_logits_process_penalized", "aki_logits_process_rows_penalized"]
    for n, count in rec.calls:
        assert count == len(L.SIGNATURES[n][1]), n
    # what has no entry point is refused, not dropped
    with pytest.raises(ops.AkiError, match="processor_sets"):
        ops.sample_pick_rows(x, ids, min_p=fq, **_rows(), **kw)
    with pytest.raises(ops.AkiError, match="scratch"):
        ops.greedy_pick(x, ids, frequency_penalty=fq, **kw)
    with pytest.raises(ops.AkiError, match="f32"):
        ops.greedy_pick(x, ids, processor_sets=_sets(), frequency_penalty=fq.double(), **kw)
    with pytest.raises(ValueError, match="min_p"):
        ops.sample_pick(x, ids, min_p=1.5, **kw)


def test_pick_stage_hands_the_per_row_values_on():
    """PickStage passes the per-row tensors through, and row(slot) cuts them to the slot's one-row views like the sampler's four."""
    from aki_amd import ops
    from aki_amd.pick_stage import PickStage
    B = 3
    x, ids, kw = _pick_buffers(B)
    pick = dict(pad_token_id=0, eos_ids=None, done=torch.zeros(B, dtype=torch.uint8), tokens=kw["tokens"], start_len=kw["start_len"],
                done_at=torch.zeros(B, dtype=torch.int32), processor_sets=_sets(), frequency_penalty=torch.arange(B, dtype=torch.float32),
                presence_penalty=torch.ones(B))
    stage = PickStage(pick, rows=dict(_rows(B), min_p=torch.arange(B, dtype=torch.float32) / 4))
    seen = []
    orig = ops.sample_pick_rows
    ops.sample_pick_rows = lambda *a, **k: seen.append(k)
    try:
        stage.run(x, ids, kw["cache_len"], advance=True)
        stage.row(2).run(x[2:3], ids[2:3], kw["cache_len"][2:3], advance=False)
    finally:
        ops.sample_pick_rows = orig
    assert seen[0]["frequency_penalty"] is pick["frequency_penalty"] and seen[0]["min_p"].shape == (B,)
    assert seen[1]["frequency_penalty"].tolist() == [2.0] and seen[1]["presence_penalty"].tolist() == [1.0] and seen[1]["min_p"].tolist() == [0.5]
    assert seen[1]["frequency_penalty"].data_ptr() == pick["frequency_penalty"][2:].data_ptr()          # a view: written in place at admit


# ---- the C entry points' own checks ------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20      # never dereferenced: every call below must be refused on the host


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_typed_and_exported(lib):
    import os
    import re
    import subprocess
    from aki_amd import _lib
    from conftest import ROOT
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aki_mi355x.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\bT {name}\b", exported), name
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name     # the ctypes table has the header's argument count
    assert lib.aki_abi_version() == 17 and _lib.AKI_PROCESSOR_SET_WORDS == 9


def _common(**over):
    a = dict(logits=FAKE, B=2, V=100, ld=100, eos=None, n_eos=0, pad=0, done=None, ids=FAKE, tokens=FAKE, tokens_ld=8, cache_len=FAKE,
             start_len=FAKE, advance=1, done_at=None, w=None, extra=None, max_orig=0, n_add=0, d=0, emb_out=None, scores=FAKE, ld_scores=100)
    a.update({k: v for k, v in over.items() if k in a})
    return a


def _wide(over):
    a = dict(penalty=1.2, ngram=2, min_len=0, sup=None, n_sup=0, bsup=None, n_bsup=0, bad=FAKE, off=FAKE, n_bad=1, n_bad_ids=2)
    a.update({k: v for k, v in over.items() if k in a})
    return a


def _sets_args(over):
    a = dict(sets=FAKE, n_sets=1, row_set=FAKE, set_ids=None, n_set_ids=0, bad_offsets=FAKE, n_words=0)
    a.update({k: v for k, v in over.items() if k in a})
    return a


def _con(over, rows):
    a = dict(table=None, table_ld=0, n_states=0, states=None, states_ld=0)
    if rows:
        a.update(row_base=None, row_states=None)
    a.update({k: v for k, v in over.items() if k in a})
    return a


def _greedy(lib, **o):
    return lib.aki_greedy_pick_penalized(*_common(**o).values(), *_wide(o).values(), *_con(o, False).values(), o.get("fq", FAKE), o.get("pr"), None)


def _sample(lib, **o):
    s = dict(step=0, T=1.0, k=0, p=1.0, seed=1, offset=0, probs=None, ld_probs=0)
    s.update({k: v for k, v in o.items() if k in s})
    return lib.aki_sample_pick_penalized(*_common(**o).values(), *_wide(o).values(), *s.values(), *_con(o, False).values(), o.get("fq"),
                                         o.get("pr"), o.get("mp", FAKE), None)


def _greedy_rows(lib, **o):
    return lib.aki_greedy_pick_rows_penalized(*_common(**o).values(), *_sets_args(o).values(), *_con(o, True).values(), o.get("fq", FAKE),
                                              o.get("pr"), None)


def _sample_rows(lib, **o):
    s = dict(step=0, T=FAKE, k=FAKE, p=FAKE, seed=FAKE, probs=None, ld_probs=0)
    s.update({k: v for k, v in o.items() if k in s})
    return lib.aki_sample_pick_rows_penalized(*_common(**o).values(), *_sets_args(o).values(), *s.values(), *_con(o, True).values(),
                                              o.get("fq"), o.get("pr"), o.get("mp", FAKE), None)


def _process(lib, rows, **o):
    a = dict(logits=FAKE, dtype=0, B=2, V=100, ld=100, out=FAKE, ld_out=100, tokens=FAKE, tokens_ld=8, cache_len=None, start_len=None, step=0,
             done=None)
    a.update({k: v for k, v in o.items() if k in a})
    if rows:
        mid = dict(eos=None, n_eos=0, **_sets_args(o))
        fn = lib.aki_logits_process_rows_penalized
    else:
        w = _wide(o)
        mid = dict(penalty=w["penalty"], ngram=w["ngram"], min_len=w["min_len"], eos=None, n_eos=0, sup=w["sup"], n_sup=w["n_sup"], bsup=w["bsup"],
                   n_bsup=w["n_bsup"], bad=w["bad"], off=w["off"], n_bad=w["n_bad"], n_bad_ids=w["n_bad_ids"])
        fn = lib.aki_logits_process_penalized
    return fn(*a.values(), *mid.values(), *_con(o, rows).values(), o.get("fq", FAKE), o.get("pr"), None)


def test_new_entry_points_validate_on_the_host(lib):
    from aki_amd import _lib
    bad, align = -1, -3                                     # AKI_ERR_INVALID_ARG, AKI_ERR_ALIGNMENT
    for call in (_greedy, _sample, _greedy_rows, _sample_rows):
        assert call(lib, logits=None) == bad
        assert call(lib, ids=None) == bad
        assert call(lib, scores=None) == bad
        assert call(lib, ld_scores=99) == bad
        assert call(lib, cache_len=None) == bad             # advance without the counters
        assert call(lib, emb_out=FAKE) == bad               # an embedding output without a table
        assert call(lib, V=_lib.AKI_LOGITS_PROCESS_MAX_V + 1, ld=1 << 20, ld_scores=1 << 20) == bad
        assert call(lib, scores=FAKE + 4) == align
        assert call(lib, ld_scores=102) == align
        # a table is optional; one that is given is checked
        assert call(lib, table=FAKE, table_ld=100, n_states=3, states=None, states_ld=4, row_base=FAKE, row_states=FAKE) == bad
        assert call(lib, table=FAKE, table_ld=50, n_states=3, states=FAKE, states_ld=4, row_base=FAKE, row_states=FAKE) == bad
    for call in (_greedy, _sample):
        assert call(lib, penalty=0.0) == bad
        assert call(lib, ngram=-1) == bad
        assert call(lib, n_bad_ids=0) == bad
        assert call(lib, table=FAKE, table_ld=100, n_states=40000, states=FAKE, states_ld=4) == bad        # one automaton: below 32768 states
    for call in (_greedy_rows, _sample_rows):
        assert call(lib, sets=None) == bad
        assert call(lib, n_sets=0) == bad
        assert call(lib, row_set=None) == bad
        assert call(lib, table=FAKE, table_ld=100, n_states=3, states=FAKE, states_ld=4, row_base=None, row_states=FAKE) == bad
    assert _sample(lib, T=0.0) == bad and _sample(lib, p=0.0) == bad and _sample(lib, k=-1) == bad and _sample(lib, step=-1) == bad
    assert _sample(lib, probs=FAKE, ld_probs=50) == bad
    assert _sample_rows(lib, T=None) == bad and _sample_rows(lib, seed=None) == bad and _sample_rows(lib, step=-1) == bad
    for rows in (False, True):
        assert _process(lib, rows, logits=None) == bad
        assert _process(lib, rows, out=None) == bad
        assert _process(lib, rows, ld=99) == bad
        assert _process(lib, rows, ld_out=50) == bad
        assert _process(lib, rows, step=-1) == bad
        assert _process(lib, rows, dtype=_lib.AKI_DT_FP8_E4M3) == -2                                       # AKI_ERR_UNSUPPORTED
        assert _process(lib, rows, table=FAKE, table_ld=100, n_states=3, states=None, states_ld=4, row_base=FAKE, row_states=FAKE) == bad
    assert _process(lib, False, penalty=float("nan")) == bad and _process(lib, True, n_sets=0) == bad
