"""Stop sequences end to end on the tiny model of test_slots_gpu.  The oracle needs no tolerance: stops never change a pick, so a run with
stops equals the same run without them, cut by the pure-Python reference (stop_cases.first_stop) - bit for bit at the same batch size, in
fp32 and bf16.  The sequences are taken from the free run's own tokens: a bigram from the middle of a row and a unigram of another row
(choose_stops).  Every test asserts, as a condition, that at least two rows are cut strictly short of the free run and that at least one
row is not cut at all.

How the two statements about the width are read together: under the chosen pair a row stays uncut, so the call returns max_new_tokens
columns; with one bigram more from the middle of every uncut row every row finishes, and the width is the longest first finish + 1, below
max_new_tokens.  The first test checks both."""
import math

import pytest
import torch

import stop_cases as sc
from conftest import load_golden
from test_model_gpu import batch, DEV
from test_slots_gpu import BUDGETS, tiny, with_budgets

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NEW = 12
_BATCH, _FREE = {}, {}


def inputs(dtype):
    """(model, vision_x, lang_x, attention_mask) of the golden batch of 4."""
    if dtype not in _BATCH:
        m, _ = tiny(dtype)
        vx, lx, am, _ = batch(load_golden("tiny_e2e.npz"), dtype)
        _BATCH[dtype] = (m, vx, lx, am)
    return _BATCH[dtype]


def free_run(dtype):
    """The greedy run at batch 4 without an EOS and without stops, computed once per dtype: [4][NEW]."""
    if dtype not in _FREE:
        m, vx, lx, am = inputs(dtype)
        _FREE[dtype] = m.generate(vx, lx, attention_mask=am, max_new_tokens=NEW, eos_token_id=[]).tolist()
        assert m.last_stop_hits is None
    return _FREE[dtype]


def stop_kw(seqs):
    """The keyword as a dict (test_logits_processors_cpu lists the keywords a literal .generate( call in tests/ may spell out)."""
    return {"stop_sequences": seqs}


def lengths(rows, eos, seqs):
    return [len(sc.cut(r, eos, seqs)) for r in rows]


def conditions(rows, eos, sets):
    """At least two rows cut strictly short of the run without stops, at least one not cut at all.  sets: one per row."""
    with_, without = [len(sc.cut(r, eos, s)) for r, s in zip(rows, sets)], lengths(rows, eos, ())
    return sum(a < b for a, b in zip(with_, without)) >= 2 and any(a == b for a, b in zip(with_, without))


def choose_stops(rows, eos=()):
    """((a bigram from the middle of a row), (a unigram of another row)) under which `conditions` hold; the first such pair."""
    for a, ra in enumerate(rows):
        for i in range(2, len(ra) - 3):
            for b, rb in enumerate(rows):
                for k in range(1, len(rb) - 1):
                    seqs = ((ra[i], ra[i + 1]), (rb[k],))
                    if b != a and conditions(rows, eos, [seqs] * len(rows)):
                        return seqs
    raise AssertionError(f"no bigram / unigram of the free run cuts two rows short and leaves one whole: {rows}")


def expected(rows, eos, seqs, pad):
    """(the returned tensor as lists, the hits): every row cut behind its first finish and padded with pad.  The width is the longest
    first finish + 1 where every row finishes, else the free run's."""
    cuts = [sc.cut(r, eos, seqs) for r in rows]
    every = all(sc.first_stop(r, eos, seqs)[0] is not None for r in rows)
    width = max(len(c) for c in cuts) if every else len(rows[0])
    return [c + [pad] * (width - len(c)) for c in cuts], [sc.first_stop(r, eos, seqs)[1] for r in rows]


def check_hits(m, want):
    hits = m.last_stop_hits
    assert torch.is_tensor(hits) and hits.dtype == torch.int32 and hits.is_cuda and tuple(hits.shape) == (len(want),)
    assert hits.tolist() == want


def all_finish(rows, eos, seqs):
    """seqs plus a bigram from the middle of every row they leave whole: every row finishes short of its end."""
    more = tuple((r[5], r[6]) for r in rows if len(sc.cut(r, eos, seqs)) == len(sc.cut(r, eos, ())) == len(r))
    return seqs + more


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_eos", [False, True], ids=["no_eos", "eos"])
def test_generate_with_stops_is_the_free_run_cut(dtype, with_eos):
    """Greedy at batch 4: bf16 runs the device loop (the check inside the graph), f32 the host loop.  with_eos: the id row 0 emits at step 3
    of the free run, as test_slots_gpu.references chooses it."""
    m, vx, lx, am = inputs(dtype)
    free = free_run(dtype)
    eos = (free[0][3],) if with_eos else ()
    seqs = choose_stops(free, eos)
    out = m.generate(vx, lx, attention_mask=am, max_new_tokens=NEW, eos_token_id=list(eos), **stop_kw([list(s) for s in seqs]))
    want, hits = expected(free, eos, seqs, m.pad_token_id)
    assert with_eos or len(want[0]) == NEW                       # a row is left whole: the call returns max_new_tokens columns
    assert out.tolist() == want
    check_hits(m, hits)
    assert any(h >= 0 for h in hits)
    every = all_finish(free, eos, seqs)                          # every row finishes: the width is the longest first finish + 1
    out = m.generate(vx, lx, attention_mask=am, max_new_tokens=NEW, eos_token_id=list(eos), **stop_kw(every))
    want, hits = expected(free, eos, every, m.pad_token_id)
    assert out.shape[1] == max(lengths(free, eos, every)) < NEW
    assert out.tolist() == want
    check_hits(m, hits)
    m.generate(vx, lx, attention_mask=am, max_new_tokens=2, eos_token_id=[])
    assert m.last_stop_hits is None                              # a call without stops


def test_generate_with_stops_without_a_graph():
    m, vx, lx, am = inputs(torch.bfloat16)
    free = m.generate(vx, lx, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], use_graph=False).tolist()
    seqs = choose_stops(free)
    out = m.generate(vx, lx, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], use_graph=False, **stop_kw(seqs))
    want, hits = expected(free, (), seqs, m.pad_token_id)
    assert out.tolist() == want
    check_hits(m, hits)


@pytest.mark.parametrize("n_ret", [1, 2])
def test_generate_with_stops_on_the_device_sampler(n_ret):
    """do_sample with a DeviceGenerator: the draws depend on (seed, call, token index, row), so a second generator of the same seed repeats
    them; num_return_sequences = 2: eight rows behind one prefill, one hit per row."""
    from aki_amd import ops
    m, vx, lx, am = inputs(torch.bfloat16)
    kw = dict(attention_mask=am, max_new_tokens=NEW, eos_token_id=[], do_sample=True, temperature=1.5, top_k=50, num_return_sequences=n_ret)
    free = m.generate(vx, lx, generator=ops.DeviceGenerator(11), **kw).tolist()
    assert len(free) == 4 * n_ret
    seqs = choose_stops(free)
    out = m.generate(vx, lx, generator=ops.DeviceGenerator(11), **stop_kw(seqs), **kw)
    want, hits = expected(free, (), seqs, m.pad_token_id)
    assert out.tolist() == want
    check_hits(m, hits)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generate_with_stops_and_logprobs(dtype):
    """The values equal the free run's up to the cut and are 0.0 / -1 / 0.0 behind it."""
    m, vx, lx, am = inputs(dtype)
    kw = dict(attention_mask=am, max_new_tokens=NEW, eos_token_id=[], output_logprobs=True, top_logprobs=2)
    free = m.generate(vx, lx, **kw)
    rows = free.sequences.tolist()
    seqs = choose_stops(rows)
    out = m.generate(vx, lx, **stop_kw(seqs), **kw)
    want, hits = expected(rows, (), seqs, m.pad_token_id)
    assert out.sequences.tolist() == want
    check_hits(m, hits)
    for b, n in enumerate(lengths(rows, (), seqs)):
        assert torch.equal(out.logprobs[b, :n], free.logprobs[b, :n]) and torch.equal(out.top_token_ids[b, :n], free.top_token_ids[b, :n])
        assert torch.equal(out.top_logprobs[b, :n], free.top_logprobs[b, :n])
        assert bool((out.logprobs[b, n:] == 0).all()) and bool((out.top_token_ids[b, n:] == -1).all()) and bool((out.top_logprobs[b, n:] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generate_with_stops_from_a_cache(dtype):
    """Four text-only rows continued from a cache: cache_len ends right before each row's last returned token."""
    m, _ = tiny(dtype)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 32000, (4, 11), generator=g).to(DEV)

    def run(**kw):
        cache = m.lang_model(input_ids=ids[:, :-1], use_cache=True, cache_capacity=ids.shape[1] + NEW, last_token_logits=True).past_key_values
        before = cache.cache_len.clone()
        out = m.generate(None, ids[:, -1:], past_key_values=cache, max_new_tokens=NEW, eos_token_id=[], **kw)
        return out.tolist(), (cache.cache_len - before).tolist()

    free, grown = run()
    assert grown == [1 + NEW - 1] * 4
    seqs = choose_stops(free)
    out, grown = run(**stop_kw(seqs))
    want, hits = expected(free, (), seqs, m.pad_token_id)
    assert out == want
    check_hits(m, hits)
    assert grown == [1 + n - 1 for n in lengths(free, (), seqs)]


# ---- generate_many ------------------------------------------------------------------------------------------------------------------
_MANY = {}


def many_free(dtype):
    """The stop-free generate_many run at slots = 3 with BUDGETS and no EOS, once per dtype: (the rows as lists, its stats)."""
    if dtype not in _MANY:
        m, reqs = tiny(dtype)
        outs = m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[])
        assert m.last_stop_hits is None
        _MANY[dtype] = ([o.tolist() for o in outs], dict(m.last_many_stats))
    return _MANY[dtype]


def many_sets(free):
    """(the call-wide default, the per-request RequestParams or None, every request's resolved set).  Requests 0, 1 and 4 take the call-wide
    default - a bigram from the middle of request 0 and a unigram of request 3; request 3 has (), though the default would cut it; request
    2's one-id stop is its token 0; requests 5 and 6 bring two sequences of their own, the later-matching one first."""
    from aki_amd import RequestParams
    default = ((free[0][4], free[0][5]), (free[3][6],))
    own = {2: ((free[2][0],),), 3: (), 5: ((free[5][3], free[5][4]), (free[5][2],)), 6: ((free[6][6], free[6][7]), (free[6][4], free[6][5]))}
    params = [RequestParams(stop_sequences=[list(s) for s in own[r]]) if r in own else None for r in range(len(free))]
    return default, params, [own.get(r, default) for r in range(len(free))]


def many_requests(reqs, params):
    return [(vx, lx, b) if p is None else (vx, lx, b, p) for (vx, lx), b, p in zip(reqs, BUDGETS, params)]


def check_many(m, outs, free, sets):
    want = [sc.cut(f, (), s) for f, s in zip(free, sets)]
    assert conditions(free, (), sets)
    assert [o.tolist() for o in outs] == want
    assert m.last_stop_hits == [sc.first_stop(f, (), s)[1] for f, s in zip(free, sets)]
    assert len(want[2]) == 1 and m.last_stop_hits[2] == 0       # ended at its prefill
    assert want[3] == free[3] and len(sc.cut(free[3], (), sets[0])) < len(free[3])       # () overrides a default that would cut it
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generate_many_with_per_request_stops(dtype):
    m, reqs = tiny(dtype)
    free, free_stats = many_free(dtype)
    default, params, sets = many_sets(free)
    outs = m.generate_many(many_requests(reqs, params), slots=3, eos_token_id=[], stop_sequences=[list(s) for s in default])
    want = check_many(m, outs, free, sets)
    st = m.last_many_stats
    assert st["steps"] < free_stats["steps"], (st, free_stats)
    assert st["live_row_steps"] == sum(len(w) for w in want) - len(want) and st["admits"] == len(want)
    # the same default through params=, the plain requests without RequestParams of their own
    from aki_amd import RequestParams
    outs = m.generate_many(many_requests(reqs, params), slots=3, eos_token_id=[], params=RequestParams(stop_sequences=default),
                           stop_sequences=[[free[0][0]]])
    check_many(m, outs, free, sets)


def test_generate_many_with_stops_over_one_slot():
    m, reqs = tiny(torch.float32)
    free, _ = many_free(torch.float32)
    default, params, sets = many_sets(free)
    outs = m.generate_many(many_requests(reqs, params), slots=1, eos_token_id=[], stop_sequences=default)
    check_many(m, outs, free, sets)
    assert m.last_many_stats["per_request_generate"]
    outs = m.generate_many(many_requests(reqs, params)[6:7], slots=3, eos_token_id=[], stop_sequences=default)      # a single request
    assert [o.tolist() for o in outs] == [sc.cut(free[6], (), sets[6])] and m.last_stop_hits == [sc.first_stop(free[6], (), sets[6])[1]]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generate_many_with_stops_captures_once_and_never_syncs_per_token(dtype, monkeypatch):
    from aki_amd.phi3 import DecodeGraph
    m, reqs = tiny(dtype)
    free, _ = many_free(dtype)
    default, params, sets = many_sets(free)
    captures = []
    real = DecodeGraph._capture
    monkeypatch.setattr(DecodeGraph, "_capture", lambda self: (captures.append(1), real(self))[1])
    outs = m.generate_many(many_requests(reqs, params), slots=3, eos_token_id=[], stop_sequences=default)
    check_many(m, outs, free, sets)
    st = m.last_many_stats
    assert len(captures) == 1
    assert st["steps"] > 8 and st["looks"] <= math.ceil(st["steps"] / 8) + st["admits"] + 1, st


def test_calls_without_stops_never_reach_the_new_ops(monkeypatch):
    from aki_amd import RequestParams, ops

    def refuse(*a, **k):
        raise AssertionError("a call without stops reached the stop-sequence ops")

    real_tick = ops.slot_tick

    def tick(*a, **k):
        assert "stops" not in k and "tokens" not in k and len(a) <= 5
        return real_tick(*a, **k)

    monkeypatch.setattr(ops, "stop_check", refuse)
    monkeypatch.setattr(ops, "StopSets", refuse)
    monkeypatch.setattr(ops, "slot_tick", tick)
    for dtype in DTYPES:
        m, vx, lx, am = inputs(dtype)
        _, reqs = tiny(dtype)
        free, (many, _) = free_run(dtype), many_free(dtype)
        for kw in ({}, {"stop_sequences": []}, {"stop_sequences": None}):
            assert m.generate(vx, lx, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], **kw).tolist() == free
            assert m.last_stop_hits is None
            assert [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[], **kw)] == many
            assert m.last_stop_hits is None
        none = [(vx_, lx_, b, RequestParams(stop_sequences=())) for (vx_, lx_), b in zip(reqs, BUDGETS)]
        assert [o.tolist() for o in m.generate_many(none, slots=3, eos_token_id=[])] == many and m.last_stop_hits is None


def test_bad_stop_sets_are_refused_before_any_device_work(monkeypatch):
    from aki_amd import RequestParams, ops
    m, vx, lx, am = inputs(torch.bfloat16)
    _, reqs = tiny(torch.bfloat16)
    width = m._logits_width()

    def refuse(*a, **k):
        raise AssertionError("device work ahead of the validation")

    monkeypatch.setattr(m, "_prefill_prompt", refuse)
    monkeypatch.setattr(m, "_prefill_request", refuse)
    monkeypatch.setattr(ops, "kv_slot_admit", refuse)
    many = with_budgets(reqs)
    many[2] = many[2] + (RequestParams(stop_sequences=[[1, 2], [width]]),)
    with pytest.raises(ValueError, match="^request 2: "):
        m.generate_many(many, slots=3)
    many[2] = many[2][:3]
    with pytest.raises(ValueError, match="^request 0: "):
        m.generate_many(many, slots=3, stop_sequences=[[width]])
    with pytest.raises(ValueError, match="^request 4: "):
        m.generate_many(many[:4] + [many[4] + (RequestParams(stop_sequences=[[1] * 33]),)], slots=3)
    with pytest.raises(ValueError, match="^generate: "):
        m.generate(vx, lx, attention_mask=am, **stop_kw([[width]]))
    with pytest.raises(NotImplementedError, match="stop_sequences"):
        m.generate(vx, lx, attention_mask=am, num_beams=2, **stop_kw([[1]]))
