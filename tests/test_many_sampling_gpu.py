"""Per-request sampling and log-probabilities in generate_many, on the GPU: ops.sample_pick_rows against the float64 reference of
tests/sampling_cases.py on the row table of tests/many_sampling_cases.py (every row its own temperature, top_k, top_p and Philox
key), and AKI.generate_many with RequestParams end to end on the tiny bf16 model.  Every test here needs the feature."""
import math

import numpy as np
import pytest
import torch

import logprob_cases as LC
import many_sampling_cases as M
import sampling_cases as S
from test_logprob_gpu import BF16_ROUTE_BAR
from test_slots_gpu import BUDGETS, check_structure, generate_alone, references, tiny, with_budgets

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- ops.sample_pick_rows -------------------------------------------------------------------------------------------------------------
def _device_rows(table):
    """bf16 logits [B, V] and the four parameter arrays of a row table, on the device."""
    x = torch.from_numpy(np.stack([S.logits(c) for c, _ in table])).to(DEV).to(torch.bfloat16).contiguous()
    T, k, p, seed = (torch.from_numpy(a).to(DEV) for a in M.param_arrays(table))
    return x, dict(temperature=T, top_k=k, top_p=p, seed=seed)


_DRAWN = {}


def _drawn(which):
    """(x, params, tokens [steps, B] as numpy) of the six-row table over 256 steps / the V_MAIN rows over 64 - launched once, shared."""
    from aki_amd import ops
    if which not in _DRAWN:
        table, steps = (M.rows(), M.STEPS) if which == "small" else (M.main_rows(), M.MAIN_STEPS)
        x, params = _device_rows(table)
        out = torch.full((steps, len(table)), -1, dtype=torch.long, device=DEV)
        for n in range(steps):
            ops.sample_pick_rows(x, out[n], step=n, **params)
        _DRAWN[which] = (x, params, out.cpu().numpy())
    return _DRAWN[which]


@pytest.mark.parametrize("which", ["small", "main"])
def test_every_row_draws_from_its_own_parameters_and_seed(which):
    table = M.rows() if which == "small" else M.main_rows()
    _, _, got = _drawn(which)
    for b, (c, seed) in enumerate(table):
        u = M.draws(seed, got.shape[0])
        ok = S.accepted(M.reference(c), got[:, b], u)
        assert ok.all(), (b, int((~ok).sum()), got[:, b][~ok][:8].tolist(), u[~ok][:8].tolist())


def test_the_greedy_row_and_the_twin_rows():
    from aki_amd import ops
    x, _, got = _drawn("small")
    want = torch.zeros(x.shape[0], dtype=torch.long, device=DEV)
    ops.greedy_pick(x, want)
    assert (got[:, 1] == int(want[1])).all()                    # top_k == 1: the greedy pick's token on every step
    assert np.array_equal(got[:, 0], got[:, 5])                 # the same logits, parameters and seed in rows 0 and 5
    assert len(set(got[:, 0].tolist())) > 32                    # ... and they are draws, not one token
    for a, b in ((0, 2), (0, 4), (2, 4)):
        assert not np.array_equal(got[:, a], got[:, b])


def test_a_row_is_bit_equal_to_the_scalar_sampler_at_batch_one():
    """ops.sample_pick at B = 1, offset 0 and seed s draws with the counter (n, 0, 0, 0): row b of sample_pick_rows with that row's
    parameters returns its token and its filtered distribution, bit for bit."""
    from aki_amd import ops
    table = M.rows()
    x, params, got = _drawn("small")
    B, V = x.shape
    for n in range(32):
        probs = torch.full((B, V), -1.0, dtype=torch.float32, device=DEV)
        ids = torch.zeros(B, dtype=torch.long, device=DEV)
        ops.sample_pick_rows(x, ids, step=n, probs_out=probs, **params)
        assert np.array_equal(ids.cpu().numpy(), got[n])
        for b, (c, seed) in enumerate(table):
            p1 = torch.full((1, V), -1.0, dtype=torch.float32, device=DEV)
            i1 = torch.zeros(1, dtype=torch.long, device=DEV)
            ops.sample_pick(x[b:b + 1], i1, step=n, temperature=c.T, top_k=c.k, top_p=c.p, seed=seed, offset=0, probs_out=p1)
            assert int(i1[0]) == int(ids[b]) and torch.equal(p1[0], probs[b]), (n, b)


def test_bookkeeping_follows_the_row():
    """tokens / cache_len / start_len / done / done_at with rows at different generated-token indices: the index written and the n of the
    draw are the row's own; a done row writes pad whatever its parameters are; a row whose token is an eos id becomes done there."""
    from aki_amd import ops
    table = M.rows()
    x, params, _ = _drawn("small")
    B = x.shape[0]
    start = torch.tensor([7, 3, 0, 5, 1, 2], dtype=torch.int32, device=DEV)
    n_row = [0, 5, 17, 40, 3, 9]
    gen_idx = torch.tensor(n_row, dtype=torch.int32, device=DEV)
    width, pad = 64, 11

    def run(eos):
        st = dict(ids=torch.full((B,), -1, dtype=torch.long, device=DEV), tokens=torch.full((B, width), -7, dtype=torch.long, device=DEV),
                  done=torch.zeros(B, dtype=torch.uint8, device=DEV), done_at=torch.full((B,), -1, dtype=torch.int32, device=DEV),
                  cache_len=start + gen_idx - 1)
        st["done"][3] = 1
        ops.sample_pick_rows(x, st["ids"], pad_token_id=pad, eos_ids=eos, done=st["done"], tokens=st["tokens"], cache_len=st["cache_len"],
                             start_len=start, advance=True, done_at=st["done_at"], **params)
        return st

    probe = run(None)
    eos = torch.tensor([int(probe["ids"][4]), S.V_SMALL + 5], dtype=torch.long, device=DEV)
    st = run(eos)
    ids = st["ids"].tolist()
    assert ids == probe["ids"].tolist()
    for b, (c, seed) in enumerate(table):
        if b == 3:
            assert ids[b] == pad                                 # finished before the launch (its parameters: T 0.7, k 1000, p 0.5)
        else:
            u = M.draws(seed, 64)[n_row[b]:n_row[b] + 1]         # the draw of generated token n_row[b], not of another row's index
            assert S.accepted(M.reference(c), np.array([ids[b]]), u).all(), b
        want = torch.full((width,), -7, dtype=torch.long, device=DEV)
        want[n_row[b]] = ids[b]
        assert torch.equal(st["tokens"][b], want), b             # written at the row's own index, nothing else touched
    assert torch.equal(st["cache_len"], start + gen_idx)
    assert st["done"].tolist() == [0, 0, 0, 1, 1, 0] and st["done_at"].tolist() == [-1, -1, -1, -1, n_row[4], -1]


def test_processed_rows_draw_from_the_processed_scores():
    """One LogitsProcessors for all rows (small-proc's repetition penalty, history and suppressed ids), per-row sampler parameters behind it."""
    from aki_amd import ops
    base = next(c for c in S.cases() if c.name == "small-proc")
    scores = S.processed_scores(base, S.logits(base))
    own = [(base.T, base.k, base.p), (1.0, 1, 1.0), (0.7, 0, 1.0)]
    table = [(S.Case(f"rows-proc-{b}", base.V, base.sigma, T, k, p), M.row_seed(16 + b)) for b, (T, k, p) in enumerate(own)]
    refs = [S.reference(c, x=scores) for c, _ in table]
    B, H, steps = len(table), len(base.history), 64
    x = torch.from_numpy(S.logits(base)).to(DEV).to(torch.bfloat16)[None].repeat(B, 1).contiguous()
    T, k, p, seed = (torch.from_numpy(a).to(DEV) for a in M.param_arrays(table))
    proc = ops.LogitsProcessors(base.V, DEV, repetition_penalty=base.penalty, suppress_tokens=list(base.suppress))
    tokens = torch.zeros((B, H + steps), dtype=torch.long, device=DEV)
    tokens[:, :H] = torch.tensor(base.history, dtype=torch.long, device=DEV)
    tokens[:, H:] = base.history[0]                    # what the picks append must not change the set of penalised tokens
    out = torch.zeros((steps, B), dtype=torch.long, device=DEV)
    for st in range(steps):
        ops.sample_pick_rows(x, out[st], tokens=tokens.clone(), step=H + st, processors=proc, temperature=T, top_k=k, top_p=p, seed=seed)
    got = out.cpu().numpy()
    for b, (c, s) in enumerate(table):
        u = S.uniform(H + np.arange(steps), 0, 0, seed=s)
        if c.k == 1:
            want = torch.zeros(B, dtype=torch.long, device=DEV)
            ops.greedy_pick(x, want, tokens=tokens.clone(), processors=proc, cache_len=torch.full((B,), H, dtype=torch.int32, device=DEV))
            assert (got[:, b] == int(want[b])).all()
            continue
        assert (S.accept_set_sizes(refs[b], u) > 1).mean() <= (M.MULTI_CAP if c.filtered else M.MAIN_UNFILTERED_CAP)
        ok = S.accepted(refs[b], got[:, b], u)
        assert ok.all(), (b, int((~ok).sum()))
    assert not set(got[:, 2].tolist()) & set(base.suppress)


def test_host_validation_of_the_row_arrays():
    from aki_amd import ops
    x, params, _ = _drawn("small")
    ids = torch.zeros(x.shape[0], dtype=torch.long, device=DEV)
    for name, bad in (("temperature", params["temperature"].double()), ("top_k", params["top_k"].long()), ("top_p", params["top_p"][:5]),
                      ("seed", params["seed"].int()), ("seed", params["seed"].cpu()), ("top_k", None),
                      ("temperature", params["temperature"].repeat(2)[::2])):
        with pytest.raises(ops.AkiError):
            ops.sample_pick_rows(x, ids, **dict(params, **{name: bad}))
    with pytest.raises(ops.AkiError):
        ops.sample_pick_rows(x.float(), ids, **params)
    with pytest.raises(ValueError):
        ops.sample_pick_rows(x, ids, step=-1, **params)


# ---- generate_many with RequestParams on the tiny bf16 model --------------------------------------------------------------------------
SLOTS = 3
GREEDY_REQUESTS = (1, 4)


def seed_of(r):
    return M.row_seed(32 + r)


def sampled_params(r, **kw):
    import aki_amd
    return aki_amd.RequestParams(do_sample=True, top_k=8, seed=seed_of(r), **kw)


def with_params(reqs, params, budgets=BUDGETS):
    return [(vx, lx, b, p) for (vx, lx), b, p in zip(reqs, budgets, params)]


_CALLS = {}


def call(name):
    """The token lists of the calls several tests compare, each made once: all greedy, all sampled, mixed."""
    import aki_amd
    if name not in _CALLS:
        m, reqs = tiny(torch.bfloat16)
        if name == "greedy":
            outs = m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[])
        elif name == "sampled":
            outs = m.generate_many(with_params(reqs, [sampled_params(r) for r in range(7)]), slots=SLOTS, eos_token_id=[])
        else:
            params = [aki_amd.RequestParams() if r in GREEDY_REQUESTS else sampled_params(r) for r in range(7)]
            outs = m.generate_many(with_params(reqs, params), slots=SLOTS, eos_token_id=[])
        _CALLS[name] = ([o.tolist() for o in outs], dict(m.last_many_stats))
    return _CALLS[name]


_FORWARDS = {}


def teacher_forced_logits(r, row):
    """f32 logits [n, V] of the full forward over request r's prompt followed by `row`: the rows that predict row[0..n-1].  Kept per sequence."""
    key = (r, tuple(row))
    if key not in _FORWARDS:
        m, reqs = tiny(torch.bfloat16)
        vx, lx = reqs[r]
        ids = torch.cat([lx[0], torch.tensor(row, dtype=torch.long, device=DEV)])[None]
        with torch.no_grad():
            _FORWARDS[key] = m(vx, ids, attention_mask=torch.ones_like(ids)).logits[0, -(len(row) + 1):-1].float()
    return _FORWARDS[key]


def test_sampled_requests_sample_and_stay_inside_their_top_k():
    greedy, _ = call("greedy")
    sampled, stats = call("sampled")
    assert [len(x) for x in sampled] == BUDGETS == [len(x) for x in greedy] and stats["admits"] == 7 and stats["slots"] == SLOTS
    assert any(s != g for s, g in zip(sampled, greedy)), "no sampled request differs from the greedy call: the tests here would show nothing"
    for r, row in enumerate(sampled):                          # validity: every token is one of the 8 best of its teacher-forced step
        full = teacher_forced_logits(r, row)
        kth = full.topk(8, dim=-1).values[:, -1]
        chosen = full.gather(1, torch.tensor(row, device=DEV)[:, None])[:, 0]
        bar = 0.05 * max(1.0, float(full.abs().max()))
        assert bool((chosen >= kth - bar).all()), (r, (kth - chosen).max().item(), bar)


def test_a_requests_tokens_do_not_depend_on_the_schedule():
    """Reversed order over the same 3 slots: other slots, other neighbours, other admit times - the same tokens per request (bf16 at the same
    batch size is bit-identical per row; the draw depends on the request's seed and token index only)."""
    m, reqs = tiny(torch.bfloat16)
    sampled, _ = call("sampled")
    params = [sampled_params(r) for r in range(7)]
    rev = m.generate_many(with_params(reqs, params)[::-1], slots=SLOTS, eos_token_id=[])[::-1]
    assert [o.tolist() for o in rev] == sampled


def test_greedy_requests_in_a_sampled_batch_return_the_greedy_tokens():
    greedy, gstats = call("greedy")
    mixed, mstats = call("mixed")
    sampled, _ = call("sampled")
    assert {k: mstats[k] for k in ("steps", "admits", "looks")} == {k: gstats[k] for k in ("steps", "admits", "looks")}     # budgets only: one schedule
    for r in GREEDY_REQUESTS:
        assert mixed[r] == greedy[r], r
    for r in set(range(7)) - set(GREEDY_REQUESTS):             # the others keep their own stream whatever the neighbours want
        assert mixed[r] == sampled[r], r


def test_one_slot_falls_back_to_generate_with_the_requests_own_stream():
    from aki_amd import ops
    m, reqs = tiny(torch.bfloat16)
    params = [sampled_params(r) for r in range(7)]
    outs = m.generate_many(with_params(reqs, params), slots=1, eos_token_id=[])
    assert m.last_many_stats["per_request_generate"]
    for r, ((vx, lx), budget) in enumerate(zip(reqs, BUDGETS)):
        alone = generate_alone(m, vx, lx, max_new_tokens=budget, eos_token_id=[], do_sample=True, top_k=8, generator=ops.DeviceGenerator(seed_of(r)))
        assert outs[r].tolist() == alone.tolist(), r
    greedy, _ = call("greedy")
    assert any(o.tolist() != g for o, g in zip(outs, greedy))


def test_seeds_derived_from_a_device_generator():
    import aki_amd
    from aki_amd.slots import request_seed
    m, reqs = tiny(torch.bfloat16)
    base = 0xC0FFEE_0123_4567
    g = aki_amd.DeviceGenerator(base)
    default = aki_amd.RequestParams(do_sample=True, top_k=8)
    explicit = lambda off: [o.tolist() for o in m.generate_many(
        with_params(reqs, [aki_amd.RequestParams(do_sample=True, top_k=8, seed=request_seed(base, off, r)) for r in range(7)]),
        slots=SLOTS, eos_token_id=[])]
    first = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], params=default, generator=g)]
    assert g.offset == 1 and first == explicit(0)
    second = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], params=default, generator=g)]
    assert g.offset == 2 and second == explicit(1) and second != first
    m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], generator=g)      # nothing samples: the offset is bumped all the same
    assert g.offset == 3
    # without a generator the seeds come from torch's CPU generator on the host
    torch.manual_seed(5)
    a = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], params=default)]
    b = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], params=default)]
    torch.manual_seed(5)
    assert [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], params=default)] == a and a != b


def test_a_sampled_call_captures_once_and_never_syncs_per_token(monkeypatch):
    from aki_amd import ops
    from aki_amd.phi3 import DecodeGraph
    m, reqs = tiny(torch.bfloat16)
    captures, picks = [], []
    real, real_pick = DecodeGraph._capture, ops.sample_pick_rows
    monkeypatch.setattr(DecodeGraph, "_capture", lambda self: (captures.append(1), real(self))[1])
    monkeypatch.setattr(ops, "sample_pick_rows", lambda *a, **kw: (picks.append(a[0].shape[0]), real_pick(*a, **kw))[1])
    outs = m.generate_many(with_params(reqs, [sampled_params(r) for r in range(7)]), slots=SLOTS, eos_token_id=[])
    st = m.last_many_stats
    assert [o.tolist() for o in outs] == call("sampled")[0]
    assert len(captures) == 1
    assert st["steps"] > 8 and st["looks"] <= math.ceil(st["steps"] / 8) + st["admits"] + 1, st
    assert sorted(picks) == [1] * 7 + [SLOTS]                   # one pick per admit on row views, one inside the captured step


def test_a_greedy_call_takes_the_greedy_path(monkeypatch):
    """No request samples, none asks for log-probabilities: neither the per-row sampler nor ops.token_logprob is launched."""
    from aki_amd import ops

    def boom(*a, **kw):
        raise AssertionError("a greedy generate_many reached the sampler or the log-probability launch")

    m, reqs = tiny(torch.bfloat16)
    monkeypatch.setattr(ops, "sample_pick_rows", boom)
    monkeypatch.setattr(ops, "token_logprob", boom)
    outs = m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[])
    assert [o.tolist() for o in outs] == call("greedy")[0]


def test_sampled_requests_stop_at_an_eos():
    m, reqs = tiny(torch.bfloat16)
    eos, _ = references(torch.bfloat16)
    params = [sampled_params(r) for r in range(7)]
    outs = m.generate_many(with_params(reqs, params), slots=SLOTS, eos_token_id=[eos])
    check_structure(outs, BUDGETS, eos)
    free, _ = call("sampled")
    for r, (o, f) in enumerate(zip(outs, free)):                # up to its EOS a request draws what it draws without one
        assert o.tolist() == f[:len(o)], r


def test_a_sampled_request_on_an_f32_model_is_refused_before_any_launch(monkeypatch):
    from aki_amd import ops
    m, reqs = tiny(torch.float32)

    def boom(*a, **kw):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(ops, "kv_slot_admit", boom)
    monkeypatch.setattr(type(m), "_prefill_request", boom)
    monkeypatch.setattr(type(m), "generate", boom)
    for slots in (SLOTS, 1):
        with pytest.raises(ValueError, match="bf16"):
            m.generate_many(with_params(reqs, [sampled_params(r) for r in range(7)]), slots=slots, eos_token_id=[])


# ---- log-probabilities ----------------------------------------------------------------------------------------------------------------
def _logprob_params(mode, pattern, r):
    import aki_amd
    k = {"all0": 0, "all3": 3, "mixed": (3, 0, None)[r % 3]}[pattern]
    base = dict(do_sample=True, top_k=8, seed=seed_of(r)) if mode == "sampled" else {}
    return aki_amd.RequestParams(**base) if k is None else aki_amd.RequestParams(logprobs=True, top_logprobs=k, **base)


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_log_probabilities_per_request(mode):
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    plain, _ = call(mode)
    runs = {}
    for pattern in ("all0", "all3", "mixed"):
        params = [_logprob_params(mode, pattern, r) for r in range(7)]
        outs = m.generate_many(with_params(reqs, params), slots=SLOTS, eos_token_id=[])
        assert all(isinstance(o, aki_amd.AkiRequestOutput) for o in outs)
        assert [o.tokens.tolist() for o in outs] == plain, pattern          # bit-identical tokens with and without log-probabilities
        runs[pattern] = (params, outs)
    V = None
    for pattern, (params, outs) in runs.items():
        for r, (rp, o) in enumerate(zip(params, outs)):
            n = o.tokens.numel()
            if not rp.logprobs:                                             # did not ask: None fields
                assert o.logprobs is None and o.top_token_ids is None and o.top_logprobs is None
                continue
            assert o.logprobs.shape == (n,) and o.logprobs.dtype == torch.float32
            assert bool(torch.isfinite(o.logprobs).all()) and bool((o.logprobs <= 0).all())
            assert torch.equal(o.logprobs, runs["all3"][1][r].logprobs), (pattern, r)      # whatever top_logprobs the kernel ran with
            k = rp.top_logprobs
            if k == 0:
                assert o.top_token_ids is None and o.top_logprobs is None
                continue
            assert o.top_token_ids.shape == (n, k) and o.top_logprobs.shape == (n, k) and o.top_token_ids.dtype == torch.long
            assert bool((o.logprobs <= o.top_logprobs[:, 0]).all()) and bool((o.top_logprobs[:, :-1] >= o.top_logprobs[:, 1:]).all())
            assert bool((o.top_token_ids >= 0).all())
    # every request of the all3 call against the f32 log-softmax of its teacher-forced full forward: seven requests over three slots, so
    # the second and third occupant of a slot are checked against the columns their predecessors left
    for r, o in enumerate(runs["all3"][1]):
        full = teacher_forced_logits(r, o.tokens.tolist())
        V = full.shape[-1]
        want = torch.log_softmax(full, dim=-1)
        big = max(1.0, float(full.abs().max()))
        bar = 2 * LC.logprob_bound(big, V) + BF16_ROUTE_BAR * big
        err = (o.logprobs - want.gather(1, o.tokens[:, None])[:, 0]).abs().max().item()
        top_err = (o.top_logprobs - want.topk(3, dim=-1).values).abs().max().item()
        print(f"{mode} request {r}: max |logprob - full forward| = {err:.3g}, top-3 {top_err:.3g}, bar {bar:.3g}")
        assert err <= bar and top_err <= bar, (r, err, top_err, bar)


def test_log_probabilities_through_the_one_slot_fallback():
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    params = [_logprob_params("sampled", "mixed", r) for r in range(7)]
    outs = m.generate_many(with_params(reqs, params), slots=1, eos_token_id=[])
    plain = m.generate_many(with_params(reqs, [sampled_params(r) for r in range(7)]), slots=1, eos_token_id=[])
    for r, (rp, o, p) in enumerate(zip(params, outs, plain)):
        assert isinstance(o, aki_amd.AkiRequestOutput) and o.tokens.tolist() == p.tolist()
        n = o.tokens.numel()
        if not rp.logprobs:
            assert o.logprobs is None and o.top_logprobs is None
        else:
            assert o.logprobs.shape == (n,) and bool((o.logprobs <= 0).all())
            assert (o.top_logprobs is None) if rp.top_logprobs == 0 else (o.top_logprobs.shape == (n, rp.top_logprobs))
