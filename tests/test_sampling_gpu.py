"""The device sampler on the GPU: ops.sample_pick against the float64 reference of tests/sampling_cases.py on every case, and
`generate(..., do_sample=True, generator=DeviceGenerator(seed))` on the tiny full-width model.  Every test here needs the feature."""
import numpy as np
import pytest
import torch

import sampling_cases as S
from test_decode_gpu import _tiny_full_width_aki
from test_logits_processors_gpu import _multi

pytestmark = pytest.mark.gpu
DEV = "cuda"

# probs_out against float64: expf is within 1 ulp (2 eps) and its argument y - max carries |y - max| eps; the f32 total is within DELTA / 2
# of float64 in relative terms (tests/test_sampling_cases_cpu.py) and the division adds one rounding.  |y - max| < 104 for a non-zero f32
# weight, but only weights above 1e-30 (|y - max| < 70) are compared: (2 + 70 + 1) 2^-24 + 1e-6 < 6e-6.
PROBS_RTOL = 6e-6


def _setup(c):
    """bf16 logits [ROWS, V] (the case's row on every row), processors and the token buffer that carries the case's history."""
    from aki_amd import ops
    x = torch.from_numpy(S.logits(c)).to(DEV).to(torch.bfloat16)[None].repeat(S.ROWS, 1).contiguous()
    proc = None
    H = len(c.history)
    tokens = torch.zeros((S.ROWS, H + S.STEPS), dtype=torch.long, device=DEV)
    if c.processed:
        proc = ops.LogitsProcessors(c.V, DEV, repetition_penalty=c.penalty, suppress_tokens=list(c.suppress))
        tokens[:, :H] = torch.tensor(c.history, dtype=torch.long, device=DEV)
        tokens[:, H:] = c.history[0]                  # what the picks append must not change the set of penalised tokens
    return x, proc, tokens


def _run_draws(c, x, proc, tokens, **kw):
    """The case's 2000 draws: ids [len(OFFSETS), STEPS, ROWS]."""
    from aki_amd import ops
    out = torch.zeros((len(S.OFFSETS), S.STEPS, S.ROWS), dtype=torch.long, device=DEV)
    H = len(c.history)
    for oi, off in enumerate(S.OFFSETS):
        for st in range(S.STEPS):
            tk = tokens.clone()
            ops.sample_pick(x, out[oi, st], tokens=tk, step=H + st, processors=proc, temperature=c.T, top_k=c.k, top_p=c.p, seed=S.SEED,
                            offset=off, **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("c", S.cases(), ids=lambda c: c.name)
def test_kernel_draws_are_accepted(c):
    from aki_amd import ops
    x, proc, tokens = _setup(c)
    r = S.reference(c)
    got = _run_draws(c, x, proc, tokens)
    u = S.uniform(*S.draws(c))
    ok = S.accepted(r, got, u)
    assert got.size >= 2000 and ok.all(), (int((~ok).sum()), got[~ok][:8].tolist(), u[~ok][:8].tolist())
    # the distribution the draw was made from, and bit-equal repeats
    probs = torch.full((S.ROWS, c.V), -1.0, dtype=torch.float32, device=DEV)
    ids = torch.zeros(S.ROWS, dtype=torch.long, device=DEV)
    H = len(c.history)
    ops.sample_pick(x, ids, tokens=tokens.clone(), step=H + 3, processors=proc, temperature=c.T, top_k=c.k, top_p=c.p, seed=S.SEED, offset=5,
                    probs_out=probs)
    probs2, ids2 = torch.full_like(probs, -1.0), torch.zeros_like(ids)
    ops.sample_pick(x, ids2, tokens=tokens.clone(), step=H + 3, processors=proc, temperature=c.T, top_k=c.k, top_p=c.p, seed=S.SEED, offset=5,
                    probs_out=probs2)
    assert torch.equal(ids, ids2) and torch.equal(probs, probs2)
    assert np.array_equal(ids.cpu().numpy(), got[S.OFFSETS.index(5), 3])
    pr = probs.cpu().numpy().astype(np.float64)
    for b in range(S.ROWS):
        if c.k == 1:                                        # the greedy rows: one-hot on the greedy pick
            assert pr[b].sum() == 1.0 and pr[b, int(ids[b])] == 1.0
            continue
        assert (pr[b][~r.kept] == 0).all() and (pr[b][r.kept & (r.probs > 1e-37)] > 0).all()
        big = r.probs > 1e-30
        assert np.abs(pr[b][big] / r.probs[big] - 1.0).max() <= PROBS_RTOL
    # top_k = 1 and top_p = 1e-6 are the greedy pick
    if c.k == 1 or c.p <= 1e-6:
        want = torch.zeros(S.ROWS, dtype=torch.long, device=DEV)
        ops.greedy_pick(x, want, tokens=tokens.clone(), processors=proc, cache_len=torch.full((S.ROWS,), H, dtype=torch.int32, device=DEV))
        assert (torch.from_numpy(got).to(DEV) == want[None, None, :]).all()


@pytest.mark.parametrize("name", ["main-s2-T0.7-k50-p0.9", "proc-T1.3-k0-p0.9", "small-proc", "main-s4-T1-k1-p1"])
def test_bookkeeping_is_the_greedy_picks(name):
    """tokens, done, done_at, cache_len, next ids and the embedding row: what greedy_pick writes when its argmax is the sampled id.  Row 2
    is finished before the launch (takes pad), row 5's id is made an eos id."""
    from aki_amd import ops
    c = next(k for k in S.cases() if k.name == name)
    x, proc, tokens = _setup(c)
    H, B, d = len(c.history), S.ROWS, 64
    g = torch.Generator(device="cpu").manual_seed(1)
    table = torch.randn((c.V - 100, d), generator=g).to(DEV, torch.bfloat16)
    extra = torch.randn((100, d), generator=g).to(DEV, torch.bfloat16)
    embed = (table, extra, c.V - 101)
    probe = torch.zeros(B, dtype=torch.long, device=DEV)
    start = torch.tensor([7, 3, 0, 5, 1, 2, 9, 4], dtype=torch.int32, device=DEV)
    ops.sample_pick(x, probe, tokens=tokens.clone(), cache_len=start + H + 2, start_len=start, advance=True, processors=proc,
                    temperature=c.T, top_k=c.k, top_p=c.p, seed=S.SEED, offset=2)
    eos = torch.tensor([int(probe[5]), c.V + 5], dtype=torch.long, device=DEV)

    def run(op, logits, **kw):
        st = dict(ids=torch.zeros(B, dtype=torch.long, device=DEV), tokens=tokens.clone(), done=torch.zeros(B, dtype=torch.uint8, device=DEV),
                  done_at=torch.full((B,), -1, dtype=torch.int32, device=DEV), cache_len=(start + H + 2).clone(),
                  emb=torch.zeros((B, d), dtype=torch.bfloat16, device=DEV))
        st["done"][2] = 1
        op(logits, st["ids"], pad_token_id=11, eos_ids=eos, done=st["done"], tokens=st["tokens"], cache_len=st["cache_len"], start_len=start,
           advance=True, done_at=st["done_at"], embed=embed, next_embeds=st["emb"], **kw)
        return st

    a = run(ops.sample_pick, x, processors=proc, temperature=c.T, top_k=c.k, top_p=c.p, seed=S.SEED, offset=2)
    onehot = torch.zeros((B, c.V), dtype=torch.bfloat16, device=DEV)
    onehot[torch.arange(B), probe] = 1.0
    w = run(ops.greedy_pick, onehot)
    assert int(a["ids"][2]) == 11 and int(a["done"][5]) == 1 and int(a["done_at"][5]) == H + 3
    unfinished = [b for b in range(B) if b != 2]
    assert torch.equal(a["ids"][unfinished], probe[unfinished])
    for k in a:
        assert torch.equal(a[k], w[k]), k


def test_host_validation():
    from aki_amd import ops
    x = torch.zeros((2, 64), dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros(2, dtype=torch.long, device=DEV)
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1)):
        with pytest.raises(ValueError):
            ops.sample_pick(x, ids, **kw)
    with pytest.raises(ops.AkiError):
        ops.sample_pick(x.float(), ids)


def _case_for(row_logits, T, k, p):
    """The reference on one row of raw logits (no processors)."""
    x = row_logits.float().cpu().numpy()
    c = S.Case("generate-row", len(x), 0.0, T, k, p)
    return S.reference(c, x)


GEN = dict(max_new_tokens=20, do_sample=True, temperature=0.8, top_k=50, top_p=0.9, eos_token_id=[])


def _gen(m, vx, ids, am, seed=5, gen=None, **kw):
    import aki_amd
    g = aki_amd.DeviceGenerator(seed) if gen is None else gen
    return m.generate(vx, ids, attention_mask=am, generator=g, **dict(GEN, **kw))


@pytest.mark.parametrize("B", [1, 3])
def test_generate_seeds_offsets_and_graph(B):
    import aki_amd
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, B)
    a, b = _gen(m, vx, ids, am), _gen(m, vx, ids, am)
    assert a.shape == (B, 20) and torch.equal(a, b)
    assert not torch.equal(a, _gen(m, vx, ids, am, seed=6))
    g = aki_amd.DeviceGenerator(5)
    first, second = _gen(m, vx, ids, am, gen=g), _gen(m, vx, ids, am, gen=g)
    assert torch.equal(first, a) and not torch.equal(second, a) and g.offset == 2
    assert torch.equal(_gen(m, vx, ids, am, gen=g.manual_seed(5)), a)
    for ug in (False, True):
        assert torch.equal(_gen(m, vx, ids, am, use_graph=ug), a), ug


def test_generate_rows_are_the_kernel_level_restatement(monkeypatch):
    """Every token of every row of a batch: accepted by the reference fed the logits that row was drawn from, with the draw of
    (token index, row, offset) - so a row's tokens do not depend on the rest of the batch's."""
    import aki_amd
    from aki_amd import ops
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, 3)
    seen = []
    orig = ops.sample_pick

    def spy(logits, next_ids, **kw):
        out = orig(logits, next_ids, **kw)
        seen.append((logits.clone(), kw["step"], out.clone()))
        return out

    monkeypatch.setattr(ops, "sample_pick", spy)
    g = aki_amd.DeviceGenerator(S.SEED)
    g.offset = 4
    toks = m.generate(vx, ids, attention_mask=am, generator=g, use_graph=False, **GEN)
    assert len(seen) == 20
    checked = 0
    for lg, step, out in seen:
        assert torch.equal(out, toks[:, step])
        for b in range(3):
            r = _case_for(lg[b], 0.8, 50, 0.9)
            if r.boundary_gap <= 8 * S.DELTA:
                continue
            u = S.uniform(np.int64(step), np.int64(b), np.int64(4))
            assert S.accepted(r, np.asarray(int(out[b])), u), (step, b)
            checked += 1
    assert checked >= 50
    monkeypatch.setattr(ops, "sample_pick", orig)
    g2 = aki_amd.DeviceGenerator(S.SEED)
    g2.offset = 4
    assert torch.equal(m.generate(vx, ids, attention_mask=am, generator=g2, use_graph=True, **GEN), toks)


def test_generate_eos_stops_and_pads_as_greedy_does():
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, 3)
    free = _gen(m, vx, ids, am)
    eos = [int(free[0, 4])]
    for ug in (False, True):
        got = _gen(m, vx, ids, am, eos_token_id=eos, pad_token_id=0, use_graph=ug)
        stop = [row.index(eos[0]) if eos[0] in row else None for row in free.tolist()]
        width = 20 if any(s is None for s in stop) else max(stop) + 1
        assert got.shape[1] == width
        for b, s in enumerate(stop):
            end = width if s is None else s + 1
            assert got[b, :end].tolist() == free[b, :end].tolist() and (got[b, end:] == 0).all(), (ug, b)


@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_honours_the_processors(use_graph):
    m, vx, ids, am = _tiny_full_width_aki()
    free = _gen(m, vx, ids, am, top_k=3, top_p=1.0, use_graph=use_graph)[0].tolist()
    ban = max(set(free), key=free.count)
    toks = _gen(m, vx, ids, am, top_k=3, top_p=1.0, use_graph=use_graph, no_repeat_ngram_size=1, suppress_tokens=[ban])[0].tolist()
    assert len(toks) == 20 and len(set(toks)) == 20 and ban not in toks, toks


def test_generate_with_the_fp8_kv_cache():
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, 3)
    m.lang_model.set_kv_cache_dtype("fp8_e4m3")
    try:
        a = _gen(m, vx, ids, am, use_graph=True)
        assert a.shape == (3, 20) and torch.equal(a, _gen(m, vx, ids, am, use_graph=True)) and torch.equal(a, _gen(m, vx, ids, am, use_graph=False))
    finally:
        m.lang_model.set_kv_cache_dtype("bf16")


def test_chain_recovery_returns_the_unfaulted_tokens():
    from aki_amd import _lib
    m, vx, ids, am = _tiny_full_width_aki()
    kw = dict(max_new_tokens=24, no_repeat_ngram_size=2, repetition_penalty=1.3)
    m.lang_model.model.use_decode_chain = False
    want = _gen(m, vx, ids, am, **kw)
    m.lang_model.model.use_decode_chain = True
    with _lib.use_lab(0) as lab:
        clean = _gen(m, vx, ids, am, **kw)
        assert torch.equal(clean, want)
        lab.aki_lab_set_chain_fault((1 << 8) | 3, 11)
        with pytest.warns(RuntimeWarning, match="decode chain"):
            got = _gen(m, vx, ids, am, **kw)
        lab.aki_lab_set_chain_fault(0, 0)
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def test_invalid_combinations_and_the_torch_generator_path(monkeypatch):
    import aki_amd
    import aki_amd.aki as A
    m, vx, ids, am = _tiny_full_width_aki()
    g = aki_amd.DeviceGenerator(1)
    with pytest.raises(ValueError):
        m.generate(vx, ids, attention_mask=am, max_new_tokens=4, do_sample=False, generator=g)
    with pytest.raises(ValueError):
        m.generate(vx, ids, attention_mask=am, max_new_tokens=4, do_sample=True, num_beams=2, generator=g)
    with pytest.raises(ValueError):
        m.generate(vx, ids, attention_mask=am, max_new_tokens=4, do_sample=True, top_p=0.0, generator=g)
    assert g.offset == 0
    calls = []
    orig = A.sample_next
    monkeypatch.setattr(A, "sample_next", lambda *a, **k: calls.append(1) or orig(*a, **k))
    tg = torch.Generator(device=DEV).manual_seed(11)
    m.generate(vx, ids, attention_mask=am, max_new_tokens=6, eos_token_id=[], do_sample=True, top_k=20, generator=tg)
    assert len(calls) == 6
    m.generate(vx, ids, attention_mask=am, max_new_tokens=6, eos_token_id=[], do_sample=True, top_k=20, generator=g)
    assert len(calls) == 6 and g.offset == 1
