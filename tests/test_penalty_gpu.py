"""min_p and the frequency / presence penalties on the GPU: every case of tests/penalty_cases.py through the process, greedy-pick and
sample-pick entry points (scores bit-equal to the f32 restatement, the support of probs_out equal to the reference's kept set, every
draw accepted, repeats bit-identical), the per-row form against scalar launches, and generate / generate_many on the tiny models.
Every test here needs the feature: on the parent commit the keywords are refused."""
import numpy as np
import pytest
import torch

import penalty_cases as P
import sampling_cases as S
from test_decode_gpu import _tiny_full_width_aki
from test_logits_processors_gpu import _multi, _teacher_forced_check
from test_sampling_gpu import PROBS_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 11


def _bits(t):
    return t.contiguous().view(torch.int32)


def _setup(c):
    """bf16 logits [ROWS, V] (the case's row on every row), the processors, the token buffer with the case's history on every row and
    the finished flags (rows P.DONE_ROWS of a `done` case)."""
    from aki_amd import ops
    x = torch.from_numpy(P.logits(c)).to(DEV).to(torch.bfloat16)[None].repeat(S.ROWS, 1).contiguous()
    proc = None
    if c.processed:
        proc = ops.LogitsProcessors(c.V, DEV, repetition_penalty=c.penalty, suppress_tokens=list(c.suppress), frequency_penalty=c.frequency,
                                    presence_penalty=c.presence)
    tokens = torch.from_numpy(P.history(c)).to(DEV)[None].repeat(S.ROWS, 1).contiguous()
    done = None
    if c.done:
        done = torch.zeros(S.ROWS, dtype=torch.uint8, device=DEV)
        done[list(P.DONE_ROWS)] = 1
    return x, proc, tokens, done


def _sample(c, x, proc, tokens, done, out, step, offset, **kw):
    from aki_amd import ops
    return ops.sample_pick(x, out, pad_token_id=PAD, tokens=tokens.clone(), done=None if done is None else done.clone(), step=step,
                           processors=proc, temperature=c.T, top_k=c.k, top_p=c.p, seed=S.SEED, offset=offset, min_p=c.min_p, **kw)


def _expected_scores(c):
    """f32 [ROWS, V]: the restatement on live rows, the plain copy on finished ones."""
    live, plain = P.scores(c), P.logits(c).astype(np.float32)
    rows = [plain if c.done and b in P.DONE_ROWS else live for b in range(S.ROWS)]
    return torch.from_numpy(np.stack(rows)).to(DEV)


@pytest.mark.parametrize("c", P.cases(), ids=lambda c: c.name)
def test_kernel_draws_are_accepted(c):
    x, proc, tokens, done = _setup(c)
    r = P.reference(c)
    H = len(c.history)
    got = torch.zeros((len(S.OFFSETS), S.STEPS, S.ROWS), dtype=torch.long, device=DEV)
    for oi, off in enumerate(S.OFFSETS):
        for st in range(S.STEPS):
            _sample(c, x, proc, tokens, done, got[oi, st], H + st, off)
    got = got.cpu().numpy()
    u = S.uniform(*S.draws(c))
    live = [b for b in range(S.ROWS) if not (c.done and b in P.DONE_ROWS)]
    ok = S.accepted(r, got[..., live], u[..., live])
    assert got.size >= 2000 and ok.all(), (int((~ok).sum()), got[..., live][~ok][:8].tolist(), u[..., live][~ok][:8].tolist())
    if c.done:
        assert (got[..., list(P.DONE_ROWS)] == PAD).all()
    # the distribution the draw was made from: its support is the reference's kept set; and bit-equal repeats
    runs = []
    for _ in range(2):
        probs = torch.full((S.ROWS, c.V), -1.0, dtype=torch.float32, device=DEV)
        ids = torch.zeros(S.ROWS, dtype=torch.long, device=DEV)
        _sample(c, x, proc, tokens, done, ids, H + 3, 5, probs_out=probs)
        runs.append((ids, probs))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert np.array_equal(runs[0][0].cpu().numpy(), got[S.OFFSETS.index(5), 3])
    pr = runs[0][1].cpu().numpy().astype(np.float64)
    for b in live:
        assert (pr[b][~r.kept] == 0).all() and (pr[b][r.kept & (r.probs > 1e-37)] > 0).all(), (b, int((pr[b] > 0).sum()), int(r.kept.sum()))
        big = r.probs > 1e-30
        assert np.abs(pr[b][big] / r.probs[big] - 1.0).max() <= PROBS_RTOL
    for b in set(range(S.ROWS)) - set(live):
        assert (pr[b] == 0).all()


@pytest.mark.parametrize("c", [k for k in P.cases() if k.processed], ids=lambda c: c.name)
def test_processed_scores_are_the_f32_restatement(c):
    """Bit for bit, through the three entry points: aki_logits_process_penalized, and the scores scratch of aki_greedy_pick_penalized and
    of aki_sample_pick_penalized at T = 1 (x / 1 is x).  A case without the additive penalties takes the entry points it always took: the
    restatement holds there too."""
    from aki_amd import ops
    x, proc, tokens, done = _setup(c)
    want = _expected_scores(c)
    H = len(c.history)
    n = torch.full((S.ROWS,), H, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        outs.append(proc.apply(x, tokens=tokens.clone(), step=H, done=done))
    assert torch.equal(_bits(outs[0]), _bits(want)), int((_bits(outs[0]) != _bits(want)).sum())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    by_cache_len = proc.apply(x, tokens=tokens.clone(), cache_len=n + 7, start_len=torch.full_like(n, 7), done=done)
    assert torch.equal(_bits(by_cache_len), _bits(want))
    ids = torch.zeros(S.ROWS, dtype=torch.long, device=DEV)
    ops.greedy_pick(x, ids, pad_token_id=PAD, tokens=tokens.clone(), cache_len=n.clone(), done=None if done is None else done.clone(), processors=proc)
    assert torch.equal(_bits(proc.scores(S.ROWS, x.device)[:, :c.V]), _bits(want))
    best = want.cpu().numpy().argmax(axis=-1)               # the lowest index among equal maxima, as the pick's ordering
    for b in range(S.ROWS):
        assert int(ids[b]) == (PAD if c.done and b in P.DONE_ROWS else int(best[b]))
    ops.sample_pick(x, ids, pad_token_id=PAD, tokens=tokens.clone(), done=None if done is None else done.clone(), step=H, processors=proc,
                    temperature=1.0, top_k=c.k, top_p=c.p, seed=S.SEED, offset=1, min_p=c.min_p)
    assert torch.equal(_bits(proc.scores(S.ROWS, x.device)[:, :c.V]), _bits(want))


# ---- the per-row form ------------------------------------------------------------------------------------------------------------------------
ROW_VALUES = [  # (min_p, frequency, presence, repetition penalty, temperature, top_k, top_p)
    (0.0, 0.0, 0.0, 1.0, 1.0, 0, 1.0), (0.1, 0.0, 0.0, 1.0, 0.7, 50, 0.9), (0.0, 0.7, 0.0, 1.0, 1.0, 50, 1.0), (0.0, 0.0, -1.5, 1.3, 1.3, 0, 0.9),
    (0.5, 0.3, 0.6, 1.3, 1.0, 1000, 0.5), (1.0, 2.0, 2.0, 1.0, 0.7, 0, 1.0), (0.02, -0.7, 1.1, 1.0, 1.3, 50, 0.9), (0.3, 0.25, 0.0, 1.3, 1.0, 0, 1.0)]


@pytest.mark.parametrize("V", [S.V_MAIN, S.V_SMALL])
def test_eight_rows_in_one_launch_are_eight_scalar_launches(V):
    """sample_pick_rows / greedy_pick / ProcessorSets.apply with a different (min_p, frequency, presence) on every row: row by row the ids,
    probs and scores bits of a B = 1 scalar launch with that row's values (key = the row's seed, offset 0: the same stream)."""
    from aki_amd import ops
    from aki_amd.slots import NEUTRAL_SET_KEY
    B, H = len(ROW_VALUES), 41
    g = np.random.default_rng(V)
    x = torch.from_numpy(S.bf16_round(g.standard_normal((B, V)).astype(np.float32) * 2)).to(DEV).to(torch.bfloat16).contiguous()
    hist = g.integers(0, 24, (B, H)).astype(np.int64) * 13           # 24 distinct ids: every row repeats some
    hist[:, 5] = V + 3
    tokens = torch.cat([torch.from_numpy(hist), torch.full((B, 2), V + 7, dtype=torch.long)], 1).to(DEV)
    rep_key = (float(np.float32(1.3)),) + NEUTRAL_SET_KEY[1:]
    ps = ops.ProcessorSets(V, DEV, [], [rep_key], B)
    col = lambda i, dt: torch.tensor([r[i] for r in ROW_VALUES], dtype=dt, device=DEV)
    mp, fq, pr = col(0, torch.float32), col(1, torch.float32), col(2, torch.float32)
    ps.row_set.copy_(torch.tensor([ps.index[rep_key] if r[3] != 1.0 else 0 for r in ROW_VALUES], dtype=torch.int32))
    seeds = torch.tensor([S.SEED + 977 * b for b in range(B)], dtype=torch.int64, device=DEV)
    rows = dict(temperature=col(4, torch.float32), top_k=col(5, torch.int32), top_p=col(6, torch.float32), seed=seeds)
    pen = dict(frequency_penalty=fq, presence_penalty=pr)
    ids, probs = torch.zeros(B, dtype=torch.long, device=DEV), torch.zeros((B, V), dtype=torch.float32, device=DEV)
    ops.sample_pick_rows(x, ids, tokens=tokens.clone(), step=H, processor_sets=ps, probs_out=probs, min_p=mp, **rows, **pen)
    y = ps.scores(B, x.device)[:, :V].clone()
    gids = torch.zeros(B, dtype=torch.long, device=DEV)
    ops.greedy_pick(x, gids, tokens=tokens.clone(), cache_len=torch.full((B,), H, dtype=torch.int32, device=DEV), processor_sets=ps, **pen)
    gsc = ps.scores(B, x.device)[:, :V].clone()
    applied = ps.apply(x, tokens=tokens.clone(), step=H, **pen).clone()
    assert torch.equal(_bits(applied), _bits(gsc))
    for b, (m_, f_, p_, rep, T, k, tp) in enumerate(ROW_VALUES):
        proc = ops.LogitsProcessors(V, DEV, repetition_penalty=rep, frequency_penalty=f_, presence_penalty=p_)
        one, pr1 = torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros((1, V), dtype=torch.float32, device=DEV)
        sc1 = torch.zeros((1, (V + 3) // 4 * 4), dtype=torch.float32, device=DEV)
        ops.sample_pick(x[b:b + 1], one, tokens=tokens[b:b + 1].clone(), step=H, processors=proc, temperature=T, top_k=k, top_p=tp,
                        seed=S.SEED + 977 * b, offset=0, probs_out=pr1, scores=sc1, min_p=m_)
        assert int(one[0]) == int(ids[b]), b
        assert torch.equal(_bits(pr1[0]), _bits(probs[b])), b
        assert torch.equal(_bits(sc1[0, :V]), _bits(y[b])), b
        if proc.active:
            want = proc.apply(x[b:b + 1], tokens=tokens[b:b + 1].clone(), step=H)
            assert torch.equal(_bits(want[0]), _bits(gsc[b])), b
            assert int(gids[b]) == int(want[0].cpu().numpy().argmax())
        else:
            assert torch.equal(_bits(x[b].float()), _bits(gsc[b])), b


def test_bad_bits_stay_in_their_row():
    """Nothing validates the arrays on the device: a min_p outside (0, 1] is no filter and a penalty that is not finite reads as 0 - the
    row is the row of a launch with zeros there, and its neighbours are untouched."""
    from aki_amd import ops
    from aki_amd.slots import NEUTRAL_SET_KEY
    V, B, H = S.V_SMALL, 4, 9
    g = np.random.default_rng(5)
    x = torch.from_numpy(S.bf16_round(g.standard_normal((B, V)).astype(np.float32) * 2)).to(DEV).to(torch.bfloat16).contiguous()
    tokens = torch.from_numpy(g.integers(0, 6, (B, H + 1)).astype(np.int64)).to(DEV)
    ps = ops.ProcessorSets(V, DEV, [], [NEUTRAL_SET_KEY], B)
    rows = dict(temperature=torch.ones(B, device=DEV), top_k=torch.zeros(B, dtype=torch.int32, device=DEV), top_p=torch.ones(B, device=DEV),
                seed=torch.arange(B, dtype=torch.int64, device=DEV) + 3)
    nan, inf = float("nan"), float("inf")

    def run(mp, fq, pr):
        ids, probs = torch.zeros(B, dtype=torch.long, device=DEV), torch.zeros((B, V), dtype=torch.float32, device=DEV)
        t = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
        ops.sample_pick_rows(x, ids, tokens=tokens.clone(), step=H, processor_sets=ps, probs_out=probs, min_p=t(mp), frequency_penalty=t(fq),
                             presence_penalty=t(pr), **rows)
        return ids, probs, ps.scores(B, x.device)[:, :V].clone()

    bad = run([nan, 1.5, -0.2, 0.1], [inf, 0.5, nan, 0.5], [0.5, -inf, nan, 0.5])
    clean = run([0.0, 0.0, 0.0, 0.1], [0.0, 0.5, 0.0, 0.5], [0.5, 0.0, 0.0, 0.5])
    for a, b in zip(bad, clean):
        assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)


# ---- generate on the tiny full-width model ---------------------------------------------------------------------------------------------------
PEN_KW = dict(frequency_penalty=0.8, presence_penalty=0.6, repetition_penalty=1.2)


def _restated(history, lg):
    """_teacher_forced_check's processor: the f32 restatement on one row of raw logits with the emitted prefix as history."""
    V = lg.shape[-1]
    c = P.Case("generate-row", V, 0.0, 1.0, 0, 1.0, penalty=PEN_KW["repetition_penalty"], history=tuple(history[0].tolist()),
               frequency=PEN_KW["frequency_penalty"], presence=PEN_KW["presence_penalty"])
    return torch.from_numpy(P.scores(c, lg[0].numpy()))[None]


@pytest.mark.parametrize("B", [1, 3])
def test_greedy_generate_is_teacher_forced_right_and_replays_equal(B):
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, B)
    base = dict(attention_mask=am, max_new_tokens=16, eos_token_id=[])
    plain = m.generate(vx, ids, **base)
    eager = m.generate(vx, ids, use_graph=False, **base, **PEN_KW)
    replayed = m.generate(vx, ids, use_graph=True, **base, **PEN_KW)
    assert torch.equal(eager, replayed) and eager.shape == (B, 16)
    assert not torch.equal(eager, plain), "the penalties change nothing on these prompts: the test would show nothing"
    assert _teacher_forced_check(m, vx, ids, eager, _restated) >= B * 2


def test_sampled_generate_stays_inside_the_min_p_set(monkeypatch):
    """Every token of every row lies inside the reference's kept set for the logits its step was drawn from, wherever the row is clear
    of the min_p and top-p boundaries; the replayed graph draws the same tokens."""
    import aki_amd
    from aki_amd import ops
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, 3)
    kw = dict(max_new_tokens=20, do_sample=True, temperature=0.8, top_k=50, top_p=0.9, eos_token_id=[])
    extra = {"min_p": 0.2}
    seen = []
    orig = ops.sample_pick

    def spy(logits, next_ids, **k):
        out = orig(logits, next_ids, **k)
        seen.append((logits.clone(), k["step"], out.clone(), k.get("min_p")))
        return out

    monkeypatch.setattr(ops, "sample_pick", spy)
    toks = m.generate(vx, ids, attention_mask=am, generator=aki_amd.DeviceGenerator(S.SEED), use_graph=False, **kw, **extra)
    monkeypatch.setattr(ops, "sample_pick", orig)
    assert len(seen) == 20 and all(s[3] == float(np.float32(extra["min_p"])) for s in seen)
    checked = dropped = 0
    for lg, step, out, _ in seen:
        assert torch.equal(out, toks[:, step])
        for b in range(3):
            c = P.Case("generate-row", lg.shape[1], 0.0, 0.8, 50, 0.9, min_p=extra["min_p"])
            row = lg[b].float().cpu().numpy()
            r, base = P.reference(c, row), S.reference(c, row)
            if base.boundary_gap <= 8 * S.DELTA or P.facts(c, row).minp_gap <= P.MINP_MARGIN:
                continue
            assert r.kept[int(out[b])], (step, b)
            assert S.accepted(r, np.asarray(int(out[b])), S.uniform(np.int64(step), np.int64(b), np.int64(0))), (step, b)
            checked += 1
            dropped += int(base.kept.sum() - r.kept.sum())
    assert checked >= 50 and dropped > 0, (checked, dropped)
    again = m.generate(vx, ids, attention_mask=am, generator=aki_amd.DeviceGenerator(S.SEED), use_graph=True, **kw, **extra)
    assert torch.equal(again, toks)
    free = m.generate(vx, ids, attention_mask=am, generator=aki_amd.DeviceGenerator(S.SEED), use_graph=True, **kw)
    assert not torch.equal(free, toks), "min_p changes nothing on these prompts: the test would show nothing"


def test_torch_generator_loop_and_f32_model_take_the_keywords(monkeypatch):
    """The host loops: sample_next's min_p behind top-p under a torch.Generator, and the f32 model's torch pick over the kernel's scores."""
    import aki_amd.aki as A
    from test_model_gpu import batch, build_tiny
    m, vx, ids, am = _tiny_full_width_aki()
    kw = dict(max_new_tokens=8, do_sample=True, top_k=50, eos_token_id=[])
    extra = {"min_p": 1.0}                                   # only the row's maxima survive
    seen = []
    orig = A.sample_next

    def spy(x, *a, **k):
        tok = orig(x, *a, **k)
        seen.append((x.float().clone(), tok.clone(), a[4] if len(a) > 4 else k.get("min_p")))
        return tok

    monkeypatch.setattr(A, "sample_next", spy)
    tg = torch.Generator(device=DEV).manual_seed(11)
    sampled = m.generate(vx, ids, attention_mask=am, generator=tg, **kw, **extra)
    monkeypatch.setattr(A, "sample_next", orig)
    assert len(seen) == 8 and sampled.shape == (1, 8)
    for x, tok, mp in seen:
        assert mp == 1.0 and bool((x.gather(1, tok[:, None])[:, 0] == x.max(dim=-1).values).all())
    m32, g = build_tiny(torch.float32)
    vx32, lx32, am32, _ = batch(g, torch.float32)
    base = dict(attention_mask=am32, max_new_tokens=10, eos_token_id=[])
    plain = m32.generate(vx32, lx32, **base)
    a = m32.generate(vx32, lx32, use_graph=False, **base, **PEN_KW)
    b = m32.generate(vx32, lx32, use_graph=True, **base, **PEN_KW)
    assert torch.equal(a, b) and not torch.equal(a, plain)


# ---- generate_many ---------------------------------------------------------------------------------------------------------------------------
def test_generate_many_requests_equal_generate_alone():
    """Seven requests that mix all three values over 4 slots (slots are refilled): each request's tokens are generate()'s for that request
    alone with the same seed and values.  (The model is the generate tests' full-width one.  The step's logits at 4 rows and at 1 row
    come from different bf16 GEMM kernels, so the equality rests on these prompts' margins, as it does wherever the suite compares a
    queue with generate() alone; what the values themselves change is held bit for bit by the kernel-level tests above.)"""
    import aki_amd
    from aki_amd import ops
    from test_slots_gpu import BUDGETS
    m, vx7, ids7, am7 = _tiny_full_width_aki()
    vx7, ids7, am7 = _multi(m, vx7, ids7, am7, 7)
    assert bool(am7.all()), "the prompts carry no padding: a request is its row as it stands"
    reqs = [(vx7[b:b + 1], ids7[b:b + 1]) for b in range(7)]
    with_budgets = lambda rs: [(vx, lx, b) for (vx, lx), b in zip(rs, BUDGETS)]
    generate_alone = lambda m_, vx, lx, **kw: m_.generate(vx, lx, attention_mask=torch.ones_like(lx), **kw)[0]
    seed = lambda r: S.SEED + 31 * r
    own = [dict(frequency_penalty=1.2), dict(presence_penalty=1.0), dict(do_sample=True, top_k=8, min_p=0.3),
           dict(do_sample=True, top_k=8, min_p=0.1, frequency_penalty=0.9, presence_penalty=0.5), dict(presence_penalty=-1.0, min_p=0.5),
           dict(do_sample=True, top_k=8), dict(frequency_penalty=0.6, presence_penalty=0.4, repetition_penalty=1.3)]
    params = [aki_amd.RequestParams(seed=seed(r) if s.get("do_sample") else None, **s) for r, s in enumerate(own)]
    queue = [(vx, lx, b, p) for (vx, lx), b, p in zip(reqs, BUDGETS, params)]
    outs = [o.tolist() for o in m.generate_many(queue, slots=4, eos_token_id=[])]
    stats = dict(m.last_many_stats)
    assert stats["slots"] == 4 and stats["admits"] == 7 and not stats.get("per_request_generate")
    plain = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=4, eos_token_id=[])]
    assert sum(a != b for a, b in zip(outs, plain)) >= 3, "the values change nothing on these prompts: the test would show nothing"
    for r, ((vx, lx), budget, s) in enumerate(zip(reqs, BUDGETS, own)):
        kw = dict(s)
        if kw.get("do_sample"):
            kw["generator"] = ops.DeviceGenerator(seed(r))
        alone = generate_alone(m, vx, lx, max_new_tokens=budget, eos_token_id=[], **kw)
        assert outs[r] == alone.tolist(), (r, outs[r], alone.tolist())
    # the call-wide keyword is the default of a request that sets nothing; an explicit 0.0 belongs to the request
    wide = {"frequency_penalty": 1.2}
    mixed = [aki_amd.RequestParams(), aki_amd.RequestParams(frequency_penalty=0.0)] + [aki_amd.RequestParams()] * 5
    got = [o.tolist() for o in m.generate_many([(vx, lx, b, p) for (vx, lx), b, p in zip(reqs, BUDGETS, mixed)], slots=4, eos_token_id=[], **wide)]
    assert got[0] == outs[0] and got[1] == plain[1]
