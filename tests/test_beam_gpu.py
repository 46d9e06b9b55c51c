"""Beam search on the device: ops.beam_logprob, ops.beam_step and ops.kv_beam_reorder against the float64 reference and the scripted
cases of tests/beam_cases.py (whose margins tests/test_beam_cases_cpu.py checks), then AKI.generate(num_beams=K) with
lang_model.device_beam_search = True on the tiny model."""
import functools

import numpy as np
import pytest
import torch

import beam_cases as bc
from test_model_gpu import build_tiny, batch, DEV

pytestmark = pytest.mark.gpu


# ---- 1. the log-softmax --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.NAMES)
def test_beam_logprob_against_f64(name):
    from aki_amd import ops
    c = bc.case(name)
    T, R, V = c.logits.shape
    x = torch.from_numpy(c.logits.reshape(T * R, V)).to(DEV)
    want = bc.logprob_ref(c.logits.reshape(T * R, V))
    wide = torch.zeros((T * R, V + 5), dtype=torch.float32, device=DEV)
    wide[:, :V] = x
    worst = 0.0
    for what, inp in (("f32", x), ("bf16", x.to(torch.bfloat16)), ("f32, row stride V + 5", wide[:, :V]),
                      ("bf16, row stride V + 5", wide.to(torch.bfloat16)[:, :V])):
        got = ops.beam_logprob(inp)
        again = ops.beam_logprob(inp)
        assert got.dtype == torch.float32 and tuple(got.shape) == (T * R, V) and torch.equal(got, again), what
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        worst = max(worst, err)
        assert err <= c.logprob_bound, f"{name} ({what}): |error| {err:.3g} above the bound {c.logprob_bound:.3g}"
    print(f"{name}: logprob |error| {worst:.3g}, bound {c.logprob_bound:.3g}")


# ---- 2. the step ---------------------------------------------------------------------------------------------------------------------
def _run_case(c):
    from aki_amd import ops
    s = c.spec
    st = ops.BeamState(s["B"], s["K"], s["T"], DEV, s["eos"], bc.PAD, s["lp"], s["es"])
    steps = []
    for t in range(s["T"]):
        logp = ops.beam_logprob(torch.from_numpy(c.logits[t]).to(DEV).to(torch.bfloat16))
        ops.beam_step(logp, st, t, last=t + 1 == s["T"])
        steps.append({k: getattr(st, k).cpu().clone() for k in ("parent", "next_ids", "beam_scores", "done")})
        steps[-1]["seqs"] = st.seqs[:, : t + 1].cpu().clone()
    final = {k: getattr(st, k).cpu().clone() for k in ("hyp_score", "hyp_len", "hyp_tokens", "hyp_count", "done")}
    return steps, final


@pytest.mark.parametrize("name", bc.NAMES)
def test_beam_step_follows_the_f64_search(name):
    c = bc.case(name)
    s, ref = c.spec, c.ref
    B, K = s["B"], s["K"]
    steps, final = _run_case(c)
    worst = 0.0
    for t, (got, want) in enumerate(zip(steps, ref.steps)):
        assert got["parent"].tolist() == want["parent"].tolist(), f"{name}: parents of step {t}"
        assert got["next_ids"].tolist() == want["next_ids"].tolist(), f"{name}: next ids of step {t}"
        assert got["seqs"].tolist() == want["seqs"].tolist(), f"{name}: sequences after step {t}"
        assert got["done"].tolist() == want["done"].tolist(), f"{name}: done flags after step {t}"
        err = float(np.abs(got["beam_scores"].numpy().astype(np.float64) - want["beam_scores"]).max())
        worst = max(worst, err)
        assert err <= c.bound, f"{name}: beam scores of step {t} off by {err:.3g}, bound {c.bound:.3g}"
    assert final["hyp_count"].tolist() == [len(h) for h in ref.hyps], f"{name}: hypotheses kept"
    for b in range(B):
        for i, (sc, toks) in enumerate(ref.hyps[b]):           # the same slots: the eviction rule is part of the contract
            assert int(final["hyp_len"][b, i]) == len(toks) and final["hyp_tokens"][b, i, : len(toks)].tolist() == toks, (name, b, i)
            err = abs(float(final["hyp_score"][b, i]) - sc)
            worst = max(worst, err)
            assert err <= c.bound, f"{name}: hypothesis score off by {err:.3g}, bound {c.bound:.3g}"
    print(f"{name}: largest score error {worst:.3g}, bound {c.bound:.3g}, smallest margin {c.min_margin:.3g}")
    steps2, final2 = _run_case(c)                               # the same bits on every run
    for a, b_ in zip(steps + [final], steps2 + [final2]):
        for k in a:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                               b_[k].view(torch.int32) if b_[k].dtype == torch.float32 else b_[k]), f"{name}: {k} differs between two runs"


def test_beam_step_ranking_does_not_depend_on_where_the_large_scores_sit():
    """A thread of the kernel owns the columns v = tid (mod 1024) of all K beams, and its threshold pass keeps at most 1024 survivors.
    Sample 0 puts 8 * 16 * 15 = 1920 large scores into the columns of 15 threads: the survivors overflow and the ranking takes the
    pass-per-rank path.  Sample 1 puts 240 there: a long list, ranked by counting.  Scores are distinct f32 numbers and the running scores
    are 0, so the ranking is exact: tokens, parents and scores must equal a sort."""
    from aki_amd import ops
    B, K, V = 2, 8, 16384
    rng = np.random.default_rng(5)
    logp = np.empty((B, K * V), dtype=np.float32)
    for b in range(B):
        logp[b] = -20.0 - 1e-3 * rng.permutation(K * V).astype(np.float32)
        cols = np.flatnonzero((np.arange(K * V) % V) % bc.KERNEL_THREADS < 15)
        if b == 1:
            cols = cols[cols < V]                                     # beam 0 only
        logp[b, cols] = -1.0 - 1e-3 * rng.permutation(cols.size).astype(np.float32)
    assert all(np.unique(logp[b]).size == K * V for b in range(B))
    st = ops.BeamState(B, K, 2, DEV)
    st.beam_scores.zero_()
    ops.beam_step(torch.from_numpy(logp.reshape(B * K, V)).to(DEV), st, 0)
    for b in range(B):
        order = np.argsort(-logp[b], kind="stable")[:K]
        assert st.next_ids[b * K:(b + 1) * K].tolist() == (order % V).tolist()
        assert st.parent[b * K:(b + 1) * K].tolist() == (b * K + order // V).tolist()
        assert st.beam_scores[b].cpu().numpy().tolist() == logp[b, order].tolist()


# ---- 3. the in-place re-ordering of the cache rows -----------------------------------------------------------------------------------
REORDER_CHUNK = 16          # positions one workgroup of aki_kv_beam_reorder owns (AKI_KV_BEAM_REORDER_CHUNK); chunks start at multiples of it


def _parents(pattern, B, K, rng):
    ident = np.arange(B * K).reshape(B, K)
    if pattern == "identity":
        local = np.tile(np.arange(K), (B, 1))
    elif pattern == "beam0":
        local = np.zeros((B, K), dtype=np.int64)
    elif pattern == "reversal":
        local = np.tile(np.arange(K)[::-1], (B, 1))
    else:
        local = rng.integers(0, K, size=(B, K))
        if pattern == "mixed":
            local[0] = np.arange(K)
    return (ident - ident % K + local).reshape(-1).astype(np.int32)


@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kv_beam_reorder_moves_the_new_rows_only(dtype, B, K):
    from aki_amd import ops
    assert ops.KV_BEAM_REORDER_CHUNK == REORDER_CHUNK
    cap, Dh, n_layers = 80, 96, 2
    ints = torch.int16 if dtype == torch.bfloat16 else torch.int32
    nan_bits = 0x7FC1 if dtype == torch.bfloat16 else 0x7FC00001
    rng = np.random.default_rng(1000 * B + K)
    gen = torch.Generator().manual_seed(B * 100 + K)
    start = np.repeat(np.array([37, 20, 51][:B], dtype=np.int32), K)                # ragged per sample
    for H in (2, 3):
        datas = [torch.randn((B * K, H, cap, Dh), generator=gen).to(dtype).view(ints) for _ in range(2 * n_layers)]
        for suffix in (0, 1, REORDER_CHUNK - 1, REORDER_CHUNK, REORDER_CHUNK + 1):
            for pattern in ("identity", "beam0", "reversal", "random", "mixed"):
                length = start + suffix
                pos = torch.arange(cap)[None, :]
                moving = ((pos >= torch.from_numpy(start)[:, None]) & (pos < torch.from_numpy(length)[:, None]))[:, None, :, None]
                parent = _parents(pattern, B, K, rng)
                tensors, want = [], []
                for data in datas:                   # prompt rows and the rows past cache_len: a NaN pattern, compared as integers
                    t_ = torch.where(moving, data, torch.full_like(data, nan_bits))
                    tensors.append(t_)
                    want.append(torch.where(moving, t_[torch.from_numpy(parent).long()], t_))     # index_select on the moving rows only
                dev = [t_.to(DEV).view(dtype) for t_ in tensors]
                table = ops.KVBeamTable(dev)
                ops.kv_beam_reorder(table, torch.from_numpy(parent).to(DEV), torch.from_numpy(start).to(DEV),
                                    torch.from_numpy(length).to(DEV), K, int(start.min()), int(length.max()))
                for i, (d, w) in enumerate(zip(dev, want)):
                    same = torch.equal(d.view(ints).cpu(), w)
                    assert same, f"tensor {i}, H {H}, suffix {suffix}, parents {pattern}: {int((d.view(ints).cpu() != w).sum())} elements differ"


# ---- 4. end to end on the tiny model -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny(dtype):
    m, g = build_tiny(dtype)
    return m, batch(g, dtype)


def _both(m, *args, **kw):
    """generate with the host loop and with the device path."""
    lm = m.lang_model
    assert lm.device_beam_search is False, "the switch is off by default"
    host = m.generate(*args, **kw)
    lm.device_beam_search = True
    try:
        m.last_beam_scores = None
        dev = m.generate(*args, **kw)
        assert m.last_beam_scores is not None, "the device path was not taken"
    finally:
        lm.device_beam_search = False
    return host, dev


@pytest.mark.parametrize("K", [2, 3])
def test_fp32_generate_returns_the_host_loops_tokens(K):
    m, (vx, lx, am, _) = _tiny(torch.float32)
    host, dev = _both(m, vx, lx, attention_mask=am, max_new_tokens=4, num_beams=K, eos_token_id=[])
    assert dev.shape == (lx.shape[0], 4) and torch.equal(host, dev), (host.tolist(), dev.tolist())
    free, free_dev = _both(m, vx, lx, attention_mask=am, max_new_tokens=3, num_beams=K, eos_token_id=[])
    assert torch.equal(free, free_dev)
    eos = sorted(set(free[:, 1].tolist()))                    # the second token of every sample's best beam ends it
    for es in (False, True):
        host, dev = _both(m, vx, lx, attention_mask=am, max_new_tokens=6, num_beams=K, eos_token_id=eos, pad_token_id=0, early_stopping=es)
        assert torch.equal(host, dev), (es, host.tolist(), dev.tolist())
    host, dev = _both(m, vx, lx, attention_mask=am, max_new_tokens=6, num_beams=K, eos_token_id=[], no_repeat_ngram_size=2,
                      repetition_penalty=1.2)
    assert torch.equal(host, dev), (host.tolist(), dev.tolist())
    host, dev = _both(m, vx, lx, attention_mask=am, max_new_tokens=0, num_beams=K)
    assert host.shape == dev.shape == (lx.shape[0], 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_and_eager_steps_return_the_same_tokens(dtype):
    m, (vx, lx, am, _) = _tiny(dtype)
    m.lang_model.device_beam_search = True
    try:
        kw = dict(attention_mask=am, max_new_tokens=10, num_beams=3, eos_token_id=[])
        eager = m.generate(vx, lx, use_graph=False, **kw)
        graph = m.generate(vx, lx, use_graph=True, **kw)
    finally:
        m.lang_model.device_beam_search = False
    assert eager.shape == (lx.shape[0], 10) and torch.equal(eager, graph), (eager.tolist(), graph.tolist())


def _teacher_forced_logprob(m, vx, lx, am, toks, K):
    """Sum of the float64 log-softmax values of `toks` [B, n] under decode steps that feed them, at the beam search's own batch of B*K
    rows (every sample K times): the logits a row meets are then the bits the search met.  Also max |logit| and V."""
    lm = m.lang_model
    B, n = toks.shape
    with torch.no_grad():
        plan = m._start_splice_plan(lx)
        vt = m.vision_tokenizer(m._encode_vision_x(vision_x=vx))
        ni = m._prepare_inputs_for_forward(vision_tokens=vt, lang_x=lx, attention_mask=am, padding_side="right", splice_plan=plan)
        L = ni["inputs_embeds"].shape[1]
        out = lm(inputs_embeds=ni["inputs_embeds"], attention_mask=ni["attention_mask"], use_cache=True, cache_capacity=L + n,
                 last_token_logits=True)
        m._post_forward_hook()
        cache, logits = out.past_key_values, out.logits[:, 0].repeat_interleave(K, dim=0)
        cache.select_rows(torch.arange(B, device=DEV).repeat_interleave(K))
        total, M = np.zeros(B), 0.0
        for j in range(n):
            x = logits[::K].double().cpu().numpy()
            M = max(M, float(np.abs(x).max()))
            total += bc.logprob_ref(x)[np.arange(B), toks[:, j].cpu().numpy()]
            if j + 1 < n:
                logits = lm.decode_step(input_ids=toks[:, j].repeat_interleave(K).contiguous(), past_key_values=cache)
    return total, M, logits.shape[-1]


@pytest.mark.parametrize("K", [2, 3])
def test_bf16_generate_scores_what_it_reports_and_is_not_worse_than_greedy(K):
    """bf16 logits tie and torch.topk has no tie rule: no comparison with the host loop.  The returned sequence's log-probability under
    teacher-forced decode steps is the reported hypothesis score times its length normalisation, within the cases' bound for that length
    (tests/beam_cases.py: hyp_bound, in the normalised score's units, times the normalisation)."""
    m, (vx, lx, am, _) = _tiny(torch.bfloat16)
    n, lp = 5, 1.0
    lm = m.lang_model
    lm.device_beam_search = True
    try:
        got = m.generate(vx, lx, attention_mask=am, max_new_tokens=n, num_beams=K, eos_token_id=[], length_penalty=lp)
        reported = list(m.last_beam_scores)
        again = m.generate(vx, lx, attention_mask=am, max_new_tokens=n, num_beams=K, eos_token_id=[], length_penalty=lp)
    finally:
        lm.device_beam_search = False
    assert got.shape == (lx.shape[0], n) and torch.equal(got, again)
    greedy = m.generate(vx, lx, attention_mask=am, max_new_tokens=n, eos_token_id=[])
    s_beam, M, V = _teacher_forced_logprob(m, vx, lx, am, got, K)
    s_greedy, M2, _ = _teacher_forced_logprob(m, vx, lx, am, greedy, K)
    bound = bc.hyp_bound(max(M, M2), V, n - 1) * n ** lp
    for b in range(lx.shape[0]):
        print(f"K {K}, sample {b}: reported {reported[b] * n ** lp:.6f}, teacher-forced {s_beam[b]:.6f}, greedy {s_greedy[b]:.6f}, bound {bound:.3g}")
        assert abs(reported[b] * n ** lp - s_beam[b]) <= bound, (b, reported[b] * n ** lp, s_beam[b], bound)
        assert s_beam[b] >= s_greedy[b] - bound, (b, s_beam[b], s_greedy[b])


def test_fp8_kv_cache_keeps_the_host_loop():
    m, (vx, lx, am, _) = _tiny(torch.bfloat16)
    lm = m.lang_model
    lm.set_kv_cache_dtype("fp8_e4m3")
    lm.device_beam_search = True
    try:
        m.last_beam_scores = None
        out = m.generate(vx, lx, attention_mask=am, max_new_tokens=5, num_beams=2, eos_token_id=[])
        assert out.shape == (lx.shape[0], 5) and int(out.min()) >= 0 and m.last_beam_scores is None
    finally:
        lm.device_beam_search = False
        lm.set_kv_cache_dtype("bf16")
