"""Chunk attention on the GPU: every case of tests/chunk_attn_cases.py on both input families against the float64 reference (the
prefill core's bf16 bar, per (sample, token) row), appended rows bit-exact, everything else in the cache untouched;
determinism; the ABI's status codes; Phi3ForCausalLM._continue on the chunked route against the T decode steps; and
AKI.generate(past_key_values=...) against a hand loop.

Measured worst err / tol per case: DESIGN.md section 2."""
import numpy as np
import pytest
import torch

import chunk_attn_cases as C
from test_kernels_gpu import DEV
from test_model_gpu import build_tiny, batch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# The decode attention tests' bar is tolerance(ref_row, 2.0).  Those kernels keep the probabilities in f32; this one hands them to the MFMA as
# bf16 (2^-9 relative each), which on the diffuse family (V ~ sqrt(n), |o| ~ 1) is an error of ~2e-3 sigma per element - measured worst
# err / tol 1.07 at 2.0 (b1-h2-cap128-len3-T64, diffuse), 0.94 and below elsewhere.  So the bar is the one the prefill core's sweeps use
# in test_kernels_gpu.py, scale_atol = 4.0: the same bf16 probabilities, the same MFMA arithmetic.
SCALE_ATOL = 4.0


def _launch(inp, ws=None):
    from aki_amd import ops
    c = inp.case
    bits = c.bits()
    k, v = inp.k.to(DEV), inp.v.to(DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    n_new = torch.tensor(c.n_new, dtype=torch.int32, device=DEV) if c.ragged else None
    o = ops.chunk_attn(inp.qkv.to(DEV), torch.from_numpy(inp.cos).to(DEV), torch.from_numpy(inp.sin).to(DEV), lens, n_new, k, v, c.H, C.SCALE,
                       None if bits is None else torch.from_numpy(bits).to(DEV), None, ws)
    torch.cuda.synchronize()
    return o, k, v, lens


_REF = {}


def _reference(case, family):
    key = (case.id, family)
    if key not in _REF:
        inp = C.make_inputs(case, family)
        _REF[key] = (inp, C.reference(inp))
    return _REF[key]


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_chunk_kernel_against_float64_reference(case, family):
    from conftest import record_parity
    inp, ref = _reference(case, family)
    o, k, v, lens = _launch(inp)
    got = o.float().cpu().numpy().reshape(case.B, case.T, case.H * C.DH).astype(np.float64)
    assert np.isfinite(got).all(), "non-finite output"
    worst = 0.0
    for b in range(case.B):
        nn = case.n_new[b]
        for t in range(nn):
            worst = max(worst, float((np.abs(got[b, t] - ref[b, t]) / C.tolerance(ref[b, t], SCALE_ATOL)).max()))
        assert not o.cpu().view(torch.int16).reshape(case.B, case.T, -1)[b, nn:].any(), f"sample {b}: rows past n_new are not +0.0 bit for bit"
    print(f"{case.id} {family}: worst err / tol {worst:.3f}")
    record_parity(f"chunk attention {case.id} {family}", BF, worst, worst, 1.0, f"err/tol <= 1 (tolerance(ref_row, {SCALE_ATOL:g}) per row)")
    kc, vc = k.cpu(), v.cpu()
    for b in range(case.B):
        ln, nn = case.lens[b], case.n_new[b]
        k_app, v_app = C.appended_rows(inp, b)
        assert np.array_equal(kc[b, :, ln:ln + nn].float().numpy(), k_app), f"appended k rows of sample {b}"
        assert np.array_equal(vc[b, :, ln:ln + nn].float().numpy(), v_app), f"appended v rows of sample {b}"
        for name, new, old in (("k", kc, inp.k), ("v", vc, inp.v)):
            assert torch.equal(new[b, :, :ln].view(torch.int16), old[b, :, :ln].view(torch.int16)), f"cached {name} rows of sample {b} were written"
            assert new[b, :, ln + nn:].isnan().all(), f"{name} rows past the chunk of sample {b} were written"
    assert lens.cpu().tolist() == list(case.lens), "cache_len was advanced"
    assert worst <= 1.0, f"{case.id} {family}: worst err / tol {worst:.2f}"


def test_chunk_kernel_is_deterministic_through_one_workspace():
    from aki_amd import _lib
    case = C.CASE_BY_ID[C.LARGEST]
    inp, _ = _reference(case, "diffuse")
    nbytes = int(_lib.load().aki_chunk_attn_workspace_bytes(case.B, case.H, case.T, C.DH))
    assert nbytes == case.B * case.H * case.T * C.DH * 2
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    first = None
    for _ in range(20):
        o = _launch(inp, ws)[0].cpu().view(torch.int16)
        first = o if first is None else first
        assert torch.equal(o, first)


def test_chunk_abi_status_codes():
    from aki_amd import _lib
    lib = _lib.load()
    assert lib.aki_chunk_attn_workspace_bytes(1, 2, 4, 96) == 2 * 4 * 96 * 2 and lib.aki_chunk_attn_workspace_bytes(1, 2, 4, 64) == 0
    t = torch.zeros(1 << 16, dtype=BF, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)
    p = lambda x: x.data_ptr()
    args = lambda Dh, dt, wsb, T=4, cap=64: (p(t), p(f), p(f), p(i), None, p(t), p(t), p(t), None, 0, 1, 2, Dh, T, 0, cap, 0.1, dt, p(f), wsb, None)
    BF16, F32, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, -1, -2, -4      # AKI_DT_* and AKI_ERR_* of include/aki_mi355x.h
    assert lib.aki_chunk_attn_fwd(*args(64, BF16, f.numel() * 4)) == UNSUPPORTED
    assert lib.aki_chunk_attn_fwd(*args(96, F32, f.numel() * 4)) == UNSUPPORTED
    assert lib.aki_chunk_attn_fwd(*args(96, BF16, 16)) == WORKSPACE
    assert lib.aki_chunk_attn_fwd(*args(96, BF16, f.numel() * 4, T=0)) == INVALID
    assert lib.aki_chunk_attn_fwd(*args(96, BF16, f.numel() * 4, cap=0)) == INVALID
    torch.cuda.synchronize()


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _prefill(m, vx, lx, am, cap_extra):
    vt = m.vision_tokenizer(m._encode_vision_x(vx))
    prep = m._prepare_inputs_for_forward(vision_tokens=vt, lang_x=lx, attention_mask=am, padding_side="right")
    L = prep["inputs_embeds"].shape[1]
    out = m.lang_model(inputs_embeds=prep["inputs_embeds"], attention_mask=prep["attention_mask"], use_cache=True, cache_capacity=L + cap_extra,
                       last_token_logits=True)
    return out.past_key_values, out.logits[:, 0]


def _count_chunk_attn(monkeypatch):
    from aki_amd import ops
    calls, orig = [], ops.chunk_attn
    monkeypatch.setattr(ops, "chunk_attn", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    return calls


def _ids(B, T, vocab, seed=3):
    return torch.randint(3, vocab - 1, (B, T), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bar(x):
    return 2e-2 * max(1.0, x.float().abs().max().item())


def _bits(x):
    return x.contiguous().view(torch.int16)


def test_chunked_continue_matches_the_decode_steps_and_the_chain_keeps_working(monkeypatch):
    calls = _count_chunk_attn(monkeypatch)
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    B = lx.shape[0]
    with torch.no_grad():
        caches = [_prefill(m, vx, lx, am, 40) for _ in range(3)]
        vocab = caches[0][1].shape[-1]
        new = _ids(B, 9, 1000)
        seq, chk, chk5 = (c for c, _ in caches)
        want = lm(input_ids=new, past_key_values=seq).logits
        assert not calls
        lm.chunked_continue = True
        got = lm(input_ids=new, past_key_values=chk).logits
        got5 = lm(input_ids=new, past_key_values=chk5).logits
        lm.chunked_continue = False
        assert len(calls) == 2 * len(lm.model.layers)
        assert got.shape == want.shape == (B, 9, vocab) and torch.equal(_bits(got), _bits(got5))
        err = (got.float() - want.float()).abs().max().item()
        print(f"chunked vs sequential logits: err {err:.3g}, bar {_bar(want):.3g}")
        assert err <= _bar(want)
        assert torch.equal(seq.cache_len, chk.cache_len) and seq.host_len == chk.host_len
        step_ids = _ids(B, 3, 1000, seed=4)
        for t in range(3):
            a = lm.decode_step(input_ids=step_ids[:, t], past_key_values=seq)
            lm.model.use_decode_chain = True
            b = lm.decode_step(input_ids=step_ids[:, t], past_key_values=chk)
            lm.model.use_decode_chain = False
            try:
                c = lm.decode_step(input_ids=step_ids[:, t], past_key_values=chk5)
            finally:
                lm.model.use_decode_chain = True
            assert torch.equal(_bits(b), _bits(c)), f"step {t}: the chain and the five-launch path differ after a chunk"
            assert (b.float() - a.float()).abs().max().item() <= _bar(a), f"step {t} after the chunk"
        assert lm.decode_verified(chk)


def test_chunked_continue_batch_one_on_the_chain():
    """One sequence: the decode steps after the chunk run on the one-launch chain."""
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    with torch.no_grad():
        seq, chk, chk5 = (_prefill(m, vx[:1], lx[:1], am[:1], 40)[0] for _ in range(3))
        new = _ids(1, 9, 50)
        want = lm(input_ids=new, past_key_values=seq).logits
        lm.chunked_continue = True
        got = lm(input_ids=new, past_key_values=chk).logits
        lm(input_ids=new, past_key_values=chk5)
        lm.chunked_continue = False
        assert (got.float() - want.float()).abs().max().item() <= _bar(want)
        for t in range(3):
            ids = new[:, t]
            a = lm.decode_step(input_ids=ids, past_key_values=seq)
            b = lm.decode_step(input_ids=ids, past_key_values=chk)
            lm.model.use_decode_chain = False
            try:
                c = lm.decode_step(input_ids=ids, past_key_values=chk5)
            finally:
                lm.model.use_decode_chain = True
            assert torch.equal(_bits(b), _bits(c)) and (b.float() - a.float()).abs().max().item() <= _bar(a)
        assert lm.decode_verified(chk) and lm.decode_verified(seq)


def test_flag_off_is_the_loop_of_decode_steps(monkeypatch):
    calls = _count_chunk_attn(monkeypatch)
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    assert type(lm).chunked_continue is False
    with torch.no_grad():
        a, b = (_prefill(m, vx, lx, am, 40)[0] for _ in range(2))
        new = _ids(lx.shape[0], 5, 50)
        got = lm(input_ids=new, past_key_values=a).logits
        want = torch.stack([lm.decode_step(input_ids=new[:, t], past_key_values=b) for t in range(5)], dim=1)
    assert not calls and torch.equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):
        lm._continue(new, None, a, n_new=torch.tensor([5] * (lx.shape[0] - 1) + [3]))


@pytest.mark.parametrize("kind", ["fp8_cache", "grouped_cache", "f32_model"])
def test_ineligible_caches_take_the_decode_steps(monkeypatch, kind):
    calls = _count_chunk_attn(monkeypatch)
    dt = torch.float32 if kind == "f32_model" else BF
    m, g = build_tiny(dt)
    vx, lx, am, _ = batch(g, dt)
    lm = m.lang_model
    rows = lx.shape[0] * (2 if kind == "grouped_cache" else 1)
    new = _ids(rows, 4, 50)
    outs = []
    if kind == "fp8_cache":
        lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.no_grad():
            for flag in (False, True):
                cache = _prefill(m, vx, lx, am, 40)[0]
                if kind == "grouped_cache":
                    cache.share_prefix(2)
                lm.chunked_continue = flag
                outs.append(lm(input_ids=new, past_key_values=cache).logits)
    finally:
        lm.chunked_continue = False
        lm.set_kv_cache_dtype("bf16")
    assert not calls
    view = (lambda x: x.contiguous().view(torch.int32)) if dt == torch.float32 else _bits
    assert torch.equal(view(outs[0]), view(outs[1]))


def test_a_chunk_past_the_capacity_raises_before_anything_is_written():
    from aki_amd import ops
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    with torch.no_grad():
        cache = _prefill(m, vx, lx, am, 4)[0]
        spare = cache.capacity - cache.host_len
        kv, lens, host = cache._store[0].clone(), cache.cache_len.clone(), cache.host_len
        lm.chunked_continue = True
        try:
            with pytest.raises(ops.AkiError):
                lm(input_ids=_ids(lx.shape[0], spare + 1, 50), past_key_values=cache)
        finally:
            lm.chunked_continue = False
        torch.cuda.synchronize()
    assert torch.equal(kv.view(torch.int16), cache._store[0].view(torch.int16)) and torch.equal(lens, cache.cache_len) and host == cache.host_len


# ---- generate(past_key_values=...) ----------------------------------------------------------------------------------------------------
def _mask(cache, tail):
    past = cache.get_seq_length()
    return torch.cat([torch.ones((tail.shape[0], past), dtype=torch.long, device=DEV), tail.to(DEV)], dim=1)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("flag", [False, True])
def test_generate_from_a_cache_equals_a_hand_loop(flag, use_graph):
    """Plumbing, so token for token."""
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    B, T, N = lx.shape[0], 5, 6
    new = _ids(B, T, 50)
    lm.chunked_continue = flag
    try:
        with torch.no_grad():
            cache, cache2 = (_prefill(m, vx, lx, am, 32)[0] for _ in range(2))
            got = m.generate(None, new, attention_mask=_mask(cache, torch.ones(B, T, dtype=torch.long)), past_key_values=cache, max_new_tokens=N,
                             eos_token_id=[], use_graph=use_graph)
            logits = lm(input_ids=new, past_key_values=cache2).logits[:, -1]
            want = []
            for t in range(N):
                tok = logits.float().argmax(-1)
                want.append(tok)
                if t + 1 < N:
                    logits = lm.decode_step(input_ids=tok, past_key_values=cache2)
            want = torch.stack(want, dim=1)
    finally:
        lm.chunked_continue = False
    assert got.shape == (B, N) and torch.equal(got, want), f"generate {got.tolist()} vs the hand loop {want.tolist()}"
    assert torch.equal(cache.cache_len, cache2.cache_len), "the last returned token is not in the cache"


def _greedy_hand_loop(lm, cache, ids, n):
    """The new ids, then n greedy tokens: the last of them is not fed back."""
    logits = lm(input_ids=ids, past_key_values=cache).logits[:, -1]
    out = []
    for t in range(n):
        out.append(logits.float().argmax(-1))
        if t + 1 < n:
            logits = lm.decode_step(input_ids=out[-1], past_key_values=cache)
    return torch.stack(out, dim=1)


def _first_hit(row, eos):
    hits = (row == eos).nonzero()
    return int(hits[0]) if hits.numel() else None


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("flag", [False, True])
def test_generate_from_a_cache_stops_the_cache_before_the_eos_and_a_second_turn_follows(flag, use_graph):
    """The chat loop at B = 1: a turn that ends at an EOS leaves the cache right before that EOS, whatever the loop stepped past it (the
    device loop looks at the flags every 8th token), and the next turn - lang_x beginning with the EOS - equals a hand loop that never
    stepped past it."""
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    vx, lx, am = vx[:1], lx[:1], am[:1]
    lm = m.lang_model
    T, N = 5, 12
    new = _ids(1, T, 50)
    lm.chunked_continue = flag
    try:
        with torch.no_grad():
            cache, probe, hand = (_prefill(m, vx, lx, am, 48)[0] for _ in range(3))
            free = _greedy_hand_loop(lm, probe, new, N)                   # without an EOS: the tokens the turn would produce
            eos = int(free[0, 2])
            e = _first_hit(free[0], eos)                                   # 2, or earlier if the tiny model repeats itself
            start, host = cache.cache_len.clone(), cache.host_len
            got = m.generate(None, new, attention_mask=_mask(cache, torch.ones(1, T, dtype=torch.long)), past_key_values=cache,
                             max_new_tokens=N, eos_token_id=[eos], use_graph=use_graph)
            assert got.shape == (1, e + 1) and torch.equal(got, free[:, :e + 1]), f"generate {got.tolist()} vs {free[:, :e + 1].tolist()}"
            assert (cache.cache_len - start).cpu().tolist() == [T + e] and cache.host_len == host + T + e, \
                f"cache_len advanced by {(cache.cache_len - start).cpu().tolist()}, host_len by {cache.host_len - host}: expected T + returned - 1 = {T + e}"
            turn2 = torch.cat([got[:, -1:], _ids(1, 3, 50, seed=5)], dim=1)
            got2 = m.generate(None, turn2, past_key_values=cache, max_new_tokens=4, eos_token_id=[], use_graph=use_graph)
            assert torch.equal(_greedy_hand_loop(lm, hand, new, e + 1), got)            # the hand cache: the new ids and tokens 0 .. e - 1
            want2 = _greedy_hand_loop(lm, hand, turn2, 4)
            assert torch.equal(hand.cache_len, cache.cache_len) and hand.host_len == cache.host_len
    finally:
        lm.chunked_continue = False
    assert torch.equal(got2, want2), f"second turn {got2.tolist()} vs the hand loop {want2.tolist()}"


@pytest.mark.parametrize("use_graph", [True, False])
def test_generate_from_a_cache_cuts_every_finished_row_of_a_batch_before_its_eos(use_graph):
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    B, T, N = lx.shape[0], 5, 12
    new = _ids(B, T, 50)
    with torch.no_grad():
        cache, probe = (_prefill(m, vx, lx, am, 48)[0] for _ in range(2))
        free = _greedy_hand_loop(lm, probe, new, N)
        eos = int(free[0, 1])
        hits = [_first_hit(free[b], eos) for b in range(B)]
        steps = N if None in hits else max(hits) + 1                      # the loop ends when every row has finished
        kept = [steps - 1 if h is None or h >= steps else h for h in hits]
        start = cache.cache_len.clone()
        got = m.generate(None, new, past_key_values=cache, max_new_tokens=N, eos_token_id=[eos], use_graph=use_graph)
    assert got.shape == (B, steps)
    for b in range(B):
        assert torch.equal(got[b, :kept[b] + 1], free[b, :kept[b] + 1]), f"row {b}"
    assert (cache.cache_len - start).cpu().tolist() == [T + k for k in kept]


def test_generate_from_a_cache_ragged_chunk_equals_per_sample_calls():
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    B, T = lx.shape[0], 7
    assert B >= 2, "a ragged chunk needs two samples: batch() must keep at least two"
    n_new = [T - 3 * (b % 2) for b in range(B)]
    new = _ids(B, T, 50)
    tail = (torch.arange(T)[None, :] < torch.tensor(n_new)[:, None]).long()
    lm.chunked_continue = True
    try:
        with torch.no_grad():
            cache = _prefill(m, vx, lx, am, 32)[0]
            start = cache.cache_len.clone()
            got = m.generate(None, new, attention_mask=_mask(cache, tail), past_key_values=cache, max_new_tokens=1, eos_token_id=[])
            assert (cache.cache_len - start).cpu().tolist() == n_new
            skipped = 0
            for b in range(B):
                one = _prefill(m, vx[b:b + 1], lx[b:b + 1], am[b:b + 1], 32)[0]
                lg = lm(input_ids=new[b:b + 1, :n_new[b]], past_key_values=one).logits[0, -1].float()
                top = lg.topk(2)
                if (top.values[0] - top.values[1]).item() < _bar(lg):
                    skipped += 1
                    continue
                assert int(got[b, 0]) == int(top.indices[0]), f"sample {b}: token 0 of the ragged batch vs the batch-1 call"
            assert skipped <= 1, f"{skipped} samples have a top-2 margin below the bar: the comparison shows nothing"
    finally:
        lm.chunked_continue = False


def test_generate_from_a_cache_refusals():
    from aki_amd import ops
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    B, T = lx.shape[0], 4
    new = _ids(B, T, 50)
    ones = torch.ones(B, T, dtype=torch.long)
    with torch.no_grad():
        cache = _prefill(m, vx, lx, am, 32)[0]
        lens, host = cache.cache_len.clone(), cache.host_len
        kw = dict(past_key_values=cache, max_new_tokens=3, eos_token_id=[])
        with pytest.raises(ValueError):
            m.generate(None, new, attention_mask=_mask(cache, ones)[:, 1:], **kw)                     # wrong width
        hole = ones.clone()
        hole[0, 1] = 0
        with pytest.raises(ValueError):
            m.generate(None, new, attention_mask=_mask(cache, hole), **kw)                            # not ones followed by zeros
        ragged = ones.clone()
        ragged[0, -1] = 0
        with pytest.raises(ValueError):
            m.generate(None, new, attention_mask=_mask(cache, ragged), **kw)                          # ragged with the flag off
        with pytest.raises(NotImplementedError):
            m.generate(None, new, num_beams=2, **kw)
        with pytest.raises(NotImplementedError):
            m.generate(None, new, do_sample=True, num_return_sequences=2, **kw)
        with pytest.raises(ops.AkiError):
            m.generate(None, new, **dict(kw, max_new_tokens=40))
        with pytest.raises(NotImplementedError):
            m.generate(vx, new, **kw)
        torch.cuda.synchronize()
        assert torch.equal(lens, cache.cache_len) and host == cache.host_len, "a refused call changed the cache"
        out = m.generate(None, new, **kw)                                                             # and the cache still serves
        assert out.shape == (B, 3)
