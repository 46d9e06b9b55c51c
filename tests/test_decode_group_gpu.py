"""The grouped decode attention kernel and generate(num_return_sequences=N) on the GPU: every case of tests/decode_group_cases.py on
both input families against the float64 reference (bf16 bar, per row), appended rows bit-exact, prefix untouched; determinism;
eager against replayed steps; the grouped cache against the replicated one at the model level; generate's shapes, order and errors."""
import numpy as np
import pytest
import torch

import decode_group_cases as G
from test_kernels_gpu import DEV
from test_model_gpu import build_tiny, batch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _launch(inp, bounds, ws=None):
    from aki_amd import ops
    c = inp.case
    bits = c.bits()
    dev = lambda t: t.to(DEV)
    ks, vs = dev(inp.ks), dev(inp.vs)
    kp, vp = dev(inp.kp), dev(inp.vp)
    o = ops.decode_attn_group(dev(inp.qkv), torch.from_numpy(inp.cos).to(DEV), torch.from_numpy(inp.sin).to(DEV),
                              torch.tensor(c.lens(), dtype=torch.int32, device=DEV), torch.tensor(c.plens, dtype=torch.int32, device=DEV),
                              kp, vp, ks, vs, c.H, G.SCALE, None if bits is None else torch.from_numpy(bits).to(DEV), bounds[0], bounds[1], ws)
    torch.cuda.synchronize()
    return o, kp, vp, ks, vs


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_group_kernel_against_float64_reference(case, family):
    from conftest import record_parity
    inp = G.make_inputs(case, family)
    ref = G.reference(inp)
    k_app, v_app = G.appended_rows(inp)
    outs = []
    for bounds in case.key_bounds():                    # an eager step's grid and a captured one's
        o, kp, vp, ks, vs = _launch(inp, bounds)
        got = o.float().cpu().numpy().reshape(case.rows, case.H, G.DH).astype(np.float64)
        worst = 0.0
        for r in range(case.rows):
            ratio = float((np.abs(got[r] - ref[r]) / G.tolerance(ref[r], 2.0)).max())
            assert np.isfinite(got[r]).all(), f"row {r}: non-finite output"
            worst = max(worst, ratio)
        print(f"{case.id} {family} bounds {bounds}: worst err / tol {worst:.3f}")
        record_parity(f"grouped decode attention {case.id} {family}", BF, worst, worst, 1.0, "err/tol <= 1 (tolerance(ref, 2.0) per row)")
        assert worst <= 1.0, f"{case.id} {family}: worst err / tol {worst:.2f}"
        for r in range(case.rows):
            sl = case.slens[r]
            assert np.array_equal(ks[r, :, sl].float().cpu().numpy(), k_app[r]), f"appended k of row {r}"
            assert np.array_equal(vs[r, :, sl].float().cpu().numpy(), v_app[r]), f"appended v of row {r}"
        assert torch.equal(kp.cpu().view(torch.int16), inp.kp.view(torch.int16)) and torch.equal(vp.cpu().view(torch.int16), inp.vp.view(torch.int16)), \
            "the prefix was written"
        outs.append(o.cpu().view(torch.int16))
    assert torch.equal(outs[0], outs[1]), "an eager grid and a captured grid give different bits"


def test_group_kernel_is_deterministic_through_one_workspace():
    from aki_amd import ops
    case = G.CASE_BY_ID[G.LARGEST]
    inp = G.make_inputs(case, "diffuse")
    ws = ops.decode_attn_group_workspace(case.B0, case.N, case.H, G.DH, case.pcap, case.scap, DEV)
    first = None
    for _ in range(20):
        o = _launch(inp, case.key_bounds()[0], ws)[0].cpu().view(torch.int16)
        first = o if first is None else first
        assert torch.equal(o, first)


def test_group_abi_status_codes():
    from aki_amd import _lib
    lib = _lib.load()
    assert lib.aki_decode_attn_group_workspace_bytes(1, 2, 2, 96, 64, 64) > 0
    t = torch.zeros(1 << 16, dtype=BF, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)
    p = lambda x: x.data_ptr()
    args = lambda Dh, dt, wsb: (p(t), p(f), p(f), p(i), p(i), p(t), p(t), p(t), p(t), p(t), None, 0, 1, 2, 2, Dh, 64, 64, 0, 0, 0.1, dt, p(f), wsb, None)
    BF16, F32, UNSUPPORTED, WORKSPACE = 0, 1, -2, -4               # AKI_DT_* and AKI_ERR_* of include/aki_mi355x.h
    assert lib.aki_decode_attn_group_fwd(*args(64, BF16, f.numel() * 4)) == UNSUPPORTED
    assert lib.aki_decode_attn_group_fwd(*args(96, F32, f.numel() * 4)) == UNSUPPORTED
    assert lib.aki_decode_attn_group_fwd(*args(96, BF16, 16)) == WORKSPACE


def _prefill(m, vx, lx, am, cap_extra):
    vt = m.vision_tokenizer(m._encode_vision_x(vx))
    prep = m._prepare_inputs_for_forward(vision_tokens=vt, lang_x=lx, attention_mask=am, padding_side="right")
    L = prep["inputs_embeds"].shape[1]
    out = m.lang_model(inputs_embeds=prep["inputs_embeds"], attention_mask=prep["attention_mask"], use_cache=True, cache_capacity=L + cap_extra,
                       last_token_logits=True)
    return out.past_key_values, out.logits[:, 0]


def test_grouped_cache_matches_replicated_cache_teacher_forced_and_replays_bit_exactly():
    from aki_amd.phi3 import DecodeGraph
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm, N, steps = m.lang_model, 4, 12
    B0 = lx.shape[0]
    with torch.no_grad():
        # 300 rows past the prompt: the suffix slab is five 64-key tiles and the prefix capacity five tiles past the prompt's, so the
        # captured grid carries four trailing empty items per segment that the eager grid (sized by the keys in use) does not
        grouped, logits = _prefill(m, vx, lx, am, 300)
        repl, _ = _prefill(m, vx, lx, am, 300)
        graphed, _ = _prefill(m, vx, lx, am, 300)
        assert grouped.k[0].shape[3] == 96, "the tiny model's head_dim is the grouped kernel's"
        grouped.share_prefix(N)
        graphed.share_prefix(N)
        repl.select_rows(torch.arange(B0, device=DEV).repeat_interleave(N))
        assert grouped.k[0].shape[0] == B0 and grouped.k_suffix[0].shape[0] == B0 * N and repl.k[0].shape[0] == B0 * N
        assert grouped.suffix_capacity >= 4 * 64 and grouped.capacity - grouped.prefix_host_len >= 4 * 64
        stepper = DecodeGraph(lm, graphed)
        gen_ = torch.Generator().manual_seed(5)
        worst = 0.0
        for t in range(steps):
            ids = torch.randint(3, logits.shape[-1] - 1, (B0 * N,), generator=gen_).to(DEV)
            a = lm.decode_step(input_ids=ids, past_key_values=grouped)
            b = lm.decode_step(input_ids=ids, past_key_values=repl)
            c = stepper.step(ids)
            assert torch.equal(a.view(torch.int16), c.view(torch.int16)), f"step {t}: eager and replayed grouped steps differ"
            err = (a.float() - b.float()).abs().max().item()
            bar = 2e-2 * max(1.0, b.float().abs().max().item())
            worst = max(worst, err / bar)
            assert err <= bar, f"step {t}: grouped vs replicated logits differ by {err:.3g} (bar {bar:.3g})"
        print(f"grouped vs replicated: worst err / bar {worst:.3f}")


def _count_share_prefix(monkeypatch):
    from aki_amd.phi3 import AkiKVCache
    calls, orig = [], AkiKVCache.share_prefix
    monkeypatch.setattr(AkiKVCache, "share_prefix", lambda self, n: (calls.append(n), orig(self, n))[1])
    return calls


@pytest.mark.parametrize("use_graph", [True, False])
def test_generate_shared_equals_a_loop_of_decode_step_and_sample_pick(use_graph):
    """Plumbing, so bit for bit: the draw's row index b * N + j, the call's offset, token 0 from the repeated prefill logits."""
    from aki_amd import DeviceGenerator, ops
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    B0, N, T, pad = lx.shape[0], 3, 12, 0
    lm = m.lang_model
    lm.share_prompt_kv = True
    got = m.generate(vx, lx, attention_mask=am, max_new_tokens=T, do_sample=True, temperature=1.5, top_k=40, top_p=0.9, eos_token_id=[],
                     pad_token_id=pad, num_return_sequences=N, generator=DeviceGenerator(11), use_graph=use_graph)
    with torch.no_grad():
        cache, logits = _prefill(m, vx, lx, am, T)
        logits = logits.repeat_interleave(N, dim=0).contiguous()
        cache.share_prefix(N)
        R = B0 * N
        tokens = torch.full((R, T), pad, dtype=torch.long, device=DEV)
        ids = torch.zeros(R, dtype=torch.long, device=DEV)
        kw = dict(pad_token_id=pad, done=torch.zeros(R, dtype=torch.uint8, device=DEV), tokens=tokens, start_len=cache.cache_len.clone(),
                  done_at=torch.full((R,), -1, dtype=torch.int32, device=DEV), temperature=1.5, top_k=40, top_p=0.9, seed=11,
                  offset=DeviceGenerator(11).next_offset())
        ops.sample_pick(logits, ids, cache_len=cache.cache_len, advance=False, **kw)
        for _ in range(1, T):
            lg = lm.decode_step(input_ids=ids, past_key_values=cache, advance=False)
            ops.sample_pick(lg, ids, cache_len=cache.cache_len, advance=True, **kw)
        torch.cuda.synchronize()
    assert got.shape == (R, T)
    assert torch.equal(got, tokens), f"rows that differ: {(got != tokens).any(1).nonzero().flatten().tolist()}"


def test_generate_num_return_sequences(monkeypatch):
    from aki_amd import DeviceGenerator
    shared_calls = _count_share_prefix(monkeypatch)
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    B0, N, T = lx.shape[0], 3, 16
    m.lang_model.share_prompt_kv = True
    kw = dict(attention_mask=am, max_new_tokens=T, do_sample=True, temperature=1.5, eos_token_id=[], pad_token_id=0, num_return_sequences=N)
    a = m.generate(vx, lx, generator=DeviceGenerator(7), **kw)
    b = m.generate(vx, lx, generator=DeviceGenerator(7), **kw)
    assert shared_calls == [N, N], "a bf16 model with a bf16 cache shares the prompt K/V"
    assert a.shape == (B0 * N, T) and torch.equal(a, b)
    for s0 in range(B0):
        rows = a[s0 * N:(s0 + 1) * N]
        assert all(not torch.equal(rows[0], rows[j]) for j in range(1, N)), f"sample {s0}: two continuations drew the same 16 tokens"
    m.lang_model.share_prompt_kv = False
    try:
        r = m.generate(vx, lx, generator=DeviceGenerator(7), **kw)
    finally:
        m.lang_model.share_prompt_kv = True
    assert len(shared_calls) == 2, "share_prompt_kv = False takes the replicated form"
    assert r.shape == a.shape and torch.equal(r[:, 0], a[:, 0]), "token 0 comes from the same prefill logits"
    forks = int((r != a).any(1).sum())
    print(f"shared vs replicated: {forks} of {B0 * N} rows fork")
    torch_rng = torch.Generator(device=DEV).manual_seed(1)          # the sample_next path draws on the logits' device
    e = m.generate(vx, lx, generator=torch_rng, use_graph=False, **kw)
    assert e.shape == (B0 * N, T)
    one = m.generate(vx, lx, generator=DeviceGenerator(7), **dict(kw, max_new_tokens=1))
    assert one.shape == (B0 * N, 1) and torch.equal(one[:, 0], a[:, 0])
    # eos per row: the token row 1 drew at index 2 ends every row that draws it, and no other
    eos = int(a[1, 2])
    z = m.generate(vx, lx, generator=DeviceGenerator(7), **dict(kw, eos_token_id=eos))
    assert z.shape[0] == B0 * N
    for r_, row in enumerate(a.tolist()):
        want = row[:row.index(eos) + 1] if eos in row else row
        want = (want + [0] * T)[:z.shape[1]]
        assert z[r_].tolist() == want, f"row {r_}: eos handling"
    assert z[1].tolist()[:3] == a[1].tolist()[:3] or eos in a[1].tolist()[:2]
    plain = m.generate(vx, lx, generator=DeviceGenerator(7), **dict(kw, num_return_sequences=3))
    p = m.generate(vx, lx, generator=DeviceGenerator(7), repetition_penalty=1.3, no_repeat_ngram_size=2, **kw)
    assert p.shape == plain.shape and torch.equal(p[:, 0], plain[:, 0]), "nothing to penalise before the first token"
    for row in p.tolist():
        grams = [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
        assert len(grams) == len(set(grams)), "no_repeat_ngram_size=2 was not honoured per row"
    with pytest.raises(ValueError):
        m.generate(vx, lx, attention_mask=am, max_new_tokens=3, num_return_sequences=2)
    with pytest.raises(ValueError):
        m.generate(vx, lx, attention_mask=am, max_new_tokens=3, do_sample=True, num_return_sequences=0)
    with pytest.raises(NotImplementedError):
        m.generate(vx, lx, attention_mask=am, max_new_tokens=3, num_beams=2, num_return_sequences=2)
    n_shared = len(shared_calls)
    m.lang_model.set_kv_cache_dtype("fp8_e4m3")
    try:
        f8 = m.generate(vx, lx, generator=DeviceGenerator(7), **kw)
    finally:
        m.lang_model.set_kv_cache_dtype("bf16")
    assert f8.shape == (B0 * N, T) and len(shared_calls) == n_shared, "an fp8_e4m3 cache takes the replicated form"
    m32, g32 = build_tiny(torch.float32)
    m32.lang_model.share_prompt_kv = True
    vx32, lx32, am32, _ = batch(g32, torch.float32)
    f32 = m32.generate(vx32, lx32, **dict(kw, attention_mask=am32))
    assert f32.shape == (B0 * N, T) and len(shared_calls) == n_shared, "an fp32 model takes the replicated form"
