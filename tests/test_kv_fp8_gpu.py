"""fp8 (e4m3) KV cache on the GPU: the one-launch conversion of the prefill's bf16 rows, the fused decode step on e4m3 rows (against
an f32 reference built from the kernel's own stored bytes and scales), graph replay, the model level (prefill bit-identical to the bf16
cache, decode equal to a bf16 cache holding the same quantised rows) and every decoding path of AKI.generate."""
import numpy as np
import pytest
import torch

import aki_oracle as O
from test_kernels_gpu import check, n, DEV
from test_model_gpu import build_tiny, batch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def ref_quant(x: torch.Tensor):
    """The documented rule in f32 on the host: s = max(amax, 1e-12) / 448 per row of 96, bytes = e4m3(x / s), RNE, saturating."""
    x = x.detach().float().cpu()
    s = x.abs().amax(-1).clamp(min=1e-12) / 448.0
    q = (x / s[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s


def deq(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).float() * s.float()[..., None]


# ---- 1. the quantiser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers,B,H,Ls,cap", [(2, 2, 3, 70, 100), (1, 3, 32, 655, 655)])
def test_kv_cache_quantiser_matches_torch_e4m3_byte_for_byte(n_layers, B, H, Ls, cap):
    from aki_amd import ops
    g = torch.Generator().manual_seed(Ls)
    src = (torch.randn((2, n_layers, B, H, Ls, 96), generator=g) * 3).to(BF)
    src[0, 0, 0, 0, 0] = 0.0                                          # an all-zero head row
    src[1, -1, -1, -1, 1] = 0.0
    src[0, 0, 0, 1, 2, :5] = torch.tensor([448.0, -448.0, 1e-3, 0.0, 17.0])   # the e4m3 edges
    src[1, 0, 0, 0, 3, 7] = -448.0
    src[0, 0, -1, 0, 4] *= 1e-4                                       # small rows: e4m3 subnormals
    dst = torch.full((2, n_layers, B, H, cap, 96), 0x5A, dtype=torch.uint8, device=DEV)
    sc = torch.full((2, n_layers, B, H, cap), -1.0, dtype=torch.float32, device=DEV)
    ops.kv_cache_quant_fp8(src.to(DEV), dst, sc, Ls)
    torch.cuda.synchronize()
    q_ref, s_ref = ref_quant(src)
    got_q, got_s = dst[..., :Ls, :].cpu(), sc[..., :Ls].cpu()
    assert torch.equal(got_s, s_ref), f"{int((got_s != s_ref).sum())} scales differ"
    assert torch.equal(got_q, q_ref), f"{int((got_q != q_ref).sum())} of {q_ref.numel()} bytes differ from torch's e4m3 cast"
    assert bool((got_q[0, 0, 0, 0, 0] == 0).all()) and float(got_s[0, 0, 0, 0, 0]) == np.float32(1e-12) / np.float32(448)
    assert bool((dst[..., Ls:, :] == 0x5A).all()) and bool((sc[..., Ls:] == -1.0).all()), "rows past the staged ones were written"


# ---- 2. the fused decode step -------------------------------------------------------------------------------------------------
def _rotate_bf16(x, c, s):
    """RoPE rotate-half in f32 as the kernels do it (two products, one add), then rounded to bf16."""
    h = x.shape[-1] // 2
    lo = x[..., :h] * c[..., :h] - x[..., h:] * s[..., :h]
    hi = x[..., h:] * c[..., h:] + x[..., :h] * s[..., h:]
    return torch.cat([lo, hi], -1).to(BF).float()


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("n_keys", [1, 63, 64, 65, 655, 4096])
def test_fused_fp8kv_decode_step_against_its_own_stored_rows(B, n_keys):
    from aki_amd import ops
    H, Dh = 4, 96
    cap = n_keys + 5
    g = torch.Generator().manual_seed(1000 * B + n_keys)
    lens = [max(0, n_keys - 1 - 7 * (b % 3)) for b in range(B)]      # per-sample lengths, the longest n_keys - 1
    lens[0] = n_keys - 1
    k8 = torch.empty((B, H, cap, Dh), dtype=torch.uint8, device=DEV)
    v8 = torch.empty_like(k8)
    ks = torch.empty((B, H, cap), dtype=torch.float32, device=DEV)
    vs = torch.empty_like(ks)
    kv = (torch.randn((2, B, H, cap, Dh), generator=g) * 2).to(BF).to(DEV)
    both = torch.empty((2, B, H, cap, Dh), dtype=torch.uint8, device=DEV)
    bsc = torch.empty((2, B, H, cap), dtype=torch.float32, device=DEV)
    ops.kv_cache_quant_fp8(kv, both, bsc, cap)
    k8.copy_(both[0]); v8.copy_(both[1]); ks.copy_(bsc[0]); vs.copy_(bsc[1])
    for b, ln in enumerate(lens):                 # rows at and past the append position are unwritten cache: NaN bytes and scales
        k8[b, :, ln:] = 0x7F
        v8[b, :, ln:] = 0xFF
        ks[b, :, ln:] = float("nan")
        vs[b, :, ln:] = float("nan")
    qkv = torch.randn((B, 3 * H * Dh), generator=g).to(BF)
    cos, sin = O.rope_cos_sin(np.arange(cap)[None], Dh)
    tc, ts = torch.from_numpy(cos[0]).to(DEV), torch.from_numpy(sin[0]).to(DEV)
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    am = np.ones((B, cap), dtype=bool)                # holes in the prompt masks
    for b, ln in enumerate(lens):
        if ln > 8:
            am[b, 3:7] = False
        if ln > 200:
            am[b, 100:170] = False
    bits = ops.MaskTable.from_host([[(0, 0, 0, 0)]] * B, am, None, DEV).col_valid_bits
    ws = ops.decode_attn_workspace(B, H, Dh, cap, DEV)
    k0, v0, ks0, vs0 = k8.clone(), v8.clone(), ks.clone(), vs.clone()
    scale = Dh ** -0.5
    for rep in range(2):                          # twice through one workspace: the arrival counters re-arm themselves
        k8.copy_(k0); v8.copy_(v0); ks.copy_(ks0); vs.copy_(vs0)
        got = ops.decode_attn_fused(qkv.to(DEV), tc, ts, cl, k8, v8, H, scale, bits, max(lens) + 1, ws, ks, vs)
        torch.cuda.synchronize()
        # the appended rows: torch's quantisation of the bf16-rounded rotated k and of v
        q3 = qkv.float().view(B, 3, H, Dh)
        for b, ln in enumerate(lens):
            c, s = torch.from_numpy(cos[0][ln]), torch.from_numpy(sin[0][ln])
            qk, sk = ref_quant(_rotate_bf16(q3[b, 1], c, s))
            qv, sv = ref_quant(q3[b, 2])
            assert torch.equal(k8[b, :, ln].cpu(), qk) and torch.equal(ks[b, :, ln].cpu(), sk), f"appended k row of sample {b}"
            assert torch.equal(v8[b, :, ln].cpu(), qv) and torch.equal(vs[b, :, ln].cpu(), sv), f"appended v row of sample {b}"
            assert torch.equal(k8[b, :, :ln], k0[b, :, :ln]) and torch.equal(vs[b, :, :ln], vs0[b, :, :ln]), "cached rows changed"
        # the output: f32 attention over the kernel's own stored bytes and scales
        want = np.zeros((B, H * Dh), dtype=np.float64)
        K, V = deq(k8.cpu(), ks.cpu()).double(), deq(v8.cpu(), vs.cpu()).double()
        for b, ln in enumerate(lens):
            nk = ln + 1
            c, s = torch.from_numpy(cos[0][ln]), torch.from_numpy(sin[0][ln])
            qr = _rotate_bf16(q3[b, 0], c, s).double()
            keep = torch.from_numpy(am[b, :nk])
            for h in range(H):
                sc_ = (K[b, h, :nk] @ qr[h]) * scale
                sc_ = torch.where(keep, sc_, torch.tensor(-float("inf"), dtype=torch.float64))
                want[b, h * Dh:(h + 1) * Dh] = (torch.softmax(sc_, -1) @ V[b, h, :nk]).numpy()
        check(n(got), want.astype(np.float32), BF, f"fused fp8-KV decode B={B} n_keys={n_keys} (pass {rep})", scale_atol=2.0)
    assert int(ws[: B * H].abs().sum()) == 0


# ---- 3./4. the model level, on the tiny AKI ---------------------------------------------------------------------------------
def _prefill(m, vx, lx, am):
    with torch.no_grad():
        out = m(vx, lx, attention_mask=am, use_cache=True)
    return out.logits, out.past_key_values


def test_prefill_is_bit_identical_and_the_graph_replays_the_eager_steps():
    from aki_amd.phi3 import DecodeGraph
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    lg16, c16 = _prefill(m, vx, lx, am)
    lm.set_kv_cache_dtype("fp8_e4m3")
    lg8, c8 = _prefill(m, vx, lx, am)
    assert c16.kv_dtype == "bf16" and c8.kv_dtype == "fp8_e4m3" and c8.k[0].dtype == torch.uint8
    assert torch.equal(lg16, lg8), "the prefill must not see the cache format"
    assert torch.equal(c16.cache_len, c8.cache_len) and c16.host_len == c8.host_len
    # the converted rows are the quantised bf16 rows of the bf16 prefill
    L = int(c8.host_len)
    for i in range(len(c8.k)):
        qk, sk = ref_quant(c16.k[i][:, :, :L])
        assert torch.equal(c8.k[i][:, :, :L].cpu(), qk) and torch.equal(c8.k_scale[i][:, :, :L].cpu(), sk)
        qv, sv = ref_quant(c16.v[i][:, :, :L])
        assert torch.equal(c8.v[i][:, :, :L].cpu(), qv) and torch.equal(c8.v_scale[i][:, :, :L].cpu(), sv)
    # 16 steps eager and replayed from two identical fp8 prefills: the same bits
    res = {}
    with torch.no_grad():
        for mode in ("eager", "graph"):
            _, cache = _prefill(m, vx, lx, am)
            ids = lg8[torch.arange(lx.shape[0]), cache.cache_len.long() - 1].float().argmax(-1)
            st = DecodeGraph(lm, cache) if mode == "graph" else None
            steps = []
            for _ in range(16):
                lg = st.step(ids) if st is not None else lm.decode_step(input_ids=ids, past_key_values=cache)
                steps.append(lg.clone())
                ids = lg.float().argmax(-1)
            res[mode] = torch.stack(steps)
            assert cache.chain is None
    assert torch.equal(res["eager"], res["graph"]), f"{int((res['eager'] != res['graph']).sum())} logits differ"
    lm.set_kv_cache_dtype("bf16")


def test_teacher_forced_decode_equals_a_bf16_cache_holding_the_quantised_rows():
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model
    _, c16 = _prefill(m, vx, lx, am)              # the plain bf16 cache
    _, cq = _prefill(m, vx, lx, am)               # a bf16 cache that will hold the fp8 cache's rows, dequantised
    lm.set_kv_cache_dtype("fp8_e4m3")
    _, c8 = _prefill(m, vx, lx, am)
    lm.set_kv_cache_dtype("bf16")
    B = lx.shape[0]
    toks = torch.randint(0, 32000, (32, B), generator=torch.Generator().manual_seed(3)).to(DEV)
    worst_q = worst_plain = 0.0
    with torch.no_grad():
        for t in range(32):
            for i in range(len(c8.k)):            # cq := dequant(c8) over every row written so far
                n_rows = int(c8.host_len)
                cq.k[i][:, :, :n_rows] = deq(c8.k[i][:, :, :n_rows], c8.k_scale[i][:, :, :n_rows]).to(BF)
                cq.v[i][:, :, :n_rows] = deq(c8.v[i][:, :, :n_rows], c8.v_scale[i][:, :, :n_rows]).to(BF)
            l8 = lm.decode_step(input_ids=toks[t], past_key_values=c8).float()
            lq = lm.decode_step(input_ids=toks[t], past_key_values=cq).float()
            l16 = lm.decode_step(input_ids=toks[t], past_key_values=c16).float()
            mx = max(1.0, float(lq.abs().max()))
            worst_q = max(worst_q, float((l8 - lq).abs().max()) / mx)
            worst_plain = max(worst_plain, float((l8 - l16).abs().max()) / mx)
    print(f"fp8 cache vs bf16 cache of the same quantised rows: {worst_q:.3g}; vs the plain bf16 cache: {worst_plain:.3g} (of max |logit|)")
    assert worst_q <= 3e-2, worst_q               # the bf16 decode tolerance (test_decode_gpu.py: continuation vs full forward)
    assert worst_plain <= 0.5, worst_plain        # reported; only a sanity bound


# ---- 5. the decoding paths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
def test_generate_paths_on_the_fp8_cache(rows):
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    vx, lx, am = vx[:rows], lx[:rows], am[:rows]
    if rows == 1:
        lx, am = lx[:, : int(am[0].sum())], am[:, : int(am[0].sum())]
    m.lang_model.set_kv_cache_dtype("fp8_e4m3")
    try:
        eager = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=False)
        graph = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=True)
        assert eager.shape == (rows, 9) and torch.equal(eager, graph)
        g1, g2 = (torch.Generator(device=DEV).manual_seed(7) for _ in range(2))
        a = m.generate(vx, lx, attention_mask=am, max_new_tokens=6, eos_token_id=[], do_sample=True, top_k=5, generator=g1)
        b = m.generate(vx, lx, attention_mask=am, max_new_tokens=6, eos_token_id=[], do_sample=True, top_k=5, generator=g2)
        assert a.shape == (rows, 6) and torch.equal(a, b)
        beam = m.generate(vx, lx, attention_mask=am, max_new_tokens=5, num_beams=2, eos_token_id=[])
        assert beam.shape == (rows, 5) and int(beam.min()) >= 0
        proc = m.generate(vx, lx, attention_mask=am, max_new_tokens=6, eos_token_id=[], repetition_penalty=1.3, no_repeat_ngram_size=2)
        assert proc.shape == (rows, 6)
    finally:
        m.lang_model.set_kv_cache_dtype("bf16")


def test_beam_reorder_keeps_the_scales_with_their_rows():
    """Expand one prompt to two beams, decode different tokens, swap the beams, decode again: each beam's logits equal those of its token
    sequence decoded alone - with scales left behind by the gather, the swapped rows would be dequantised with the other beam's scales."""
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    n0 = int(am[0].sum())
    vx, lx, am = vx[:1], lx[:1, :n0], am[:1, :n0]
    lm = m.lang_model
    lm.set_kv_cache_dtype("fp8_e4m3")
    seqs = [[11, 502, 77], [9000, 31, 4242]]
    with torch.no_grad():
        _, cache = _prefill(m, vx, lx, am)
        cache.select_rows(torch.tensor([0, 0], device=DEV))
        lm.decode_step(input_ids=torch.tensor([seqs[0][0], seqs[1][0]], device=DEV), past_key_values=cache)
        cache.select_rows(torch.tensor([1, 0], device=DEV))          # beam 0 now continues sequence 1
        lm.decode_step(input_ids=torch.tensor([seqs[1][1], seqs[0][1]], device=DEV), past_key_values=cache)
        both = lm.decode_step(input_ids=torch.tensor([seqs[1][2], seqs[0][2]], device=DEV), past_key_values=cache).float()
        alone = []
        for sq in (seqs[1], seqs[0]):
            _, c1 = _prefill(m, vx, lx, am)
            for tok in sq:
                lg = lm.decode_step(input_ids=torch.tensor([tok], device=DEV), past_key_values=c1)
            alone.append(lg.float()[0])
    lm.set_kv_cache_dtype("bf16")
    for r in range(2):
        err = float((both[r] - alone[r]).abs().max())
        assert err <= 1e-2 * max(1.0, float(alone[r].abs().max())), f"beam {r}: {err:.3g}"


def _full_width_lm(n_layers, seed=0):
    from aki_amd.phi3 import Phi3ForCausalLM, make_phi3_config
    torch.manual_seed(seed)
    cfg = make_phi3_config(num_hidden_layers=n_layers, vocab_size=4096, pad_token_id=0, eos_token_id=2)
    lm = Phi3ForCausalLM(cfg)
    gg = torch.Generator().manual_seed(seed)
    for _, p in lm.named_parameters():
        p.data.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=gg) if p.dim() == 1 else torch.randn(p.shape, generator=gg) * 0.02)
    return lm.to(DEV).to(BF).eval(), cfg


def test_chain_stays_off_and_fp8_weights_combine_with_the_fp8_cache():
    from aki_amd import ops
    lm, cfg = _full_width_lm(1, seed=4)
    x = (torch.randn(2, 64, cfg.hidden_size, generator=torch.Generator().manual_seed(5)) * 0.5).to(BF).to(DEV)
    table = ops.MaskTable.from_host([[(0, 0, 0, 0)]] * 2, np.ones((2, 64), dtype=bool), None, DEV)

    toks = torch.randint(0, 4096, (3, 2), generator=torch.Generator().manual_seed(6)).to(DEV)

    def run(kv, fp8_weights, rows=2, steps=3):
        lm.enable_fp8(fp8_weights)
        lm.set_kv_cache_dtype(kv)
        with torch.no_grad():                     # teacher-forced: both formats see the same tokens
            out = lm(inputs_embeds=x[:rows], attention_mask=table if rows == 2 else None, use_cache=True, cache_capacity=80)
            cache, lgs = out.past_key_values, []
            for t in range(steps):
                lgs.append(lm.decode_step(input_ids=toks[t, :rows], past_key_values=cache).float())
        lm.set_kv_cache_dtype("bf16")
        lm.enable_fp8(False)
        return out.logits, torch.stack(lgs), cache

    _, _, c_bf16 = run("bf16", False, rows=1, steps=1)
    _, _, c_fp8 = run("fp8_e4m3", False, rows=1, steps=1)
    assert c_bf16.chain is not None and c_fp8.chain is None, "one sequence at Phi-3.5-mini's width: the chain serves bf16 caches only"
    p16, d16, _ = run("bf16", True)
    p8, d8, _ = run("fp8_e4m3", True)
    assert torch.equal(p16, p8)
    assert bool(torch.isfinite(d8).all())
    err = float((d8 - d16).abs().max()) / max(1.0, float(d16.abs().max()))
    print(f"e4m3 weights, fp8 vs bf16 cache: {err:.3g} of max |logit|")
    assert err <= 0.5


def test_switching_back_to_bf16_is_bit_identical_to_never_switching():
    m, g = build_tiny(BF)
    vx, lx, am, _ = batch(g, BF)
    lm = m.lang_model

    def run():
        with torch.no_grad():
            lg, cache = _prefill(m, vx, lx, am)
            ids = lg[torch.arange(lx.shape[0]), cache.cache_len.long() - 1].float().argmax(-1)
            out = [lg]
            for _ in range(4):
                lg = lm.decode_step(input_ids=ids, past_key_values=cache)
                out.append(lg.reshape(lg.shape[0], 1, -1))
                ids = lg.float().argmax(-1)
        return cache, out

    c0, before = run()
    lm.set_kv_cache_dtype("fp8_e4m3")
    c1, _ = run()
    lm.set_kv_cache_dtype("bf16")
    c2, after = run()
    assert c0.kv_dtype == c2.kv_dtype == "bf16" and c1.kv_dtype == "fp8_e4m3"
    assert all(torch.equal(a, b) for a, b in zip(before, after))
