"""Opt-in MXFP4 weight-only decode on the GPU: the quantiser bit for bit against the numpy reference (mxfp4_cases.py), ops.linear_w4 on
every case of the table against the f64 reference on the dequantised weights, the error paths of the C entry point, and the model switch
(Phi3ForCausalLM.enable_mxfp4) on a small Phi-3 stack and through generate."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxfp4_cases as MC
from conftest import record_parity
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _t(a, dtype=BF):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


# ---- 1. / 2. quantiser and dequantiser -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,K", [("spread", 13, 32), ("edges", 13, 2080), ("spread", 36, 3072), ("edges", 20, 8192), ("spread", 300, 256)])
def test_quantiser_is_bit_equal_to_the_reference(family, N, K):
    from aki_amd import ops
    w = MC.weights(family, N, K)
    wq_ref, ws_ref = MC.quant_ref(w)
    wq, ws = ops.quant_mxfp4(_t(w))
    assert wq.dtype == torch.uint8 and ws.dtype == torch.uint8 and wq.shape == (N, K // 2) and ws.shape == (N, K // 32)
    assert np.array_equal(ws.cpu().numpy(), ws_ref), "scale bytes"
    assert np.array_equal(wq.cpu().numpy(), wq_ref), f"{int((wq.cpu().numpy() != wq_ref).sum())} nibble bytes differ"
    # dequantiser: exactly the reference's values
    wd = ops.dequant_mxfp4(wq, ws)
    assert wd.dtype == BF and np.array_equal(wd.float().cpu().numpy().astype(np.float64), MC.dequant_ref(wq_ref, ws_ref))


def test_quantiser_strided_rows_subnormals_and_untouched_neighbours():
    from aki_amd import _lib as L, ops
    N, K, ld = 11, 96, 136                                       # rows 136 bf16 apart: 40 columns of other data between them
    w = MC.weights("edges", N, K)
    w[3, :32] = 0.0
    w[3, 5] = 2.0 ** -130                                        # a bf16 subnormal as a block's largest value: the byte clamps at 0
    w[4, 64:] *= 2.0 ** 100                                      # and large exponents
    w = MC.to_bf16(w)
    big = torch.full((N, ld), float("nan"), dtype=BF, device=DEV)
    big[:, :K] = _t(w)
    wq_ref, ws_ref = MC.quant_ref(w)
    pad = 64
    qbuf = torch.full((N * K // 2 + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((N * K // 32 + 2 * pad,), 0x5A, dtype=torch.uint8, device=DEV)
    wq, ws = qbuf[pad:pad + N * K // 2].view(N, K // 2), sbuf[pad:pad + N * K // 32].view(N, K // 32)
    L.check(L.load().aki_quant_mxfp4(big.data_ptr(), N, K, ld, wq.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(wq.cpu().numpy(), wq_ref) and np.array_equal(ws.cpu().numpy(), ws_ref)
    assert int(ws_ref[3, 0]) == 0
    assert bool((qbuf[:pad] == 0xA5).all() and (qbuf[-pad:] == 0xA5).all() and (sbuf[:pad] == 0x5A).all() and (sbuf[-pad:] == 0x5A).all())
    assert bool(torch.isnan(big[:, K:]).all())
    with pytest.raises(ops.AkiError):
        ops.quant_mxfp4(torch.zeros(4, 48, dtype=BF, device=DEV))     # K % 32 != 0


# ---- 3. / 4. the linear ------------------------------------------------------------------------------------------------------------
def _run_case(case):
    from aki_amd import ops
    d = MC.inputs(case)
    wq_ref, ws_ref, ref, tol = MC.reference(case)
    wq, ws = torch.from_numpy(wq_ref.copy()).to(DEV), torch.from_numpy(ws_ref.copy()).to(DEV)
    kw = dict(bias=_t(d["bias"]), residual=_t(d["residual"]), act=case.act, res_row_mod=case.res_row_mod)
    if case.norm:
        kw.update(rms_weight=_t(d["g"]), eps=MC.EPS)
    x = _t(d["x"])
    y = ops.linear_w4(x, wq, ws, **kw)
    y2 = ops.linear_w4(x, wq, ws, **kw)
    return y, y2, ref, tol


@pytest.mark.parametrize("case", MC.CASES, ids=[c.name for c in MC.CASES])
def test_linear_w4_against_f64_on_the_dequantised_weights(case):
    y, y2, ref, tol = _run_case(case)
    assert y.shape == (case.M, case.n_out) and y.dtype == BF
    got = y.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref) / tol
    i = np.unravel_index(ratio.argmax(), ratio.shape)
    record_parity(f"linear_w4 {case.name}: worst err/tol {ratio.max():.3f}", BF, np.abs(got - ref).max(), np.abs(got - ref).mean(),
                  np.abs(ref).max(), "2^-8|ref| + K 2^-24 S" if case.act == MC.ACT_NONE else "2^-7|ref| + 2e-3 max|ref|")
    print(f"{case.name}: worst err/tol {ratio.max():.3f} at {i} (got {got[i]:.6g}, ref {ref[i]:.6g})")
    assert ratio.max() <= 1.0, (case.name, i, got[i], ref[i], tol[i])
    assert torch.equal(y, y2), "two launches must give the same bits"


# ---- 5. bad calls ------------------------------------------------------------------------------------------------------------------
def test_bad_calls_answer_without_launching():
    from aki_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(17, 2048 + 16, dtype=BF, device=DEV)
    wq = torch.zeros(16 * 1024 + 64, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(16 * 64, dtype=torch.uint8, device=DEV)
    y = torch.full((17, 16), 7.0, dtype=BF, device=DEV)

    def call(M=1, N=16, K=2048, w=None, scale=ws.data_ptr(), ldw=None, dtype=L.AKI_DT_BF16, xp=x.data_ptr()):
        a = L.LinearArgs(xp, wq.data_ptr() if w is None else w, None, None, y.data_ptr(), M, N, K, x.stride(0), K // 2 if ldw is None else ldw,
                         y.stride(0), 0, 0, 0, dtype)
        return lib.aki_linear_w4_fwd(C.byref(a), scale, None, 0.0, st)

    assert call() == 0 and call(M=16) == 0                        # the well-formed calls go through
    y.fill_(7.0)
    assert call(K=2048 + 16) == -2                                # K % 32 != 0: AKI_ERR_UNSUPPORTED
    assert call(M=17) == -2
    assert call(M=2, K=64) == -2                                  # K = 64 at two rows: outside the skinny GEMM's gates
    assert call(dtype=L.AKI_DT_F32) == -2
    assert call(scale=None) == -1                                 # AKI_ERR_INVALID_ARG
    assert call(xp=None) == -1
    assert call(w=wq.data_ptr() + 8) == -3                        # AKI_ERR_ALIGNMENT
    assert call(M=4, w=wq.data_ptr() + 8) == -3
    assert call(ldw=1024 + 8) == -2                               # rows of w not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call must not launch"
    assert lib.aki_quant_mxfp4(x.data_ptr(), 4, 48, 64, wq.data_ptr(), ws.data_ptr(), st) == -2
    assert lib.aki_quant_mxfp4(None, 4, 64, 64, wq.data_ptr(), ws.data_ptr(), st) == -1
    assert lib.aki_quant_mxfp4(x.data_ptr() + 2, 4, 64, 64, wq.data_ptr(), ws.data_ptr(), st) == -3


# ---- 6. / 7. the model switch ------------------------------------------------------------------------------------------------------
def _small_lm():
    """The small Phi-3 stack of test_fp8_prefill_into_cache_and_w8_decode whose projection weights ARE MXFP4 values (dequant(quant(W))): the
    model itself is the bf16 twin of its own MXFP4 configuration - quantising it again is lossless, and both share the prefill bit for bit."""
    from aki_amd import ops
    from aki_amd.phi3 import Phi3ForCausalLM, make_phi3_config
    torch.manual_seed(0)
    cfg = make_phi3_config(vocab_size=1024, hidden_size=384, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=4,
                           num_key_value_heads=4, pad_token_id=0)
    lm = Phi3ForCausalLM(cfg)
    for p in lm.parameters():
        if p.dim() > 1:
            p.data.normal_(0, 0.05)
    lm = lm.to(DEV).to(BF).eval()
    with torch.no_grad():
        for ly in lm.model.layers:
            ly.input_layernorm.weight.add_(0.2 * torch.randn_like(ly.input_layernorm.weight))
            for lin in (ly.self_attn.qkv_proj, ly.self_attn.o_proj, ly.mlp.gate_up_proj, ly.mlp.down_proj):
                lin.weight.copy_(ops.dequant_mxfp4(*ops.quant_mxfp4(lin.weight.detach())))
        lm.lm_head.weight.copy_(ops.dequant_mxfp4(*ops.quant_mxfp4(lm.lm_head.weight.detach())))
    return lm, cfg


@torch.no_grad()
def _f32_last_logits(lm, cfg, seq):
    """The same weights evaluated in f32 by torch (the oracle's Phi-3 forward) on the whole sequence [B, L]: last-token logits [B, V]."""
    import aki_torch as OT
    p = {k: v.detach().float().cpu() for k, v in lm.state_dict().items()}
    B, L = seq.shape
    emb = lm.get_input_embeddings()(seq).detach().float().cpu()
    mask = torch.tril(torch.ones(L, L, dtype=torch.int64))[None, None].expand(B, 1, L, L)
    H = cfg.num_attention_heads
    cos, sin = OT.rope_cos_sin(np.arange(L)[None], cfg.hidden_size // H, float(cfg.rope_theta))
    add = OT.invert_mask_441(mask, torch.float32)
    h = emb
    for l in range(cfg.num_hidden_layers):
        h = OT.phi3_decoder_layer(h, OT._sub(p, f"model.layers.{l}."), cos, sin, add, H, float(cfg.rms_norm_eps))
    h = OT.rms_norm(h[:, -1], p["model.norm.weight"], float(cfg.rms_norm_eps))
    return h @ p["lm_head.weight"].T


@pytest.mark.parametrize("B", [1, 3])
def test_model_decode_against_its_bf16_twin_and_switching_off(B):
    from aki_amd import ops
    lm, cfg = _small_lm()
    lm.model.use_decode_chain = False                              # the twin's five-launch-per-layer path
    L0 = 70
    ids = torch.randint(1, 1000, (B, L0), generator=torch.Generator().manual_seed(3)).to(DEV)
    toks = torch.randint(1, 1000, (3, B), generator=torch.Generator().manual_seed(4)).to(DEV)

    def prefill():
        table = ops.MaskTable.causal(B, L0, DEV)
        return lm(inputs_embeds=lm.get_input_embeddings()(ids), attention_mask=table, use_cache=True, cache_capacity=L0 + 8).past_key_values

    with torch.no_grad():
        c_twin, c_w4 = prefill(), prefill()
        twin = [lm.decode_step(input_ids=toks[t], past_key_values=c_twin).float().cpu() for t in range(3)]
        lm.enable_mxfp4()
        assert lm.model.layers[0]._w4 is not None and set(lm.model.layers[0]._w4) == {"qkv", "o", "gate_up", "down"}
        w4 = [lm.decode_step(input_ids=toks[t], past_key_values=c_w4).float().cpu() for t in range(3)]
        assert c_w4.chain is None
        lm.enable_mxfp4(False)
        assert lm.model.layers[0]._w4 is None
        c_off = prefill()
        off = [lm.decode_step(input_ids=toks[t], past_key_values=c_off).float().cpu() for t in range(3)]
    for t in range(3):
        assert torch.equal(off[t], twin[t]), "enable_mxfp4(False) must restore the bf16 decode bit for bit"
        seq = torch.cat([ids, toks[:t + 1].T], 1)
        ref = _f32_last_logits(lm, cfg, seq)
        e_twin, e_w4 = float((twin[t] - ref).abs().max()), float((w4[t] - ref).abs().max())
        record_parity(f"MXFP4 decode step {t} batch {B} vs f32 torch: {e_w4:.4g} (its bf16 twin: {e_twin:.4g})", BF, e_w4,
                      float((w4[t] - ref).abs().mean()), float(ref.abs().max()), "2 x the bf16 twin's error")
        print(f"batch {B} step {t}: MXFP4 {e_w4:.4g}, bf16 twin {e_twin:.4g}, max |logit| {float(ref.abs().max()):.3g}")
        assert e_twin > 0 and e_w4 <= 2.0 * e_twin, (t, e_w4, e_twin)


def test_enable_mxfp4_refuses_what_it_cannot_quantise():
    from aki_amd import ops
    lm, _ = _small_lm()
    with torch.no_grad():
        lm.model.layers[1].mlp.down_proj.weight[5, 7] = float("inf")
    with pytest.raises(ops.AkiError):
        lm.enable_mxfp4()
    with pytest.raises(ops.AkiError):
        lm.float().enable_mxfp4()


# ---- 8. generate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
def test_generate_graph_and_eager_agree_with_mxfp4_weights(rows):
    from golden import gen
    from conftest import load_golden
    from test_model_gpu import batch
    from aki_amd.factory import build_aki
    from aki_amd.phi3 import make_phi3_config
    from aki_amd.siglip import make_siglip_config
    T = gen.TINY                                                   # the tiny model's vision tower and prompts; a decoder wide enough for the e4m3 prefill
    m = build_aki(make_phi3_config(vocab_size=T["vocab"], hidden_size=384, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, pad_token_id=T["pad_token_id"]),
                  make_siglip_config(hidden_size=T["vis_hidden"], intermediate_size=T["vis_inter"], num_hidden_layers=T["vis_layers"],
                                     num_attention_heads=T["vis_heads"], image_size=T["image"], patch_size=T["patch"]),
                  initial_tokenizer_len=T["vocab"], pad_token_id=T["pad_token_id"], num_vision_tokens=T["num_vision_tokens"], dtype=BF, device=DEV,
                  init_std=0.05, seed=3).eval()
    vx, lx, am, _ = batch(load_golden("tiny_e2e.npz"), BF)
    vx, lx, am = vx[:rows], lx[:rows], am[:rows]
    if rows == 1:
        lx, am = lx[:, : int(am[0].sum())], am[:, : int(am[0].sum())]
    plain = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=False)
    m.lang_model.enable_mxfp4()
    eager = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=False)
    graph = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=True)
    assert eager.shape == (rows, 9) and torch.equal(eager, graph)
    m.lang_model.enable_fp8()                                      # both switches on: prefill e4m3, decode rows MXFP4
    eager8 = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=False)
    graph8 = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=True)
    assert eager8.shape == (rows, 9) and torch.equal(eager8, graph8)
    m.lang_model.enable_fp8(False)
    m.lang_model.enable_mxfp4(False)
    again = m.generate(vx, lx, attention_mask=am, max_new_tokens=9, eos_token_id=[], use_graph=False)
    assert torch.equal(again, plain)
