"""MXFP4 decode weights on the one-launch decode chain (Phi3Model.decode_chain_w4, aki_decode_chain_fwd with AKI_DT_W4A16): the chained step
reproduces the five launches per layer of enable_mxfp4() bit for bit.  The chain exists at Phi-3.5-mini's width only (d 3072, F 8192, 32 heads
of 96), so a 3-layer stack of that width with a 4096-token vocabulary is the smallest model these tests can use; it is built once."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _full_width_lm(n_layers, seed=0):
    from aki_amd.phi3 import Phi3ForCausalLM, make_phi3_config
    torch.manual_seed(seed)
    cfg = make_phi3_config(num_hidden_layers=n_layers, vocab_size=4096, pad_token_id=0, eos_token_id=2)
    lm = Phi3ForCausalLM(cfg)
    g = torch.Generator().manual_seed(seed)
    for n, p in lm.named_parameters():
        if p.dim() == 1:
            p.data.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))          # non-unit RMSNorm gains
        else:
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return lm.to(DEV).to(torch.bfloat16).eval(), cfg


@functools.lru_cache(maxsize=None)
def _models():
    """(the 3-layer model with MXFP4 decode weights, a copy of it that was never quantised, the config)."""
    lm, cfg = _full_width_lm(3)
    twin = copy.deepcopy(lm)
    lm.enable_mxfp4()
    return lm, twin, cfg


def _prompt(cfg, prompt, B=1):
    from aki_amd import ops
    x = (torch.randn(B, prompt, cfg.hidden_size, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(DEV)
    am = np.ones((B, prompt), dtype=bool)
    am[:, 3:9] = False                                        # a hole in the prompt: the valid-column bits are honoured
    table = ops.MaskTable.from_host([[(4, 40, 40, prompt - 8)]] * B, am, [prompt] * B, DEV)
    return x, table


def _decode(lm, cfg, prompt, steps, B=1, graph=False):
    """Prefill + `steps` greedy decode steps -> (logits of every step, the K rows, the V rows, the cache)."""
    from aki_amd.phi3 import DecodeGraph
    x, table = _prompt(cfg, prompt, B)
    with torch.no_grad():
        out = lm(inputs_embeds=x, attention_mask=table, use_cache=True, cache_capacity=prompt + steps + 3)
        cache = out.past_key_values
        ids = out.logits[:, -1].float().argmax(-1)
        stepper = DecodeGraph(lm, cache) if graph else None
        logits = []
        for _ in range(steps):
            lg = stepper.step(ids) if graph else lm.decode_step(input_ids=ids, past_key_values=cache)
            logits.append(lg.clone())
            ids = lg.float().argmax(-1)
    torch.cuda.synchronize()
    return torch.stack(logits), cache


def _rows(cache, n):
    return [t[:, :, :n].clone() for t in list(cache.k) + list(cache.v)]


class _switch:
    """`decode_chain_w4` on one model for the length of a with block."""

    def __init__(self, lm, on):
        self.m, self.on = lm.model, on

    def __enter__(self):
        self.m.decode_chain_w4 = self.on

    def __exit__(self, *exc):
        del self.m.decode_chain_w4                             # back to the class default


@pytest.mark.parametrize("prompt,steps", [(655, 6), (70, 70)])
def test_w4_chain_is_bit_identical_to_the_five_launch_w4_path(prompt, steps):
    """enable_mxfp4(), a prompt with a hole in its mask, greedy decode steps: with `decode_chain_w4` the step is ONE launch whose logits and
    appended K/V rows equal the five launches per layer bit for bit - at the flagship prompt length, and over 70 steps from 70 keys (across a
    64-key tile boundary, 70 calls on one workspace).  The chain exists exactly when the switch is on, and no dependency wait gave up."""
    lm, _, cfg = _models()
    outs = {}
    for on in (False, True):
        with _switch(lm, on):
            logits, cache = _decode(lm, cfg, prompt, steps)
        chain = getattr(cache, "chain", None)
        assert (chain is not None) == on
        if on:
            assert chain.fmt == "w4" and not chain.w8 and chain.error_code() == 0
        outs[on] = (logits, _rows(cache, prompt + steps))
    a, b = outs[False], outs[True]
    assert bool(torch.isfinite(a[0].float()).all())
    assert torch.equal(a[0], b[0]), f"{int((a[0] != b[0]).sum())} logits differ over {steps} steps"
    for ra, rb in zip(a[1], b[1]):
        assert torch.equal(ra, rb)


def test_w4_chain_graph_replay_equals_eager_chained_steps():
    """The MXFP4 chained step captured into a hipGraph and replayed (DecodeGraph) equals the eager chained steps bit for bit over 8 steps."""
    lm, _, cfg = _models()
    res = {}
    with _switch(lm, True):
        for graph in (False, True):
            logits, cache = _decode(lm, cfg, 200, 8, graph=graph)
            assert cache.chain is not None and cache.chain.fmt == "w4" and cache.chain.error_code() == 0
            res[graph] = logits
    assert torch.equal(res[False], res[True]), f"{int((res[False] != res[True]).sum())} logits differ between eager and replayed steps"


def test_generate_with_the_w4_chain_equals_generate_on_five_launches(monkeypatch):
    """AKI.generate (a 2-layer full-width decoder behind a small vision tower, MXFP4 decode weights, 24 greedy tokens): the tokens with the
    switch on equal the tokens with it off, in the eager loop and in the captured one; with the switch off no chain is ever built."""
    from aki_amd import ops
    from aki_amd.factory import build_aki
    from aki_amd.phi3 import make_phi3_config
    from aki_amd.siglip import make_siglip_config
    m = build_aki(lm_config=make_phi3_config(num_hidden_layers=2), vis_config=make_siglip_config(num_hidden_layers=1, image_size=224),
                  dtype=torch.bfloat16, device=DEV, seed=3).eval()
    m.lang_model.enable_mxfp4()
    built = []

    class Counting(ops.DecodeChain):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self.fmt)

    monkeypatch.setattr(ops, "DecodeChain", Counting)
    g = torch.Generator(device="cpu").manual_seed(5)
    n_txt = 40
    ids = torch.randint(3, 32000, (1, n_txt), generator=g)
    ids[0, 0], ids[0, 6] = 1, m.media_token_id
    vx = ((torch.rand((1, 1, 1, 3, 224, 224), generator=g) - 0.5) / 0.5).to(DEV, torch.bfloat16)
    ids, am = ids.to(DEV), torch.ones(1, n_txt, dtype=torch.long, device=DEV)
    for use_graph in (False, True):
        outs = {}
        for on in (False, True):
            del built[:]
            with _switch(m.lang_model, on):
                outs[on] = m.generate(vx, ids, attention_mask=am, max_new_tokens=24, do_sample=False, eos_token_id=[], use_graph=use_graph)
            assert built == (["w4"] if on else []), (use_graph, on, built)
        assert outs[True].shape == (1, 24) and torch.equal(outs[True], outs[False]), use_graph


def test_w4_chain_with_fp8_prefill_weights_too():
    """enable_fp8() + enable_mxfp4(): the decode rows are MXFP4 (Phi3DecoderLayer.decode prefers them), so the chain is the MXFP4 one and its
    logits equal the five-launch logits."""
    lm, _, cfg = _models()
    lm.enable_fp8()
    try:
        outs = {}
        for on in (False, True):
            with _switch(lm, on):
                outs[on], cache = _decode(lm, cfg, 200, 4)
            chain = getattr(cache, "chain", None)
            assert (chain is not None) == on
            if on:
                assert chain.fmt == "w4" and chain.error_code() == 0
        assert torch.equal(outs[False], outs[True])
    finally:
        lm.enable_fp8(False)


@pytest.mark.parametrize("case", ["fp8_kv_cache", "batch_2"])
def test_the_chains_other_gates_still_hold_with_the_switch_on(case):
    """An fp8_e4m3 KV cache, and two sequences: no chain with the switch on either, and the results of the switch-off run."""
    lm, _, cfg = _models()
    B = 2 if case == "batch_2" else 1
    if case == "fp8_kv_cache":
        lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        outs = {}
        for on in (False, True):
            with _switch(lm, on):
                outs[on], cache = _decode(lm, cfg, 200, 4, B=B)
            assert getattr(cache, "chain", None) is None
        assert torch.equal(outs[False], outs[True])
    finally:
        lm.set_kv_cache_dtype("bf16")


def test_switching_mxfp4_off_after_a_w4_chained_run_rebuilds_a_bf16_chain():
    """enable_mxfp4(False) after MXFP4-chained steps: the next cache's chain is the bf16 one and its logits equal those of a copy of the model
    that was never quantised, bit for bit."""
    lm, twin, cfg = _models()
    try:
        with _switch(lm, True):
            _, cache = _decode(lm, cfg, 200, 3)
            assert cache.chain is not None and cache.chain.fmt == "w4"
            lm.enable_mxfp4(False)
            got, cache = _decode(lm, cfg, 200, 3)
            assert cache.chain is not None and cache.chain.fmt == "bf16" and cache.chain.error_code() == 0
        want, tcache = _decode(twin, cfg, 200, 3)
        assert tcache.chain is not None and tcache.chain.fmt == "bf16"
        assert torch.equal(got, want)
    finally:
        lm.enable_mxfp4()


def test_abi_errors_of_the_w4_chain():
    """aki_decode_chain_fwd with AKI_DT_W4A16: two sequences -> AKI_ERR_UNSUPPORTED, a NULL descriptor table -> AKI_ERR_INVALID_ARG (the
    answers AKI_DT_W8A16 gives), nothing launched.  The descriptors themselves live in device memory, out of the entry point's sight - for
    MXFP4 as for e4m3 - so missing or misshapen scale tensors are refused where the table is built: ops.DecodeChain raises."""
    from aki_amd import _lib as L
    from aki_amd import ops
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    H, Dh, d, F, cap, n_layers = 32, 96, 3072, 8192, 64, 1
    nbytes = int(lib.aki_decode_chain_batch_workspace_bytes(n_layers, d, H, F, cap, 1))
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=DEV)
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    table = torch.zeros((n_layers, 12), dtype=torch.int64, device=DEV)
    h = torch.zeros((2, d), dtype=torch.bfloat16, device=DEV)
    h_out = torch.full((2, d), 7.0, dtype=torch.bfloat16, device=DEV)
    cs = torch.zeros((cap, Dh), dtype=torch.float32, device=DEV)
    ln = torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(dtype, batch, layers=table.data_ptr()):
        a = L.DecodeChainArgs(layers, h.data_ptr(), h_out.data_ptr(), cs.data_ptr(), cs.data_ptr(), ln.data_ptr(), None, ws_ptr, nbytes,
                              n_layers, 0, d, H, Dh, F, cap, 1, Dh ** -0.5, 1e-5, dtype, batch)
        return lib.aki_decode_chain_fwd(C.byref(a), st)

    assert L.AKI_DT_W4A16 == 4
    assert call(L.AKI_DT_W4A16, 2) == -2                          # AKI_ERR_UNSUPPORTED
    assert call(L.AKI_DT_W4A16, 1, layers=None) == call(L.AKI_DT_W8A16, 1, layers=None) == -1       # AKI_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((h_out == 7.0).all()) and not bool(ws.any()), "a refused call must not launch"

    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    n1 = torch.ones(d, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros((1, H, cap, Dh), dtype=torch.bfloat16, device=DEV)
    wq, wo, wg, wd = u8(3 * d, d // 2), u8(d, d // 2), u8(2 * F, d // 2), u8(d, F // 2)
    sq, so, sg, sd = u8(3 * d, d // 32), u8(d, d // 32), u8(2 * F, d // 32), u8(d, F // 32)
    build = lambda row, fmt="w4": ops.DecodeChain([row], [kc], [kc], H, Dh, d, F, cap, Dh ** -0.5, 1e-5, DEV, fmt)
    assert build((wq, wo, wg, wd, n1, n1, sq, so, sg, sd)).fmt == "w4"
    assert build((wq.view(torch.bfloat16), wo.view(torch.bfloat16), wg.view(torch.bfloat16), wd.view(torch.bfloat16), n1, n1, None, None, None, None),
                 False).fmt == "bf16"                             # the argument's earlier values still work
    with pytest.raises(ops.AkiError):
        build((wq, wo, wg, wd, n1, n1, sq, None, sg, sd))         # a missing scale tensor
    with pytest.raises(ops.AkiError):
        build((wq, wo, wg, wd, n1, n1, sq, so, sg, u8(d, F // 64)))       # scales of the wrong shape
    with pytest.raises(ops.AkiError):
        build((wq, wo, wg, wd, n1, n1, sq.float(), so, sg, sd))   # f32 scales are the e4m3 format's
    with pytest.raises(ops.AkiError):
        build((wq, wo, wg, wd, n1, n1, sq, so, sg, sd), "w2")
