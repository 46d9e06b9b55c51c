"""fp8 (e4m3) KV cache, the parts that need no GPU: the two C entry points are exported, listed in the ctypes table and validate
their arguments on the host; Phi3ForCausalLM.set_kv_cache_dtype accepts the documented formats only; an fp8 AkiKVCache has the
documented layout, about half the bytes of the bf16 one, and beam search's row gather moves its scales with its bytes."""
import ctypes as C

import pytest
import torch

AKI_ERR_INVALID_ARG, AKI_ERR_UNSUPPORTED, AKI_DT_BF16, AKI_DT_F32 = -1, -2, 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()                                    # cross-compiles for gfx950 without a GPU
    from aki_amd import _lib
    return _lib.load()


def test_fp8_kv_symbols_are_exported_and_bound(lib):
    from aki_amd import _lib
    for name in ("aki_kv_cache_quant_fp8", "aki_decode_attn_fused_fp8kv_fwd"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.aki_abi_version() == 17


def test_quantiser_validates_on_the_host(lib):
    f = lib.aki_kv_cache_quant_fp8
    p = C.c_void_p(4096)                          # never dereferenced: every call below is refused before a launch
    assert f(None, 8, p, p, 8, 4, 8, 96, AKI_DT_BF16, None) == AKI_ERR_INVALID_ARG
    assert f(p, 8, None, p, 8, 4, 8, 96, AKI_DT_BF16, None) == AKI_ERR_INVALID_ARG
    assert f(p, 8, p, None, 8, 4, 8, 96, AKI_DT_BF16, None) == AKI_ERR_INVALID_ARG
    assert f(p, 8, p, p, 8, 4, 9, 96, AKI_DT_BF16, None) == AKI_ERR_INVALID_ARG          # more rows than the staging cache holds
    assert f(p, 8, p, p, 8, 4, 8, 64, AKI_DT_BF16, None) == AKI_ERR_UNSUPPORTED
    assert f(p, 8, p, p, 8, 4, 8, 96, AKI_DT_F32, None) == AKI_ERR_UNSUPPORTED


def test_fused_fp8kv_decode_validates_on_the_host(lib):
    f = lib.aki_decode_attn_fused_fp8kv_fwd
    p = C.c_void_p(4096)

    def call(ptrs, Dh=96, dtype=AKI_DT_BF16):
        return f(*ptrs, None, 0, 2, 32, Dh, 128, 0, 96 ** -0.5, dtype, p, 1 << 20, None)

    for i in range(9):                            # qkv, cos, sin, cache_len, k, v, k_scale, v_scale, o
        ptrs = [p] * 9
        ptrs[i] = None
        assert call(ptrs) == AKI_ERR_INVALID_ARG, i
    assert call([p] * 9, Dh=64) == AKI_ERR_UNSUPPORTED
    assert call([p] * 9, Dh=128) == AKI_ERR_UNSUPPORTED
    assert call([p] * 9, dtype=AKI_DT_F32) == AKI_ERR_UNSUPPORTED


def _tiny_lm():
    from aki_amd.phi3 import Phi3ForCausalLM, make_phi3_config
    with torch.device("meta"):
        return Phi3ForCausalLM(make_phi3_config(vocab_size=64, pad_token_id=0, hidden_size=192, intermediate_size=256, num_hidden_layers=2,
                                                num_attention_heads=2, num_key_value_heads=2))


def test_set_kv_cache_dtype_accepts_bf16_and_fp8_e4m3_only():
    lm = _tiny_lm()
    assert lm.kv_cache_dtype == "bf16"
    assert lm.set_kv_cache_dtype("fp8_e4m3") is lm and lm.kv_cache_dtype == "fp8_e4m3"
    assert lm.set_kv_cache_dtype("bf16").kv_cache_dtype == "bf16"
    for bad in ("fp8", "e4m3", "int8", "BF16", "float8_e4m3fn", None, torch.float8_e4m3fn, torch.bfloat16):
        with pytest.raises(ValueError):
            lm.set_kv_cache_dtype(bad)
    assert lm.kv_cache_dtype == "bf16"


def test_fp8_cache_layout_bytes_and_row_gather():
    from aki_amd.phi3 import AkiKVCache
    n_layers, B, H, Dh, cap = 3, 4, 2, 96, 70
    c8 = AkiKVCache(n_layers, B, H, Dh, cap, torch.bfloat16, "cpu", kv_dtype="fp8_e4m3")
    c16 = AkiKVCache(n_layers, B, H, Dh, cap, torch.bfloat16, "cpu")
    assert c8.kv_dtype == "fp8_e4m3" and c16.kv_dtype == "bf16"
    assert c16.k_scale is None and c16.v_scale is None and c16.scales(0) == (None, None)
    assert len(c8.k) == len(c8.v) == len(c8.k_scale) == len(c8.v_scale) == n_layers
    for i in range(n_layers):
        for t in (c8.k[i], c8.v[i]):
            assert t.dtype == torch.uint8 and tuple(t.shape) == (B, H, cap, Dh)
        for t in (c8.k_scale[i], c8.v_scale[i]):
            assert t.dtype == torch.float32 and tuple(t.shape) == (B, H, cap)
    # one allocation each for the bytes and the scales, laid out [2, n_layers, B, H, capacity(, 96)]
    kv, sc = c8._store
    assert tuple(kv.shape) == (2, n_layers, B, H, cap, Dh) and tuple(sc.shape) == (2, n_layers, B, H, cap)
    assert c8.k[1].data_ptr() == kv[0, 1].data_ptr() and c8.v_scale[2].data_ptr() == sc[1, 2].data_ptr()
    assert c16.nbytes() == 2 * n_layers * B * H * cap * Dh * 2
    assert c8.nbytes() == 2 * n_layers * B * H * cap * (Dh + 4)
    assert abs(c8.nbytes() / c16.nbytes() - 0.52) < 0.01
    # beam search's gather: the scales follow their rows
    for j, (k, v, ks, vs) in enumerate(zip(c8.k, c8.v, c8.k_scale, c8.v_scale)):
        k.copy_(torch.arange(B, dtype=torch.uint8)[:, None, None, None] + 10 * j)
        v.copy_(k + 1)
        ks.copy_(torch.arange(B, dtype=torch.float32)[:, None, None] + 100 * j)
        vs.copy_(ks + 0.5)
    idx = torch.tensor([2, 2, 0, 3, 1])
    c8.select_rows(idx)
    assert c8.cache_len.shape == (5,)
    for j in range(n_layers):
        assert tuple(c8.k_scale[j].shape) == (5, H, cap)
        for r, src in enumerate(idx.tolist()):
            assert bool((c8.k[j][r] == src + 10 * j).all()) and bool((c8.v[j][r] == src + 10 * j + 1).all())
            assert bool((c8.k_scale[j][r] == src + 100 * j).all()) and bool((c8.v_scale[j][r] == src + 100 * j + 0.5).all())
    assert c8.scales(1)[0] is c8.k_scale[1]


def test_fp8_cache_needs_a_bf16_model_with_96_wide_heads():
    from aki_amd import ops
    from aki_amd.phi3 import AkiKVCache
    with pytest.raises(ops.AkiError):
        AkiKVCache(1, 1, 2, 96, 8, torch.float32, "cpu", kv_dtype="fp8_e4m3")
    with pytest.raises(ops.AkiError):
        AkiKVCache(1, 1, 2, 64, 8, torch.bfloat16, "cpu", kv_dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        AkiKVCache(1, 1, 2, 96, 8, torch.bfloat16, "cpu", kv_dtype="int8")
