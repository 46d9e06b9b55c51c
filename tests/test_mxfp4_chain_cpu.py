"""What the MXFP4 decode chain rests on that needs no GPU: the dtype constant of the C header and its Python twin, the switch's default, and the
lane -> chunk map of the chain's GEMV phase against the sweep order of mxfp4.hip's gemv_w4_kernel (the bit identity of the two paths needs every
lane to add the same blocks of 32 k in the same order)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_headers_w4a16_constant_equals_the_bindings():
    from aki_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "aki_mi355x.h")).read()
    m = re.search(r"\bAKI_DT_W4A16\s*=\s*(\d+)", text)
    assert m is not None and int(m.group(1)) == L.AKI_DT_W4A16 == 4
    w8 = re.search(r"\bAKI_DT_W8A16\s*=\s*(\d+)", text)
    assert int(w8.group(1)) == L.AKI_DT_W8A16 == 3             # additive: the older values did not move
    assert int(re.search(r"#define\s+AKI_ABI_VERSION\s+(\d+)", text).group(1)) == L.AKI_ABI_VERSION


def test_the_w4_chain_is_off_by_default():
    from aki_amd.phi3 import Phi3Model
    assert Phi3Model.decode_chain_w4 is False
    assert Phi3Model.decode_chain_w8 is True


def _chain_lane_chunks(K):
    """chain_gemv<FMT = CH_W4>: KC = ceil(NBLK / 64) unrolled passes, chunk c = lane + 64 kc, load and dot product predicated on c < NBLK."""
    nblk = K // 32
    kc_n = -(-nblk // 64)
    return [[lane + 64 * kc for kc in range(kc_n) if lane + 64 * kc < nblk] for lane in range(64)]


def _gemv_w4_lane_chunks(K):
    """gemv_w4_kernel's three loops (sweeps of 4, 2 and 1 chunks per lane; a sweep of U handles chunks c, c + 64, ... c + 64 (U - 1) in that order)."""
    nblk = K // 32
    out = []
    for lane in range(64):
        seq, c = [], lane
        while c + 64 * 3 < nblk:
            seq += [c + 64 * u for u in range(4)]
            c += 64 * 4
        while c + 64 < nblk:
            seq += [c + 64 * u for u in range(2)]
            c += 128
        while c < nblk:
            seq.append(c)
            c += 64
        out.append(seq)
    return out


@pytest.mark.parametrize("K", [3072, 8192])
def test_the_chains_lane_chunk_map_is_gemv_w4s_sweep_order(K):
    chain, gemv = _chain_lane_chunks(K), _gemv_w4_lane_chunks(K)
    nblk = K // 32
    visited = np.sort(np.concatenate([np.asarray(s, dtype=np.int64) for s in chain]))
    assert np.array_equal(visited, np.arange(nblk)), "every block of a row exactly once"
    assert chain == gemv, "per lane: the same chunks in the same order"
    for lane, seq in enumerate(chain):
        assert seq == sorted(seq)                              # ascending
        # chunk c is block c: its scale byte is ws[row * K/32 + c], its 16 weight bytes end inside the row, and it meets x chunks 4c .. 4c+3
        assert all(16 * (c + 1) <= K // 2 and 4 * c + 3 < K // 8 for c in seq)
    if K == 3072:                                              # 96 blocks = 1.5 per lane: lanes 32-63 have no second chunk
        assert [len(s) for s in chain] == [2] * 32 + [1] * 32
    else:                                                      # 256 blocks: four per lane, nothing predicated
        assert [len(s) for s in chain] == [4] * 64
