"""MXFP4 weight format: properties of the numpy reference that the GPU tests compare against, and the mutation table - every plausible
mistake of a kernel (mxfp4_cases.MUTATIONS) must move some output of some case of the ops.linear_w4 table by at least 8 tolerances, so
that passing the table means something.  No GPU needed."""
import numpy as np
import pytest

import mxfp4_cases as MC


def _blockwise(w):
    return np.asarray(w, dtype=np.float64).reshape(w.shape[0], -1, 32)


@pytest.mark.parametrize("family", ["spread", "edges"])
def test_requantising_the_dequantised_weights_is_the_identity(family):
    w = MC.weights(family, 13, 2080)
    wq, ws = MC.quant_ref(w)
    wd = MC.dequant_ref(wq, ws)
    assert np.array_equal(MC.to_bf16(wd).astype(np.float64), wd), "dequantised values must be exact in bf16"
    wq2, ws2 = MC.quant_ref(wd)
    assert np.array_equal(wq2, wq) and np.array_equal(ws2, ws)
    assert wq.shape == (13, 1040) and ws.shape == (13, 65) and wq.dtype == np.uint8 and ws.dtype == np.uint8
    assert int(ws.max()) <= 254


def test_ties_go_to_the_even_code_and_values_saturate_at_six():
    # one block per row, largest value 7 (in (6, 8)): e = floor(log2 7) - 2 = 0, so the values are their own quotients
    vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, -0.25, -1.25, -5.0, -7.0, 6.5, 0.2, 0.3, 5.5, 4.9]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, -0.0, -1.0, -4.0, -6.0, 6.0, 0.0, 0.5, 6.0, 4.0]
    w = np.zeros((1, 32))
    w[0, :len(vals)] = vals
    w = MC.to_bf16(w)
    wq, ws = MC.quant_ref(w)
    assert ws[0, 0] == 127
    wd = MC.dequant_ref(wq, ws)[0]
    exp = np.zeros(32)
    exp[:len(want)] = want
    exp[[13, 15, 16]] = [0.0, 6.0, 4.0]
    # bf16(0.2) < 0.25 -> 0, bf16(0.3) > 0.25 -> 0.5, 5.5 > 5 -> 6, bf16(4.9) < 5 -> 4
    assert np.array_equal(wd, exp), (wd, exp)
    codes = np.stack((wq[0] & 15, wq[0] >> 4), -1).reshape(-1)
    assert list(codes[:8]) == [0, 2, 2, 4, 4, 6, 6, 7], "ties must land on the even code"
    assert list(codes[8:12]) == [8, 10, 14, 15], "the sign sits in bit 3"
    assert wq[0, 0] == (0 | (2 << 4)), "k = 2j in the low nibble, k = 2j + 1 in the high nibble"


def test_scale_byte_follows_floor_log2_amax_minus_two():
    rows = []
    for e in (-140, -130, -126, -20, -1, 0, 1, 2, 60, 127):
        for m in (1.0, 1.5, 1.984375):
            rows.append(np.concatenate(([m * 2.0 ** e], np.zeros(31))))
    w = MC.to_bf16(np.array(rows)).astype(np.float64)
    keep = w[:, 0] > 0                                         # 2^-140 is below the smallest bf16 subnormal: that row is a zero block
    wq, ws = MC.quant_ref(w)
    fl = np.floor(np.log2(w[keep, 0]))
    assert np.array_equal(ws[keep, 0].astype(np.int64), np.clip(fl - 2 + 127, 0, 254).astype(np.int64))
    assert (ws[~keep, 0] == 127).all() and (wq[~keep] == 0).all()
    q = np.ldexp(w[keep, 0], -(ws[keep, 0].astype(np.int64) - 127))
    assert ((q >= 4) & (q < 8))[ws[keep, 0] > 0].all(), "amax / 2^e lies in [4, 8) wherever the byte is not clamped"


def test_zero_blocks_get_byte_127_and_zero_nibbles():
    w = MC.weights("edges", 6, 96)
    wq, ws = MC.quant_ref(w)
    assert (_blockwise(w)[:, 1] == 0).all() and (ws[:, 1] == 127).all() and (wq[:, 16:32] == 0).all()
    single = _blockwise(MC.dequant_ref(wq, ws))[:, 2]
    assert ((single != 0).sum(-1) == 1).all(), "the single non-zero value of block 2 survives"
    assert np.array_equal(np.abs(single).max(-1), 0.8 * np.abs(_blockwise(w)[:, 2]).max(-1)), "5 x 2^e' is a tie between 4 and 6: the even code is 4"


def test_the_families_make_every_block_count():
    w = MC.weights("spread", 20, 8192)
    _, ws = MC.quant_ref(w)
    assert int(ws.max()) - int(ws.min()) >= 9, "block amplitudes spread over 2^-6 .. 2^3"
    assert (ws[:, 1:] != ws[:, :-1]).mean() > 0.8, "neighbouring blocks carry different scales"
    x = MC.x_rows(2, 8192)
    assert (np.abs(x[:, 1:]) != np.abs(x[:, :-1])).all(), "x differs in magnitude from k to k"
    names = [c.name for c in MC.CASES]
    assert len(set(names)) == len(names)
    assert {c.K for c in MC.CASES} >= {32, 2048, 2080, 3072, 8192} and {c.M for c in MC.CASES} >= {1, 2, 3, 8, 9, 16}


@pytest.mark.parametrize("mutation", MC.MUTATIONS)
def test_every_mutation_moves_an_output_by_eight_tolerances(mutation):
    """A condition on the inputs, not a measurement of any kernel: max over cases and elements of |mutated - ref| / tol >= 8."""
    worst, where = 0.0, None
    for case in MC.CASES:
        if mutation == "swiglu_up_rows_at_wrong_offset" and case.act != MC.ACT_SWIGLU:
            continue
        _, _, ref, tol = MC.reference(case)
        r = float((np.abs(MC.mutated(case, mutation) - ref) / tol).max())
        if r > worst:
            worst, where = r, case.name
    print(f"{mutation}: {worst:.3g} tolerances at {where}")
    assert worst >= 8.0, (mutation, worst, where)


@pytest.mark.parametrize("mutation", MC.MUTATIONS)
def test_every_k_of_the_table_sees_the_mutations_it_can(mutation):
    """Stronger than the cap: at EVERY K of the table some case catches the mutation (a one-block K cannot see a wrong block index)."""
    for K in sorted({c.K for c in MC.CASES}):
        if K == 32 and mutation == "scale_index_off_by_one_block":
            continue
        worst = 0.0
        for case in MC.CASES:
            if case.K != K or (mutation == "swiglu_up_rows_at_wrong_offset" and case.act != MC.ACT_SWIGLU):
                continue
            _, _, ref, tol = MC.reference(case)
            worst = max(worst, float((np.abs(MC.mutated(case, mutation) - ref) / tol).max()))
        assert worst >= 8.0, (mutation, K, worst)
