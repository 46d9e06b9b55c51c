"""The prompt-assembly kernels of aki_amd/csrc/aux_kernels.hip on the device, against the references of tests/assembly_cases.py: the
splice plan, the splice, its mask table, the dense mask and its way back to a table, the SFT collate and im2col.  Every output is an
integer or a copied bit pattern, so every comparison below is an equality."""

import numpy as np
import pytest
import torch

import assembly_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def _ops():
    from aki_amd import ops
    return ops


def _t(x, dtype=None):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


# ---- splice ------------------------------------------------------------------------------------------------------------------------------
_SPLICE = {}


def _splice_case(c):
    """Inputs and expected outputs of a case, computed once and shared by the tests that need them."""
    if c.id not in _SPLICE:
        inp = A.splice_inputs(c)
        _SPLICE[c.id] = (inp, A.splice_expected(c, inp))
    return _SPLICE[c.id]


def _splice(c, inp, lang_x, plan=None):
    return _ops().splice(lang_x, _t(inp["attention_mask"]), _t(inp["labels"]), _t(inp["W"], DT[c.dtype]), _t(inp["Wadd"], DT[c.dtype]),
                         inp["max_original_id"], _t(inp["vt"], DT[c.dtype]), inp["media"], c.pad_id, assistant_token_id=inp["assistant"],
                         padding_side=c.side, max_rects=c.max_rects, plan=plan)


def _check_splice(c, want, got, how):
    ops = _ops()
    emb, lab, table, plan_h = got
    assert np.array_equal(plan_h.numpy(), want["plan"][:c.B]), (c.id, how, "plan")
    assert emb.dtype == DT[c.dtype] and tuple(emb.shape) == want["inputs_embeds"].shape, (c.id, how)
    assert np.array_equal(_np(emb), want["inputs_embeds"]), (c.id, how, "inputs_embeds")
    if want["labels"] is None:
        assert lab is None
    else:
        assert np.array_equal(_np(lab), want["labels"]), (c.id, how, "labels")
    assert table.L == want["L_out"]
    assert np.array_equal(_np(table.rects), want["rects"]), (c.id, how, "rects")
    assert np.array_equal(_np(table.col_valid_bits), want["col_valid_bits"]), (c.id, how, "col_valid_bits")
    assert np.array_equal(_np(table.seq_lens), want["seq_lens"]), (c.id, how, "seq_lens")
    assert np.array_equal(_np(table.mask_1d), want["mask_1d"]), (c.id, how, "mask_1d")
    assert torch.equal(ops.mask_dense(table, c.B), _t(want["dense"])), (c.id, how, "dense")


@pytest.mark.parametrize("c", A.SPLICE_RUN, ids=repr)
def test_splice(c):
    """ops.splice planning by itself, and with a plan started ahead of it (splice_plan_async + plan=)."""
    ops = _ops()
    inp, want = _splice_case(c)
    lang_x = _t(inp["lang_x"])
    _check_splice(c, want, _splice(c, inp, lang_x), "direct")
    plan = ops.splice_plan_async(lang_x, inp["media"], inp["assistant"], c.Nv)
    assert np.array_equal(_np(plan.plan), want["plan"][:c.B])
    _check_splice(c, want, _splice(c, inp, lang_x, plan), "planned ahead")


@pytest.mark.parametrize("c", A.SPLICE_CASES, ids=repr)
def test_splice_plan_raw(c):
    """aki_splice_plan itself: n_img is not capped, only AKI_MAX_RECTS indices are stored, and nothing is written behind the last row."""
    from aki_amd import _lib as L
    inp, want = _splice_case(c)
    lang_x = _t(inp["lang_x"])
    plan = torch.full((c.B + 1, A.PLAN_STRIDE), A.GUARD, dtype=torch.int32, device=DEV)
    L.check(L.load().aki_splice_plan(lang_x.data_ptr(), c.B, c.T, inp["media"], inp["assistant"], c.Nv, plan.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "aki_splice_plan")
    assert np.array_equal(_np(plan), want["plan"])


@pytest.mark.parametrize("cid", ["lout129-three", "t200-7img-left"])
def test_stale_plan_is_replanned(cid):
    """A plan made from other ids, or from ids that were changed in place afterwards, must not be used."""
    ops = _ops()
    c = A.SPLICE_BY_ID[cid]
    inp, want = _splice_case(c)
    other = np.roll(inp["lang_x"], 7, axis=1)
    assert not np.array_equal(A.splice_expected(c, dict(inp, lang_x=other), only_plan=True)["plan"], want["plan"])
    other_dev, lang_x = _t(other), _t(inp["lang_x"])
    stale = ops.splice_plan_async(other_dev, inp["media"], inp["assistant"], c.Nv)
    _check_splice(c, want, _splice(c, inp, lang_x, stale), "a plan of other ids")
    stale = ops.splice_plan_async(other_dev, inp["media"], inp["assistant"], c.Nv)
    other_dev.copy_(lang_x)
    _check_splice(c, want, _splice(c, inp, other_dev, stale), "ids changed in place")


def test_nine_images_are_refused_before_the_splice_launch(monkeypatch):
    from aki_amd import AkiError, _lib as L
    c = A.SPLICE_BY_ID["nimg9"]
    inp, want = _splice_case(c)
    assert c.refused and c.T_img > max(c.n_img) and int(want["plan"][:c.B, 0].max()) == A.MAX_RECTS + 1
    lib, calls = L.load(), []
    real = lib.aki_splice_fwd
    monkeypatch.setattr(lib, "aki_splice_fwd", lambda *a: calls.append(a) or real(*a))
    with pytest.raises(AkiError, match=f"{A.MAX_RECTS + 1} images"):
        _splice(c, inp, _t(inp["lang_x"]))
    assert not calls
    ok = A.SPLICE_BY_ID["t1-img"]                                  # the spy itself works
    inp_ok, want_ok = _splice_case(ok)
    _check_splice(ok, want_ok, _splice(ok, inp_ok, _t(inp_ok["lang_x"])), "direct")
    assert len(calls) == 1


# ---- mask tables -------------------------------------------------------------------------------------------------------------------------
def _live(rects):
    return [tuple(r) for r in rects.tolist() if r[3] > r[2]]


@pytest.mark.parametrize("c", A.MASK_CASES, ids=repr)
def test_mask_dense_and_mask_to_table(c):
    from aki_amd import AkiError
    ops = _ops()
    rects, valid, seq = A.mask_arrays(c)
    dense = A.dense_from_table(rects, valid, seq)
    dense_dev = _t(dense)
    if c.refused:
        with pytest.raises(AkiError, match=f"needs {c.refused} row groups"):
            ops.mask_to_table(dense_dev)
        return
    table = ops.MaskTable(_t(rects[:, :A.MAX_RECTS]), _t(A.pack_bits(valid)), _t(seq), c.L)
    assert torch.equal(ops.mask_dense(table, c.B), dense_dev), (c.id, "mask_dense")
    back = ops.mask_to_table(dense_dev)
    want = A.table_from_mask(dense)
    assert np.array_equal(_np(back.seq_lens), np.asarray([w[2] for w in want], dtype=np.int32)), (c.id, "seq_lens")
    assert np.array_equal(_np(back.col_valid_bits), A.pack_bits(np.stack([w[1] for w in want]))), (c.id, "col_valid_bits")
    got = _np(back.rects)
    for b, s in enumerate(c.samples):
        assert _live(got[b]) == want[b][0], (c.id, b, "rects by the written rule")
        if c.canonical:
            assert np.array_equal(got[b], rects[b, :A.MAX_RECTS]), (c.id, b, "the generating rectangles")
        assert len(_live(got[b])) <= len(s.rects), (c.id, b, "no more rectangles than the generator used")
    assert torch.equal(ops.mask_dense(back, c.B), dense_dev), (c.id, "round trip")


# ---- SFT collate -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.COLLATE_CASES, ids=repr)
def test_sft_collate(c):
    from aki_amd import _lib as L
    from aki_amd.sft_collate import IGNORE_INDEX, batch_collate_pad
    inp = A.collate_inputs(c)
    want = A.collate_expected(c, inp)
    batch = [{k: (torch.from_numpy(inp[k][b]) if b % 2 else inp[k][b].tolist()) for k in inp} for b in range(c.B)]
    out = batch_collate_pad(batch, "max_length", c.side, c.pad_id, c.T_out - 1)
    for k in want:
        assert out[k].is_cuda and out[k].dtype == torch.int64 and np.array_equal(_np(out[k]), want[k]), (c.id, k)
    # the raw entry, with the labels and mask outputs absent and with all three
    flat = {k: _t(np.concatenate(inp[k])) for k in inp}
    offsets = _t(np.concatenate([[0], np.cumsum(c.lengths)]).astype(np.int32))
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    for with_rest in (False, True):
        outs = [torch.empty((c.B, c.T_out), dtype=torch.int64, device=DEV) for _ in range(3 if with_rest else 1)]
        ptrs = [o.data_ptr() for o in outs] + [None] * (3 - len(outs))
        L.check(lib.aki_sft_collate_pad(flat["input_ids"].data_ptr(), flat["labels"].data_ptr() if with_rest else None,
                                        flat["attention_mask"].data_ptr() if with_rest else None, offsets.data_ptr(), c.B, c.T_out, c.pad_id,
                                        IGNORE_INDEX, 1 if c.side == "left" else 0, *ptrs, stream), "aki_sft_collate_pad")
        for o, k in zip(outs, ("input_ids", "labels", "attention_mask")):
            assert np.array_equal(_np(o), want[k]), (c.id, k, "raw", with_rest)


# ---- im2col ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.IM2COL_CASES, ids=repr)
def test_im2col_through_an_identity_patch_embedding(c):
    """patch_embed = im2col + GEMM.  With the Kp x Kp identity as weight and neither bias nor position embedding every product is x * 1
    or x * 0 with finite non-zero x, so the output is the im2col matrix bit for bit - the zero columns 3 P P .. Kp of a workspace that
    comes out of the allocator dirty included."""
    ops = _ops()
    pix = A.im2col_inputs(c)
    want = A.im2col_expected(c, pix)
    eye = torch.eye(c.Kp, dtype=DT[c.dtype], device=DEV)
    y = ops.patch_embed(_t(pix, DT[c.dtype]), eye, None, None, c.P)
    assert tuple(y.shape) == (c.N, c.G * c.G, c.Kp) and y.dtype == DT[c.dtype]
    got = _np(y).reshape(-1, c.Kp)
    assert np.array_equal(got[:, 3 * c.P * c.P:], want[:, 3 * c.P * c.P:]), (c.id, "the zero columns")
    assert np.array_equal(got, want), c.id
