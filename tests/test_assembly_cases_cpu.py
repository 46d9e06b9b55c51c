"""The case tables of tests/assembly_cases.py, checked without a GPU: the stream model of the splice against the reference-pinned
oracle (at most one image per sample, both padding sides) and against the written multi-image rule (oracle/aki_torch.py), every named
edge reached by a case, every mutation of a reference visible in the output it names, the mask family against the oracle's
mask_to_table, the collate and im2col references against the oracle's."""
import dataclasses

import numpy as np
import pytest
import torch

import aki_oracle as O
import aki_torch as OT
import assembly_cases as A


@pytest.fixture
def assistant_id(monkeypatch):
    """The oracle hard-codes the product's <|assistant|> id; the small vocabulary has its own."""
    def use(inp):
        monkeypatch.setattr(O, "ASSISTANT_TOKEN_ID", inp["assistant"])
    return use


def _lang_embeds(inp):
    return O.decoupled_embedding(inp["lang_x"], inp["W"], inp["Wadd"], inp["max_original_id"])


def _ones_if_none(inp):
    return inp["attention_mask"] if inp["attention_mask"] is not None else np.ones_like(inp["lang_x"])


def test_constants_are_parsed_and_the_abi_constants_agree():
    assert set(A.K) >= {"PLAN_CHUNK", "SPLICE_THREADS", "VEC_BYTES", "COLLATE_THREADS", "DENSE_THREADS", "SCAN_THREADS", "CH", "AKI_MAX_RECTS", "AKI_PLAN_STRIDE"}
    assert A.PLAN_STRIDE == 4 + A.MAX_RECTS
    assert len({c.id for c in A.SPLICE_CASES}) == len(A.SPLICE_CASES) and len({c.id for c in A.MASK_CASES}) == len(A.MASK_CASES)


ONE_IMAGE = [c for c in A.SPLICE_RUN if max(c.n_img) <= 1]
MULTI = [c for c in A.SPLICE_RUN if max(c.n_img) > 1]


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("c", ONE_IMAGE, ids=repr)
def test_stream_model_equals_the_pinned_oracle(c, side, assistant_id):
    c = dataclasses.replace(c, side=side)
    inp = A.splice_inputs(c)
    assistant_id(inp)
    got = A.splice_expected(c, inp)
    want = O.prepare_inputs_for_forward(inp["vt"], inp["lang_x"], _ones_if_none(inp), inp["labels"], _lang_embeds(inp), inp["media"],
                                        A.pad_value(c.pad_id, c.dtype), c.Nv, side)
    assert np.array_equal(got["inputs_embeds"], want["inputs_embeds"])
    assert (got["labels"] is None and want["labels"] is None) or np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["dense"], want["attention_mask"])
    assert np.array_equal(got["mask_1d"], want["mask_1d"])
    assert got["seq_lens"].tolist() == want["lengths"]
    for b in range(c.B):
        assert [tuple(r) for r in got["rects"][b].tolist()] == [tuple(s) for s in want["spans"][b]] + [(0, 0, 0, 0)] * (c.max_rects - 1)


@pytest.mark.parametrize("c", A.SPLICE_RUN, ids=repr)
def test_stream_model_equals_the_written_multi_image_rule(c, assistant_id):
    c = dataclasses.replace(c, side="right", has_labels=False)
    inp = A.splice_inputs(c)
    assistant_id(inp)
    got = A.splice_expected(c, inp)
    want = OT.prepare_inputs_multi_image(torch.from_numpy(inp["vt"]), torch.from_numpy(inp["lang_x"]), torch.from_numpy(_ones_if_none(inp)),
                                         torch.from_numpy(_lang_embeds(inp)), inp["media"], A.pad_value(c.pad_id, c.dtype), c.Nv)
    assert np.array_equal(got["inputs_embeds"], want["inputs_embeds"].numpy())
    assert np.array_equal(got["dense"], want["attention_mask"].numpy())
    assert np.array_equal(got["mask_1d"], want["mask_1d"])
    assert got["seq_lens"].tolist() == want["lengths"]
    for b in range(c.B):
        n = c.n_img[b]
        assert [tuple(r) for r in got["rects"][b].tolist()] == [tuple(s) for s in want["spans"][b]] + [(0, 0, 0, 0)] * (c.max_rects - n)


def test_plan_rows():
    c = A.SPLICE_BY_ID["nimg9"]
    inp = A.splice_inputs(c)
    plan = A.splice_expected(c, inp)["plan"]
    assert c.refused and plan.shape == (3, A.PLAN_STRIDE)
    assert plan[1].tolist() == [9, 50, 70 + 9 * 3, 0, 0, 5, 6, 20, 40, 63, 64, 66] and plan[0].tolist() == [2, 30, 76, 0, 1, 9] + [-1] * 6
    assert (plan[2] == A.GUARD).all()
    c = A.SPLICE_BY_ID["lout65-left"]
    plan = A.splice_expected(c, A.splice_inputs(c))["plan"]
    assert plan[1, :6].tolist() == [1, 30, 62, 0, 20, -1] and plan[2, :5].tolist() == [0, 0, 59, 0, -1]


def test_every_splice_edge_is_reached():
    reached = set()
    for c in A.SPLICE_CASES:
        reached |= A.splice_edges(c, A.splice_inputs(c))
    assert not set(A.SPLICE_EDGES) - reached, sorted(set(A.SPLICE_EDGES) - reached)
    multi = [c for c in MULTI if c.Nv > 1]
    assert any(c.side == "left" for c in multi) and any(c.side == "right" for c in multi)
    for dt, size in (("bf16", 2), ("f32", 4)):           # the copy loop's second trip in both types
        assert any(c.dtype == dt and c.d * size // A.K["VEC_BYTES"] > A.K["SPLICE_THREADS"] for c in A.SPLICE_RUN)
    assert any(c.T // A.K["PLAN_CHUNK"] >= 15 for c in A.SPLICE_RUN)


@pytest.mark.parametrize("mut", sorted(A.SPLICE_MUTATIONS))
def test_every_splice_mutation_is_visible(mut):
    changed = {}
    for c in A.SPLICE_CASES:
        inp = A.splice_inputs(c)
        good, bad = A.splice_expected(c, inp), A.splice_expected(c, inp, mut)
        for key in good:
            if key != "L_out" and good[key] is not None and not np.array_equal(good[key], bad[key]):
                changed.setdefault(key, []).append(c.id)
    for key in A.SPLICE_MUTATIONS[mut]:
        assert changed.get(key), f"{mut} changes {key} in no case (it changes {changed})"


# ---- mask tables -----------------------------------------------------------------------------------------------------------------------
def test_every_mask_edge_is_reached():
    reached = set()
    for c in A.MASK_CASES:
        reached |= A.mask_edges(c)
    assert not set(A.MASK_EDGES) - reached, sorted(set(A.MASK_EDGES) - reached)
    assert {f"L={A.K['CH'] + d}" for d in (-1, 0, 1, 52)} <= reached


@pytest.mark.parametrize("c", A.MASK_CASES, ids=repr)
def test_mask_family_against_the_oracle(c):
    rects, valid, seq = A.mask_arrays(c)
    dense = A.dense_from_table(rects, valid, seq)
    for b, s in enumerate(c.samples):                      # the closed form of the oracle, rows below seq_len
        want = O.mask_from_spans(valid[b], s.rects)[0]
        want[s.seq_len:] = 0
        assert np.array_equal(dense[b, 0], want)
    tables = A.table_from_mask(dense)
    back = np.zeros_like(rects)
    for b, (r, v, n) in enumerate(tables):
        s = c.samples[b]
        if c.canonical:
            assert A.is_canonical(s, c.L)
            assert r == list(s.rects), (c.id, b)
        assert len(r) <= len(s.rects), (c.id, b, r)
        back[b, :len(r)] = np.asarray(r, dtype=np.int32).reshape(-1, 4)
    if c.refused:
        assert [len(t[0]) for t in tables] == [c.refused] and O.mask_to_table(dense[0, 0], A.MAX_RECTS) is None
    again = A.dense_from_table(back, np.stack([t[1] for t in tables]), np.asarray([t[2] for t in tables]))
    assert np.array_equal(again, dense)


@pytest.mark.parametrize("mut", sorted(A.MASK_MUTATIONS))
def test_every_mask_mutation_is_visible(mut):
    hit = []
    for c in A.MASK_CASES:
        rects, valid, seq = A.mask_arrays(c)
        dense = A.dense_from_table(rects, valid, seq)
        if A.MASK_MUTATIONS[mut] == "dense":
            if not np.array_equal(A.dense_from_table(rects, valid, seq, mut), dense):
                hit.append(c.id)
        elif [t[0] for t in A.table_from_mask(dense, mut)] != [t[0] for t in A.table_from_mask(dense)]:
            hit.append(c.id)
    assert hit, mut
    if mut == "run_split_at_2048":
        assert len(hit) >= 2


# ---- collate ---------------------------------------------------------------------------------------------------------------------------
def test_collate_edges_and_mutations():
    reached = set()
    hits = {m: [] for m in A.COLLATE_MUTATIONS}
    for c in A.COLLATE_CASES:
        reached |= A.collate_edges(c)
        inp = A.collate_inputs(c)
        good = A.collate_expected(c, inp)
        batch = [{k: inp[k][b].tolist() for k in inp} for b in range(c.B)]
        ref = O.sft_batch_collate_pad(batch, "max_length", c.side, c.pad_id, c.T_out - 1)      # the + 1 of the caller included
        for k in good:
            assert good[k].shape == (c.B, c.T_out) and np.array_equal(good[k], ref[k])
        for m in A.COLLATE_MUTATIONS:
            bad = A.collate_expected(c, inp, m)
            if all(not np.array_equal(bad[k], good[k]) for k in ("input_ids", "labels")):
                hits[m].append(c.id)
    assert not set(A.COLLATE_EDGES) - reached, sorted(set(A.COLLATE_EDGES) - reached)
    assert all(hits.values()), hits
    assert any("right" in i for i in hits["truncation_keeps_last_tokens"])


# ---- im2col ----------------------------------------------------------------------------------------------------------------------------
def test_im2col_edges_reference_and_mutations():
    reached = set()
    hits = {m: [] for m in A.IM2COL_MUTATIONS}
    for c in A.IM2COL_CASES:
        reached |= A.im2col_edges(c)
        pix = A.im2col_inputs(c)
        good = A.im2col_expected(c, pix)
        K3 = 3 * c.P * c.P
        assert good.shape == (c.N * c.G * c.G, c.Kp) and (good[:, K3:] == 0).all() and (good[:, :K3] != 0).all()
        if c.S <= 32:                                      # the oracle's patch embedding with an identity kernel is the unfold itself
            eye = np.eye(K3, dtype=np.float32).reshape(K3, 3, c.P, c.P)
            want = O.siglip_patch_embed(pix, eye, np.zeros(K3, np.float32), np.zeros((c.G * c.G, K3), np.float32))
            assert np.array_equal(good[:, :K3], want.reshape(-1, K3))
        for m in A.IM2COL_MUTATIONS:
            if not np.array_equal(A.im2col_expected(c, pix, m), good):
                hits[m].append(c.id)
    assert not set(A.IM2COL_EDGES) - reached, sorted(set(A.IM2COL_EDGES) - reached)
    assert all(hits.values()), hits


def test_mutation_names():
    assert set(A.MUTATIONS["splice"]) == {"later_image_offset_dropped", "text_end_counts_all_images", "text_end_without_plus_one", "assistant_last_not_first",
                                          "left_shift_applied_to_mask", "image_rows_keep_labels", "image_slots_take_prompt_mask", "vision_row_of_sample_zero",
                                          "additional_ids_from_main_table", "pad_rows_zero", "placeholder_at_chunk_start_lost", "ninth_index_stored"}
    assert set(A.MUTATIONS["mask"]) == {"rect_row_hi_inclusive", "seq_len_ignored", "valid_bit_64_in_word_0", "run_split_at_2048", "last_column_dropped"}
    assert set(A.MUTATIONS["collate"]) == {"truncation_keeps_last_tokens", "left_shift_when_truncated"}
    assert set(A.MUTATIONS["im2col"]) == {"py_px_swapped", "remainder_pixels_used", "pad_columns_carry_pixels"}
