"""Case tables, references and reference mutations of the prompt-assembly kernels of aki_amd/csrc/aux_kernels.hip: splice_plan_kernel,
splice_kernel<T>, splice_table_kernel, mask_dense_kernel, mask_rows_scan_kernel + mask_table_build_kernel, sft_collate_kernel and
im2col_kernel<T>.  Every output of these kernels is an integer or a copied bit pattern: there is no bar anywhere, only equality.

numpy only.  tests/test_assembly_cases_cpu.py checks the tables themselves - the stream model against the reference-pinned oracle
(one image) and against the written multi-image rule, every named edge reached (from the constants parsed out of the sources), every
mutation visible - and tests/test_assembly_gpu.py runs every case on the device.

The splice reference is a STREAM MODEL.  A sample's prompt is walked once and every position emits stream items: ("tok", t) for an
ordinary token, ("img", k, slot) for slot = 0 .. Nv - 1 at the k-th placeholder.  Nothing below computes t_k + k (Nv - 1): an image's
rows are wherever its items landed in the list, text_end is the number of items that positions before the first <|assistant|> emitted,
plus one.  Embeds, labels, the 1-D mask, the rectangles, the valid bits and the dense mask are all read off that list.

Vocabularies.  'small': ids 0..39 in the main table (max_original_id 39), 40..45 additional, <image> = 40, <|assistant|> = 33, the
token that fills a prompt's padded tail = 32.  'product': max_original_id 32010, <image> = 32011, <|assistant|> = 32001, tail 32000.
The main table carries decoy rows for the additional ids as well: without an additional table those rows are what the reference
reads, and with one they are what a kernel that ignores it would read - inside the allocation either way.
"""
import os
import re
import zlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np

import aki_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -7777                      # what the row behind the last plan row holds before and after aki_splice_plan
IGNORE = -100

VOCABS = {
    "small": dict(max_original_id=39, n_add=6, media=40, assistant=33, tail=32, plain_hi=32, extra=(41, 42, 45)),
    "product": dict(max_original_id=32010, n_add=2, media=32011, assistant=32001, tail=32000, plain_hi=31000, extra=(32012,)),
}


def kernel_constants():
    """The plan kernel's chunk, the block sizes of the copy loops, the LDS chunk of the table build and the two ABI constants, as the
    sources have them: a changed constant moves an edge, and the CPU test then fails the table instead of silently testing beside it."""
    def read(*p):
        with open(os.path.join(ROOT, *p)) as f:
            return f.read()
    src, hdr, lib = read("aki_amd", "csrc", "aux_kernels.hip"), read("include", "aki_mi355x.h"), read("aki_amd", "_lib.py")

    def body(name):
        m = re.search(r"void\s+%s\s*\(" % name, src)
        assert m, f"{name} not found in aux_kernels.hip"
        end = src.find("\n}\n", m.end())
        return src[m.start():end]

    def one(pat, text, what):
        m = re.search(pat, text)
        assert m, f"{what} not found"
        return int(m.group(1))
    out = {}
    plan = body("splice_plan_kernel")
    out["PLAN_CHUNK"] = one(r"t0\s*\+=\s*(\d+)", plan, "the plan kernel's chunk")
    assert one(r"splice_plan_kernel,\s*dim3\(B\),\s*dim3\((\d+)\)", src, "the plan kernel's launch") == out["PLAN_CHUNK"]
    out["SPLICE_THREADS"] = one(r"c\s*<\s*nvec;\s*c\s*\+=\s*(\d+)", body("splice_kernel"), "the splice copy loop")
    assert one(r"splice_kernel<float>,\s*grid,\s*dim3\((\d+)\)", src, "the splice launch") == out["SPLICE_THREADS"]
    out["VEC_BYTES"] = one(r"sizeof\(T\)\s*/\s*(\d+)", body("splice_kernel"), "the splice vector width")
    out["COLLATE_THREADS"] = one(r"t\s*<\s*T_out;\s*t\s*\+=\s*(\d+)", body("sft_collate_kernel"), "the collate loop")
    assert one(r"sft_collate_kernel,\s*dim3\(B\),\s*dim3\((\d+)\)", src, "the collate launch") == out["COLLATE_THREADS"]
    out["DENSE_THREADS"] = one(r"c\s*<\s*L;\s*c\s*\+=\s*(\d+)", body("mask_dense_kernel"), "the dense mask loop")
    out["SCAN_THREADS"] = one(r"c0\s*<\s*L;\s*c0\s*\+=\s*(\d+)", body("mask_rows_scan_kernel"), "the row scan loop")
    out["CH"] = one(r"constexpr\s+int\s+CH\s*=\s*(\d+)", body("mask_table_build_kernel"), "CH")
    for name in ("AKI_MAX_RECTS", "AKI_PLAN_STRIDE"):
        h = one(r"#define\s+%s\s+(\d+)" % name, hdr, name + " in the header")
        p = one(r"(?m)^%s\s*=\s*(\d+)" % name, lib, name + " in _lib.py")
        assert h == p, f"{name}: header {h}, _lib.py {p}"
        out[name] = h
    return out


K = kernel_constants()
MAX_RECTS, PLAN_STRIDE = K["AKI_MAX_RECTS"], K["AKI_PLAN_STRIDE"]


def rng_of(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


def pack_bits(valid):
    """bool [B, L] -> the bit pattern of uint64 [B, ceil(L / 64)] as int64: column c is bit c % 64 of word c // 64."""
    valid = np.asarray(valid) != 0
    B, L = valid.shape
    nw = (L + 63) // 64
    out = np.zeros((B, nw), dtype=np.uint64)
    for b in range(B):
        for c in np.flatnonzero(valid[b]):
            out[b, c // 64] |= np.uint64(1) << np.uint64(c % 64)
    return out.view(np.int64)


# =====================================================================================================================================
# splice
# =====================================================================================================================================
@dataclass(frozen=True)
class S:
    """One sample of a prompt batch: its own length (the rest of the row is padded tail), the placeholder positions, the
    <|assistant|> positions and the positions inside the prompt whose attention-mask entry is 0."""
    nlen: int
    imgs: Tuple[int, ...] = ()
    asst: Tuple[int, ...] = ()
    holes: Tuple[int, ...] = ()


@dataclass(frozen=True)
class SpliceCase:
    id: str
    T: int
    samples: Tuple[S, ...]
    Nv: int
    d: int
    dtype: str                      # "bf16" | "f32"
    side: str = "right"
    has_mask: bool = True
    has_labels: bool = True
    has_additional: bool = True
    T_img: int = 3
    pad_id: int = 32000
    vocab: str = "small"
    max_rects: int = MAX_RECTS
    why: str = ""

    def __repr__(self):
        return self.id

    @property
    def B(self):
        return len(self.samples)

    @property
    def n_img(self):
        return tuple(len(s.imgs) for s in self.samples)

    @property
    def refused(self):
        return max(self.n_img) > self.max_rects

    @property
    def L_b(self):                  # a count, used to name edges only: the expected outputs take every length from the stream
        return tuple(self.T + n * (self.Nv - 1) for n in self.n_img)

    @property
    def L_out(self):
        return max(self.L_b)


def _splice_cases():
    C, out = SpliceCase, []
    out.append(C("t1-noimg", 1, (S(1),), 4, 8, "bf16", has_mask=False, has_labels=False, has_additional=False, max_rects=1,
                 why="T = 1, nothing to splice, every optional input absent"))
    out.append(C("t1-img", 1, (S(1, (0,)),), 4, 4, "f32", max_rects=1, why="the placeholder is the whole prompt: index 0 and T - 1"))
    out.append(C("t63-nv1-left", 63, (S(63, (62,)), S(40, (0,), (5,), holes=(0, 7))), 1, 64, "bf16", side="left", max_rects=1,
                 why="placeholder at T - 1 and at 0; Nv = 1: the stream is as long as the prompt; a masked placeholder position"))
    out.append(C("t64-lout64", 64, (S(64, (63,), (0,)), S(40, (0,), (39,))), 1, 64, "f32", max_rects=1,
                 why="placeholder in the last lane of the only chunk; <|assistant|> at 0; L_out = 64: one full word of valid bits"))
    out.append(C("t65-img63-64", 65, (S(65, (63, 64), (10,)), S(65, (64,), (63,))), 4, 8, "bf16",
                 why="adjacent placeholders across the chunk seam; <|assistant|> before every image; an image after it"))
    out.append(C("lout65-left", 59, (S(59, (3, 20), (10,)), S(50, (20,), (30, 40)), S(59)), 4, 8, "bf16", side="left", has_additional=False,
                 why="L_out = 65: one bit in the second word; <|assistant|> between two images; ragged, left-padded"))
    out.append(C("t128-lout128", 128, (S(128, (5, 70), (100,)), S(100, (99,), (64,), holes=(99,))), 1, 4, "f32", has_labels=False,
                 why="one placeholder per chunk; <|assistant|> in a later chunk than a placeholder; L_out = 128"))
    out.append(C("lout129-three", 120, (S(120, (70, 71, 100), (101,)), S(120, (0, 119), (60,)), S(90, (64,), (110,))), 4, 8, "bf16", T_img=4,
                 why="three placeholders in the second chunk, two adjacent; <|assistant|> right after an image: a one-column rectangle; "
                     "<|assistant|> inside the padded tail; L_out = 129"))
    out.append(C("t200-7img-left", 200, (S(200, (0, 1, 63, 64, 65, 130, 199), (128, 150)), S(150, (10, 140), (5, 9)), S(200)), 4, 8, "bf16",
                 side="left", T_img=8, pad_id=32011, why="seven images, <|assistant|> twice; 32011 is not a bf16 number"))
    out.append(C("t200-8img-b5", 200, (S(200, (2, 30, 63, 64, 100, 127, 128, 192), (129,)), S(200, (50,), (100,)), S(120),
                                      S(180, (60, 61), ()), S(200, (1, 3, 5, 7, 9, 11, 13), (12,), holes=(3, 20))), 4, 4, "f32", T_img=9,
                 has_mask=True, why="eight images: every index slot and every rectangle used; B = 5, ragged"))
    out.append(C("t1000-nv144", 1000, (S(1000, (0, 63, 64, 300, 301, 640, 900, 999), (950,)), S(700, (699,), (10,))), 144, 8, "bf16", T_img=9,
                 why="T about 1000, sixteen chunks, Nv = 144: L_out = 2144; <|assistant|> in chunk 14"))
    out.append(C("nv144-one", 10, (S(10, (4,), (8,)), S(7, (), (3,))), 144, 64, "bf16", max_rects=1, has_mask=False,
                 why="Nv = 144 with one image, against the pinned oracle; no attention mask"))
    out.append(C("d3072-bf16", 20, (S(20, (2, 9), (15,)), S(12, (11,), (5,))), 4, 3072, "bf16", T_img=3, pad_id=32011,
                 why="the product's width: 384 vectors per row, the copy loop's second trip; pad rows at 32011 -> 32000.0"))
    out.append(C("d1032-f32-left", 20, (S(14, (3,), (9,)), S(20, (19,))), 4, 1032, "f32", side="left", max_rects=1, has_additional=False,
                 why="258 vectors per row: two in the second trip"))
    out.append(C("product-ids", 65, (S(65, (64,), (20,)), S(30, (7,), (40,))), 4, 8, "bf16", vocab="product", max_rects=1,
                 why="the product's ids: the main table read at row 32001, the additional one at 32012 - 32011"))
    out.append(C("d64-f32-nolabels", 70, (S(70, (10, 65), (66,)), S(33, (32,), ())), 4, 64, "f32", has_labels=False, has_additional=False, T_img=3,
                 why="d = 64 in f32; <|assistant|> right behind the second image, absent in the second sample"))
    out.append(C("nimg9", 70, (S(70, (1, 9), (30,)), S(70, (0, 5, 6, 20, 40, 63, 64, 66, 69), (50,))), 4, 8, "bf16", T_img=10,
                 why="nine placeholders: the plan counts nine and stores eight; the splice is refused on the host"))
    return tuple(out)


SPLICE_CASES = _splice_cases()
SPLICE_BY_ID = {c.id: c for c in SPLICE_CASES}
SPLICE_RUN = tuple(c for c in SPLICE_CASES if not c.refused)


def _round(x, dtype):
    x = np.asarray(x, dtype=np.float32)
    return O.bf16_round(x).astype(np.float32) if dtype == "bf16" else x


def pad_value(pad_id, dtype):
    """pad_token_id as the embedding rows hold it: cast to the dtype, round to nearest even."""
    return float(_round(np.asarray([pad_id], dtype=np.float32), dtype)[0])


def splice_inputs(c):
    """lang_x, attention_mask, labels [B, T] int64; the tables and vision tokens as float32 arrays that hold values of c.dtype."""
    v, g = VOCABS[c.vocab], rng_of("splice", c.id)
    B, T = c.B, c.T
    plain = np.concatenate([np.setdiff1d(np.arange(3, v["plain_hi"]), [v["assistant"], v["tail"]]), np.asarray(v["extra"])])
    lang_x = plain[g.integers(0, len(plain), size=(B, T))].astype(np.int64)
    am = np.ones((B, T), dtype=np.int64)
    for b, s in enumerate(c.samples):
        assert 0 < s.nlen <= T and not set(s.imgs) & set(s.asst) and all(0 <= t < s.nlen for t in s.imgs) and list(s.imgs) == sorted(set(s.imgs))
        lang_x[b, s.nlen:] = v["tail"]
        am[b, s.nlen:] = 0
        lang_x[b, list(s.imgs)] = v["media"]
        lang_x[b, list(s.asst)] = v["assistant"]
        am[b, list(s.holes)] = 0
    if c.has_additional:
        lang_x[0, [t for t in range(min(T, 4)) if lang_x[0, t] not in (v["media"], v["assistant"])][:1]] = v["extra"][0]
    labels = np.where(am == 0, IGNORE, lang_x * 3 + 1)           # not the ids: a label read from lang_x would show
    n_rows = v["max_original_id"] + 1 + v["n_add"]
    if c.vocab == "product":                                        # rows drawn lazily would not be simpler: 32013 x 8 floats is 1 MB
        assert c.d <= 8
    W = _round(g.standard_normal((n_rows, c.d)), c.dtype)
    Wadd = _round(g.standard_normal((v["n_add"], c.d)), c.dtype) if c.has_additional else None
    vt = _round(g.standard_normal((B, c.T_img, c.Nv, c.d)), c.dtype)
    assert c.T_img > max(n for n in c.n_img if n <= c.max_rects)
    return dict(lang_x=lang_x, attention_mask=am if c.has_mask else None, labels=labels if c.has_labels else None, W=W, Wadd=Wadd, vt=vt,
                max_original_id=v["max_original_id"], media=v["media"], assistant=v["assistant"])


def stream_of(row, media, Nv, lost=()):
    """The stream items of one prompt, and for every prompt position the number of items emitted before it."""
    items, before, k = [], [], 0
    for t, tok in enumerate(row):
        before.append(len(items))
        if tok == media and t not in lost:
            items += [("img", k, slot) for slot in range(Nv)]
            k += 1
        else:
            items.append(("tok", t))
    return items, before, k


SPLICE_OUTPUTS = ("plan", "inputs_embeds", "labels", "mask_1d", "rects", "seq_lens", "col_valid_bits", "dense")


def splice_expected(c, inp, mut=None, only_plan=False):
    """Every output of plan + splice + table + dense for case c; `mut` names the one fault the walk below then has."""
    lang_x, am, labels, W, Wadd, vt = inp["lang_x"], inp["attention_mask"], inp["labels"], inp["W"], inp["Wadd"], inp["vt"]
    media, assistant, mo, Nv, B, T = inp["media"], inp["assistant"], inp["max_original_id"], c.Nv, c.B, c.T
    plan = np.full((B + 1, PLAN_STRIDE), GUARD, dtype=np.int32)
    walks = []
    for b in range(B):
        lost = [t for t in range(0, T, K["PLAN_CHUNK"])] if mut == "placeholder_at_chunk_start_lost" else ()
        items, before, n_img = stream_of(lang_x[b], media, Nv, lost)
        where = [t for t in range(T) if lang_x[b, t] == assistant]
        q = (where[-1] if mut == "assistant_last_not_first" else where[0]) if where else 0
        t_img = [t for t in range(T) if lang_x[b, t] == media and t not in lost]
        plan[b, :4] = (n_img, q, len(items), 0)
        plan[b, 4:] = -1
        for k, t in enumerate(t_img):
            if k < MAX_RECTS:
                plan[b, 4 + k] = t
            elif mut == "ninth_index_stored":
                plan.reshape(-1)[b * PLAN_STRIDE + 4 + k] = t
        walks.append((items, before, n_img, q, t_img))
    out = dict(plan=plan)
    if only_plan or c.refused:
        return out
    L_out = max(len(w[0]) for w in walks)
    fill = 0.0 if mut == "pad_rows_zero" else pad_value(c.pad_id, c.dtype)
    embeds = np.empty((B, L_out, c.d), dtype=np.float32)
    labs = np.empty((B, L_out), dtype=np.int64)
    m1d = np.zeros((B, L_out), dtype=np.int64)
    rects = np.zeros((B, c.max_rects, 4), dtype=np.int32)
    dense = np.zeros((B, 1, L_out, L_out), dtype=np.int64)
    for b, (items, before, n_img, q, t_img) in enumerate(walks):
        Lb = len(items)
        rows, lab, msk = [], [], []
        for it in items:
            if it[0] == "tok":
                tok = int(lang_x[b, it[1]])
                if tok > mo and Wadd is not None and mut != "additional_ids_from_main_table":
                    rows.append(Wadd[tok - mo - 1])
                else:
                    rows.append(W[tok])
                lab.append(labels[b, it[1]] if labels is not None else IGNORE)
                msk.append(am[b, it[1]] if am is not None else 1)
            else:
                _, k, slot = it
                rows.append(vt[0 if mut == "vision_row_of_sample_zero" else b, k, slot])
                lab.append(labels[b, t_img[k]] if mut == "image_rows_keep_labels" and labels is not None else IGNORE)
                msk.append(am[b, t_img[k]] if mut == "image_slots_take_prompt_mask" and am is not None else 1)
        pad_rows = [np.full(c.d, fill, dtype=np.float32)] * (L_out - Lb)
        left = c.side == "left"
        embeds[b] = np.stack(pad_rows + rows if left else rows + pad_rows)
        labs[b] = np.asarray([IGNORE] * (L_out - Lb) + lab if left else lab + [IGNORE] * (L_out - Lb), dtype=np.int64)
        m1d[b] = [0] * (L_out - Lb) + msk if left and mut == "left_shift_applied_to_mask" else msk + [0] * (L_out - Lb)
        # rectangles: image k's rows are where its items lie; they see the columns from their end up to text_end
        text_end = before[q] + 1
        if mut == "text_end_without_plus_one":
            text_end = before[q]
        if mut == "text_end_counts_all_images":
            text_end = q + n_img * (Nv - 1) + 1
        for k in range(n_img):
            mine = [i for i, it in enumerate(items) if it[0] == "img" and it[1] == k]
            lo, hi = mine[0], mine[-1] + 1
            if mut == "later_image_offset_dropped":
                lo, hi = t_img[k], t_img[k] + Nv
            r = (min(lo, Lb), min(hi, Lb), min(hi, Lb), min(text_end, Lb))
            if r[1] > r[0] and r[3] > r[2]:
                rects[b, k] = r
        dense[b, 0, :Lb, :Lb] = O.mask_from_spans(m1d[b, :Lb], [tuple(int(x) for x in r) for r in rects[b]])[0]
    out.update(inputs_embeds=embeds, labels=labs if labels is not None else None, mask_1d=m1d, rects=rects,
               seq_lens=np.asarray([len(w[0]) for w in walks], dtype=np.int32), col_valid_bits=pack_bits(m1d), dense=dense, L_out=L_out)
    return out


def splice_edges(c, inp):
    """The named edges that case c reaches, read off its materialised inputs."""
    CHK, e = K["PLAN_CHUNK"], set()
    T, media, assistant = c.T, inp["media"], inp["assistant"]
    for name, val in (("T=1", 1), ("T=63", CHK - 1), ("T=64", CHK), ("T=65", CHK + 1), ("T=128", 2 * CHK), ("T=200", 200)):
        if T == val:
            e.add(name)
    if 900 <= T <= 1100:
        e.add("T~1000")
    e.add(f"Nv={c.Nv}")
    e.add(f"d={c.d}-{c.dtype}")
    if c.d * (2 if c.dtype == "bf16" else 4) // K["VEC_BYTES"] > K["SPLICE_THREADS"]:
        e.add("copy-second-trip")
    e.add(f"side={c.side}")
    e.add("B=5" if c.B == 5 else "B<5")
    for name, has in (("mask", c.has_mask), ("labels", c.has_labels), ("additional", c.has_additional)):
        e.add(f"{name}={'given' if has else 'none'}")
    for b, s in enumerate(c.samples):
        row = inp["lang_x"][b]
        imgs = [t for t in range(T) if row[t] == media]
        asst = [t for t in range(T) if row[t] == assistant]
        e.add(f"n_img={len(imgs)}")
        if 0 in imgs:
            e.add("img@0")
        if T - 1 in imgs:
            e.add("img@T-1")
        if CHK - 1 in imgs and CHK in imgs:
            e.add("img@63+64")
        per_chunk = [sum(1 for t in imgs if t // CHK == ch) for ch in range((T + CHK - 1) // CHK)]
        if max(per_chunk) >= 3:
            e.add("three-in-chunk")
        if len(per_chunk) >= 2 and all(n == 1 for n in per_chunk):
            e.add("one-per-chunk")
        if any(a + 1 == b_ for a, b_ in zip(imgs, imgs[1:])):
            e.add("adjacent-images")
        if not asst:
            e.add("asst-absent")
        else:
            q = asst[0]
            if q == 0:
                e.add("asst@0")
            if imgs and q < imgs[0]:
                e.add("asst-before-all")
            if imgs and imgs[0] < q < imgs[-1]:
                e.add("asst-between")
            if q - 1 in imgs:
                e.add("asst-right-after-image")
            if imgs and q > imgs[-1]:
                e.add("asst-after-all")
            if len(asst) >= 2:
                e.add("asst-twice")
            if any(q // CHK > t // CHK for t in imgs):
                e.add("asst-later-chunk")
            if q >= s.nlen:
                e.add("asst-in-pad-tail")
        if c.has_mask and any(inp["attention_mask"][b, t] == 0 for t in imgs):
            e.add("masked-placeholder")
        if len(imgs) <= c.max_rects and c.T_img > len(imgs) and b > 0 and imgs:
            e.add("T_img>n_img-in-later-sample")
    if not c.refused:
        e.add(f"L_out={c.L_out}")
        if len(set(c.L_b)) > 1:
            e.add("ragged")
        if pad_value(c.pad_id, "bf16") != c.pad_id and c.dtype == "bf16" and len(set(c.L_b)) > 1:
            e.add("pad-inexact-bf16")
        if pad_value(c.pad_id, "bf16") == c.pad_id and c.dtype == "bf16" and len(set(c.L_b)) > 1:
            e.add("pad-exact-bf16")
    return e


SPLICE_EDGES = ("T=1", "T=63", "T=64", "T=65", "T=128", "T=200", "T~1000", "img@0", "img@T-1", "img@63+64", "three-in-chunk", "one-per-chunk",
                "adjacent-images", "n_img=0", "n_img=1", "n_img=2", "n_img=7", "n_img=8", "n_img=9", "asst-absent", "asst@0", "asst-before-all",
                "asst-between", "asst-right-after-image", "asst-after-all", "asst-twice", "asst-later-chunk", "asst-in-pad-tail", "Nv=1", "Nv=4",
                "Nv=144", "d=8-bf16", "d=4-f32", "d=64-bf16", "d=64-f32", "d=3072-bf16", "d=1032-f32", "copy-second-trip", "B=5", "ragged",
                "side=left", "side=right", "mask=given", "mask=none", "labels=given", "labels=none", "additional=given", "additional=none",
                "T_img>n_img-in-later-sample", "L_out=64", "L_out=65", "L_out=128", "L_out=129", "pad-inexact-bf16", "pad-exact-bf16",
                "masked-placeholder")

SPLICE_MUTATIONS = {                     # mutation -> the outputs it must change in at least one case
    "later_image_offset_dropped": ("rects", "dense"),
    "text_end_counts_all_images": ("rects", "dense"),
    "text_end_without_plus_one": ("rects", "dense"),
    "assistant_last_not_first": ("plan", "rects"),
    "left_shift_applied_to_mask": ("mask_1d", "col_valid_bits", "dense"),
    "image_rows_keep_labels": ("labels",),
    "image_slots_take_prompt_mask": ("mask_1d", "col_valid_bits", "dense"),
    "vision_row_of_sample_zero": ("inputs_embeds",),
    "additional_ids_from_main_table": ("inputs_embeds",),
    "pad_rows_zero": ("inputs_embeds",),
    "placeholder_at_chunk_start_lost": ("plan",),
    "ninth_index_stored": ("plan",),
}


# =====================================================================================================================================
# mask tables
# =====================================================================================================================================
@dataclass(frozen=True)
class MaskSample:
    rects: Tuple[Tuple[int, int, int, int], ...]
    seq_len: int
    invalid: Tuple[int, ...] = ()


@dataclass(frozen=True)
class MaskCase:
    id: str
    L: int
    samples: Tuple[MaskSample, ...]
    canonical: bool                 # the device must give back exactly these rectangles
    refused: int = 0                # the number of row groups that ops.mask_to_table must name when it refuses
    why: str = ""

    def __repr__(self):
        return self.id

    @property
    def B(self):
        return len(self.samples)


def is_canonical(s, L):
    """col_lo >= row_hi, interval ends valid, neighbours that touch differ in their columns, rows below seq_len, ascending and disjoint."""
    inv, prev = set(s.invalid), None
    for r in s.rects:
        r0, r1, c0, c1 = r
        if not (0 <= r0 < r1 <= min(s.seq_len, L) and r1 <= c0 < c1 <= L) or c0 in inv or c1 - 1 in inv:
            return False
        if prev is not None and (r0 < prev[1] or (r0 == prev[1] and (c0, c1) == prev[2:]) or (r0 == prev[1] and c1 == prev[3] and c0 == r0 + 1)):
            return False
        prev = r
    return True


def draw_mask_sample(g, L, n, canonical):
    """One table of the family: n (or as many as fit) rectangles on ascending disjoint row ranges, column intervals right of the
    diagonal, about a tenth of the columns invalid, seq_len < L about half of the time."""
    seq = L if g.random() < 0.5 else int(g.integers((L + 1) // 2, L + 1))
    top = min(seq, L - 1)                                     # a row needs a column to its right
    n = min(n, (top + 1) // 2)
    cuts = sorted(g.choice(top + 1, size=2 * n, replace=False).tolist()) if n else []
    rects, protect = [], set()
    for i in range(n):
        r0, r1 = cuts[2 * i], cuts[2 * i + 1]
        c0 = int(g.integers(r1, L)) if canonical or g.random() < 0.3 else int(g.integers(r0 + 1, L))
        c1 = int(g.integers(c0 + 1, L + 1))
        rects.append((r0, r1, c0, c1))
        protect |= {c0, c1 - 1} if canonical else set(range(r0, min(r1 + 2, L)))
    invalid = tuple(sorted(int(x) for x in np.flatnonzero(g.random(L) < 0.1) if x not in protect))
    return MaskSample(tuple(rects), seq, invalid)


def _mask_cases():
    out, CH = [], K["CH"]
    for L in (1, 2, 63, 64, 65, 255, 256, 257):
        for canonical in (True, False):
            g = rng_of("mask", L, canonical)
            B = 3 if L <= 65 else 2
            samples = tuple(draw_mask_sample(g, L, int(g.integers(1, MAX_RECTS + 1)), canonical) for _ in range(B))
            if L == 64 and canonical:                          # an all-zero sample inside the batch
                samples = (samples[0], MaskSample((), 0, tuple(range(L))), samples[2])
            out.append(MaskCase(f"L{L}-{'canon' if canonical else 'free'}", L, samples, canonical and all(is_canonical(s, L) for s in samples),
                                why="drawn from the family"))
    out.append(MaskCase("L65-edges", 65, (MaskSample(((0, 3, 64, 65), (10, 11, 11, 12), (20, 30, 63, 65)), 65, (5, 62)),
                                            MaskSample(((0, 64, 64, 65),), 65, ()),
                                            MaskSample((), 65, tuple(range(1, 64)))), True,
                        why="a set column at L - 1 = 64 (bit 0 of the second word); a row whose only extra column is r + 1; a column that only "
                            "the last row sees"))
    out.append(MaskCase("L257-eight", 257, (MaskSample(tuple((30 * i, 30 * i + 7 + i, 240 + i, 250 + i) for i in range(MAX_RECTS)), 257, (3, 100)),), True,
                        why="exactly AKI_MAX_RECTS row groups are accepted"))
    out.append(MaskCase("L257-nine", 257, (MaskSample(tuple((25 * i, 25 * i + 7, 240 + i, 250 + i) for i in range(MAX_RECTS + 1)), 257, ()),), False,
                        refused=MAX_RECTS + 1, why="one row group more is refused, and the message says how many"))
    out.append(MaskCase(f"L{CH - 1}", CH - 1, (MaskSample(((5, 9, 100, CH - 1), (CH - 10, CH - 2, CH - 2, CH - 1)), CH - 1, (50, 1000)),), True,
                        why="one row short of the LDS chunk"))
    out.append(MaskCase(f"L{CH}", CH, (MaskSample(((0, 1, 1, CH), (CH - 9, CH - 1, CH - 1, CH)), CH, (2, CH - 5)),), True,
                        why="exactly one LDS chunk; the last run closes at row L - 1"))
    out.append(MaskCase(f"L{CH + 1}-ends-at-chunk", CH + 1, (MaskSample(((7, 8, 8, 9), (CH - 8, CH, CH, CH + 1)), CH + 1, (9, 77)),), True,
                        why="a rectangle that ends at row CH: the run is closed by the first row of the second chunk; a set column at L - 1"))
    out.append(MaskCase(f"L{CH + 52}-spans-chunk", CH + 52, (MaskSample(((100, 140, 1000, 1500), (CH - 8, CH + 13, CH + 22, CH + 42)), CH + 40, (1200, CH + 30)),), True,
                        why="a rectangle on rows CH - 8 .. CH + 12: its run is open across the chunk seam; seq_len < L"))
    out.append(MaskCase(f"L{CH + 52}-meets-chunk", CH + 52, (MaskSample(((CH - 18, CH, CH + 12, CH + 32), (CH, CH + 7, CH + 22, CH + 52)), CH + 52, (CH + 1,)),), True,
                        why="one rectangle ends at row CH and the next starts there"))
    out.append(MaskCase(f"L{CH + 52}-free", CH + 52, (MaskSample(((CH - 30, CH + 20, CH - 10, CH + 40), (CH + 30, CH + 45, CH + 31, CH + 52)), CH + 50, (17,)),), False,
                        why="column intervals clipped by the diagonal across the chunk seam: rows whose interval starts at r + 1 join the run"))
    return tuple(out)


MASK_CASES = _mask_cases()
MASK_BY_ID = {c.id: c for c in MASK_CASES}


def mask_arrays(c):
    """rects int32 [B, MAX_RECTS or more, 4], valid bool [B, L], seq_lens int32 [B] of a mask case."""
    k = max(MAX_RECTS, max(len(s.rects) for s in c.samples))
    rects = np.zeros((c.B, k, 4), dtype=np.int32)
    valid = np.ones((c.B, c.L), dtype=bool)
    for b, s in enumerate(c.samples):
        for i, r in enumerate(s.rects):
            rects[b, i] = r
        valid[b, list(s.invalid)] = False
    return rects, valid, np.asarray([s.seq_len for s in c.samples], dtype=np.int32)


def dense_from_table(rects, valid, seq_lens, mut=None):
    """(B, 1, L, L) int64: row r of sample b sees column c iff r < seq_len, c is valid, and c <= r or a rectangle covers (r, c)."""
    B, L = valid.shape
    out = np.zeros((B, 1, L, L), dtype=np.int64)
    r, col = np.arange(L)[:, None], np.arange(L)[None, :]
    for b in range(B):
        vis = col <= r
        for r0, r1, c0, c1 in rects[b]:
            if c1 > c0:
                vis = vis | ((r >= r0) & ((r <= r1) if mut == "rect_row_hi_inclusive" else (r < r1)) & (col >= c0) & (col < c1))
        v = valid[b].copy()
        if mut == "valid_bit_64_in_word_0":
            v = v[np.arange(L) % 64]
        if mut == "last_column_dropped":
            v[L - 1] = False
        live = np.ones(L, dtype=bool) if mut == "seq_len_ignored" else np.arange(L) < seq_lens[b]
        out[b, 0] = vis & v[None, :] & live[:, None]
    return out


def table_from_mask(dense, mut=None):
    """Per sample (rects, valid, seq_len) by the written rule (aki_oracle.mask_to_table), without the limit on the number of rectangles."""
    out = []
    for b in range(dense.shape[0]):
        rects, valid, seq = O.mask_to_table(dense[b, 0], max_rects=1 << 30)
        if mut == "run_split_at_2048":
            CH = K["CH"]
            rects = [p for r in rects for p in (((r[0], CH, r[2], r[3]), (CH, r[1], r[2], r[3])) if r[0] < CH < r[1] else (r,))]
        out.append(([tuple(int(x) for x in r) for r in rects], valid, seq))
    return out


def mask_edges(c):
    CH, e = K["CH"], {f"L={c.L}"}
    for s in c.samples:
        n = len(s.rects)
        if n == MAX_RECTS:
            e.add("eight-groups")
        if n == MAX_RECTS + 1:
            e.add("nine-groups")
        if s.seq_len == 0:
            e.add("all-zero-sample-in-batch" if c.B > 1 else "all-zero")
        if s.seq_len < c.L:
            e.add("seq_len<L")
        if s.invalid:
            e.add("invalid-columns")
        if s.seq_len == c.L and c.L - 1 not in s.invalid and not any(r[3] == c.L for r in s.rects) and c.L > 1:
            e.add("column-only-the-last-row-sees")
        for r0, r1, c0, c1 in s.rects:
            if c1 == c.L and c.L - 1 not in s.invalid:
                e.add("set-column-at-L-1")
            if (r1 - r0, c0, c1) == (1, r0 + 1, r0 + 2):
                e.add("only-extra-column-r+1")
            if r0 < CH < r1:
                e.add("rows-span-chunk")
            if r0 <= CH - 8 and r1 >= CH + 12:
                e.add("rows-span-2040-2060")
            if r0 == CH:
                e.add("starts-at-chunk")
            if r1 == CH:
                e.add("ends-at-chunk")
            if c0 < r1:
                e.add("clipped-by-diagonal")
    e.add("canonical" if c.canonical else "free")
    return e


MASK_EDGES = tuple(f"L={L}" for L in (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2100)) + (
    "eight-groups", "nine-groups", "all-zero-sample-in-batch", "seq_len<L", "invalid-columns", "column-only-the-last-row-sees", "set-column-at-L-1",
    "only-extra-column-r+1", "rows-span-chunk", "rows-span-2040-2060", "starts-at-chunk", "ends-at-chunk", "clipped-by-diagonal", "canonical", "free")

MASK_MUTATIONS = {"rect_row_hi_inclusive": "dense", "seq_len_ignored": "dense", "valid_bit_64_in_word_0": "dense", "last_column_dropped": "dense",
                  "run_split_at_2048": "rects"}


# =====================================================================================================================================
# SFT collate
# =====================================================================================================================================
@dataclass(frozen=True)
class CollateCase:
    id: str
    T_out: int
    lengths: Tuple[int, ...]
    side: str
    pad_id: int = 32000
    why: str = ""

    def __repr__(self):
        return self.id

    @property
    def B(self):
        return len(self.lengths)


def _collate_cases():
    out = []
    for T_out, side in ((1, "right"), (1, "left"), (255, "left"), (256, "right"), (256, "left"), (257, "right"), (257, "left"), (1000, "right"), (1000, "left")):
        lengths = tuple(n for n in (T_out + 300, T_out, T_out - 1, 1, T_out + 1, T_out // 2, 2 * T_out + 5) if n > 0)
        out.append(CollateCase(f"t{T_out}-{side}", T_out, lengths, side, why="a sample longer than T_out, one equal to it, shorter ones"))
    g = rng_of("collate-b70")
    out.append(CollateCase("t257-b70-left", 257, tuple(int(x) for x in g.integers(1, 600, 70)), "left", pad_id=0, why="70 samples: one block each"))
    out.append(CollateCase("t300-b70-right", 300, tuple(int(x) for x in g.integers(1, 600, 70)), "right", pad_id=7))
    return tuple(out)


COLLATE_CASES = _collate_cases()


def collate_inputs(c):
    g = rng_of("collate", c.id)
    ids = [g.integers(3, 32000, n).astype(np.int64) for n in c.lengths]
    labels = [np.where(g.random(n) < 0.3, IGNORE, x * 2 + 1).astype(np.int64) for n, x in zip(c.lengths, ids)]
    mask = [(g.random(n) < 0.9).astype(np.int64) for n in c.lengths]
    return dict(input_ids=ids, labels=labels, attention_mask=mask)


COLLATE_PADS = {"input_ids": None, "labels": IGNORE, "attention_mask": 0}


def collate_expected(c, inp, mut=None):
    out = {}
    for key, pad in COLLATE_PADS.items():
        pad = c.pad_id if pad is None else pad
        want = O.sft_pad_trunc(inp[key], "max_length", c.side, pad, c.T_out)
        if mut:
            for b, s in enumerate(inp[key]):
                if len(s) > c.T_out and (mut == "truncation_keeps_last_tokens" or (mut == "left_shift_when_truncated" and c.side == "left")):
                    want[b] = s[len(s) - c.T_out:]
        out[key] = want
    return out


def collate_edges(c):
    e = {f"T_out={c.T_out}", f"side={c.side}"}
    if c.T_out > K["COLLATE_THREADS"]:
        e.add("second-trip")
    if c.B >= 70:
        e.add("B=70")
    for n in c.lengths:
        e.add("longer" if n > c.T_out else "equal" if n == c.T_out else "shorter")
    if c.T_out > K["COLLATE_THREADS"] and c.side == "left" and any(n > c.T_out for n in c.lengths):
        e.add("truncation+left+second-trip")
    return e


COLLATE_EDGES = ("T_out=1", "T_out=255", "T_out=256", "T_out=257", "T_out=1000", "side=left", "side=right", "second-trip", "B=70", "longer", "equal",
                 "shorter", "truncation+left+second-trip")
COLLATE_MUTATIONS = ("truncation_keeps_last_tokens", "left_shift_when_truncated")


# =====================================================================================================================================
# im2col
# =====================================================================================================================================
@dataclass(frozen=True)
class Im2colCase:
    S: int
    P: int
    N: int
    dtype: str

    @property
    def id(self):
        return f"s{self.S}-p{self.P}-n{self.N}-{self.dtype}"

    def __repr__(self):
        return self.id

    @property
    def G(self):
        return self.S // self.P

    @property
    def Kp(self):
        return (3 * self.P * self.P + 63) // 64 * 64


IM2COL_CASES = tuple(Im2colCase(S_, P, N, dt) for (S_, P), N, dt in (
    ((8, 4), 1, "bf16"), ((8, 4), 3, "f32"), ((30, 14), 3, "bf16"), ((30, 14), 1, "f32"), ((32, 16), 1, "bf16"), ((32, 16), 3, "f32"),
    ((336, 14), 1, "bf16"), ((336, 14), 3, "f32"), ((384, 14), 3, "bf16"), ((384, 14), 1, "f32")))


def im2col_inputs(c):
    """Pixels [N, 3, S, S] of c.dtype as float32, none of them zero: x * 1 + 0 + ... is x bit for bit only while x is not -0."""
    g = rng_of("im2col", c.id)
    x = _round(g.standard_normal((c.N, 3, c.S, c.S)), c.dtype)
    x[x == 0] = 1.0
    return x


def im2col_expected(c, pix, mut=None):
    """[N * G * G, Kp]: row n G G + gy G + gx, column ch P P + py P + px = pix[n, ch, gy P + py, gx P + px]; columns >= 3 P P are zero."""
    N, S_, P, G, Kp = c.N, c.S, c.P, c.G, c.Kp
    out = np.zeros((N, G, G, Kp), dtype=np.float32)
    src = pix
    if mut == "remainder_pixels_used":                         # the image read as if it were G P pixels wide
        flat = pix.reshape(N, 3, S_ * S_)
        src = flat[:, :, :G * P * G * P].reshape(N, 3, G * P, G * P)
    for ch in range(3):
        for py in range(P):
            for px in range(P):
                col = ch * P * P + ((px * P + py) if mut == "py_px_swapped" else (py * P + px))
                out[:, :, :, col] = src[:, ch, py:py + (G - 1) * P + 1:P, px:px + (G - 1) * P + 1:P]
    if mut == "pad_columns_carry_pixels":
        for col in range(3 * P * P, Kp):
            out[:, :, :, col] = out[:, :, :, col - 3 * P * P]
    return out.reshape(N * G * G, Kp)


def im2col_edges(c):
    e = {f"S={c.S}-P={c.P}", f"N={c.N}", c.dtype}
    if c.S % c.P:
        e.add("remainder-pixels")
    if c.Kp > 3 * c.P * c.P:
        e.add("pad-columns")
    else:
        e.add("no-pad-columns")
    return e


IM2COL_EDGES = ("S=8-P=4", "S=30-P=14", "S=32-P=16", "S=336-P=14", "S=384-P=14", "N=1", "N=3", "bf16", "f32", "remainder-pixels", "pad-columns",
                "no-pad-columns")
IM2COL_MUTATIONS = ("py_px_swapped", "remainder_pixels_used", "pad_columns_carry_pixels")

MUTATIONS = {"splice": tuple(SPLICE_MUTATIONS), "mask": tuple(MASK_MUTATIONS), "collate": COLLATE_MUTATIONS, "im2col": IM2COL_MUTATIONS}
