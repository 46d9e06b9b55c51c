"""The case table of tests/fwd_row_cases.py checked on the CPU with the references alone: the numpy e4m3 rounding against torch's cast,
every float64 reference against torch in float64, a plain float32 torch implementation and the cast of the reference itself inside
every bar, the shares of undecided elements and of elements with more than one admissible byte under their caps, every structural edge
reached (from the constants read out of the .hip sources) and every mutation visible at MIN_RATIO or at its derived cap."""
import numpy as np
import pytest
import torch

import fwd_row_cases as T

K = T.kernel_constants()
_ids = lambda cs: [c.id for c in cs]
NORM_KERNELS = ("norm_bf16", "norm_f32", "row_stats")


# ---- e4m3 ----------------------------------------------------------------------------------------------------------------------------
def _torch_e4m3(v32):
    return torch.from_numpy(v32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_e4m3_rne_matches_torch_on_every_code_midpoint_and_neighbour():
    """All 256 codes decode and re-encode to themselves (the two NaN codes aside, which the kernels' clamp never produces); every
    midpoint of adjacent values, one f32 ulp below and above each of them, both zeros and the saturating range up to 464 and past it
    round as CPU torch's float8_e4m3fn cast does."""
    codes = np.arange(256, dtype=np.uint8)
    val = T.e4m3_decode(codes)
    finite = np.isfinite(val)
    assert finite.sum() == 254 and np.isnan(val[0x7F]) and np.isnan(val[0xFF]) and val[0x7E] == 448.0 and val[0x01] == 2.0 ** -9
    assert np.array_equal(T.e4m3_rne(val[finite]), codes[finite])
    pos = np.sort(val[:0x7F])
    mids = 0.5 * (pos[1:] + pos[:-1])
    pts = np.concatenate([pos, mids, [464.0, 448.0, 456.0, 2.0 ** -10, 2.0 ** -11, 480.0, 1e4]]).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64)[:len(pos) + len(mids)], np.concatenate([pos, mids]))      # all exact in f32
    pts = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))])
    pts = np.concatenate([pts, -pts])
    assert np.array_equal(T.e4m3_rne(pts.astype(np.float64)), _torch_e4m3(pts))
    assert T.e4m3_rne(np.array([0.0, -0.0, -2.0 ** -11])).tolist() == [0x00, 0x80, 0x80]
    g = T.rng_of("e4m3")
    r = (g.standard_normal(20000) * np.exp2(g.uniform(-12, 9, 20000))).astype(np.float32)
    r = r[np.abs(r) <= 464.0]
    assert np.array_equal(T.e4m3_rne(r.astype(np.float64)), _torch_e4m3(r))


def test_e4m3_mutated_roundings_differ_where_they_should():
    t = np.array([1.0625, 1.1875, 1.03, 2.0 ** -8, 3.0])                 # two ties (to 1.0 and to 1.25), an inexact value, a subnormal
    assert T.e4m3_decode(T.e4m3_rne(t)).tolist() == [1.0, 1.25, 1.0, 2.0 ** -8, 3.0]
    assert T.e4m3_decode(T.e4m3_mutated(t, "away")).tolist() == [1.125, 1.25, 1.0, 2.0 ** -8, 3.0]
    assert T.e4m3_decode(T.e4m3_mutated(t, "trunc")).tolist() == [1.0, 1.125, 1.0, 2.0 ** -8, 3.0]
    assert T.e4m3_decode(T.e4m3_mutated(t, "flush")).tolist() == [1.0, 1.25, 1.0, 0.0, 3.0]


# ---- norms and row statistics --------------------------------------------------------------------------------------------------------
def _outs(ref):
    return {n: o for n, o in ref.items() if n != "zero_rows"}


@pytest.mark.parametrize("c", T.NORM_CASES, ids=[repr(c) for c in T.NORM_CASES])
def test_norm_reference_float32_and_cast(c):
    for fam in T.NORM_FAMILIES:
        inp = T.norm_inputs(c, fam)
        ref = T.norm_reference(c, inp)
        t64 = T.norm_torch64(c, inp)
        f32 = T.norm_f32(c, inp)
        for name, o in _outs(ref).items():
            if name == "y" and isinstance(o, T.Either):                   # the reference before its two casts
                n = T.f64(inp["x"]) * t64["rstd"][:, None]
                assert (np.abs(n * T.f64(inp["w"]) - t64["y"]) <= 1e-12 * np.abs(t64["y"]) + 1e-300).all()
                cast = T.f64(T.bf(o.alts[0].x))
            else:
                M = o.M + np.abs(o.x)
                assert (np.abs(o.x - t64[name].reshape(o.x.shape)) <= 1e-10 * M + 1e-300).all(), f"{c} [{fam}]: {name} differs from torch float64"
                cast = T.f64(T.bf(o.x)) if o.kind == "bf16" else o.x.astype(np.float32).astype(np.float64)
            assert o.worst(cast) <= 1.0, f"{c} [{fam}]: the cast of the reference's {name} is outside its bar"
            w = o.worst(f32[name].reshape(o.x.shape))
            assert w <= 1.0, f"{c} [{fam}]: the float32 implementation's {name} is at {w:.3f} of the bar"
        if "y" in ref:
            if isinstance(ref["y"], T.Either) and fam != "special":
                share = ref["y"].undecided.mean()
                assert share <= 0.01, f"{c} [{fam}]: {share:.4f} of the elements are undecided"
            for r in ref["zero_rows"]:                                    # exact zeros (RMS), exactly the bias (LN)
                want = np.zeros(c.cols) if inp["b"] is None else T.f64(inp["b"])
                assert np.array_equal(f32["y"][r], want) and np.array_equal(ref["y"].x[r], want)


def test_norm_families_are_what_the_docstring_says():
    c = T.CASE_BY_ID[("norm_bf16", "ln-c2048")]
    x = T.f64(T.norm_inputs(c, "offset")["x"])
    assert (np.abs(x.mean(1)) > 50 * x.std(1)).all()
    x = T.f64(T.norm_inputs(c, "small")["x"])
    assert 0.1 * T.NORM_EPS < (x * x).mean() < 10 * T.NORM_EPS
    for kernel in NORM_KERNELS:
        for c in T.CASES[kernel]:
            x = T.f64(T.norm_inputs(c, "special")["x"])
            assert not x[0].any() and ((x[1:] != 0).sum(1) == 1).all()
            for fam in T.NORM_FAMILIES:
                assert (T.f64(T.norm_inputs(c, fam)["x"]) ** 2).sum(1).max() < 2.0 ** 127
    c = T.CASE_BY_ID[("norm_bf16", "rms-c8192")]
    hot = {int(np.flatnonzero(r)[0]) for r in T.f64(T.norm_inputs(c, "special")["x"])[1:]}
    assert hot <= set(T.placed_columns(8192)) and len(hot) == 4 and T.placed_columns(8192) == [0, 507, 1536, 6144, 8191]


def test_norm_edges_are_reached():
    assert K["NORM_MAXC"] == 4 and K["NORM_THREADS"] == 256 and K["NORM_MAX_COLS"] == 8192, "re-aim the bf16 norm cases at the new constants"
    assert K["F32_THREADS"] == 256 and K["STATS_STRIDE"] == 2048, "re-aim the f32 norm / row_stats cases at the new constants"
    top = K["NORM_MAX_COLS"]
    slot = K["NORM_THREADS"] * 8
    cols = {c.cols for c in T.CASES["norm_bf16"]}
    assert {8, slot - 8, slot, slot + 8, 2 * slot, 2 * slot + 8, 3 * slot + 8, top} <= cols            # every register chunk, first and last
    assert (3 * slot + 8) // 8 - 1 >= 3 * K["NORM_THREADS"]                                             # chunk index 3 holds data at 6152
    assert f"cols-{top + 8}" in T.NORM_REJECTED
    for mode in T.NORM_MODES:
        assert any(c.mode == mode and c.ldx > c.cols and c.ldy > c.cols and c.ldx != c.ldy for c in T.CASES["norm_bf16"])
        assert any(c.mode == mode and c.ldx > c.cols for c in T.CASES["norm_f32"])
    f32 = {c.cols for c in T.CASES["norm_f32"]}
    assert {1, 255, 256, 257} <= f32 and max(f32) > 3 * 256
    st = {c.cols for c in T.CASES["row_stats"]}
    stride = K["STATS_STRIDE"]
    assert {8, stride - 8, stride, stride + 8, 2 * stride + 8, 4 * stride, 8 * stride + 8} <= st         # the stride crossed once, twice, eight times
    assert any(c.ldx > c.cols for c in T.CASES["row_stats"]) and {c.mode for c in T.CASES["row_stats"]} == {"rms", "ln"}
    assert T.chain_length(T.CASE_BY_ID[("row_stats", "ln-c16392")]) == 82 and T.chain_length(T.CASE_BY_ID[("norm_f32", "ln-c3072")]) == 22


def _norm_mutation_reach(kernel, m):
    best = 0.0
    for cid in T.MUTATIONS[kernel][m]:
        c = T.CASE_BY_ID[(kernel, cid)]
        for fam in T.NORM_FAMILIES:
            inp = T.norm_inputs(c, fam)
            ref, mut = T.norm_reference(c, inp), T.norm_reference(c, inp, m)
            best = max([best] + [o.worst(mut[n].x) for n, o in _outs(ref).items()])
    return best


@pytest.mark.parametrize("kernel,m", [(k, m) for k in NORM_KERNELS for m in T.MUTATIONS[k]])
def test_norm_mutations_are_visible(kernel, m):
    need = T.CAPPED.get((kernel, m), T.MIN_RATIO)
    best = _norm_mutation_reach(kernel, m)
    print(f"{kernel} {m}: {best:.2f}")
    assert best >= need, f"{kernel} mutation {m} reaches only {best:.2f} of the bar"


def test_each_listed_case_sees_the_edge_mutations_alone():
    """Chunk 3 and wave 3 left out are visible on EVERY case listed for them, not only on the best one."""
    for kernel in NORM_KERNELS:
        for m in ("chunk3-out", "wave3-out"):
            for cid in T.MUTATIONS[kernel][m]:
                c = T.CASE_BY_ID[(kernel, cid)]
                best = 0.0
                for fam in T.NORM_FAMILIES:
                    inp = T.norm_inputs(c, fam)
                    ref, mut = T.norm_reference(c, inp), T.norm_reference(c, inp, m)
                    best = max([best] + [o.worst(mut[n].x) for n, o in _outs(ref).items()])
                assert best >= T.MIN_RATIO, f"{kernel} {m} on {cid}: {best:.2f}"


# ---- quantisers ----------------------------------------------------------------------------------------------------------------------
def _q_inputs(c, fam):
    return T.kv_inputs(c, fam) if c.kernel == "kv_quant" else T.quant_inputs(c, fam)


QCASES = T.QUANT_CASES + T.KV_CASES


@pytest.mark.parametrize("c", QCASES, ids=[repr(c) for c in QCASES])
def test_quantiser_float32_and_float64_rules_are_admissible(c):
    for fam in T.families_of(c):
        inp = _q_inputs(c, fam)
        ref = T.QuantRef(c, inp)
        for f32 in (True, False):
            s, q = T.quant_stand_in(c, inp, f32=f32)
            what = f"{c} [{fam}, {'float32' if f32 else 'float64'}]"
            assert ref.scale_ratio(s).max() <= 1.0, f"{what}: scale at {ref.scale_ratio(s).max():.3f} of its bar"
            bad = ref.bad_bytes(s, q)
            assert not bad.any(), f"{what}: {int(bad.sum())} inadmissible bytes, first at {np.argwhere(bad)[0].tolist()}"
            assert ref.byte_ratio(s, q).max() <= 1.0
        many = (ref.choices(s) > 1).mean()
        if fam != "ties":
            assert many <= 0.02, f"{c} [{fam}]: {many:.4f} of the elements have more than one admissible byte"
            if c.mode == "rms" and fam != "special":
                assert ref.undecided.mean() <= 0.01
        else:
            assert ref.delta == 0.0 and (ref.choices(s) == 1).all(), f"{c}: a tie with more than one admissible byte"


def test_quantiser_families_are_what_the_docstring_says():
    for c in T.QUANT_CASES:
        at = T.placed_columns(c.cols)
        x = np.abs(T.f64(T.quant_inputs(c, "peak")["x"]))
        assert x.shape[0] == len(at) and x.argmax(1).tolist() == at
        for r, p in enumerate(at):
            assert np.delete(x[r], p).max() <= x[r, p] / 8
        sp = T.f64(T.quant_inputs(c, "special")["x"])
        assert not sp[0].any() and (sp[1] != 0).sum() == 1 and sp[1, -1] != 0
        if c.mode == "plain":
            ref = T.QuantRef(c, T.quant_inputs(c, "subnormal"))
            t = np.abs(ref.ya) / (np.abs(ref.ya).max(1, keepdims=True) / 448.0)
            small = t[:, 1:]
            assert small.max() < 2.0 ** -6 and (small < 2.0 ** -10).mean() > 0.2 and ((small > 2.0 ** -9) & (small < 2.0 ** -6)).mean() > 0.2
            ti = T.f64(T.quant_inputs(c, "ties")["x"])
            s = np.abs(ti).max(1, keepdims=True) / 448.0
            assert np.array_equal(np.log2(s[:, 0]), np.array(T.TIE_K, dtype=np.float64))
            tt = ti / s
            on_tie = T.e4m3_rne(tt * (1 - 2.0 ** -30)) != T.e4m3_rne(tt * (1 + 2.0 ** -30))
            assert on_tie.mean() > 0.95 if c.cols > 8 else on_tie.sum() >= 6
    assert T.placed_columns(8192) == [0, 507, 1536, 6144, 8191] and T.placed_columns(6152)[3] == 6144
    for c in T.KV_CASES:
        x = T.f64(T.kv_inputs(c, "ties")["x"])
        s = np.abs(x).max(-1, keepdims=True) / 448.0
        assert (np.log2(s) == np.round(np.log2(s))).all()
        z = T.kv_inputs(c, "zero")["x"]
        if c.rows >= 2:
            assert not T.f64(z)[0, 0].any() and bool(torch.signbit(z.float())[0, 0, 40])


def test_quantiser_edges_are_reached():
    assert K["QUANT_MAXC"] == 4 and K["QUANT_THREADS"] == 256 and K["QUANT_MAX_COLS"] == 8192, "re-aim the quant_rows cases"
    assert K["KV_ROWS_PER_BLOCK"] == 16 and K["KV_LANES"] == 16 and K["KV_LIVE_LANES"] * 8 == T.KV_DH, "re-aim the KV cases"
    slot = K["QUANT_THREADS"] * 8
    cols = {c.cols for c in T.QUANT_CASES}
    assert {8, slot - 8, slot, slot + 8, 3 * slot + 8, K["QUANT_MAX_COLS"]} <= cols
    assert all(c.ldx > c.cols and c.ldq > c.cols and c.ldq != c.ldx for c in T.QUANT_CASES)
    per = K["KV_ROWS_PER_BLOCK"]
    spans = []
    for c in T.KV_CASES:
        total = c.slabs * c.rows
        blocks = -(-total // per)
        spans.append(max(len({r // c.rows for r in range(b * per, min((b + 1) * per, total))}) for b in range(blocks)))
    assert max(spans) == 4 and 1 in spans                                                    # a block over four slabs
    assert any((c.slabs * c.rows) % per for c in T.KV_CASES) and any((c.slabs * c.rows) % per == 0 for c in T.KV_CASES)
    assert any(c.src_cap < c.dst_cap for c in T.KV_CASES) and any(c.src_cap > c.dst_cap for c in T.KV_CASES)
    assert any(c.rows < min(c.src_cap, c.dst_cap) for c in T.KV_CASES) and any(c.rows > per for c in T.KV_CASES)


def _quant_mutation_reach(kernel, m):
    best = 0.0
    for cid in T.MUTATIONS[kernel][m]:
        c = T.CASE_BY_ID[(kernel, cid)]
        for fam in T.families_of(c):
            inp = _q_inputs(c, fam)
            ref = T.QuantRef(c, inp)
            s0, _ = T.quant_stand_in(c, inp)
            s, q = T.quant_stand_in(c, inp, m)
            moved = ref.scale_ratio(s)[s != s0]                          # the scale counts where the mutation changed it
            best = max(best, float(moved.max()) if moved.size else 0.0, float(ref.bad_bytes(s, q).sum()))
    return best


@pytest.mark.parametrize("kernel,m", [(k, m) for k in ("quant_rows", "kv_quant") for m in T.MUTATIONS[k]])
def test_quantiser_mutations_are_visible(kernel, m):
    need = T.CAPPED.get((kernel, m), T.MIN_RATIO)
    best = _quant_mutation_reach(kernel, m)
    print(f"{kernel} {m}: {best:.2f}")
    assert best >= need, f"{kernel} mutation {m} reaches only {best:.2f}"


def test_capped_quantiser_mutations_are_invisible_as_derived():
    """Without the clamp every byte stays admissible: the caps of 0 are what the bars give."""
    for key, cap in T.CAPPED.items():
        if cap == 0.0:
            assert _quant_mutation_reach(*key) == 0.0


# ---- rope_append ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.ROPE_CASES, ids=_ids(T.ROPE_CASES))
def test_rope_reference_float32_and_cast(c):
    inp = T.rope_inputs(c)
    ref = T.rope_reference(c, inp)
    assert (inp["pos"] != inp["cache_len"]).all() and int(inp["pos"].max()) == T.ROPE_TABLE_ROWS - 1 and int(inp["cache_len"].max()) < c.cap
    row = inp["qkv"].to(torch.float64)
    pos = inp["pos"].long()
    cs, sn = inp["cos"].to(torch.float64)[pos][:, None], inp["sin"].to(torch.float64)[pos][:, None]
    rot = lambda t: torch.cat((-t[..., c.Dh // 2:], t[..., :c.Dh // 2]), -1)
    parts = [row[:, i * c.H * c.Dh:(i + 1) * c.H * c.Dh].reshape(c.B, c.H, c.Dh) for i in range(3)]
    for name, t in (("q", parts[0]), ("k", parts[1])):
        assert np.array_equal((t * cs + rot(t) * sn).numpy(), ref[name].x)
        cast = T.f64(T.bf(ref[name].x)) if not c.f32 else ref[name].x.astype(np.float32).astype(np.float64)
        assert ref[name].worst(cast) <= 1.0
    assert np.array_equal(parts[2].numpy(), ref["v"].x)
    f32 = T.rope_f32(c, inp)
    for name in ("q", "k"):
        assert ref[name].worst(f32[name]) <= 1.0
    assert np.array_equal(f32["v"], ref["v"].x)


def test_rope_edges_are_reached():
    assert K["ROPE_THREADS"] == 256
    hd = {c.H * c.Dh for c in T.ROPE_CASES}
    assert any(n < 256 for n in hd) and any(n > 256 and n % 256 for n in hd) and any(n % 256 == 0 for n in hd)
    assert {c.at for c in T.ROPE_CASES} == {"0", "last", "mid"} and {c.f32 for c in T.ROPE_CASES} == {False, True}
    mid = T.rope_inputs(T.CASE_BY_ID[("rope_append", "b3-h5-d96-bf16-at-mid")])["cache_len"].tolist()
    assert len(set(mid)) == 3 and all(0 <= v < T.ROPE_CAP - 1 for v in mid)


@pytest.mark.parametrize("m", list(T.MUTATIONS["rope_append"]))
def test_rope_mutations_are_visible(m):
    for cid in T.MUTATIONS["rope_append"][m]:
        c = T.CASE_BY_ID[("rope_append", cid)]
        inp = T.rope_inputs(c)
        ref, mut = T.rope_reference(c, inp), T.rope_reference(c, inp, m)
        best = max(ref[n].worst(mut[n].x) for n in ("q", "k"))
        assert best >= T.MIN_RATIO, f"rope_append mutation {m} on {cid} reaches only {best:.2f} of the bar"
