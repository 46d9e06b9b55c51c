"""Case table, inputs, float64 reference and reference mutations of the grouped decode attention kernel
(aki_amd/csrc/decode.hip: decode_attn_group_kernel - N returned rows per prompt sample over one shared copy of the prompt's K/V).

numpy and CPU torch only.  The number formats, the tolerance, the two input families and the 8x bar are those of
tests/decode_attn_cases.py and are imported from there.  tests/test_decode_group_cases_cpu.py checks the table (every REQUIRED
corner of the launch plan is reached; every mutation of the reference moves an element by at least MIN_RATIO tolerances) and
tests/test_decode_group_gpu.py runs every case on the device.

Rows of one group share the raw query up to a per-row perturbation of 1/4, so that the sentinel scores set on the SHARED prefix keys
hold for every row of the group to within that perturbation, while rows still differ in q, in position and in their suffix rows.
"""
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import aki_oracle as O
from decode_attn_cases import DH, FAMILIES, MASKED_SCORE_LIFT, MASKED_V, MIN_RATIO, SCALE, _unrotate, bf16, dec_items, rotate_bf16, tolerance  # noqa: F401


def plan(B0, N, H, pcap, scap, max_pkeys=0, max_skeys=0):
    """(Sp, Tp, Ss, Ts, NC) of decode_attn_group_launch: tiles per item from the capacities, items from the key bounds."""
    if max_pkeys <= 0 or max_pkeys > pcap:
        max_pkeys = pcap
    if max_skeys <= 0 or max_skeys > scap:
        max_skeys = scap
    NC, items = (N + 15) // 16, dec_items()
    Tp = max(1, (B0 * NC * H * ((pcap + 63) // 64) + items - 1) // items)
    Ts = max(1, (B0 * N * H * ((scap + 63) // 64) + items - 1) // items)
    return ((max_pkeys + 63) // 64 + Tp - 1) // Tp, Tp, ((max_skeys + 63) // 64 + Ts - 1) // Ts, Ts, NC


@dataclass(frozen=True)
class Case:
    id: str
    B0: int
    N: int
    H: int
    pcap: int
    scap: int
    plens: tuple                # prefix_len[b]
    slens: tuple                # per row r: cached suffix rows = cache_len[r] - prefix_len[r // N] (the new token comes on top)
    masks: tuple                # per sample: masked prefix column ranges [lo, hi)
    nwords: int

    @property
    def rows(self):
        return self.B0 * self.N

    def lens(self):
        return tuple(self.plens[r // self.N] + self.slens[r] for r in range(self.rows))

    def keep(self, b):
        k = np.ones(self.plens[b], dtype=bool)
        for lo, hi in self.masks[b]:
            k[lo:hi] = False
        return k

    def bits(self):
        if self.nwords == 0:
            return None
        pad = np.ones((self.B0, self.nwords * 64), dtype=bool)
        for b in range(self.B0):
            for lo, hi in self.masks[b]:
                pad[b, lo:hi] = False
        return np.packbits(pad.reshape(self.B0, self.nwords, 64), axis=-1, bitorder="little").view(np.uint64).reshape(
            self.B0, self.nwords).view(np.int64).copy()

    def key_bounds(self):
        """(max_prefix_keys, max_suffix_keys) of an eager step, and of a captured one (the capacities)."""
        return ((max(self.plens), max(self.slens) + 1), (0, 0))


def _case(id, B0, N, H, pcap, scap, plens, slens, masks=None, nwords=None):
    slens = tuple(slens) if len(slens) == B0 * N else tuple(slens) * (B0 * N // len(slens))
    masks = tuple(tuple(m) for m in (masks if masks is not None else [()] * B0))
    nwords = (max(plens) + 63) // 64 if nwords is None else nwords
    c = Case(id, B0, N, H, pcap, scap, tuple(plens), slens, masks, nwords)
    assert len(c.plens) == B0 and len(c.slens) == B0 * N and all(1 <= p <= pcap for p in c.plens) and all(0 <= s < scap for s in c.slens), id
    assert all(0 <= lo < hi <= min(c.plens[b], nwords * 64) for b in range(B0) for lo, hi in masks[b]), id
    return c


# The plan arithmetic is written for AKI_DEC_ITEMS = 2048; the CPU test asserts the coverage from plan().
CASES = (
    _case("n1-h2-p1-s0", 1, 1, 2, 64, 64, [1], [0], nwords=0),
    _case("n2-h2-p63-64-s1-63-holes", 2, 2, 2, 128, 128, [63, 64], [1, 63, 0, 64], [[(3, 7)], [(0, 1), (30, 40)]]),
    _case("n3-h4-p65-s64-65-300-prefix-masked", 2, 3, 4, 128, 320, [65, 40], [64, 65, 300, 0, 1, 2], [[(10, 20)], [(0, 40)]]),
    _case("n8-h2-p655-ragged-suffix", 1, 8, 2, 704, 128, [655], [0, 1, 5, 63, 64, 65, 100, 127], [[(100, 170)]]),
    _case("n16-h32-p300-T2", 1, 16, 32, 8192, 64, [300], [3], [[(60, 70)]]),
    _case("n17-h2-p655-two-chunks", 1, 17, 2, 704, 64, [655], list(range(17))),
    _case("n33-h2-p130-three-chunks", 2, 33, 2, 192, 64, [130, 70], [r % 7 for r in range(66)], [[(5, 9)], [(64, 70)]]),
    _case("n4-h32-p700-T3-b4", 4, 4, 32, 3000, 64, [700, 191, 192, 193], [2], [(), [(0, 64)], (), [(100, 140)]]),
    _case("n16-h32-p4096-flagship", 1, 16, 32, 4224, 128, [4096], [r % 5 for r in range(16)], [[(2048, 2112)]]),
)
CASE_BY_ID = {c.id: c for c in CASES}
LARGEST = "n16-h32-p4096-flagship"

REQUIRED = ("N=1", "N=2", "N=3", "N=8", "N=16", "N=17", "N=33", "plen=1", "plen=63", "plen=64", "plen=65", "plen=655", "plen=4096",
            "two-samples-different-plen-with-holes", "prefix-fully-masked", "slen=0", "slen=1", "slen=63", "slen=64", "slen=65", "slen=300",
            "ragged-suffix-in-group", "Tp=1", "Tp=2", "Tp>=3", "H=32,rows=16", "small-H")


def properties(c: Case) -> set:
    P = {f"N={c.N}"} | {f"plen={p}" for p in c.plens} | {f"slen={s}" for s in c.slens}
    Tp = plan(c.B0, c.N, c.H, c.pcap, c.scap)[1]
    P.add("Tp=1" if Tp == 1 else "Tp=2" if Tp == 2 else "Tp>=3")
    if c.B0 >= 2 and len(set(c.plens)) > 1 and sum(1 for m in c.masks if m) >= 2:
        P.add("two-samples-different-plen-with-holes")
    if any(not c.keep(b).any() for b in range(c.B0)):
        P.add("prefix-fully-masked")
    if any(len(set(c.slens[b * c.N:(b + 1) * c.N])) > 1 for b in range(c.B0)):
        P.add("ragged-suffix-in-group")
    if c.H == 32 and c.rows == 16:
        P.add("H=32,rows=16")
    if c.H < 32:
        P.add("small-H")
    return P


@dataclass
class Inputs:
    case: Case
    family: str
    qkv: torch.Tensor            # bf16 [rows, 3 * H * 96], un-rotated
    kp: torch.Tensor             # bf16 [B0, H, pcap, 96]: rows < plens[b] cached, NaN behind them
    vp: torch.Tensor
    ks: torch.Tensor             # bf16 [rows, H, scap, 96]: rows < slens[r] cached, NaN from the append row on
    vs: torch.Tensor
    cos: np.ndarray
    sin: np.ndarray
    stale_k: np.ndarray
    stale_v: np.ndarray


def _sentinel_cols(n, keep):
    want = {0, n - 1} | {e + d for e in range(64, n, 64) for d in (-1, 0)}
    cols = sorted(j for j in want if 0 <= j < n and keep[j])
    if len(cols) > 12:
        cols = [cols[i] for i in sorted({round(k * (len(cols) - 1) / 11) for k in range(12)})]
    return cols


def make_inputs(case: Case, family: str) -> Inputs:
    assert family in FAMILIES
    c, H = case, case.H
    rng = np.random.default_rng(zlib.crc32(f"{c.id}/{family}".encode()))
    npos = c.pcap + c.scap
    cos, sin = (a[0] for a in O.rope_cos_sin(np.arange(npos)[None], DH))
    kp = torch.full((c.B0, H, c.pcap, DH), float("nan"), dtype=torch.bfloat16)
    vp = torch.full((c.B0, H, c.pcap, DH), float("nan"), dtype=torch.bfloat16)
    ks = torch.full((c.rows, H, c.scap, DH), float("nan"), dtype=torch.bfloat16)
    vs = torch.full((c.rows, H, c.scap, DH), float("nan"), dtype=torch.bfloat16)
    qkv = np.zeros((c.rows, 3, H, DH), dtype=np.float32)
    lens = c.lens()
    for b in range(c.B0):
        pl, keep = c.plens[b], c.keep(b)
        r0 = b * c.N
        q_group = rng.standard_normal((H, DH), dtype=np.float32)
        Kp = rng.standard_normal((H, pl, DH), dtype=np.float32).astype(np.float64)
        n_typ = pl + c.slens[r0] + 1
        q0 = rotate_bf16(bf16(q_group), cos[lens[r0]], sin[lens[r0]]).astype(np.float64)
        qh0 = q0 / (q0 * q0).sum(-1, keepdims=True)

        def set_score(K, cols, target, q, qh):
            cols = np.asarray(cols, dtype=np.int64)
            if cols.size:
                dot = np.einsum("hcd,hd->hc", K[:, cols], q)
                K[:, cols] += (target / SCALE - dot)[..., None] * qh[:, None, :]
        if family == "diffuse":
            Vp = rng.standard_normal((H, pl, DH), dtype=np.float32) * np.float32(np.sqrt(n_typ))
        else:
            sp = _sentinel_cols(pl, keep)
            n_sent = len(sp) + 2
            level = np.log(33.0 * n_typ / n_sent)
            Vp = rng.standard_normal((H, pl, DH), dtype=np.float32) * np.float32(np.sqrt(n_sent) / 2)
            set_score(Kp, sp, level, q0, qh0)
            hidden = np.flatnonzero(~keep)
            set_score(Kp, hidden, level + MASKED_SCORE_LIFT, q0, qh0)
            Vp[:, hidden] = MASKED_V
        kp[b, :, :pl] = torch.from_numpy(Kp.astype(np.float32)).to(torch.bfloat16)
        vp[b, :, :pl] = torch.from_numpy(np.ascontiguousarray(Vp, dtype=np.float32)).to(torch.bfloat16)
        for r in range(r0, r0 + c.N):
            sl, ln = c.slens[r], lens[r]
            n = pl + sl + 1
            q_raw = bf16(q_group + 0.25 * rng.standard_normal((H, DH), dtype=np.float32))
            q = rotate_bf16(q_raw, cos[ln], sin[ln]).astype(np.float64)
            qh = q / (q * q).sum(-1, keepdims=True)
            Ks = rng.standard_normal((H, sl + 1, DH), dtype=np.float32).astype(np.float64)          # row sl: the new token's ROTATED k
            if family == "diffuse":
                Vs = rng.standard_normal((H, sl + 1, DH), dtype=np.float32) * np.float32(np.sqrt(n))
                set_score(Ks, [sl], 3.5, q, qh)                    # the new token is felt whatever the draw
            else:
                ss = sorted({0, sl - 1, sl} & set(range(sl + 1)))
                n_sent = len(_sentinel_cols(pl, keep)) + len(ss)
                level = np.log(33.0 * n / n_sent)
                Vs = rng.standard_normal((H, sl + 1, DH), dtype=np.float32) * np.float32(np.sqrt(n_sent) / 2)
                set_score(Ks, ss, level, q, qh)
            k_raw = bf16(_unrotate(Ks[:, sl], cos[ln].astype(np.float64), sin[ln].astype(np.float64)))
            qkv[r, 0], qkv[r, 1], qkv[r, 2] = q_raw, k_raw, bf16(Vs[:, sl])
            ks[r, :, :sl] = torch.from_numpy(Ks[:, :sl].astype(np.float32)).to(torch.bfloat16)
            vs[r, :, :sl] = torch.from_numpy(np.ascontiguousarray(Vs[:, :sl], dtype=np.float32)).to(torch.bfloat16)
    stale_k = bf16(rng.standard_normal((c.rows, H, DH), dtype=np.float32))
    stale_v = bf16(rng.standard_normal((c.rows, H, DH), dtype=np.float32) * 4)
    return Inputs(c, family, torch.from_numpy(qkv.reshape(c.rows, 3 * H * DH)).to(torch.bfloat16), kp, vp, ks, vs, cos, sin, stale_k, stale_v)


MUTATIONS = ("drop_prefix_tile", "drop_prefix_item", "next_sample_prefix", "next_row_suffix", "suffix_one_short", "rope_at_suffix_position",
             "merge_without_rescaling", "rows_past_16_dropped", "stale_k", "stale_v")


def applies(case: Case, mut: str, r: int) -> bool:
    b, j = divmod(r, case.N)
    if mut in ("drop_prefix_tile", "drop_prefix_item"):
        return bool(case.keep(b).any())
    if mut == "next_sample_prefix":
        return case.B0 > 1
    if mut == "next_row_suffix":
        return j + 1 < case.N and case.slens[r] > 0 and case.slens[r + 1] >= case.slens[r]
    if mut == "merge_without_rescaling":
        return bool(case.keep(b).any())
    if mut == "rows_past_16_dropped":
        return j >= 16
    return True


def reference_row(inp: Inputs, r: int, mut: str = "") -> np.ndarray:
    """float64 output [H, 96] of row r; `mut` names one deliberate error of the kernel (MUTATIONS)."""
    c = inp.case
    b, j = divmod(r, c.N)
    H, pl, sl = c.H, c.plens[b], c.slens[r]
    ln = pl + sl
    x = inp.qkv[r].float().numpy().reshape(3, H, DH)
    pos = sl if mut == "rope_at_suffix_position" else ln
    q = rotate_bf16(x[0], inp.cos[pos], inp.sin[pos]).astype(np.float64)
    k_new = rotate_bf16(x[1], inp.cos[pos], inp.sin[pos]).astype(np.float64)
    v_new = x[2].astype(np.float64)
    if mut == "stale_k":
        k_new = inp.stale_k[r].astype(np.float64)
    if mut == "stale_v":
        v_new = inp.stale_v[r].astype(np.float64)
    bp = (b + 1) % c.B0 if mut == "next_sample_prefix" else b
    plp = min(pl, c.plens[bp])
    keep = c.keep(bp)[:plp].copy()
    Tp = plan(c.B0, c.N, c.H, c.pcap, c.scap)[1]
    if mut == "drop_prefix_tile":
        t = int(np.flatnonzero(keep)[-1]) // 64           # the last tile that holds a visible key
        keep[64 * t:64 * t + 64] = False
    if mut == "drop_prefix_item":
        t = int(np.flatnonzero(keep)[0]) // (64 * Tp)     # the first item that holds a visible key
        keep[64 * Tp * t:64 * Tp * (t + 1)] = False
    Kp = inp.kp[bp, :, :plp].double().numpy()[:, keep]
    Vp = inp.vp[bp, :, :plp].double().numpy()[:, keep]
    rs = r + 1 if mut == "next_row_suffix" else r
    Ks = np.concatenate([inp.ks[rs, :, :sl].double().numpy(), k_new[:, None]], 1)
    Vs = np.concatenate([inp.vs[rs, :, :sl].double().numpy(), v_new[:, None]], 1)
    if mut == "suffix_one_short":
        Ks, Vs = Ks[:, :-1], Vs[:, :-1]
    if mut == "rows_past_16_dropped":
        return np.zeros((H, DH))

    def part(K, V):
        if K.shape[1] == 0:
            return np.full((H,), -np.inf), np.zeros((H,)), np.zeros((H, DH))
        s = np.einsum("hnd,hd->hn", K, q) * SCALE
        m = s.max(1)
        w = np.exp(s - m[:, None])
        return m, w.sum(1), np.einsum("hn,hnd->hd", w, V)
    mp, lp, ap = part(Kp, Vp)
    ms, ls_, as_ = part(Ks, Vs)
    if mut == "merge_without_rescaling":
        L = lp + ls_
        return (ap + as_) / np.where(L > 0, L, 1)[:, None]
    M = np.maximum(mp, ms)
    Mf = np.where(np.isfinite(M), M, 0.0)
    fp, fs = np.exp(mp - Mf), np.exp(ms - Mf)
    L = lp * fp + ls_ * fs
    return (ap * fp[:, None] + as_ * fs[:, None]) / np.where(L > 0, L, 1)[:, None]


def reference(inp: Inputs) -> np.ndarray:
    return np.stack([reference_row(inp, r) for r in range(inp.case.rows)])


def appended_rows(inp: Inputs):
    """bf16 rows the kernel must append at suffix row slens[r]: the rotated k and the v of the new token, [rows, H, 96] each."""
    c = inp.case
    x = inp.qkv.float().numpy().reshape(c.rows, 3, c.H, DH)
    lens = c.lens()
    k = np.stack([rotate_bf16(x[r, 1], inp.cos[lens[r]], inp.sin[lens[r]]) for r in range(c.rows)])
    return k, x[:, 2]


def mutation_ratio(inp: Inputs, mut: str, rows=None) -> float:
    """Largest |mutated - reference| / tolerance over the rows the mutation applies to (0 where it applies to none)."""
    best = 0.0
    for r in (range(inp.case.rows) if rows is None else rows):
        if not applies(inp.case, mut, r):
            continue
        ref = reference_row(inp, r)
        best = max(best, float((np.abs(reference_row(inp, r, mut) - ref) / tolerance(ref, 2.0)).max()))
    return best
