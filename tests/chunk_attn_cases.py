"""Case table, inputs, float64 reference and reference mutations of the chunk attention kernels (aki_amd/csrc/chunk_attn.hip:
chunk_rope_append_kernel + chunk_attn_kernel): T new tokens per sample appended to a KV cache and attended in one pass.

numpy and CPU torch only.  tests/test_chunk_attn_cases_cpu.py checks the table itself - every corner is reached, every mutation of the
reference moves an element of a row it applies to by at least MIN_RATIO tolerances in some case - and tests/test_chunk_attn_gpu.py
runs every case on the device.

Two input families, as for the decode kernels (decode_attn_cases.py) and for the same reason - with unit-variance V the output of n
keys is ~ n^-1/2, below the absolute term of the bf16 bar, and a kernel that drops a tile passes:
  diffuse   q, K ~ N(0, 1), V ~ N(0, 1) sqrt(n): every key carries about the same small weight and |o| ~ 1 - a missing tile, a wrong
            merge weight, another sample's cache show;
  self      every chunk token's own key gets the score ln(visible keys) + 1/2 against its own query, i.e. about half of the row's
            mass: a token that does not see itself, sees a stale row in its place or its successor's shows.  Masked cache columns are
            adversarial: V = 50 and, against the PROBE rows of the chunk (first, last, the rows around a query-block edge), the score
            of the row's own key + 4, finite as the product's padded columns are - one leaked column dominates a probe row.
Everything is rounded to bf16 before the reference is computed.  Unused cache rows - the rows the chunk will fill included - and the
qkv rows of padded tokens (t >= n_new[b]) hold NaN."""
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import aki_oracle as O
from decode_attn_cases import DH, SCALE, FAMILIES as _DECODE_FAMILIES, MIN_RATIO, MASKED_V, MASKED_SCORE_LIFT, bf16, rotate_bf16, _unrotate, tolerance

FAMILIES = (_DECODE_FAMILIES[0], "self")
assert FAMILIES[0] == "diffuse"
NW = 4                      # waves of chunk_attn_kernel: wave w walks the 64-key tiles j = w (mod 4) and the four partials are merged


@dataclass(frozen=True)
class Case:
    id: str
    B: int
    H: int
    cap: int
    lens: tuple                 # cache_len[b]
    T: int                      # rows of the chunk per sample (the padded width)
    n_new: tuple                # real tokens per sample, <= T
    masks: tuple                # per sample: ((lo, hi), ...) masked cache columns [lo, hi)
    nwords: int                 # 64-bit words of col_valid_bits per sample (0: none passed); columns past them count as valid
    why: str = ""

    @property
    def ragged(self):
        return any(n != self.T for n in self.n_new)

    def keep(self, b: int) -> np.ndarray:
        k = np.ones(self.cap, dtype=bool)
        for lo, hi in self.masks[b]:
            k[lo:hi] = False
        return k

    def bits(self) -> Optional[np.ndarray]:
        if self.nwords == 0:
            return None
        pad = np.ones((self.B, self.nwords * 64), dtype=bool)
        for b in range(self.B):
            for lo, hi in self.masks[b]:
                pad[b, lo:hi] = False
        return np.packbits(pad.reshape(self.B, self.nwords, 64), axis=-1, bitorder="little").view(np.uint64).reshape(
            self.B, self.nwords).view(np.int64).copy()

    def holes(self, b: int):
        """Masked ranges of sample b clipped to its cached keys."""
        return [(lo, min(hi, self.lens[b])) for lo, hi in self.masks[b] if lo < self.lens[b]]

    def probes(self, b: int) -> list:
        """Chunk rows of sample b against which the masked columns carry the adversarial score."""
        nn = self.n_new[b]
        return sorted({t for t in (0, 1, 31, 32, nn // 2, nn - 1) if 0 <= t < nn})


_N = ()


def _case(id, B, H, cap, lens, T, n_new=None, masks=None, nwords=None, why=""):
    n_new = tuple(n_new) if n_new is not None else (T,) * B
    masks = tuple(tuple(m) for m in (masks if masks is not None else [_N] * B))
    nwords = (cap + 63) // 64 if nwords is None else nwords
    c = Case(id, B, H, cap, tuple(lens), T, n_new, masks, nwords, why)
    assert len(c.lens) == B and len(c.masks) == B and len(c.n_new) == B, id
    assert all(0 <= n <= T and ln >= 0 and ln + n <= cap for ln, n in zip(c.lens, c.n_new)), f"{id}: the chunk does not fit"
    assert all(0 <= lo < hi <= c.lens[b] for b, m in enumerate(masks) for lo, hi in m), f"{id}: a masked range lies past the cached keys"
    return c


CASES = (
    _case("b1-h2-cap64-len0-T1", 1, 2, 64, [0], 1, nwords=0, why="empty cache, one token: the token alone, no mask words"),
    _case("b1-h2-cap64-len0-T33", 1, 2, 64, [0], 33, why="empty cache: a plain causal prefill that crosses a query block"),
    _case("b2-h2-cap128-lens1-63-T31-nnew31-2-holes", 2, 2, 128, [1, 63], 31, [31, 2], [_N, [(3, 7), (20, 21)]],
          why="ragged chunk; holes in the valid bits; the short sample's keys end inside the first tile + 1"),
    _case("b2-h2-cap192-lens64-65-T32", 2, 2, 192, [64, 65], 32, masks=[[(0, 1)], [(60, 64)]], nwords=1,
          why="one full query block behind a whole tile / a tile + 1; mask words cover only the first tile"),
    _case("b1-h2-cap256-len100-T65", 1, 2, 256, [100], 65, masks=[[(40, 50)]], why="three query blocks; the chunk crosses key 128"),
    _case("b1-h2-cap128-len3-T64", 1, 2, 128, [3], 64, why="two full query blocks, the second one's keys cross a tile"),
    _case("b2-h4-cap128-lens40-30-T16-nnew16-0-prefix-masked", 2, 4, 128, [40, 30], 16, [16, 0], [[(0, 40)], _N],
          why="sample 0's prefix fully masked: a tile of the walk holds the chunk alone; sample 1 brings nothing and gets zeros"),
    _case("b1-h2-cap704-len655-T49", 1, 2, 704, [655], 49, masks=[[(100, 170)]], why="the headline length; fills to cap - 1"),
    _case("b1-h32-cap4224-len4096-T128", 1, 32, 4224, [4096], 128, masks=[[(1000, 1030)]], why="flagship: full width, four query blocks, 66 tiles"),
)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
LARGEST = "b1-h32-cap4224-len4096-T128"


def properties(case: Case) -> set:
    P = set()
    for n in {case.T, *case.n_new}:
        if n in (1, 2, 31, 32, 33, 64, 65):
            P.add(f"T={n}")
    for ln in case.lens:
        if ln in (0, 1, 63, 64, 65, 655, 4096):
            P.add(f"len={ln}")
    if case.ragged:
        P.add("ragged-n_new")
    if 0 in case.n_new:
        P.add("n_new=0")
    for b in range(case.B):
        if case.lens[b] > 0 and case.n_new[b] > 0 and not case.keep(b)[:case.lens[b]].any():
            P.add("prefix-fully-masked")
        if case.n_new[b] > 0 and case.lens[b] + case.n_new[b] - 1 == case.cap - 1:
            P.add("last-row=cap-1")
        if case.holes(b):
            P.add("mask:holes")
    if case.nwords == 0:
        P.add("mask:no-words")
    if 0 < case.nwords * 64 < max(case.lens):
        P.add("mask:nwords-short-of-len")
    if (case.T + 31) // 32 >= 3:
        P.add("query-blocks>=3")
    P.add("H=32" if case.H == 32 else "small-H")
    return P


REQUIRED = ("T=1", "T=2", "T=31", "T=32", "T=33", "T=64", "T=65", "len=0", "len=1", "len=63", "len=64", "len=65", "len=655", "len=4096",
            "ragged-n_new", "n_new=0", "prefix-fully-masked", "last-row=cap-1", "H=32", "small-H", "mask:holes", "mask:no-words",
            "mask:nwords-short-of-len", "query-blocks>=3")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Inputs:
    case: Case
    family: str
    qkv: torch.Tensor            # bf16 [B * T, 3 * H * 96]: un-rotated q | k | v, row b * T + t; NaN for t >= n_new[b]
    k: torch.Tensor              # bf16 [B, H, cap, 96]: rows < lens[b] cached, NaN from lens[b] on
    v: torch.Tensor
    cos: np.ndarray              # f32 [cap, 96]
    sin: np.ndarray
    stale_k: np.ndarray          # f32 [B, H, T, 96]: finite stand-ins for stale cache rows at the append positions
    stale_v: np.ndarray


def visible(case: Case, b: int) -> np.ndarray:
    """bool [n_new, cache_len + n_new]: what query t of sample b sees."""
    ln, nn = case.lens[b], case.n_new[b]
    m = np.zeros((nn, ln + nn), dtype=bool)
    m[:, :ln] = case.keep(b)[:ln][None, :]
    m[:, ln:] = np.tril(np.ones((nn, nn), dtype=bool))
    return m


def make_inputs(case: Case, family: str) -> Inputs:
    assert family in FAMILIES
    B, H, cap, T = case.B, case.H, case.cap, case.T
    rng = np.random.default_rng(zlib.crc32(f"{case.id}/{family}".encode()))
    cos, sin = (a[0] for a in O.rope_cos_sin(np.arange(cap)[None], DH))
    k = torch.full((B, H, cap, DH), float("nan"), dtype=torch.bfloat16)
    v = torch.full((B, H, cap, DH), float("nan"), dtype=torch.bfloat16)
    qkv = np.full((B, T, 3, H, DH), np.nan, dtype=np.float32)
    for b, (ln, nn) in enumerate(zip(case.lens, case.n_new)):
        n = ln + nn
        if n == 0:
            continue
        pos = np.arange(ln, ln + nn)
        K = rng.standard_normal((H, n, DH), dtype=np.float32).astype(np.float64)         # chunk rows: the ROTATED k, for now
        if nn:
            q_raw = bf16(rng.standard_normal((nn, H, DH), dtype=np.float32))
            Q = rotate_bf16(q_raw, cos[pos][:, None, :], sin[pos][:, None, :]).astype(np.float64).transpose(1, 0, 2)     # [H, nn, 96]
        if family == "diffuse":
            V = rng.standard_normal((H, n, DH), dtype=np.float32).astype(np.float64) * np.sqrt(n)
        else:
            V = rng.standard_normal((H, n, DH), dtype=np.float32).astype(np.float64)
            if nn:
                vis = visible(case, b)
                level = np.log(vis.sum(1)) + 0.5                                          # [nn]: the own key's score
                qh = Q / (Q * Q).sum(-1, keepdims=True)
                dot = np.einsum("htd,htd->ht", K[:, ln:], Q)
                K[:, ln:] += (level[None, :] / SCALE - dot)[..., None] * qh
                hidden = np.flatnonzero(~case.keep(b)[:ln])
                if hidden.size:
                    pr = case.probes(b)
                    for h in range(H):                                                    # minimum-norm key with the wanted scores on the probe rows
                        K[h, hidden] = (np.linalg.pinv(Q[h, pr]) @ ((level[pr] + MASKED_SCORE_LIFT) / SCALE))[None, :]
                    V[:, hidden] = MASKED_V
        if nn:
            c, s = cos[pos].astype(np.float64)[None], sin[pos].astype(np.float64)[None]
            qkv[b, :nn, 0] = q_raw
            qkv[b, :nn, 1] = bf16(_unrotate(K[:, ln:], c, s)).transpose(1, 0, 2)
            qkv[b, :nn, 2] = bf16(V[:, ln:]).transpose(1, 0, 2)
        k[b, :, :ln] = torch.from_numpy(K[:, :ln].astype(np.float32)).to(torch.bfloat16)
        v[b, :, :ln] = torch.from_numpy(V[:, :ln].astype(np.float32)).to(torch.bfloat16)
    stale_k = bf16(rng.standard_normal((B, H, T, DH), dtype=np.float32))
    stale_v = bf16(rng.standard_normal((B, H, T, DH), dtype=np.float32))
    return Inputs(case, family, torch.from_numpy(qkv.reshape(B * T, 3 * H * DH)).to(torch.bfloat16), k, v, cos, sin, stale_k, stale_v)


# ---- reference ------------------------------------------------------------------------------------------------------------------
def sample_qkv(inp: Inputs, b: int, rope_at_chunk_index: bool = False, stale: str = "", cache_of: Optional[int] = None):
    """float64 Q [H, nn, 96], K, V [H, ln + nn, 96] of sample b as the kernels hold them after the append: RoPE in f32 rounded to bf16."""
    case = inp.case
    H, T, ln, nn = case.H, case.T, case.lens[b], case.n_new[b]
    raw = inp.qkv.float().numpy().reshape(case.B, T, 3, H, DH)[b, :nn]
    pos = np.arange(nn) if rope_at_chunk_index else np.arange(ln, ln + nn)
    c, s = inp.cos[pos][:, None, :], inp.sin[pos][:, None, :]
    Q = rotate_bf16(raw[:, 0], c, s).astype(np.float64).transpose(1, 0, 2)
    K = np.empty((H, ln + nn, DH), dtype=np.float64)
    V = np.empty((H, ln + nn, DH), dtype=np.float64)
    src = b if cache_of is None else cache_of
    K[:, :ln] = np.nan_to_num(inp.k[src, :, :ln].double().numpy(), nan=0.0)      # another sample's slab may be shorter: zeros there
    V[:, :ln] = np.nan_to_num(inp.v[src, :, :ln].double().numpy(), nan=0.0)
    K[:, ln:] = inp.stale_k[b, :, :nn] if stale == "k" else rotate_bf16(raw[:, 1], c, s).transpose(1, 0, 2)
    V[:, ln:] = inp.stale_v[b, :, :nn] if stale == "v" else raw[:, 2].transpose(1, 0, 2)
    return Q, K, V


def attend(Q, K, V, vis) -> np.ndarray:
    """Masked softmax(Q K^T scale) V in float64 -> [nn, H, 96]; a row with no visible key gives zeros."""
    S = np.where(vis[None], np.einsum("htd,hnd->htn", Q, K) * SCALE, -np.inf)
    m = S.max(-1, keepdims=True)
    W = np.where(vis[None], np.exp(S - np.where(np.isfinite(m), m, 0.0)), 0.0)
    L = W.sum(-1, keepdims=True)
    out = np.einsum("htn,hnd->htd", W, V) / np.where(L > 0, L, 1.0)
    return np.where(L > 0, out, 0.0).transpose(1, 0, 2)


def reference(inp: Inputs) -> np.ndarray:
    """float64 [B, T, H * 96]; rows t >= n_new[b] are zeros - what the kernel writes there."""
    case = inp.case
    out = np.zeros((case.B, case.T, case.H * DH))
    for b in range(case.B):
        if case.n_new[b]:
            out[b, :case.n_new[b]] = attend(*sample_qkv(inp, b), visible(case, b)).reshape(case.n_new[b], -1)
    return out


def dense_reference(inp: Inputs, b: int) -> np.ndarray:
    """The same numbers by the textbook route: an explicit [T, n] additive mask and a softmax over full rows, head by head."""
    case = inp.case
    Q, K, V = sample_qkv(inp, b)
    ln, nn = case.lens[b], case.n_new[b]
    mask = np.full((nn, ln + nn), -np.inf)
    for t in range(nn):
        for j in range(ln + nn):
            if (j < ln and case.keep(b)[j]) or (j >= ln and j - ln <= t):
                mask[t, j] = 0.0
    out = np.empty((nn, case.H, DH))
    for h in range(case.H):
        S = Q[h] @ K[h].T * SCALE + mask
        P = np.exp(S - S.max(1, keepdims=True))
        out[:, h] = (P / P.sum(1, keepdims=True)) @ V[h]
    return out.reshape(nn, -1)


def appended_rows(inp: Inputs, b: int):
    """(k rows rotated to bf16, v rows) of sample b's real tokens, f32 [H, n_new, 96] each: what the cache must hold bit for bit."""
    case = inp.case
    ln, nn = case.lens[b], case.n_new[b]
    raw = inp.qkv.float().numpy().reshape(case.B, case.T, 3, case.H, DH)[b, :nn]
    pos = np.arange(ln, ln + nn)
    return rotate_bf16(raw[:, 1], inp.cos[pos][:, None, :], inp.sin[pos][:, None, :]).transpose(1, 0, 2), raw[:, 2].transpose(1, 0, 2)


# ---- mutations of the reference ---------------------------------------------------------------------------------------------------
# name -> f(inp, b) -> [(label, out [nn, H * 96], rows it applies to (bool [nn]))].  The rule by which a row counts is written in each.
def _rows(case, b):
    return np.ones(case.n_new[b], dtype=bool)


def m_causal_one_short(inp, b):
    case = inp.case
    vis = visible(case, b)
    ln, nn = case.lens[b], case.n_new[b]
    vis[np.arange(nn), ln + np.arange(nn)] = False
    return [("a token does not see itself", attend(*sample_qkv(inp, b), vis).reshape(nn, -1), _rows(case, b))]      # rule: every row


def m_sees_next(inp, b):
    case = inp.case
    vis = visible(case, b)
    ln, nn = case.lens[b], case.n_new[b]
    if nn < 2:
        return []
    vis[np.arange(nn - 1), ln + 1 + np.arange(nn - 1)] = True
    return [("token t sees t + 1", attend(*sample_qkv(inp, b), vis).reshape(nn, -1), np.arange(nn) < nn - 1)]      # rule: a successor exists


def m_rope_at_chunk_index(inp, b):
    case = inp.case
    ln, nn = case.lens[b], case.n_new[b]
    if ln == 0 or not case.keep(b)[:ln].any():         # rule: a common rotation cancels among the chunk's keys; a cached key must be visible
        return []
    return [("RoPE at t", attend(*sample_qkv(inp, b, rope_at_chunk_index=True), visible(case, b)).reshape(nn, -1), _rows(case, b))]


def m_drop_cache_tile(inp, b):
    case = inp.case
    ln, nn = case.lens[b], case.n_new[b]
    vis = visible(case, b)
    qkv = sample_qkv(inp, b)
    res = []
    ntiles = (ln + nn + 63) // 64
    for g in sorted({0, (ln - 1) // 64 if ln else 0, ln // 64, ntiles - 1}):
        v2 = vis.copy()
        v2[:, 64 * g:64 * g + 64] = False
        hit = vis[:, 64 * g:64 * g + 64].sum(1) >= 8    # rule: the row sees at least eight keys of the tile and some key outside it
        rows = hit & v2.any(1)
        if rows.any():
            res.append((f"drop tile {g}", attend(*qkv, v2).reshape(nn, -1), rows))
    return res


def m_next_sample_cache(inp, b):
    case = inp.case
    ln, nn = case.lens[b], case.n_new[b]
    if case.B < 2 or ln == 0 or not case.keep(b)[:ln].any():        # rule: another sample exists and a cached key is visible
        return []
    return [("the next sample's cache slab", attend(*sample_qkv(inp, b, cache_of=(b + 1) % case.B), visible(case, b)).reshape(nn, -1), _rows(case, b))]


def m_unmask_hole_edge(inp, b):
    case = inp.case
    nn = case.n_new[b]
    qkv = sample_qkv(inp, b)
    rows = np.zeros(nn, dtype=bool)
    rows[case.probes(b)] = True                          # rule: the probe rows carry the adversarial score
    res = []
    for c in sorted({c for lo, hi in case.holes(b) for c in (lo, hi - 1)}):
        vis = visible(case, b)
        vis[:, c] = True
        res.append((f"unmask column {c}", attend(*qkv, vis).reshape(nn, -1), rows))
    return res


def m_stale_chunk_k(inp, b):
    case = inp.case
    nn = case.n_new[b]
    rows = visible(case, b).sum(1) >= 2                  # rule: with one visible key its score cancels in the softmax
    return [("chunk k from stale rows", attend(*sample_qkv(inp, b, stale="k"), visible(case, b)).reshape(nn, -1), rows)] if rows.any() else []


def m_stale_chunk_v(inp, b):
    case = inp.case
    nn = case.n_new[b]
    return [("chunk v from stale rows", attend(*sample_qkv(inp, b, stale="v"), visible(case, b)).reshape(nn, -1), _rows(case, b))]


def m_merge_without_rescaling(inp, b):
    """The four wave partials of the kernel (wave w: tiles j = w mod 4 of the block's walk, each relative to its OWN maximum) summed at
    weight 1 instead of exp2(m_w - M)."""
    case = inp.case
    ln, nn = case.lens[b], case.n_new[b]
    Q, K, V = sample_qkv(inp, b)
    vis = visible(case, b)
    n = ln + nn
    S = np.where(vis[None], np.einsum("htd,hnd->htn", Q, K) * SCALE, -np.inf)        # [H, nn, n]
    wave_of = (np.arange(n) // 64) % NW
    A = np.zeros((case.H, nn, DH))
    Ls = np.zeros((case.H, nn, 1))
    live = np.zeros((nn,), dtype=int)
    for w in range(NW):
        cols = wave_of == w
        if not cols.any():
            continue
        Sw = S[:, :, cols]
        m = Sw.max(-1, keepdims=True)
        Ww = np.where(np.isfinite(Sw), np.exp(Sw - np.where(np.isfinite(m), m, 0.0)), 0.0)
        A += np.einsum("htn,hnd->htd", Ww, V[:, cols])
        Ls += Ww.sum(-1, keepdims=True)
        live += vis[:, cols].any(1)
    rows = live >= 2                                      # rule: two partials of the row hold a visible key
    return [("partials merged at weight 1", (A / np.where(Ls > 0, Ls, 1.0)).transpose(1, 0, 2).reshape(nn, -1), rows)] if rows.any() else []


def m_block_rows_swapped(inp, b):
    case = inp.case
    nn = case.n_new[b]
    if nn <= 32:
        return []
    ref = attend(*sample_qkv(inp, b), visible(case, b)).reshape(nn, -1)
    out = ref.copy()
    t = np.arange(nn - 32)
    out[t], out[t + 32] = ref[t + 32], ref[t]
    rows = np.zeros(nn, dtype=bool)
    rows[t] = rows[t + 32] = True                         # rule: the partner row exists
    return [("rows t and t + 32 exchanged", out, rows)]


MUTATIONS = {
    "causal_one_short": m_causal_one_short,
    "sees_next": m_sees_next,
    "rope_at_chunk_index": m_rope_at_chunk_index,
    "drop_cache_tile": m_drop_cache_tile,
    "next_sample_cache": m_next_sample_cache,
    "unmask_hole_edge": m_unmask_hole_edge,
    "stale_chunk_k": m_stale_chunk_k,
    "stale_chunk_v": m_stale_chunk_v,
    "merge_without_rescaling": m_merge_without_rescaling,
    "block_rows_swapped": m_block_rows_swapped,
}


def applies(case: Case, mut: str, row: tuple, inp: Optional[Inputs] = None) -> bool:
    """Does mutation `mut` apply to row (b, t) of the case?  (By the rule written in the mutation; the inputs' values play no part.)"""
    b, t = row
    if t >= case.n_new[b]:
        return False
    inp = inp or make_inputs(case, "diffuse")
    return any(bool(rows[t]) for _, _, rows in MUTATIONS[mut](inp, b))


def mutation_ratios(inp: Inputs) -> dict:
    """{mutation: worst |mutated - reference| / tolerance over the rows it applies to, best variant} ({} entries for mutations that apply nowhere)."""
    case = inp.case
    res = {}
    for b in range(case.B):
        nn = case.n_new[b]
        if nn == 0:
            continue
        ref = attend(*sample_qkv(inp, b), visible(case, b)).reshape(nn, -1)
        tol = np.stack([tolerance(ref[t], 2.0) for t in range(nn)])
        for name, f in MUTATIONS.items():
            for label, out, rows in f(inp, b):
                r = float((np.abs(out - ref) / tol)[rows].max())
                res[name] = max(res.get(name, 0.0), r)
    return res
