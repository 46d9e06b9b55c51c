"""Case table, inputs, float64 reference and reference mutations of the single-query (decode) attention kernels
(aki_amd/csrc/decode.hip: decode_attn_split_kernel<false / true>, decode_attn_split_fp8kv_kernel, decode_attn_kernel<float, 96>).

numpy and CPU torch only.  tests/test_decode_attn_cases_cpu.py checks the table itself - every corner of the launch plan is reached,
and every mutation of the reference moves an output element by at least 8x the tolerance - and tests/test_decode_attn_gpu.py runs
every case on the device.

Why two input families.  With q, K, V ~ N(0, 1) and n keys the output is an average of about n unit vectors, |o| ~ n^-1/2, far below
the absolute term of the bf16 bar (2e-3 max(1, max|ref|) + 2^-8 |ref|): at 655 keys a kernel that never attends to the token it has
just appended passes.  So every case is run on
  diffuse   q, K ~ N(0, 1), V ~ N(0, 1) sqrt(n_b): every key carries about the same small weight and |o| ~ 1 - a missing tile, a
            missing item or a wrong merge weight shows (one key per item is lifted to a known maximum, see make_inputs);
  sentinel  a short list of keys per sample (the appended token, its predecessor, key 0, both neighbours of every hole, the last key
            of a tile and the first of the next at every item edge and at further tile edges up to six) gets the common score
            b = ln(33 n / |sentinels|): the other keys weigh about e^0.5 each, so the sentinels share ~95 % of the mass about equally
            and a single missing key shows.  V ~ N(0, 1) sqrt(|sentinels|) / 2 keeps |o| ~ 1 (an average of |sentinels| rows) whatever
            the length of the list.  Masked columns are adversarial: score b + 4 and V = 50, finite as the product's padded columns
            are, so one leaked column dominates the output.
Everything is rounded to bf16 before anything is computed.
"""
import os
import re
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import aki_oracle as O

DH = 96
SCALE = DH ** -0.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("diffuse", "sentinel")
VIEWS = ("bf16", "fp8")          # what the keys are attended through: the bf16 rows, or their e4m3 copies (ref_quant)
MASKED_V = 50.0
MASKED_SCORE_LIFT = 4.0
MIN_RATIO = 8.0
PEAKS = (4.2, 3.5)               # diffuse family: the largest score of even / odd items


def dec_items() -> int:
    """AKI_DEC_ITEMS as the library is compiled: a retune moves the plan of every case with it."""
    with open(os.path.join(ROOT, "aki_amd", "csrc", "aki_device.h")) as f:
        m = re.search(r"^#define\s+AKI_DEC_ITEMS\s+(\d+)", f.read(), re.M)
    assert m, "AKI_DEC_ITEMS not found in aki_device.h"
    return int(m.group(1))


def plan(B: int, H: int, cap: int, max_keys: int):
    """(S, T) of decode_attn_split_launch: T 64-key tiles per item from the cache capacity, S items per head from max_keys."""
    if max_keys <= 0 or max_keys > cap:
        max_keys = cap
    tiles, tiles_cap = (max_keys + 63) // 64, (cap + 63) // 64
    items = dec_items()
    T = max(1, (B * H * tiles_cap + items - 1) // items)
    return (tiles + T - 1) // T, T


def workspace_bytes_needed(B: int, H: int, S: int) -> int:
    """What decode_attn_split_launch asks of the workspace: the arrival counters (256-byte granules) + S partials of 104 floats per row."""
    return (B * H * 4 + 255) // 256 * 256 + B * H * S * 104 * 4


@dataclass(frozen=True)
class Case:
    id: str
    B: int
    H: int
    cap: int
    lens: tuple                 # cache_len[b]: keys cached before the step = position and append index of the new token
    masks: tuple                # per sample: ((lo, hi), ...) masked column ranges [lo, hi)
    nwords: int                 # 64-bit words of col_valid_bits per sample (0: no bits passed); columns past them count as valid
    why: str = ""

    @property
    def T(self):
        return plan(self.B, self.H, self.cap, 0)[1]

    def max_keys_options(self):
        return (max(self.lens) + 1, 0)          # an eager step, and a captured one (whole capacity)

    def keep(self, b: int) -> np.ndarray:
        """Visibility of the cache columns of sample b as the kernels read it."""
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
        """Masked ranges of sample b clipped to the keys the step attends to."""
        n = self.lens[b] + 1
        return [(lo, min(hi, n)) for lo, hi in self.masks[b] if lo < n]


_N = ()          # no masked range


def _case(id, B, H, cap, lens, masks=None, nwords=None, why=""):
    masks = tuple(tuple(m) for m in (masks if masks is not None else [_N] * B))
    nwords = (cap + 63) // 64 if nwords is None else nwords
    c = Case(id, B, H, cap, tuple(lens), masks, nwords, why)
    assert len(c.lens) == B and len(c.masks) == B and all(0 <= ln < cap for ln in c.lens), id
    assert all(0 <= lo < hi <= nwords * 64 for m in masks for lo, hi in m), f"{id}: a masked range lies past the mask words"
    for b, ln in enumerate(c.lens):             # the new position is masked only in the row that sees nothing at all
        assert c.keep(b)[ln] or not c.keep(b)[:ln + 1].any(), f"{id}: sample {b} masks its new token"
    return c


# The plan arithmetic below is written for AKI_DEC_ITEMS = 2048; test_decode_attn_cases_cpu.py asserts the coverage from plan(), so
# a retune that moves a case off its corner fails there and the table is re-aimed.
CASES = (
    _case("b1-h32-cap64-T1-S1-len0", 1, 32, 64, [0], nwords=0, why="full width, one key: the appended token alone, no mask words"),
    _case("b3-h2-cap64-T1-S1-lens62-63-0-hole-in-word-leftpad1", 3, 2, 64, [62, 63, 0], [[(3, 7)], [(0, 1)], _N],
          why="S = 1 merge; ragged: one sample fills the cache (cap - 1), one is empty; token last in its tile"),
    _case("b4-h2-cap320-T1-S5-lens64-65-319-200-leftpad64-hole-across-word-whole-word", 4, 2, 320, [64, 65, 319, 200],
          [[(0, 64)], [(58, 65)], [(64, 128)], [(0, 64)]],
          why="five items = one merge pass exactly; token first in its tile and alone in its item behind a fully masked item"),
    _case("b3-h4-cap704-T1-S11-lens654-703-0-hole-across-words-all-before-masked", 3, 4, 704, [654, 703, 0],
          [[(100, 170)], [(0, 703)], _N],
          why="the headline length; eleven items = three merge passes; ten items of m = -inf ahead of the only live one"),
    _case("b2-h2-cap384-T1-S6-lens300-130-nwords2-short-of-lens", 2, 2, 384, [300, 130], [[(3, 7)], [(120, 128)]], nwords=2,
          why="six items = a second merge pass of one; mask words cover only the prompt, keys past them are valid"),
    _case("b2-h2-cap128-T1-S2-lens70-5-no-visible-key-all-before-masked", 2, 2, 128, [70, 5], [[(0, 71)], [(0, 5)]],
          why="a row with no visible key at all (the new position inside the mask words, bit clear) returns zeros"),
    _case("b16-h32-cap300-T2-S3-lens127-128-129-leftpad131-whole-item", 16, 32, 300,
          [127, 128, 129, 0, 299, 62, 63, 64, 65, 1, 2, 270, 200, 190, 130, 126],
          [_N, _N, _N, _N, [(0, 131)], [(3, 7)], _N, _N, [(58, 65)], _N, _N, [(128, 256)], [(64, 128)], _N, [(0, 1)], _N],
          why="full width at B = 16, two tiles per item: 64 T - 1, 64 T, 64 T + 1; left padding of 64 T + 3; a whole masked item"),
    _case("b8-h32-cap1100-T3-S6-lens191-192-193-leftpad195-whole-item", 8, 32, 1100, [0, 191, 192, 193, 64, 1000, 1099, 654],
          [_N, _N, [(0, 192)], _N, [(3, 7)], [(60, 70)], [(0, 195)], [(192, 384)]],
          why="full width at B = 8, three tiles per item: token in the first / middle / last tile; alone behind a masked item"),
    _case("b2-h2-cap4200-T1-S66-lens4095-4096-whole-word", 2, 2, 4200, [4095, 4096], [_N, [(2048, 2112)]],
          why="more than sixty items through the five-slot merge; 4096 puts the token alone in the last item"),
    _case("b1-h32-cap4160-T2-S33-len4100", 1, 32, 4160, [4100], [[(1000, 1030)]],
          why="one full-width sequence past 4096: two tiles per item"),
    _case("b1-h32-cap8300-T3-S44-len8250-leftpad195-hole-across-words", 1, 32, 8300, [8250], [[(0, 195), (4000, 4100)]],
          why="one full-width sequence past 8192: three tiles per item, the plan of a long-context chain step"),
)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def properties(case: Case) -> set:
    """The corners of section 1 of the issue that this case reaches, from plan() and the table."""
    P = set()
    S_full, T = plan(case.B, case.H, case.cap, 0)
    S_eager = plan(case.B, case.H, case.cap, max(case.lens) + 1)[0]
    P.add("T=1" if T == 1 else "T=2" if T == 2 else "T>=3")
    for S in (S_full, S_eager):
        if S in (1, 5, 6, 11):
            P.add(f"S={S}")
        if S > 60:
            P.add("S>60")
    if case.H == 32 and case.B in (1, 8, 16):
        P.add(f"H=32,B={case.B}")
    if case.H < 32:
        P.add("small-H")
    named = [(0, "len=0"), (62, "len=62"), (63, "len=63"), (64, "len=64"), (65, "len=65"), (654, "len=654"), (4095, "len=4095"),
             (4096, "len=4096"), (64 * T - 1, "len=64T-1"), (64 * T, "len=64T"), (64 * T + 1, "len=64T+1")]      # at T = 1 both names count
    if 0 in case.lens and case.cap - 1 in case.lens:
        P.add("ragged:empty+cap-1")
    if case.nwords == 0:
        P.add("mask:no-words")
    for b, ln in enumerate(case.lens):
        P.update(name for v, name in named if ln == v)
        if ln > 8192:
            P.add("len>8192")
        P.add({0: "token:first-in-tile", 63: "token:last-in-tile"}.get(ln % 64, "token:middle-in-tile"))
        tile_in_item, tiles_of_item = (ln // 64) % T, T
        if tile_in_item == 0:
            P.add("token:first-tile-of-item")
        if tile_in_item == tiles_of_item - 1:
            P.add("token:last-tile-of-item")
        if 0 < tile_in_item < tiles_of_item - 1:
            P.add("token:middle-tile-of-item")
        if ln % (64 * T) == 0:
            P.add("token:alone-in-item" if ln > 0 else "token:only-key")
        keep = case.keep(b)
        n = ln + 1
        if not case.masks[b]:
            P.add("mask:none")
        for lo, hi in case.masks[b]:
            if lo > 0 and lo // 64 == (hi - 1) // 64 and hi - lo < 64:
                P.add("mask:hole-in-word")
            if lo > 0 and lo // 64 != (hi - 1) // 64 and (lo % 64 or hi % 64):
                P.add("mask:hole-across-word")
            if lo > 0 and lo % 64 == 0 and hi - lo == 64:
                P.add("mask:whole-word")
            if lo % (64 * T) == 0 and hi - lo == 64 * T:
                P.add("mask:whole-item")
            if lo == 0 and hi < ln:
                P.add({1: "leftpad=1", 64: "leftpad=64", 64 * T + 3: "leftpad=64T+3"}.get(hi, "leftpad=other"))
            if lo == 0 and hi == ln and ln > 0:
                P.add("mask:all-before-token")
        if not keep[:n].any():
            P.add("mask:no-visible-key")
        if case.nwords and case.nwords * 64 <= ln:
            P.add("mask:nwords-short-of-len")
        first_live_item = next((s for s in range((n + 64 * T - 1) // (64 * T)) if keep[s * 64 * T:min(n, (s + 1) * 64 * T)].any()), None)
        if first_live_item:
            P.add("dead-items-ahead-of-live")
    return P


REQUIRED = ("T=1", "T=2", "T>=3", "S=1", "S=5", "S=6", "S=11", "S>60", "H=32,B=1", "H=32,B=8", "H=32,B=16", "small-H",
            "len=0", "len=62", "len=63", "len=64", "len=65", "len=64T-1", "len=64T", "len=64T+1", "len=654", "len=4095", "len=4096",
            "len>8192", "ragged:empty+cap-1",
            "token:first-in-tile", "token:middle-in-tile", "token:last-in-tile", "token:first-tile-of-item",
            "token:middle-tile-of-item", "token:last-tile-of-item", "token:alone-in-item", "token:only-key",
            "mask:none", "mask:no-words", "mask:hole-in-word", "mask:hole-across-word", "mask:whole-word", "mask:whole-item",
            "leftpad=1", "leftpad=64", "leftpad=64T+3", "mask:all-before-token", "mask:nwords-short-of-len", "mask:no-visible-key",
            "dead-items-ahead-of-live")


# ---- number formats -------------------------------------------------------------------------------------------------------------
def bf16(x) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def ref_quant(x: torch.Tensor):
    """The documented e4m3 rule in f32 on the host: s = max(amax, 1e-12) / 448 per row of 96, bytes = e4m3(x / s), RNE, saturating."""
    x = x.detach().float().cpu()
    s = x.abs().amax(-1).clamp(min=1e-12) / 448.0
    q = (x / s[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s


def deq(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).float() * s.float()[..., None]


def through_e4m3(x: np.ndarray) -> np.ndarray:
    return deq(*ref_quant(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))).numpy()


def rotate_bf16(x: np.ndarray, c: np.ndarray, s: np.ndarray) -> np.ndarray:
    """RoPE rotate-half in f32 as the kernels do it (two products, one add), then rounded to bf16 - the kernels' rounding point."""
    x, c, s = (np.asarray(a, dtype=np.float32) for a in (x, c, s))
    h = x.shape[-1] // 2
    lo = x[..., :h] * c[..., :h] - x[..., h:] * s[..., :h]
    hi = x[..., h:] * c[..., h:] + x[..., :h] * s[..., h:]
    return bf16(np.concatenate([lo, hi], -1))


def rotate_f64(x, c, s) -> np.ndarray:
    x, c, s = (np.asarray(a, dtype=np.float64) for a in (x, c, s))
    h = x.shape[-1] // 2
    return np.concatenate([x[..., :h] * c[..., :h] - x[..., h:] * s[..., :h], x[..., h:] * c[..., h:] + x[..., :h] * s[..., h:]], -1)


def _unrotate(y, c, s) -> np.ndarray:
    """The inverse rotation (cos / sin repeat over the two halves)."""
    h = y.shape[-1] // 2
    return np.concatenate([y[..., :h] * c[..., :h] + y[..., h:] * s[..., :h], y[..., h:] * c[..., h:] - y[..., :h] * s[..., h:]], -1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def sentinels(case: Case, b: int) -> list:
    """Visible keys of sample b that carry the mass in the sentinel family (see the module docstring)."""
    ln, T = case.lens[b], case.T
    n = ln + 1
    keep = case.keep(b)
    want = {ln, ln - 1, 0}
    for lo, hi in case.holes(b):
        want |= {lo - 1, hi}
    item_edges = list(range(64 * T, n, 64 * T))
    tile_edges = [e for e in range(64, n, 64) if e not in item_edges]
    extra = max(0, 6 - len(item_edges))
    if extra and tile_edges:
        item_edges += [tile_edges[i] for i in sorted({round(k * (len(tile_edges) - 1) / max(1, extra - 1)) for k in range(extra)})]
    for e in item_edges:
        want |= {e - 1, e}
    return sorted(j for j in want if 0 <= j < n and keep[j])


@dataclass
class Inputs:
    case: Case
    family: str
    qkv: torch.Tensor            # bf16 [B, 3 * H * 96]: the un-rotated q | k | v of the new tokens
    k: torch.Tensor              # bf16 [B, H, cap, 96]: rows < lens[b] cached, NaN from lens[b] on (unwritten cache)
    v: torch.Tensor
    cos: np.ndarray              # f32 [cap, 96]
    sin: np.ndarray
    stale_k: np.ndarray          # f32 [B, H, 96]: finite stand-ins for the stale cache row at the append position
    stale_v: np.ndarray
    sent: list                   # per sample: the sentinel keys (also listed in the diffuse family: the single-key mutations use them)


def make_inputs(case: Case, family: str) -> Inputs:
    assert family in FAMILIES
    B, H, cap = case.B, case.H, case.cap
    rng = np.random.default_rng(zlib.crc32(f"{case.id}/{family}".encode()))
    cos, sin = (a[0] for a in O.rope_cos_sin(np.arange(cap)[None], DH))
    k = torch.full((B, H, cap, DH), float("nan"), dtype=torch.bfloat16)
    v = torch.full((B, H, cap, DH), float("nan"), dtype=torch.bfloat16)
    qkv = np.zeros((B, 3, H, DH), dtype=np.float32)
    sent = [sentinels(case, b) for b in range(B)]
    for b, ln in enumerate(case.lens):
        n = ln + 1
        keep = case.keep(b)[:n]
        q_raw = bf16(rng.standard_normal((H, DH), dtype=np.float32))
        q = rotate_bf16(q_raw, cos[ln], sin[ln]).astype(np.float64)         # what the kernels dot the keys with
        K = rng.standard_normal((H, n, DH), dtype=np.float32).astype(np.float64)      # row ln: the new token's ROTATED k, for now
        qh = q / (q * q).sum(-1, keepdims=True)                              # K += x qh moves the raw dot product by x
        if family == "diffuse":
            V = rng.standard_normal((H, n, DH), dtype=np.float32) * np.float32(np.sqrt(n))
            # the running maxima of neighbouring items differ by a known step: the largest visible score of every item is moved to
            # 4.2 (even items) or 3.5 (odd ones), above what 64 T draws of N(0, 1) reach, so that a merge that weighs an item with
            # another item's maximum is off by e^+-0.7 in that item's share whatever the draw - and item 5, the first one a merge
            # slot folds into a running maximum, lies below item 0, so that its rescaling factor is not 1
            s0 = np.where(keep, np.einsum("hnd,hd->hn", K, q) * SCALE, -np.inf)
            for it, lo in enumerate(range(0, n, 64 * case.T)):
                if keep[lo:lo + 64 * case.T].any():
                    j = lo + s0[:, lo:lo + 64 * case.T].argmax(1)
                    hh = np.arange(H)
                    K[hh, j] += ((PEAKS[it % 2] - s0[hh, j]) / SCALE)[:, None] * qh
        else:
            sb = sent[b]
            level = np.log(33.0 * n / max(1, len(sb)))
            V = rng.standard_normal((H, n, DH), dtype=np.float32) * np.float32(np.sqrt(max(1, len(sb))) / 2)

            def set_score(cols, target):
                cols = np.asarray(cols, dtype=np.int64)
                if cols.size:
                    dot = np.einsum("hcd,hd->hc", K[:, cols], q)
                    K[:, cols] += (target / SCALE - dot)[..., None] * qh[:, None, :]
            set_score(sb, level)
            hidden = np.flatnonzero(~keep)
            set_score(hidden, level + MASKED_SCORE_LIFT)
            V[:, hidden] = MASKED_V
        # the new token: stored un-rotated in qkv, so that its rotation at position ln gives the row built above
        k_raw = bf16(_unrotate(K[:, ln], cos[ln].astype(np.float64), sin[ln].astype(np.float64)))
        qkv[b, 0], qkv[b, 1], qkv[b, 2] = q_raw, k_raw, bf16(V[:, ln])
        k[b, :, :ln] = torch.from_numpy(K[:, :ln].astype(np.float32)).to(torch.bfloat16)
        v[b, :, :ln] = torch.from_numpy(np.ascontiguousarray(V[:, :ln], dtype=np.float32)).to(torch.bfloat16)
    stale_k = bf16(rng.standard_normal((B, H, DH), dtype=np.float32))
    stale_v = bf16(rng.standard_normal((B, H, DH), dtype=np.float32))
    return Inputs(case, family, torch.from_numpy(qkv.reshape(B, 3 * H * DH)).to(torch.bfloat16), k, v, cos, sin, stale_k, stale_v, sent)


# ---- reference ------------------------------------------------------------------------------------------------------------------
def tolerance(ref: np.ndarray, scale_atol: float = 2.0) -> np.ndarray:
    """The bf16 bar of test_kernels_gpu.check at every element of `ref` (one sample: the GPU test calls check per sample)."""
    return 1e-3 * scale_atol * max(1.0, float(np.abs(ref).max())) + 2.0 ** -8 * np.abs(ref)


class Terms:
    """One sample's softmax terms in float64: scores s [H, n], un-normalised weights w = exp(s - max) of ALL columns (masked ones
    too, so that a mutation can unmask one), V [H, n, 96], keep [n].  Every mutation that only changes which keys count is a sum
    over these terms."""

    def __init__(self, q, K, V, keep):
        self.s = np.matmul(K, q[:, :, None])[..., 0] * SCALE
        self.w = np.exp(self.s - self.s.max(1, keepdims=True))
        self.V, self.keep, self.n = V, keep, keep.shape[0]
        self.kw = self.w * keep
        self._tiles = None

    @staticmethod
    def _div(A, L):
        L = L[..., None]
        return np.where(L > 0, A / np.where(L > 0, L, 1.0), 0.0)

    def tiles(self):
        """Per 64-key tile: sums of kw [H, nt] and of kw V [H, nt, 96]."""
        if self._tiles is None:
            e = np.arange(0, self.n, 64)
            self._tiles = np.add.reduceat(self.kw, e, axis=1), np.add.reduceat(self.kw[:, :, None] * self.V, e, axis=1)
        return self._tiles

    def out(self):
        Lt, At = self.tiles()
        return self._div(At.sum(1), Lt.sum(1))                      # [H, 96]; a row without a visible key gives zeros

    def without_groups(self, width_tiles):
        """Outputs with one group of `width_tiles` tiles left out, for every group: [groups, H, 96]."""
        Lt, At = self.tiles()
        e = np.arange(0, Lt.shape[1], width_tiles)
        Lg, Ag = np.add.reduceat(Lt, e, axis=1), np.add.reduceat(At, e, axis=1)
        G = Lg.shape[1]
        outs = np.empty((G,) + Ag[:, 0].shape)
        for g in range(G):
            rest = np.arange(G) != g
            outs[g] = self._div(Ag[:, rest].sum(1), Lg[:, rest].sum(1))
        return outs

    def with_columns(self, cols, sign):
        """Outputs with one more (sign +1: a masked column let in) or one fewer (-1) key, for every column of `cols`: [len, H, 96]."""
        Lt, At = self.tiles()
        L, A = Lt.sum(1), At.sum(1)
        cols = np.asarray(cols, dtype=np.int64)
        wc = self.w[:, cols]                                          # [H, c]
        Lc = L[:, None] + sign * wc
        Ac = A[:, None, :] + sign * wc[..., None] * self.V[:, cols]
        if sign < 0:                                                  # the last visible key left out: nothing remains
            only = (self.kw > 0).sum(1) <= 1
            Lc = np.where(only[:, None], 0.0, Lc)
        return np.moveaxis(self._div(Ac, Lc), 1, 0)

    def swapped_item_weights(self, T):
        """Item s merged with the running-max factor of item s + 1 (two `m` swapped in the merge), for every adjacent pair of items
        that both hold a visible key: [(s, out [H, 96])]."""
        Lt, At = self.tiles()
        e = np.arange(0, Lt.shape[1], T)
        Lg, Ag = np.add.reduceat(Lt, e, axis=1), np.add.reduceat(At, e, axis=1)
        ms = np.maximum.reduceat(np.where(self.keep, self.s, -np.inf), np.arange(0, self.n, 64 * T), axis=1)     # [H, items]
        live = np.isfinite(ms).all(0)
        L, A = Lg.sum(1), Ag.sum(1)
        res = []
        for s in range(Lg.shape[1] - 1):
            if live[s] and live[s + 1]:
                g = np.exp(ms[:, s + 1] - ms[:, s]) - 1.0
                res.append((s, self._div(A + g[:, None] * Ag[:, s], L + g * Lg[:, s])))
        return res


    def merged_without_rescaling(self, T):
        """The five-slot merge of decode_attn_split_kernel (slot q folds items q, q + 5, ... into a running maximum, then the five
        slots meet) with the incoming partial taken at weight 1 instead of exp(m_s - max): [H, 96].  Items in global-max units
        (Lg, Ag) are brought back to their own maximum first, as the kernel's partials are."""
        Lt, At = self.tiles()
        e = np.arange(0, Lt.shape[1], T)
        Lg, Ag = np.add.reduceat(Lt, e, axis=1), np.add.reduceat(At, e, axis=1)
        ms = np.maximum.reduceat(np.where(self.keep, self.s, -np.inf), np.arange(0, self.n, 64 * T), axis=1)     # [H, items]
        top = self.s.max(1)                                                                                     # what w is relative to
        with np.errstate(invalid="ignore", over="ignore"):
            own = np.where(np.isfinite(ms), np.exp(top[:, None] - ms), 0.0)
        Ls, As = Lg * own, Ag * own[..., None]
        H, S = ms.shape
        M, Lq, Aq = np.full((5, H), -np.inf), np.zeros((5, H)), np.zeros((5, H) + Ag.shape[2:])
        for q in range(5):
            for s in range(q, S, 5):
                mn = np.maximum(M[q], ms[:, s])
                with np.errstate(invalid="ignore"):
                    f0 = np.where(np.isfinite(M[q]), np.exp(M[q] - mn), 0.0)
                Lq[q] = Lq[q] * f0 + Ls[:, s]                      # f1 = 1
                Aq[q] = Aq[q] * f0[:, None] + As[:, s]
                M[q] = mn
        M5 = M.max(0)
        with np.errstate(invalid="ignore"):
            f = np.where(np.isfinite(M), np.exp(M - M5), 0.0)
        return self._div((Aq * f[..., None]).sum(0), (Lq * f).sum(0))


def sample_terms(inp: Inputs, b: int, view: str = "bf16", stored=None, pos: Optional[int] = None, stale: str = "") -> Terms:
    """Terms of sample b.  view "fp8": the keys are attended through their e4m3 copies.  stored = (K, V) float tensors
    [B, H, cap, 96]: the rows a kernel left behind (fp8: dequantised) instead of cache + append.  pos: rotate q and the new k at
    this position instead of lens[b]; stale "k" / "v": the new token's row comes from the stale stand-in (both are mutations)."""
    case = inp.case
    H, ln = case.H, case.lens[b]
    n = ln + 1
    pos = ln if pos is None else pos
    raw = inp.qkv[b].float().numpy().reshape(3, H, DH)
    q = rotate_bf16(raw[0], inp.cos[pos], inp.sin[pos]).astype(np.float64)
    if stored is not None:
        K, V = (a[b, :, :n].double().numpy() for a in stored)
    else:
        K = np.empty((H, n, DH), dtype=np.float64)
        V = np.empty((H, n, DH), dtype=np.float64)
        K[:, :ln], V[:, :ln] = inp.k[b, :, :ln].double().numpy(), inp.v[b, :, :ln].double().numpy()
        K[:, ln] = inp.stale_k[b] if stale == "k" else rotate_bf16(raw[1], inp.cos[pos], inp.sin[pos])
        V[:, ln] = inp.stale_v[b] if stale == "v" else raw[2]
        if view == "fp8":
            K, V = through_e4m3(K).astype(np.float64), through_e4m3(V).astype(np.float64)
    return Terms(q, K, V, case.keep(b)[:n])


def reference(case: Case, inp: Inputs, view: str = "bf16", stored=None) -> np.ndarray:
    """float64 [B, H * 96]: RoPE of q and of the new k in f32 rounded to bf16 (the kernels' rounding point), append, masked
    softmax, P V.  A row with no visible key is zeros - what the kernels return for it."""
    return np.stack([sample_terms(inp, b, view, stored).out().reshape(case.H * DH) for b in range(case.B)])


def appended_rows(inp: Inputs):
    """The rotated bf16 k rows and the v rows of the new tokens, f32 [B, H, 96] each, and the f64 rotation of k."""
    case = inp.case
    raw = inp.qkv.float().numpy().reshape(case.B, 3, case.H, DH)
    c, s = inp.cos[list(case.lens)][:, None, :], inp.sin[list(case.lens)][:, None, :]
    return rotate_bf16(raw[:, 1], c, s), raw[:, 2], rotate_f64(raw[:, 1], c, s)


def rotated_q(inp: Inputs) -> np.ndarray:
    case = inp.case
    raw = inp.qkv.float().numpy().reshape(case.B, 3, case.H, DH)
    return rotate_bf16(raw[:, 0], inp.cos[list(case.lens)][:, None, :], inp.sin[list(case.lens)][:, None, :])


# ---- mutations of the reference's view ------------------------------------------------------------------------------------------
# name -> (family that must see it, f(inp, b, view, terms) -> [(label, out [H, 96])]).  A mutation that does not apply to a sample
# (no hole, one item, nothing cached) returns an empty list by the rule written in it.  Tiles and items are bulk faults and belong to
# the diffuse family - unless the group holds fewer than SPARSE visible keys: then it is a single-key fault (the appended token
# alone in its tile, the stub of a hole) and either family may show it, as for a single key.
SPARSE = 8


def _visible_per_group(t: Terms, width):
    return np.add.reduceat(t.keep.astype(np.int64), np.arange(0, t.n, width))


def m_n_keys_one_short(inp, b, view, t):
    ln = inp.case.lens[b]
    return [("n_keys-1", t.with_columns([ln], -1)[0])] if t.keep[ln] else []           # rule: the new position is visible


def m_drop_sentinel(inp, b, view, t):
    sb = inp.sent[b]
    return [(f"drop key {j}", o) for j, o in zip(sb, t.with_columns(sb, -1))] if sb else []


def m_unmask_hole_edge(inp, b, view, t):
    cols = sorted({c for lo, hi in inp.case.holes(b) for c in (lo, hi - 1)})             # rule: the sample has a hole among its keys
    return [(f"unmask column {c}", o) for c, o in zip(cols, t.with_columns(cols, +1))] if cols else []


def _m_drop_groups(t, width_tiles, name, dense):
    vis = _visible_per_group(t, 64 * width_tiles)
    outs = t.without_groups(width_tiles)
    return [(f"drop {name} {g}", outs[g]) for g in range(len(vis)) if vis[g] > 0 and (vis[g] >= SPARSE) == dense]


def m_drop_tile(inp, b, view, t):
    return _m_drop_groups(t, 1, "tile", True)


def m_drop_sparse_tile(inp, b, view, t):
    return _m_drop_groups(t, 1, "tile", False)


def m_drop_item(inp, b, view, t):
    return _m_drop_groups(t, inp.case.T, "item", True)


def m_drop_sparse_item(inp, b, view, t):
    return _m_drop_groups(t, inp.case.T, "item", False)


def m_swap_item_weights(inp, b, view, t):
    return [(f"item {s} merged with the m of item {s + 1}", o) for s, o in t.swapped_item_weights(inp.case.T)]


def m_merge_without_rescaling(inp, b, view, t):
    # rule: weight 1 is right for the first live item of a slot and for one that raises the slot's maximum, so a slot must fold an odd
    # item (largest score PEAKS[1]) after a live even one (PEAKS[0] > PEAKS[1]) - read off the mask, not off the draw
    T = inp.case.T
    live = _visible_per_group(t, 64 * T) > 0
    S = len(live)
    if not any(live[s] and s % 2 == 0 and any(live[s2] and s2 % 2 == 1 for s2 in range(s + 5, S, 5)) for s in range(S)):
        return []
    return [("merge folds items at weight 1", t.merged_without_rescaling(T))]


def m_rotate_one_position_early(inp, b, view, t):
    ln = inp.case.lens[b]
    if ln < 1 or not t.keep[:ln].any():                 # rule: q . k_new does not see a common rotation; a cached key must be visible
        return []
    return [("RoPE at ln-1", sample_terms(inp, b, view, pos=ln - 1).out())]


def m_stale_k(inp, b, view, t):
    ln = inp.case.lens[b]
    if not t.keep[ln] or not t.keep[:ln].any():         # rule: with one visible key its score cancels in the softmax
        return []
    return [("new k from the stale row", sample_terms(inp, b, view, stale="k").out())]


def m_stale_v(inp, b, view, t):
    return [("new v from the stale row", sample_terms(inp, b, view, stale="v").out())] if t.keep[inp.case.lens[b]] else []


MUTATIONS = {
    "n_keys-1": ("either", m_n_keys_one_short),
    "drop-sentinel": ("sentinel", m_drop_sentinel),
    "unmask-hole-edge": ("sentinel", m_unmask_hole_edge),
    "drop-tile": ("diffuse", m_drop_tile),
    "drop-sparse-tile": ("either", m_drop_sparse_tile),
    "drop-item": ("diffuse", m_drop_item),
    "drop-sparse-item": ("either", m_drop_sparse_item),
    "swap-item-weights": ("diffuse", m_swap_item_weights),
    "merge-without-rescaling": ("diffuse", m_merge_without_rescaling),
    "rope-at-ln-1": ("either", m_rotate_one_position_early),
    "stale-k": ("either", m_stale_k),
    "stale-v": ("either", m_stale_v),
}


def mutation_ratios(inp: Inputs, b: int, view: str) -> dict:
    """{mutation: {label: worst |mutated - reference| / tolerance over the sample's elements}}."""
    t = sample_terms(inp, b, view)
    ref = t.out()
    tol = tolerance(ref)
    return {name: {label: float((np.abs(o - ref) / tol).max()) for label, o in f(inp, b, view, t)} for name, (_, f) in MUTATIONS.items()}
