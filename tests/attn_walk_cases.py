"""Case table, inputs, walk plan, float64 reference and reference mutations of the attention FORWARD where a persistent workgroup
walks SEVERAL ranks of its (batch, head) pair - the loop of aki_amd/csrc/mma_attn_bf16.hip ("Persistent workgroups") and of
mma_attn64_bf16.hip (prefetch_rank, the verification word and its parity, the second walk of a failed rank) that
tests/attn_fwd_cases.py never enters: its cases have one rank per workgroup.

numpy and CPU torch only.  tests/test_attn_walk_cases_cpu.py checks the table itself and tests/test_attn_walk_gpu.py runs it on the
device.  Case, forward_rows, Reference, tol_of (KAPPA 2.5 / 4.5, ACC, the lse bar), lse_pattern, MIN_RATIO, kernel_constants and
ranks_per_workgroup are those of attn_fwd_cases.py: the bar is the one derived there, unchanged.

Replicated heads.  Several ranks per workgroup need B * H of a few hundred pairs, and a float64 reference of that many distinct heads
is hundreds of millions of query-key pairs.  The kernel cannot tell that heads share data: a case has H heads but HB = 2 BASE heads
per sample; q and k of head h are those of base head h % HB, and v of head h is s 2^e v_base with (s, e) = SCALES[h // HB] - signs
+-1, exponents -4 .. 3, no two heads of a sample alike.  The scaling is exact in bf16 and every term of the bar is homogeneous in v:
o = s 2^e o_base, M = 2^e M_base, tol = 2^e tol_base, lse = lse_base (the CPU test asserts the identity with max |diff| = 0 against a
directly computed reference).  Samples keep their own data and masks; references are computed for B * HB pairs only.

Walk plan.  walk_plan() restates the device's decomposition in numpy from constants parsed out of the sources: block_extent, the ranking
of up to kSchedMax (128 for the 64-row core) 32-row blocks by extent (descending, later block first on ties, four or eight per rank),
position order with late rows first beyond that, nqt / splits / group_bh of the two launchers, and the snake
kk * splits + (kk even ? sidx : splits - 1 - sidx).  properties() is computed from it.

What the decomposition cannot do.  In ranked order rank g + 1 never streams more tiles than rank g (ranks are cut from one descending
order and a rank streams to its largest extent) and a walk visits ranks in ascending order, so inside a ranked walk the stream
length never grows: "a previous rank of 1 or 2 tiles followed by a longer one" and light -> heavy exist only in position order (L >
4096 on the 64-row core: rows 256 .. 511 walked before rows 0 .. 255 whose rectangle reaches the end), where no rank of 256 rows
streams fewer than 4 tiles.  UNREACHABLE lists those two properties; the CPU test asserts the monotony that excludes them and
requires the reverse (a longer rank followed by one of 1 and of 2 tiles) and both hand-over directions.

Families.  diffuse and sentinel as in attn_fwd_cases.py, with more sentinel pairs: every 32-row block of every rank that is not first
in its walk (any core the case runs on, either dead-row convention) gets keys on both sides of the edges of tiles 0, 1 and 2 - the
tiles the prologue / prefetch_rank re-issue - and a key of the last tile of its rank's stream.  That is seven keys and MAX_TARGETS is
6 per row (the reason is in attn_fwd_cases.py), so they are spread over rows of the block that see them, four to a row while another
row is left.  rising (64-row core): the lifted key
band and the rows that carry the lifting feature are per-case parameters (RISE), chosen so that the walks hold fail -> pass, pass ->
fail, fail -> fail and a failing last rank ("fails": some row sum against the first tile's maximum >= 2^64; "passes": all < 2^60).

Mutations (MUTATIONS): what a wrong hand-over between ranks would return.  Two of the rising ones cannot leave this bar and are listed
in CAPPED with the reason: bf16 and f32 share an exponent range, so a blind pass 72 log2 units above its reference, or a rank run against
a reference 72 units too high, is finite and exact to rounding - the second walk is a safety margin below 2^127, not a visible change.
"""
import dataclasses
import os
import re
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import attn_bwd_cases as A
import attn_fwd_cases as F
from attn_fwd_cases import (Case, forward_rows, tol_of, KAPPA, lse_pattern, MIN_RATIO, kernel_constants, ranks_per_workgroup,   # noqa: F401
                            vis_of, bf16, TILE, MAX_TARGETS, FORBIDDEN_V, LIFT, Z, N, CUS)

HB = 2
SCALES = tuple((s, e) for s in (1.0, -1.0) for e in range(-4, 4))                 # 16 (sign, exponent): H <= 32
MAX_PAIRS = 40_000_000
RISE_Q, RISE_SENT = F.RISE_Q, F.RISE_SENT
LOG2E = 1.4426950408889634


def walk_constants() -> dict:
    """kernel_constants() plus what the walk needs: kL2Rows, the ring depth, rows per rank and slots per compute unit of each launcher."""
    rd = lambda *p: open(os.path.join(F.ROOT, "aki_amd", "csrc", *p)).read()
    src32, src64, common = rd("mma_attn_bf16.hip"), rd("mma_attn64_bf16.hip"), rd("attn_mma_common.h")
    kc = dict(kernel_constants())
    m = {
        "L2ROWS": re.search(r"constexpr int kL2Rows = (\d+);", src32),
        "NSTAGE": re.search(r"constexpr int NSTAGE = (\d+);", common),
        "NW32": re.search(r"constexpr int NW = (\d+);\s*\n\s*AttnParams p = \{\};", src32),
        "SLOTS32": re.search(r"int splits = \((\d+) \* cus \+ nbh - 1\) / nbh;", src32),
        "ROWS64": re.search(r"p\.nqt = \(p\.L \+ (\d+)\) / (\d+);", src64),
    }
    assert all(m.values()), f"walk constants not found in the sources: {[k for k, v in m.items() if not v]}"
    assert re.search(r"int splits = \(cus \+ nbh - 1\) / nbh;", src64), "the 64-row launcher's slot count moved"
    assert "kk * p.splits + ((kk & 1) ? p.splits - 1 - sidx : sidx)" in src32 and "kk * p.splits + ((kk & 1) ? p.splits - 1 - sidx : sidx)" in src64, "the snake moved"
    kc.update(L2ROWS=int(m["L2ROWS"].group(1)), NSTAGE=int(m["NSTAGE"].group(1)), ROWS32=32 * int(m["NW32"].group(1)),
              SLOTS32=int(m["SLOTS32"].group(1)), SLOTS64=1, ROWS64=int(m["ROWS64"].group(2)))
    assert int(m["ROWS64"].group(1)) == kc["ROWS64"] - 1
    return kc


WC = walk_constants()
NSTAGE = WC["NSTAGE"]


# ---- walk plan ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Rank:
    g: int
    blocks: tuple                  # 32-row block per (wave, half) slot, -1: the rank lacks it
    ext: tuple                     # extents of those blocks (0 for a missing one)
    jend: int                      # 64-key tiles the rank streams


@dataclass
class Plan:
    core: str
    nqt: int
    splits: int
    group_bh: int
    nbh: int
    sched: bool
    per_rank: int                  # blocks per rank
    walks: list                    # per sidx: ranks in walk order
    ranks: list                    # per sample: [Rank] by g

    @property
    def last_group(self):
        return self.nbh - (self.nbh - 1) // self.group_bh * self.group_bh


def block_extents(case: Case, b: int, dead_rows: int) -> np.ndarray:
    L, Lb = case.Lq, case.seq_len(b)
    ext = []
    for r0 in range(0, L, 32):
        e = min(r0 + 32, L)
        for rlo, rhi, clo, chi in case.live_rects(b):
            if rlo < r0 + 32 and rhi > r0:
                e = max(e, min(chi, L))
        if dead_rows and min(r0 + 32, L) > Lb:
            e = L
        ext.append(e)
    return np.array(ext)


def walk_plan(case: Case, core: str, cus: int = CUS, dead_rows: int = 1) -> Plan:
    L, nbh = case.Lq, case.B * case.H
    nblk = (L + 31) // 32
    if core == "64":
        rows, limit = WC["ROWS64"], WC["SCHED64"]
        nqt = (L + rows - 1) // rows
        splits = max(1, min((WC["SLOTS64"] * cus + nbh - 1) // nbh, nqt))
        grp = ((WC["SLOTS64"] * cus + splits - 1) // splits + 7) & ~7
    else:
        rows, limit = WC["ROWS32"], WC["SCHED32"]
        nqt = (L + rows - 1) // rows
        splits = max(1, min(max((WC["SLOTS32"] * cus + nbh - 1) // nbh, L // WC["L2ROWS"]), nqt))
        grp = ((WC["SLOTS32"] * cus + splits - 1) // splits + 7) & ~7
    n = rows // 32
    sched = nblk <= limit
    walks = []
    for sidx in range(splits):
        w, kk = [], 0
        while True:
            g = kk * splits + (splits - 1 - sidx if kk & 1 else sidx)
            if g >= nqt:
                break
            w.append(g)
            kk += 1
        walks.append(w)
    per_sample = []
    for b in range(case.B):
        ext = block_extents(case, b, dead_rows)
        order = sorted(range(nblk), key=lambda i: -(int(ext[i]) * 256 + i))       # extent descending, later block first on ties
        ranks = []
        for g in range(nqt):
            if sched:
                blocks = order[n * g:n * g + n]
            else:
                q0 = (nqt - 1 - g) * rows
                blocks = [i for i in range(q0 // 32, q0 // 32 + n) if i < nblk]
            blocks = tuple(blocks) + (-1,) * (n - len(blocks))
            e = tuple(int(ext[i]) if i >= 0 else 0 for i in blocks)
            ranks.append(Rank(g, blocks, e, (max(e) + 63) // 64))
        per_sample.append(ranks)
    return Plan(core, nqt, splits, min(grp, nbh), nbh, sched, n, walks, per_sample)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
_LENS655 = (655, 600, 655, 512, 655, 640, 655, 655, 655, 620, 655)                # the first eight: the benchmark-shape test's ragged batch


def _bench_mask(B, L=655, lens=_LENS655, col_hi=638):
    """The benchmark's mask: one image rectangle (rows 6 .. 150, columns to near the sample's end) per sample, ragged lengths; sample 3
    has no rectangle and five columns of left padding (rows 0 .. 4 inside seq_len see nothing), sample 2 a hole in col_valid_bits."""
    rects, holes, seq = [], [], []
    for b in range(B):
        Ls = min(lens[b % len(lens)], L)
        rects.append([Z] if b % 8 == 3 else [(6, min(150, Ls - 2), min(150, Ls - 2), min(col_hi, Ls))])
        h = [(Ls, L)] if Ls < L else []
        if b % 8 == 3:
            h = [(0, 5)] + h
        if b % 8 == 2:
            h = [(min(300, L // 2), min(330, L // 2 + 30))] + h
        holes.append(h)
        seq.append(Ls)
    return rects, holes, seq


def _w(id, B, H, L, mask, why):
    c = A._m(id, B, H, L, *mask, why=why)
    assert H % HB == 0 and H // HB <= len(SCALES)
    return c


_L200 = (200, 180, 200, 150, 200, 200, 167, 200)
_MIN = WC["MIN_L"]
CASES = (
    _w("bench-655", 8, 32, 655, _bench_mask(8), "the benchmark geometry: 32-row core nqt 6, splits 2, three ranks per workgroup, one group of 256; forced 64-row core: one workgroup walks all 3 ranks"),
    _w("uneven-655", 4, 32, 655, _bench_mask(4), "splits 4 over 6 ranks: two workgroups of a pair walk 2 ranks, two walk 1"),
    _w("short-group-655", 11, 24, 655, _bench_mask(11), "264 pairs in groups of 256: the last group holds 8 pairs"),
    _w("one-split-200", 16, 32, 200, _bench_mask(16, 200, _L200, 190), "L < kL2Rows, 512 pairs: splits 1, both ranks in one workgroup; the second rank lacks a block"),
    _w(f"below-min-{_MIN - 1}", 2, 32, _MIN - 1, ([[(6, 150, 150, _MIN - 90)], [Z]], [N, [(0, 3), (_MIN - 200, _MIN - 1)]], [_MIN - 1, _MIN - 200]),
       "32-row core by the product rule one row below AKI_ATTN64_MIN_L: nqt 14, splits 8, 56 ranked blocks"),
    _w(f"min-{_MIN}", 3, 32, _MIN, ([[(6, 150, 150, _MIN - 60)], [Z], [(6, 150, 150, 1000)]], [N, [(_MIN - 130, _MIN)], [(700, 710)]], [_MIN, _MIN - 130, _MIN]),
       "64-row core by the product rule: nqt 7, splits 3, groups of 88 of 96 pairs (short last group)"),
    _w("rise-1856", 3, 32, 1856, ([[(6, 150, 150, 1800)], [(6, 150, 150, 1700)], [Z]], [N, N, N], [1856, 1856, 1856]),
       "64-row core: nqt 8, splits 3; the rising family orders failed and passed ranks inside the walks"),
    _w("position-4160", 1, 16, 4160, ([[(6, 150, 150, 4100)]], [N], [4160]),
       "130 blocks: position order on the 64-row core, nqt 17, splits 16: one workgroup walks rows 256 .. 511, then rows 0 .. 255 (light -> heavy)"),
)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
ROUTES = {"bench-655": ("32", "64", "product"), "rise-1856": ("64", "164", "product")}
DEAD_ROWS = {"bench-655": (1, 0), "one-split-200": (1, 0)}
# rising: keys of `band` carry the lift (2^lift against the other keys, on the rows that carry the feature); `fail`[b][base head] = ranks
# (64-row plan) whose blocks from row 192 on carry it.  Walks of rise-1856: [0, 5, 6], [1, 4, 7], [2, 3].
RISE = {"rise-1856": dict(lift=72.0, band=(64, 128), min_row=192,
                          fail=(((5, 4, 7, 3), (0, 6, 1)), ((3, 6), (5, 4, 7)), ((0, 5, 6, 2), (1, 6))))}
CAPPED = {
    "rising:failed-rank-not-walked-again": (0.0, "bf16 and f32 share the exponent range: p = exp2(s c - m_ref) up to 2^72 and a row sum of 2^78 are finite and exact to "
                                                 "rounding, the blind result of a rank that fails the 2^64 test sits inside the bar (measured ratio ~0.3); only past 2^127 is it non-finite"),
    "rising:next-rank-with-failed-ranks-maximum": (0.0, "softmax is invariant to its reference: against a maximum 72 log2 units too high p >= 2^-126 still holds for every key "
                                                        "within 54 log2 units of the row's own maximum, nothing is flushed and the result is the reference's to rounding (measured ratio ~0.3)"),
}
UNREACHABLE = {
    "prev-jend=1->longer": "ranked walks never grow (module docstring); in position order only the rank of rows 0 .. is that short, and it is the pair's last",
    "prev-jend=2->longer": "as above",
}


def routes(case: Case) -> tuple:
    return ROUTES.get(case.id, ("product",))


def product_core(case: Case) -> str:
    return "64" if case.Lq >= WC["MIN_L"] else "32"


def core_of(case: Case, route: str) -> str:
    return product_core(case) if route == "product" else "32" if route == "32" else "64"


def cores(case: Case) -> tuple:
    return tuple(sorted({core_of(case, r) for r in routes(case)}))


def families(case: Case) -> tuple:
    return ("diffuse", "sentinel") + (("rising",) if case.id in RISE else ())


def dead_conventions(case: Case) -> tuple:
    return DEAD_ROWS.get(case.id, (1,))


def base_case(case: Case) -> Case:
    return dataclasses.replace(case, H=HB)


def distinct_pairs(case: Case) -> int:
    return case.B * HB * case.Lq * case.Lk


def head_scale(h: int) -> float:
    s, e = SCALES[h // HB]
    return s * 2.0 ** e


def plans(case: Case, cus: int = CUS):
    """{(core, dead_rows): Plan} for every core and convention the case runs under."""
    return {(c, d): walk_plan(case, c, cus, d) for c in cores(case) for d in dead_conventions(case)}


def later_walked(plan: Plan):
    """[(sidx, position in the walk, previous rank g, rank g)] for every rank that is not first in its walk."""
    return [(s, i, w[i - 1], w[i]) for s, w in enumerate(plan.walks) for i in range(1, len(w))]


def properties(case: Case, cus: int = CUS) -> set:
    P = set()
    for (core, dr), pl in plans(case, cus).items():
        lens = {len(w) for w in pl.walks}
        P.update(f"ranks-per-wg={n}" for n in lens)
        if len(lens) > 1:
            P.add("uneven-walks")
        P.add(f"core{core}:{'ranked' if pl.sched else 'position'}")
        if pl.nbh % pl.group_bh:
            P.add("short-last-group")
        if case.id == "bench-655" and core == "32" and (pl.nqt, pl.splits, pl.group_bh) == (6, 2, 256):
            P.add("benchmark-geometry")
        for s, i, gp, g in later_walked(pl):
            P.add("snake:even-then-rank" if (i - 1) % 2 == 0 else "snake:odd-then-rank")
            for b in range(case.B):
                rp, r = pl.ranks[b][gp], pl.ranks[b][g]
                if core == "32":
                    P.add(f"prev-jend%{NSTAGE}={rp.jend % NSTAGE}")
                if rp.jend in (1, 2) and r.jend > rp.jend:
                    P.add(f"prev-jend={rp.jend}->longer")
                if r.jend in (1, 2) and rp.jend > r.jend:
                    P.add(f"longer->jend={r.jend}")
                if rp.jend > r.jend:
                    P.add("heavy->light")
                if rp.jend < r.jend:
                    P.add("light->heavy")
                if -1 in r.blocks:
                    P.add("rank-lacking-blocks-walked-later")
                dead = dead_row_mask(case, b)
                has = lambda rk: any(bl >= 0 and dead[32 * bl:32 * bl + 32].any() for bl in rk.blocks)
                if has(rp) and not has(r):
                    P.add("dead-rank-then-live-rank")
                if has(r) and not has(rp):
                    P.add("live-rank-then-dead-rank")
    if case.id in RISE:
        P.update(rise_patterns(case))
    return P


def dead_row_mask(case: Case, b: int) -> np.ndarray:
    return ~vis_of(case, b).any(1)


REQUIRED = ("ranks-per-wg=2", "ranks-per-wg=3", "uneven-walks", "snake:even-then-rank", "snake:odd-then-rank",
            "prev-jend%3=0", "prev-jend%3=1", "prev-jend%3=2", "longer->jend=1", "longer->jend=2", "heavy->light", "light->heavy",
            "rank-lacking-blocks-walked-later", "dead-rank-then-live-rank", "live-rank-then-dead-rank", "short-last-group",
            "core64:ranked", "core64:position", "core32:ranked", "benchmark-geometry",
            "rise:fail->pass", "rise:pass->fail", "rise:fail->fail", "rise:failing-last-rank")


def rise_rows(case: Case, b: int, hb_: int) -> np.ndarray:
    """Rows of sample b, base head hb_, that carry the lifting feature."""
    R = RISE[case.id]
    pl = walk_plan(case, "64")
    rows = []
    for g in R["fail"][b][hb_]:
        for bl in pl.ranks[b][g].blocks:
            if bl >= 0 and 32 * bl >= R["min_row"]:
                rows += list(range(32 * bl, min(32 * bl + 32, case.Lq)))
    return np.array(sorted(rows), dtype=np.int64)


def rise_patterns(case: Case) -> set:
    """Which orders of failed (f) and passed (p) ranks the walks of the case hold, by the table (the CPU test checks it against the row sums)."""
    P, pl, R = set(), walk_plan(case, "64"), RISE[case.id]
    for b in range(case.B):
        for hb_ in range(HB):
            fail = set(R["fail"][b][hb_])
            for w in pl.walks:
                for gp, g in zip(w, w[1:]):
                    P.add(f"rise:{'fail' if gp in fail else 'pass'}->{'fail' if g in fail else 'pass'}")
                if w[-1] in fail:
                    P.add("rise:failing-last-rank")
    return P


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def walk_targets(case: Case, b: int) -> dict:
    """{32-row block: wanted sentinel keys} for every block of a later-walked rank: both sides of the edges of tiles 0, 1, 2 and a key of the
    last tile of the rank's stream, as far as some row of the block sees them."""
    want = {}
    for pl in plans(case).values():
        for _, _, _, g in later_walked(pl):
            r = pl.ranks[b][g]
            for bl in r.blocks:
                if bl >= 0:
                    want.setdefault(bl, set()).update((63, 64, 127, 128, 191, 192))
                    want[bl].add(("last", r.jend - 1))
    return want


def walk_pairs(case: Case, b: int):
    """(pairs, forbidden, reached): attn_fwd_cases.fwd_pairs of the sample plus the walk targets, each on a row of its block that sees the key (never past
    MAX_TARGETS on a row, so nothing listed is thinned away); reached = {block: the wanted keys (tile index for the last tile) it got}."""
    bc = base_case(case)
    vis = vis_of(bc, b)
    pairs, forbidden = F.fwd_pairs(bc, b)
    want = {}
    for r, c in forbidden:
        want.setdefault(r, {})[c] = 0
    for r, c in pairs:
        want.setdefault(r, {})[c] = 2
    reached = {}
    for bl, keys in sorted(walk_targets(case, b).items()):
        rows = [r for r in range(32 * bl, min(32 * bl + 32, case.seq_len(b))) if vis[r].any()]
        used = []                                                                # rows of the block that already carry a walk target: filled first
        for kx in sorted(keys, key=str):
            if isinstance(kx, tuple):                                            # the last tile of the stream: the largest key of it that a row sees
                t = kx[1]
                cols = [c for c in range(min(64 * t + 63, case.Lk - 1), 64 * t - 1, -1) if any(vis[r, c] for r in rows)][:1]
            else:
                cols = [kx] if any(vis[r, kx] for r in rows) else []
            for c in cols:
                have = [r for r in rows if c in want.get(r, {}) and want[r][c] != 0]
                free = [r for r in rows if vis[r, c] and len(want.get(r, {})) < MAX_TARGETS]
                if not have and free:
                    r = min(free, key=lambda r: (max(len(want.get(r, {})) + 1, 4), r not in used, -r))       # at most four targets on a row while one is left
                    want.setdefault(r, {})[c] = 1
                    used.append(r)
                    have = [r]
                if have:
                    reached.setdefault(bl, set()).add(kx)
    out_p, out_f = [], []
    for r, t in want.items():
        for c in sorted(t, key=lambda c: (t[c], min(c, case.Lk - 1 - c)))[:MAX_TARGETS]:
            (out_f if t[c] == 0 else out_p).append((r, c))
    return sorted(out_p), sorted(out_f), reached


def make_inputs(case: Case, family: str) -> F.Inputs:
    """The BASE inputs (HB heads per sample) of a case: attn_fwd_cases.make_inputs with the walk's sentinel pairs and the per-case rising
    parameters.  expand() makes the H heads the device sees."""
    assert family in families(case)
    bc = base_case(case)
    B, H, Lq, Lk, D = bc.B, bc.H, bc.Lq, bc.Lk, bc.Dh
    rng = np.random.default_rng(zlib.crc32(f"walk/{case.id}/{family}".encode()))
    q = rng.standard_normal((B, H, Lq, D))
    k = rng.standard_normal((B, H, Lk, D))
    pairs, forbidden = [[] for _ in range(B)], [[] for _ in range(B)]
    if family in ("diffuse", "rising"):
        v = np.abs(rng.standard_normal((B, H, Lk, D))) * rng.choice([-1.0, 1.0], (B, H, 1, D))
    if family == "rising":
        R = RISE[case.id]
        lo, hi = R["band"]
        q[..., D - 1] = 0.0
        k[..., D - 1] = 0.0
        k[..., lo:hi, D - 1] = float(bf16(np.array([R["lift"] * np.log(2.0) / (RISE_Q * bc.scale)]))[0])
        share = []
        for b in range(B):
            for h in range(H):
                q[b, h, rise_rows(case, b, h), D - 1] = RISE_Q
        qb, kb = bf16(q).astype(np.float64), bf16(k).astype(np.float64)
        for b in range(B):                                                        # probe: the first tile's sentinels on some lifted rows
            for h in range(H):
                rows = rise_rows(case, b, h)
                rows = rows[::max(1, len(rows) // 32)]
                s = (qb[b, h][rows] @ kb[b, h].T) * bc.scale
                s = np.where(vis_of(bc, b)[rows], s, -np.inf)
                P = np.exp(s - s.max(-1, keepdims=True))
                P /= P.sum(-1, keepdims=True)
                share.append(P[..., list(RISE_SENT)].sum(-1))
        x = np.round(np.log2(np.sqrt(2 / np.pi) / np.median(np.concatenate(share))))
        v[:, :, list(RISE_SENT)] = 2.0 ** x * np.sign(v[:, :, list(RISE_SENT)])
    if family == "sentinel":
        v = rng.standard_normal((B, H, Lk, D))
        level = np.log(100.0 * Lk)
        for b in range(B):
            pairs[b], forbidden[b], _ = walk_pairs(case, b)
            targets = {}
            for r, c in pairs[b]:
                targets.setdefault(r, {})[c] = level
            for r, c in forbidden[b]:
                targets.setdefault(r, {})[c] = level + LIFT
            keys = sorted({c for t in targets.values() for c in t})
            u = rng.standard_normal((H, len(keys), D))
            k[b][:, keys] = u / np.linalg.norm(u, axis=-1, keepdims=True) * np.sqrt(D)
            v[b][:, sorted({c for _, c in forbidden[b]})] = FORBIDDEN_V
            v[b][:, ~bc.valid(b)] = FORBIDDEN_V
            kb = bf16(k[b]).astype(np.float64)
            for r, t in targets.items():
                cols = sorted(t)
                want = np.array([t[c] for c in cols]) / bc.scale
                for h in range(H):
                    q[b, h, r] = np.linalg.lstsq(kb[h][cols], want, rcond=None)[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return F.Inputs(bc, family, t(q), t(k), t(v), pairs, forbidden)


def expand(inp: F.Inputs, case: Case):
    """(q, k, v) bf16 [B, H, L, D] of the case's H heads from the base inputs: exact in bf16 (a power of two and a sign)."""
    idx = torch.arange(case.H) % HB
    sc = torch.tensor([head_scale(h) for h in range(case.H)], dtype=torch.float32)[None, :, None, None]
    v = (inp.v[:, idx].float() * sc).to(torch.bfloat16)
    assert torch.equal(v.float(), inp.v[:, idx].float() * sc), "the V scaling is not exact in bf16"
    return inp.q[:, idx].contiguous(), inp.k[:, idx].contiguous(), v.contiguous()


# ---- reference ------------------------------------------------------------------------------------------------------------------
class Reference:
    """One (case, family): attn_fwd_cases.Reference of the B * HB base pairs, and its expansion to the H heads."""

    def __init__(self, case: Case, family: str):
        self.case, self.family = case, family
        self.inp = make_inputs(case, family)
        self.base = F.Reference(self.inp)
        self.idx = np.arange(case.H) % HB
        self.sc = np.array([head_scale(h) for h in range(case.H)])

    def base_tol(self, b, core, dead_rows=1):
        """tol_of as it stands; the rising family's score-error terms (S_o, S_lse of attn_fwd_cases.py) are added here because tol_of keys
        them on that module's own case ids."""
        t_o, t_l = self.base.tol(b, core, dead_rows)
        if self.family == "rising":
            s = self.base.S[b]
            t_o, t_l = t_o + s.S_o, t_l + s.S_lse
        return t_o, t_l

    def expected(self, b, core, dead_rows=1):
        """(o [H, L, D], tol_o, lse [H, L], tol_lse, live [L]) of sample b for all H heads."""
        o, _, _, live = self.base.expected(b, dead_rows)
        t_o, t_l = self.base_tol(b, core, dead_rows)
        sc, idx = self.sc[:, None, None], self.idx
        return sc * o[idx], np.abs(sc) * t_o[idx], self.base.S[b].lse[idx], t_l[idx], live


_REFS = {}


def reference(case: Case, family: str) -> Reference:
    key = (case.id, family)
    if key not in _REFS:
        if len(_REFS) >= 2:
            _REFS.clear()
        _REFS[key] = Reference(case, family)
    return _REFS[key]


# ---- mutations of the reference -------------------------------------------------------------------------------------------------
def eval_rows(inp, b, rows, vis=None, q_rows=None, kv=None, tile_from=None):
    """Float64 (o [HB, r, D], lse [HB, r]) of rows `rows` of sample b: own visibility unless given, Q of rows q_rows, K / V of (sample, base
    head permutation) kv = (b2, perm), keys of tile t replaced by those of tile t2 for tile_from = (t, t2)."""
    c = inp.case
    rows = np.asarray(rows, dtype=np.int64)
    vis = vis_of(c, b)[rows] if vis is None else vis
    qr = rows if q_rows is None else np.asarray(q_rows, dtype=np.int64)
    b2, perm = (b, list(range(c.H))) if kv is None else kv
    q = inp.q[b].double().numpy()[:, np.minimum(qr, c.Lq - 1)]
    k, v = inp.k[b2].double().numpy()[perm], inp.v[b2].double().numpy()[perm]
    if tile_from is not None:
        t, t2 = tile_from
        k, v = k.copy(), v.copy()
        dst = np.arange(64 * t, min(64 * t + 64, c.Lk))
        src = np.minimum(dst - 64 * t + 64 * t2, c.Lk - 1)
        k[:, dst], v[:, dst] = k[:, src], v[:, src]
    s = (q @ k.transpose(0, 2, 1)) * c.scale
    s = np.where(vis[None], s, -np.inf)
    live = vis.any(1)
    m = np.where(live, s.max(-1), 0.0)
    e = np.exp(s - m[..., None])
    l = e.sum(-1)
    with np.errstate(divide="ignore"):
        lse = np.where(live, m + np.log(np.where(l > 0, l, 1.0)), -np.inf)
    return (e / np.where(l > 0, l, 1.0)[..., None]) @ v, lse


@dataclass
class Ctx:
    """What a mutation needs of one (case, family): the base inputs.  (A Reference has the same three fields.)"""
    case: Case
    family: str
    inp: F.Inputs


def _ratio(ref, b, rows, o2, l2, dead_rows=1, core="64"):
    """Worst |mutated - reference| / tolerance on the LIVE rows `rows` of the base heads (the widest bar: the 64-row core's), as the GPU test
    compares them; the reference of just these rows is made here (forward_rows), so no mutation needs a whole case in float64."""
    inp = ref.inp
    R = forward_rows(inp, b, rows)
    assert (R.n > 0).all()
    t_o, t_l = tol_of(inp.case, core, R.o, R.M, R.n.astype(np.float64), R.lse, R.S_o, R.S_lse)
    if ref.family == "rising":
        t_o, t_l = t_o + R.S_o, t_l + R.S_lse
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(o2 - R.o)
        ro = np.where(np.isfinite(d), np.where(d > 0, d / np.where(t_o > 0, t_o, 1e-300), 0.0), np.inf)
        rl = np.where(np.isfinite(l2), np.abs(l2 - R.lse) / t_l, np.inf)
    return float(max(ro.max(), rl.max()))


def _live(ref, b, rows):
    rows = np.asarray(rows, dtype=np.int64)
    return rows[vis_of(ref.inp.case, b)[rows].any(1)]


def _block_rows(case, bl):
    return np.arange(32 * bl, min(32 * bl + 32, case.Lq))


def _rank_rows(ref, b, r):
    return _live(ref, b, np.concatenate([_block_rows(ref.case, bl) for bl in r.blocks if bl >= 0]))


def _later(ref, core, dead_rows=1):
    """The plan and the first and the last of its later-walked ranks (a mutation has to show on one element of a case, not on every rank)."""
    pl = walk_plan(ref.case, core, dead_rows=dead_rows)
    later = later_walked(pl)
    return pl, later[:1] + later[1:][-1:]


def _only(hb_, o2, l2, o_ref, l_ref):
    """The mutant on base head hb_, the reference on the other."""
    keep = np.arange(HB) == hb_
    return np.where(keep[:, None, None], o2, o_ref), np.where(keep[:, None], l2, l_ref)


def m_stale_tile(ref, b, core, which):
    """K and V of tile t of a later-walked rank are what the ring still held: the tile the previous rank streamed last ("prev-last"), or the
    last tile the previous rank wrote into stage t ("ring-stage")."""
    pl, later = _later(ref, core)
    res = {}
    for _, _, gp, g in later:
        rp, r = pl.ranks[b][gp], pl.ranks[b][g]
        for t in range(2 if core == "32" else 3):
            if t >= r.jend:
                continue
            src = rp.jend - 1 if which == "prev-last" else max((j for j in range(rp.jend) if j % NSTAGE == t), default=t)
            if src == t:
                continue
            rows = _rank_rows(ref, b, r)
            rows = rows[vis_of(ref.inp.case, b)[rows][:, 64 * t:64 * t + 64].any(1)]
            if len(rows):
                o2, l2 = eval_rows(ref.inp, b, rows, tile_from=(t, src))
                res[f"rank {g} after {gp}: tile {t} <- tile {src}"] = _ratio(ref, b, rows, o2, l2)
    return res


def m_stale_q(ref, b, core):
    """A block of a later-walked rank computed with the Q rows of the same wave's block in the previous rank."""
    pl, later = _later(ref, core)
    res = {}
    for _, _, gp, g in later:
        rp, r = pl.ranks[b][gp], pl.ranks[b][g]
        for slot, (bl, blp) in enumerate(zip(r.blocks, rp.blocks)):
            if bl >= 0 and blp >= 0:
                rows = _live(ref, b, _block_rows(ref.case, bl))
                if len(rows):
                    o2, l2 = eval_rows(ref.inp, b, rows, q_rows=32 * blp + (rows - 32 * bl))
                    res[f"rank {g} slot {slot}: Q of block {blp}"] = _ratio(ref, b, rows, o2, l2)
                    break
    return res


def m_last_tile_dropped(ref, b, core):
    pl, later = _later(ref, core)
    res = {}
    for _, _, gp, g in later:
        r = pl.ranks[b][g]
        t = r.jend - 1
        rows = _rank_rows(ref, b, r)
        vis = vis_of(ref.inp.case, b)[rows].copy()
        seen = vis[:, 64 * t:].any(1) & vis[:, :64 * t].any(1)                   # rows that lose something and keep something
        if seen.any():
            vis[:, 64 * t:] = False
            o2, l2 = eval_rows(ref.inp, b, rows[seen], vis=vis[seen])
            res[f"rank {g}: tile {t} dropped"] = _ratio(ref, b, rows[seen], o2, l2)
    return res


def m_last_rank_dropped(ref, b, core):
    pl, _ = _later(ref, core)
    res = {}
    for w in pl.walks:
        if len(w) > 1:
            rows = _rank_rows(ref, b, pl.ranks[b][w[-1]])
            if len(rows):
                res[f"rank {w[-1]}: rows zero"] = _ratio(ref, b, rows, np.zeros((HB, len(rows), ref.case.Dh)), np.zeros((HB, len(rows))))
    return res


def m_neighbour(ref, b, core, what):
    """Head h + 1 / h - 1 of the sample (the other base head and another V scale) or sample b +- 1 (other data, the same scale): its K / V under
    this pair's Q and mask, or its output.  In units of head h: the mutant is (scale of the other head / scale of h) times the base result."""
    c, res = ref.case, {}
    rows = _live(ref, b, np.arange(7, c.Lq, max(1, c.Lq // 16)))
    o_ref, l_ref = eval_rows(ref.inp, b, rows)
    for h, dh in ((0, +1), (c.H - 1, -1)):
        rel = head_scale(h + dh) / head_scale(h)
        if what == "kv":
            o2, l2 = eval_rows(ref.inp, b, rows, kv=(b, [1, 0]))                  # index i: Q of base head i against K / V of the other one
        else:
            o2, l2 = o_ref[[1, 0]], l_ref[[1, 0]]
        res[f"{what} of head {h + dh} for head {h}"] = _ratio(ref, b, rows, *_only(h % HB, rel * o2, l2, o_ref, l_ref))
    if c.B > 1:
        for db in (+1, -1):
            b2 = (b + db) % c.B
            rows2 = rows[vis_of(ref.inp.case, b2)[rows].any(1)] if what == "output" else rows
            if what == "kv":
                o2, l2 = eval_rows(ref.inp, b, rows2, kv=(b2, [0, 1]))
            else:
                o2, l2 = eval_rows(ref.inp, b2, rows2)
            res[f"{what} of sample {b2} for sample {b}"] = _ratio(ref, b, rows2, o2, l2)
    return res


def blind_rows(inp, b, rows, m_ref):
    """What the blind softmax returns on `rows` against the reference maximum m_ref [HB, r] (log2 units): p = bf16(f32(exp2(s c - m_ref))),
    the row sum and O of the rounded p; f32 overflow and flushing included."""
    c = inp.case
    q, k, v = (a[b].double().numpy() for a in (inp.q, inp.k, inp.v))
    s = (q[:, rows] @ k.transpose(0, 2, 1)) * (c.scale * LOG2E)
    vis = vis_of(c, b)[rows]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = np.where(vis[None], np.exp2(s - m_ref[..., None]), 0.0).astype(np.float32)
        p[np.abs(p) < 2.0 ** -126] = 0.0
        p = torch.from_numpy(p).to(torch.bfloat16).double().numpy()
        l = p.sum(-1).astype(np.float32).astype(np.float64)
        o = (p @ v) / l[..., None]
        lse = (m_ref + np.log2(l)) / LOG2E
    return o, lse


def m_rise_not_walked_again(ref, b, core):
    """The blind result of a failed rank is taken as it is."""
    if ref.family != "rising":
        return {}
    c, res = ref.case, {}
    for hb_ in range(HB):
        rows = rise_rows(c, b, hb_)[:64]
        if len(rows):
            R = forward_rows(ref.inp, b, rows)
            o2, l2 = blind_rows(ref.inp, b, rows, R.m0 * LOG2E)
            res[f"base head {hb_}: blind result of rows {rows[0]}.."] = _ratio(ref, b, rows, *_only(hb_, o2, l2, R.o, R.lse))
    return res


def m_rise_stale_maximum(ref, b, core):
    """The rank after a failed rank runs blind against the reference maximum its wave's block had in the failed rank (the lifted scores)."""
    if ref.family != "rising":
        return {}
    c, res = ref.case, {}
    pl = walk_plan(c, "64")
    for hb_ in range(HB):
        fail = set(RISE[c.id]["fail"][b][hb_])
        for _, _, gp, g in later_walked(pl):
            rp, r = pl.ranks[b][gp], pl.ranks[b][g]
            hit = [(bl, blp) for bl, blp in zip(r.blocks, rp.blocks) if gp in fail and bl >= 0 and blp >= 0 and 32 * blp >= RISE[c.id]["min_row"]]
            if hit and not any(k.startswith(f"base head {hb_}:") for k in res):
                bl, blp = hit[0]
                rows, prow = _block_rows(c, bl), _block_rows(c, blp)
                n = min(len(rows), len(prow))
                rows, prow = rows[:n], prow[:n]
                Rp, R = forward_rows(ref.inp, b, prow), forward_rows(ref.inp, b, rows)
                stale = np.maximum(Rp.lse - np.log(np.maximum(Rp.n, 1))[None], Rp.m0) * LOG2E     # within log2 n of the failed rows' true maximum
                o2, l2 = blind_rows(ref.inp, b, rows, np.maximum(stale, R.m0 * LOG2E))
                res[f"base head {hb_}: rank {g} against the maximum of failed rank {gp}"] = _ratio(ref, b, rows, *_only(hb_, o2, l2, R.o, R.lse))
    return res


MUTATIONS = {
    "stale-tile:prev-last": lambda r, b, c: m_stale_tile(r, b, c, "prev-last"),
    "stale-tile:ring-stage": lambda r, b, c: m_stale_tile(r, b, c, "ring-stage"),
    "stale-q": m_stale_q,
    "last-tile-of-later-rank-dropped": m_last_tile_dropped,
    "last-rank-dropped": m_last_rank_dropped,
    "neighbour:kv": lambda r, b, c: m_neighbour(r, b, c, "kv"),
    "neighbour:output": lambda r, b, c: m_neighbour(r, b, c, "output"),
    "rising:failed-rank-not-walked-again": m_rise_not_walked_again,
    "rising:next-rank-with-failed-ranks-maximum": m_rise_stale_maximum,
}


def mutation_ratios(ref, b: int, core: str, names=None) -> dict:
    """{mutation: {label: ratio}} of sample b under the plan of `core`; ref: a Reference or a Ctx."""
    return {n: f(ref, b, core) for n, f in MUTATIONS.items() if names is None or n in names}
