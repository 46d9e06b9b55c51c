"""Case table, inputs, references and reference mutations of min_p and the frequency / presence penalties (aki_amd/csrc/decode.hip:
stage 1b of process_row and the min_p compare of the sampler's draw; C entries aki_*_penalized; ops.LogitsProcessors, ops.sample_pick).

numpy only, on top of tests/sampling_cases.py (S): the logits rows, the Philox draws, the top-k / top-p reference and the acceptance of
a drawn token (S.accepted with its derived S.DELTA) are S's, unchanged.  tests/test_penalty_cases_cpu.py checks the table itself and
tests/test_penalty_gpu.py runs every case on the device.

The references.
  stage 1b  (`scores`) the f32 restatement, bit-exact: for every distinct token g of the history h[0, n) with 0 <= g < V and c
            occurrences, after the repetition penalty and before every ban,
              x = x - fl(frequency * f32(c))   when frequency != 0        (one rounded f32 product, one rounded f32 difference)
              x = x - presence                 when presence != 0         (one rounded f32 difference)
            A done row keeps the plain copy; -inf stays -inf.
  min_p     (`reference`) float64: among the tokens top-k / top-p kept (S.reference), keep iff
              exp(y64 - ymax64) >= float64(float32(min_p)),  y = f32(x / T).
            This is HF MinPLogitsWarper's probs < min_p * probs.max(): the normaliser cancels.  The maximum always stays.

The condition on the inputs that min_p adds (find_salt enforces it, with S.conditions_hold's own): no survivor of top-k / top-p lies
within relative MINP_MARGIN = 1e-5 of the min_p boundary.  The device's expf carries 2 eps and |y - max| eps of argument rounding
(eps = 2^-24); exp(y - max) >= 1e-7 means |y - max| <= 16.2, so the relative error of a weight near any boundary a case can have is
below 18.2 * 2^-24 = 1.1e-6, and the margin is 8x that (the factor S uses for its top-p boundary).  Tokens with y == max are exempt:
their weight is exp(0) = 1 exactly in every arithmetic, which is what lets min_p = 1 keep tied maxima.  The share of draws with more
than one acceptable token stays at most 0.02 on every case that filters with min_p.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import sampling_cases as S

MINP_MARGIN = 1e-5
MINP_MULTI_LIMIT = 0.02
MINP_MUTATIONS = ("minp_of_total", "minp_before_topp", "minp_strict")
PENALTY_MUTATIONS = ("count_as_presence", "presence_everywhere", "before_repetition")
MUTATIONS = MINP_MUTATIONS + PENALTY_MUTATIONS
DONE_ROWS = (2, 5)                   # the rows of a `done` case that are finished before the launch


@dataclass
class Case(S.Case):
    """S.Case (its `penalty` is the repetition penalty over `history`) with min_p, the two additive penalties, and
    full: the history fills the token buffer (tokens_ld == len(history)); done: rows DONE_ROWS are finished before the launch."""
    min_p: float = 0.0
    frequency: float = 0.0
    presence: float = 0.0
    full: bool = False
    done: bool = False

    @property
    def processed(self) -> bool:
        return self.penalty != 1.0 or bool(self.suppress) or self.frequency != 0.0 or self.presence != 0.0

    @property
    def penalized(self) -> bool:
        return self.frequency != 0.0 or self.presence != 0.0


def logits(c: Case) -> np.ndarray:
    """S.logits, plus the kind "max_ties": five more columns hold the row's maximum."""
    if c.kind != "max_ties":
        return S.logits(c)
    x = S.logits(Case(c.name, c.V, c.sigma, c.T, c.k, c.p, salt=c.salt))
    g = np.random.default_rng([7, c.salt])
    idx = g.choice(c.V, 5, replace=False)
    x[idx] = x.max()
    return x


def scores(c: Case, x: Optional[np.ndarray] = None, mutation: Optional[str] = None) -> np.ndarray:
    """The processed f32 row of a live row: repetition penalty, stage 1b, then the suppressed ids to -inf.  Every step is one f32
    operation on numpy float32 arrays, so the result is what the kernel computes, bit for bit."""
    f = np.float32
    x = (logits(c) if x is None else x).astype(f).copy()
    h = np.asarray(c.history, np.int64)
    ids, cnt = np.unique(h[(h >= 0) & (h < c.V)], return_counts=True)

    def repetition(x):
        if c.penalty != 1.0 and len(ids):
            x[ids] = np.where(x[ids] < 0, x[ids] * f(c.penalty), x[ids] / f(c.penalty)).astype(f)

    def additive(x):
        if c.frequency != 0.0 and len(ids):
            n = np.ones_like(cnt) if mutation == "count_as_presence" else cnt
            x[ids] = x[ids] - (f(c.frequency) * n.astype(f)).astype(f)
        if c.presence != 0.0:
            if mutation == "presence_everywhere":
                x[:] = x - f(c.presence)
            elif len(ids):
                x[ids] = x[ids] - f(c.presence)

    if mutation == "before_repetition":
        additive(x)
        repetition(x)
    else:
        repetition(x)
        additive(x)
    if c.suppress:
        x[list(c.suppress)] = -np.inf
    return x


@dataclass
class Facts:
    minp_gap: float                  # the smallest | exp(y - max) / min_p - 1 | over the top-k / top-p survivors with y < max
    multi: float                     # the share of the case's draws with more than one acceptable token
    kept: int


def _weights(r: S.Ref):
    y64 = r.y.astype(np.float64)
    return np.exp(y64 - y64.max())


def reference(c: Case, x: Optional[np.ndarray] = None, mutation: Optional[str] = None) -> S.Ref:
    """S.reference (temperature, top-k, top-p) on the processed row, then min_p; a Ref over the set that remains."""
    x = scores(c) if x is None else x
    base = S.reference(c, x)
    mp = np.float64(np.float32(c.min_p))
    if not mp > 0.0:
        return base
    w = _weights(base)
    if mutation == "minp_before_topp":             # min_p among top-k's survivors first, top-p over what it leaves
        only_k = S.reference(Case(c.name, c.V, c.sigma, c.T, c.k, 1.0, salt=c.salt), x)
        masked = np.where(only_k.kept & (w >= mp), x, -np.inf).astype(np.float32)
        return S.reference(c, masked)
    if mutation == "minp_of_total":                # an epsilon cutoff: the threshold against the total, not against the maximum
        stay = base.probs >= mp
    elif mutation == "minp_strict":
        stay = w > mp
    else:
        stay = w >= mp
    kept = base.kept & stay
    wk = np.where(kept, w, 0.0)
    total = wk.sum()
    probs = wk / total if total > 0 else wk
    y64 = base.y.astype(np.float64)
    return S.Ref(base.y, kept, probs, np.cumsum(probs), base.boundary_gap, base.boundary_multiplicity,
                 float((probs * np.where(probs > 0, y64.max() - y64, 0.0)).sum()))


def facts(c: Case, x: Optional[np.ndarray] = None) -> Facts:
    x = scores(c) if x is None else x
    base, r = S.reference(c, x), reference(c, x)
    gap = float("inf")
    mp = np.float64(np.float32(c.min_p))
    if mp > 0.0:
        w = _weights(base)
        below_max = base.kept & (base.y < base.y.max())
        if below_max.any():
            gap = float(np.abs(w[below_max] / mp - 1.0).min())
    multi = float((S.accept_set_sizes(r, S.uniform(*S.draws(c))) > 1).mean())
    return Facts(gap, multi, int(r.kept.sum()))


def base_conditions_hold(c: Case, x: Optional[np.ndarray] = None) -> bool:
    """S.conditions_hold's rule, restated over the row the case's own processors make (S's takes no row: it knows the repetition
    penalty and the suppressed ids only).  On a case without the additive penalties it is S.conditions_hold(c)[0] - the CPU test
    asserts that."""
    x = scores(c) if x is None else x
    r = S.reference(c, x)
    multi = float((S.accept_set_sizes(r, S.uniform(*S.draws(c))) > 1).mean())
    kept = int(r.kept.sum())
    limit = 0.02 if kept <= 1000 else 0.15 if not c.filtered else 1.0
    unique_max = int((r.y == r.y.max()).sum()) == 1
    return bool(r.boundary_gap > 8 * S.DELTA and multi <= limit and r.mean_gap <= S.MAX_MEAN_GAP and (unique_max or (c.p > 1e-5 and c.k != 1)))


def conditions_hold(c: Case):
    """(ok, Facts): S's conditions, and min_p's: the boundary margin, and at most MINP_MULTI_LIMIT of the draws ambiguous."""
    x = scores(c)
    f = facts(c, x)
    ok = base_conditions_hold(c, x) and (c.min_p <= 0.0 or (f.minp_gap > MINP_MARGIN and f.multi <= MINP_MULTI_LIMIT))
    return ok, f


def find_salt(c: Case) -> Case:
    for salt in range(64):
        c.salt = salt
        if conditions_hold(c)[0]:
            return c
    raise AssertionError(f"no salt below 64 gives {c.name} a row that meets the conditions")


def history(c: Case) -> np.ndarray:
    """The token buffer of one row, int64 [tokens_ld]: the history, then (unless it fills the buffer) S.STEPS columns the draws of the
    case write to, pre-filled with an id outside [0, V) so that what a pick appends never changes a count."""
    h = np.asarray(c.history, np.int64)
    return h if c.full else np.concatenate([h, np.full(S.STEPS, c.V + 7, np.int64)])


# a history with a token occurring once (3), twice (10), six times (20), two ids outside [0, V) and 26 distinct others: 37 entries
def _hist37(V: int) -> Tuple[int, ...]:
    return (3, 10, 20, 20, V + 5, 10, 20) + tuple(range(100, 126)) + (20, -1, 20, 20)


def _table():
    out = []
    kp = ((0, 1.0), (50, 0.9), (1000, 0.5))
    for sigma in (2.0, 4.0):
        for T in (0.7, 1.0, 1.3):
            for k, p in kp:
                for mp in (0.02, 0.1, 0.5):
                    out.append(Case(f"minp-s{sigma:g}-T{T:g}-k{k}-p{p:g}-m{mp:g}", S.V_MAIN, sigma, T, k, p, min_p=mp))
    for k, p in kp:
        for mp in (0.02, 0.1, 0.5):
            out.append(Case(f"minp-small-k{k}-p{p:g}-m{mp:g}", S.V_SMALL, 2.0, 0.7, k, p, min_p=mp))
    out.append(Case("minp-one-ties", S.V_MAIN, 2.0, 1.0, 0, 1.0, kind="max_ties", min_p=1.0))
    out.append(Case("minp-one-ties-small", S.V_SMALL, 2.0, 1.3, 50, 0.9, kind="max_ties", min_p=1.0))
    out.append(Case("minp-zero", S.V_MAIN, 2.0, 1.0, 50, 0.9, min_p=0.0))
    out.append(Case("minp-neginf", S.V_MAIN, 2.0, 1.0, 0, 1.0, kind="neg_inf", min_p=0.1))
    out.append(Case("minp-proc", S.V_MAIN, 2.0, 1.3, 50, 0.9, penalty=1.3, history=tuple(range(5, 3000, 7)),
                    suppress=tuple(range(100, 4000, 3)), min_p=0.1))
    V = S.V_SMALL
    h37 = _hist37(V)
    pen = dict(V=V, sigma=2.0, T=1.0, k=50, p=0.9)
    out.append(Case("pen-h0", history=(), frequency=0.5, presence=0.5, **pen))
    out.append(Case("pen-h1", history=(17,), frequency=0.5, presence=0.5, **pen))
    out.append(Case("pen-h37-frequency", history=h37, frequency=0.7, **pen))
    out.append(Case("pen-h37-presence", history=h37, presence=1.1, **pen))
    out.append(Case("pen-h37-both-rep", history=h37, frequency=0.3, presence=0.6, penalty=1.3, **pen))
    out.append(Case("pen-h37-negative", history=h37, frequency=-0.7, presence=-1.5, **pen))
    out.append(Case("pen-h37-suppressed", history=h37, frequency=0.9, presence=0.4, suppress=(20, 101, 500), **pen))
    out.append(Case("pen-h37-done", history=h37, frequency=0.9, presence=0.4, penalty=1.3, done=True, **pen))
    out.append(Case("pen-full", history=tuple((i * i) % 97 for i in range(64)), frequency=0.25, presence=0.75, penalty=1.3, full=True, **pen))
    out.append(Case("pen-main-minp", S.V_MAIN, 2.0, 0.7, 0, 1.0, history=tuple((i * 37) % 911 for i in range(1500)) + (S.V_MAIN + 1,),
                    frequency=0.4, presence=0.2, penalty=1.3, min_p=0.1))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = [find_salt(c) for c in _table()]
    return _CASES


def minp_cases():
    return [c for c in cases() if c.name.startswith("minp")]


def penalty_cases():
    return [c for c in cases() if c.name.startswith("pen")]
