"""Case tables and the numpy reference of per-request token constraints in generate_many (aki_amd/constraint.py: ConstraintPool;
ops.SlotConstraints; the per-row constrained picks aki_greedy_pick_constrained_rows / aki_sample_pick_rows_constrained in
aki_amd/csrc/decode.hip).  numpy only; tests/test_many_constraint_cpu.py checks this file, tests/test_many_constraint_gpu.py runs it
on the device.

The reference works on a POOL: the `with_eos` tables of several constraints one behind the other, int32 [rows, V], -1 = not allowed,
states NOT renumbered.  A row is (base, n, s): its table is pool[base : base + n], its state s is local to that table.
  mask(pool, base, n, s)          bool [V], the tokens the row's state allows - or None: the row is left untouched (s outside [0, n),
                                  or base + s outside the pool)
  pick(pool, base, n, s, x, ...)  the greedy pick's (token, next state): the allowed token with the largest score, the LOWEST id among
                                  equal maxima; an untouched row takes the plain argmax and the next state -1; a finished row pad and s
  walk(pool, base, n, start, toks)  the local states a token row passes through, -1 from the first token that is not allowed
"""
import numpy as np

from aki_amd.constraint import TokenConstraint

EOS = (0, 2)
PAD = 1


def mask(pool: np.ndarray, base: int, n: int, s: int):
    if not 0 <= s < n or not 0 <= base + s < pool.shape[0] or base < 0:
        return None
    return pool[base + s] >= 0


def pick(pool: np.ndarray, base: int, n: int, s: int, x: np.ndarray, done: bool = False, pad: int = PAD):
    if done:
        return pad, s
    m = mask(pool, base, n, s)
    x = np.asarray(x, dtype=np.float64)
    if m is None:
        return int(np.argmax(x)), -1
    tok = int(np.argmax(np.where(m, x, -np.inf)))             # the first of equal maxima, as the pick
    return tok, int(pool[base + s, tok])


def walk(pool: np.ndarray, base: int, n: int, start: int, toks) -> list:
    out, s = [int(start)], int(start)
    for t in toks:
        m = mask(pool, base, n, s)
        s = int(pool[base + s, int(t)]) if m is not None else -1
        out.append(s)
    return out


def greedy(pool: np.ndarray, base: int, n: int, start: int, scores: np.ndarray, eos, pad: int):
    """constraint_cases.greedy over a pool row: scores [steps, V] -> (tokens, states [steps + 1], done_at or -1)."""
    toks, states, s, done_at = [], [int(start)], int(start), -1
    for t in range(scores.shape[0]):
        tok, s = pick(pool, base, n, s, scores[t], done_at >= 0, pad)
        toks.append(tok)
        states.append(s)
        if done_at < 0 and tok in eos:
            done_at = t
    return toks, states, done_at


def cycle(V: int, n: int, first: int, width: int, accepting=()) -> TokenConstraint:
    """n states in a ring: state i allows the `width` tokens from first + i * width on and goes to state (i + 1) % n.  Every state allows
    something, so the automaton needs no eos id."""
    nxt = np.full((n, V), -1, dtype=np.int32)
    for i in range(n):
        nxt[i, first + i * width: first + (i + 1) * width] = (i + 1) % n
    acc = np.zeros(n, dtype=bool)
    acc[list(accepting)] = True
    return TokenConstraint.from_table(nxt, acc, 0)


# ---- the row table of the op-level tests -------------------------------------------------------------------------------------------------
def members(V: int):
    """Three automata over any V >= 8 that touch the first and the last columns and never use an eos id (EOS) as a transition:
    A  a trie (constraint_cases' shape): root {V-1, 3, 4}, behind V-1 {1, V-2}, accepting leaves allow the eos ids only
    B  a ring of three states {1, 3} -> {4, 5} -> {V-2, V-1} -> back; the last one accepts (the eos ids are allowed there too)
    C  a two-choice trie ((5, 6), (6,))"""
    a = TokenConstraint.from_choices(((V - 1, 1), (V - 1, V - 2, 5), (3, 3, 3, 3), (4,)), V)
    nxt = np.full((3, V), -1, dtype=np.int32)
    nxt[0, [1, 3]], nxt[1, [4, 5]], nxt[2, [V - 2, V - 1]] = 1, 2, 0
    b = TokenConstraint.from_table(nxt, [False, False, True], 0)
    c = TokenConstraint.from_choices(((5, 6), (6,)), V)
    return a, b, c


# (member index or None, the row's state, its generated-token index t, finished): two rows in A in different states, one in B (an accepting
# state), one in C, one unconstrained row (state -1, no table), one finished row
ROWS = [(0, 0, 0, False), (0, 1, 2, False), (1, 2, 5, False), (2, 1, 1, False), (None, -1, 3, False), (0, 1, 4, True)]
ROW_START = [7, 3, 0, 5, 1, 2]                                 # start_len of every row: the index is cache_len + advance - start_len
HISTORY = 8                                                    # columns of the state history: every t + 1 above fits


def row_scores(V: int, pool: np.ndarray, placed, seed: int = 0) -> np.ndarray:
    """f32 scores [rows, V] (values a bf16 holds exactly are not needed: the device test rounds them first and hands the rounded values
    back).  Random weights; for every constrained row the global argmax is put on a column its state does NOT allow."""
    rng = np.random.Generator(np.random.PCG64(seed + V))
    x = rng.standard_normal((len(ROWS), V)).astype(np.float32) * 2
    for b, ((mem, s, _, _), (base, n)) in enumerate(zip(ROWS, placed)):
        m = mask(pool, base, n, s)
        if m is not None:
            x[b, int(np.flatnonzero(~m)[0])] = 9.0
    return x


def place(tables, order=(0, 1, 2)):
    """The pool of the members' tables in `order`, and (base, n) per row of ROWS ((0, 0) for the unconstrained row)."""
    base, off = {}, 0
    for i in order:
        base[i] = off
        off += tables[i].shape[0]
    pool = np.concatenate([tables[i] for i in order], axis=0)
    return pool, [(0, 0) if mem is None else (base[mem], tables[mem].shape[0]) for mem, *_ in ROWS]


# ---- the request pattern of the end-to-end tests (the tiny model of tests/test_slots_gpu.py: 7 requests, BUDGETS, 3 slots) --------------
BUDGETS = [12, 1, 5, 12, 3, 9, 12]                             # tests/test_slots_gpu.py's, restated: this file imports no torch
SLOTS = 3
PATTERN = ["A", "B", "C", None, "A", None, "B"]                # request -> its constraint; requests 0 and 4, 1 and 6 share one OBJECT


def request_constraints(V: int):
    """The 7 requests' constraints for an eos-free run: rings, so every state allows something.  Equal letters are the same object."""
    made = {"A": cycle(V, 4, 100, 5), "B": cycle(V, 3, 1000, 3), "C": cycle(V, 5, 20000, 2)}
    return [None if k is None else made[k] for k in PATTERN]


CHOICES = [((11, 12), (13,)), ((21,), (22, 23, 24)), ((31, 32, 33),), ((41,), (42,)), ((51, 52), (53, 54)), ((61,),), ((71, 72, 73, 74), (75,))]
CHOICE_BUDGET = 8                                              # every choice and its eos fit with room to spare: the rows retire early


def choice_constraints(V: int):
    """One from_choices trie per request; no choice is a prefix of another, so behind a choice only the eos id is allowed."""
    return [TokenConstraint.from_choices(ch, V) for ch in CHOICES]


def slot_history(budgets=BUDGETS, slots=SLOTS, period=8):
    """SlotScheduler's own loop over a fake token source (a request of n tokens: token 0 at its admit, one per step): per slot, the
    requests it served in order."""
    from aki_amd.slots import SlotScheduler
    sched = SlotScheduler(len(budgets), slots, period)
    request, generated, served = [None] * slots, [0] * slots, [[] for _ in range(slots)]

    def admit(req, slot):
        request[slot], generated[slot] = req, 1
        served[slot].append(req)
        return budgets[req] == 1

    def step(n):
        for s in range(slots):
            if request[s] is not None:
                generated[s] = min(generated[s] + n, budgets[request[s]])

    def look():
        return [request[s] is None or generated[s] >= budgets[request[s]] for s in range(slots)], [g - 1 for g in generated]

    def retire(req, slot, n):
        request[slot] = None

    sched.run(admit, step, look, retire)
    return served
