"""Stop sequences: the shared tables and a pure-Python reference of the rule (aki_amd/stops.py states it).  No torch, no device.

The reference has a one-step form - stop_step / tick_step: state in, state out, what one launch of ops.stop_check / ops.slot_tick does -
and a whole-row form, first_stop.  The tables use an alphabet of 3 ids so that matches are frequent; tokens_ld is 12, or 40 for the one
case with a 32-id sequence."""
import itertools
import random

ALPHABET = 3
LD, LD_LONG = 12, 40
PAD = 0                              # what stands behind a row's t in the tables: the tail of row b - 1 lies in front of row b in memory


def match_at(row, t, seqs):
    """The lowest j such that seqs[j], of n <= t + 1 ids, equals row[t - n + 1 .. t]; -1 when there is none."""
    for j, s in enumerate(seqs):
        n = len(s)
        if 1 <= n <= t + 1 and list(row[t - n + 1:t + 1]) == list(s):
            return j
    return -1


def first_stop(row, eos, seqs):
    """The whole-row form: (the index of the token that ends the row, stop_hit) - the first t at which row[t] is an eos id (hit -1: EOS wins
    a tie) or a sequence of seqs matches (the lowest-numbered one); (None, -1) for a row that nothing ends."""
    eos = set(eos or ())
    for t in range(len(row)):
        if row[t] in eos:
            return t, -1
        j = match_at(row, t, seqs)
        if j >= 0:
            return t, j
    return None, -1


def cut(row, eos, seqs):
    """row cut behind its first finish (the matched sequence and the EOS stay)."""
    t, _ = first_stop(row, eos, seqs)
    return list(row) if t is None else list(row[:t + 1])


def stop_step(tokens, cache_len, start_len, done, done_at, stop_hit, sets, row_set):
    """One ops.stop_check: tokens [B][ld], the state lists [B], sets the pool's keys, row_set [B] -> new (done, done_at, stop_hit)."""
    done, done_at, stop_hit = list(done), list(done_at), list(stop_hit)
    for b in range(len(done)):
        t = cache_len[b] - start_len[b]
        if done[b] or not 0 <= t < len(tokens[b]):
            continue
        seqs = sets[row_set[b]] if 0 <= row_set[b] < len(sets) else ()
        j = match_at(tokens[b], t, seqs[:64])
        if j >= 0:
            done[b], done_at[b], stop_hit[b] = 1, t, j
    return done, done_at, stop_hit


def tick_step(done, done_at, cache_len, start_len, limit):
    """One ops.slot_tick -> new (done, done_at, cache_len)."""
    done, done_at, cache_len = list(done), list(done_at), list(cache_len)
    for b in range(len(done)):
        if not done[b]:
            generated = cache_len[b] - start_len[b] + 1
            if generated >= limit[b]:
                done[b], done_at[b] = 1, generated - 1
        if done[b] and done_at[b] >= 0:
            cache_len[b] = start_len[b] + done_at[b]
    return done, done_at, cache_len


# ---- the hand-written table: 16 rows at tokens_ld = 12 over one pool ------------------------------------------------------------------
LANE63 = tuple(itertools.islice(itertools.product(range(ALPHABET), repeat=4), 63)) + ((2, 2),)      # none of the first 63 is all 2s
LONG_SEQ = tuple((i * i + i // 3) % ALPHABET for i in range(32))
SETS = [(),                                  # 0: the empty set
        ((1,),),                             # 1: one id
        ((0, 1, 2),),                        # 2
        ((2, 1), (1,), (0, 2, 1)),           # 3: several can match at one t
        LANE63,                              # 4: 64 sequences, only the last one can match a run of 2s
        (LONG_SEQ,)]                         # 5: 32 ids


def _row(head, t, row_set, done=0, done_at=-1, limit=100, ld=LD, t_state=None):
    """tokens = head, padded with PAD; the state says the pick just wrote index t (t_state overrides it: an index outside the buffer)."""
    assert len(head) <= ld
    return dict(tokens=list(head) + [PAD] * (ld - len(head)), t=t if t_state is None else t_state, row_set=row_set, done=done, done_at=done_at,
                limit=limit)


ROWS = [
    _row([1, 1, 1], 2, 0),                                   # 0  the empty set: nothing
    _row([1, 1, 1], 2, 99),                                  # 1  a row_set past the pool: neutral
    _row([1, 1, 1], 2, -3),                                  # 2  a negative row_set: neutral
    _row([2, 2, 1, 0, 1], 4, 1, done=1, done_at=2),          # 3  a done row stays untouched (the fused tick parks it at start + 2)
    _row([1], 0, 1),                                         # 4  a one-id sequence at t = 0
    _row([1, 2], 1, 2),                                      # 5  n = t + 2: row 4's tail (PAD = 0) in front would complete (0, 1, 2) - no match
    _row([0, 1, 2], 2, 2, limit=3),                          # 6  n = t + 1 matches exactly; the budget ends at the same token: a stop
    _row([0, 1, 2, 2, 2, 2], 5, 4),                          # 7  64 sequences, only the last one matches: lane 63
    _row([0, 2, 1], 2, 3),                                   # 8  all three match at t = 2: the lowest index wins
    _row([1, 1], 1, 3),                                      # 9  (2, 1) does not match, (1,) does: hit 1
    _row([2, 0, 1], 2, 1, done=1, done_at=2),                # 10 the pick's EOS check ended it at this very t: stop_hit stays -1
    _row([0, 0, 0], 2, 3, limit=3),                          # 11 no match; the budget alone ends it (hit -1)
    _row([1] * LD, LD - 1, 1, t_state=LD),                   # 12 t == tokens_ld: skipped
    _row([1, 1], 0, 1, t_state=-1),                          # 13 t < 0: skipped
    _row([1, 0], 1, 1),                                      # 14 a match at an earlier index only: the check looks at t alone
    _row([2, 2, 2, 0, 1, 2], 5, 2),                          # 15 a match in the middle of the buffer
]
LONG_ROW = _row(list(LONG_SEQ), 31, 5, ld=LD_LONG)           # a 32-id sequence at t = 31
SUBSETS = {16: list(range(16)), 5: [6, 3, 11, 5, 8], 1: [6]}     # B -> the rows of the table (row 5 keeps a PAD tail in front of it)


def table_state(rows, start0=7):
    """The device-side state of `rows` as Python lists: (tokens, cache_len, start_len, done, done_at, stop_hit, row_set, limit)."""
    start = [start0 + 3 * b for b in range(len(rows))]
    return ([list(r["tokens"]) for r in rows], [s + r["t"] for s, r in zip(start, rows)], start, [r["done"] for r in rows],
            [r["done_at"] for r in rows], [-1] * len(rows), [r["row_set"] for r in rows], [r["limit"] for r in rows])


# ---- random rows --------------------------------------------------------------------------------------------------------------------
def random_sets(rng, n_sets=4, max_seqs=5, max_len=4):
    """n_sets random non-empty sets over the alphabet (duplicates inside a set are allowed: the lower index wins)."""
    return [tuple(tuple(rng.randrange(ALPHABET) for _ in range(rng.randint(1, max_len))) for _ in range(rng.randint(1, max_seqs)))
            for _ in range(n_sets)]


def random_rows(seed, B, ld=LD):
    """(tokens [B][ld], sets with the empty set in front, row_set [B]) drawn from the small alphabet."""
    rng = random.Random(seed)
    sets = [()] + random_sets(rng)
    tokens = [[rng.randrange(ALPHABET) for _ in range(ld)] for _ in range(B)]
    return tokens, sets, [rng.randrange(len(sets)) for _ in range(B)]
