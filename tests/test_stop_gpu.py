"""Stop sequences on the GPU, op level: ops.stop_check against the one-step reference of stop_cases, bit for bit on done, done_at and stop_hit
with cache_len and the tokens untouched; ops.slot_tick(stops=...) against stop_check followed by the plain slot_tick on every state array;
the refusals."""
import pytest
import torch

import stop_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _stops(sets, row_set):
    """An ops.StopSets over `sets` with the rows' places filled in: the pool deduplicates by value, so a place in `sets` is mapped through
    its index; a place outside `sets` is outside the pool too and stays as it is."""
    from aki_amd import ops
    st = ops.StopSets(DEV, sets, len(row_set))
    assert len(st.keys) <= max(len(sets), 1) + 1
    placed = [st.index[tuple(sets[r])] if 0 <= r < len(sets) else r for r in row_set]
    assert all(not 0 <= r < len(st.keys) for r, q in zip(placed, row_set) if not 0 <= q < len(sets))
    st.row_set.copy_(torch.tensor(placed, dtype=torch.int32))
    return st


def _upload(state, guard_front=None):
    """The lists of stop_cases.table_state as device tensors.  guard_front: ids that lie right in front of row 0 in memory."""
    tokens, cache_len, start_len, done, done_at, stop_hit, row_set, limit = state
    B, ld = len(tokens), len(tokens[0])
    flat = torch.zeros(ld + B * ld, dtype=torch.long, device=DEV)
    if guard_front is not None:
        flat[ld - len(guard_front):ld] = torch.tensor(guard_front, dtype=torch.long, device=DEV)
    tok = flat[ld:].view(B, ld)
    tok.copy_(torch.tensor(tokens, dtype=torch.long))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    return flat, tok, i32(cache_len), i32(start_len), torch.tensor(done, dtype=torch.uint8, device=DEV), i32(done_at), i32(limit)


def _check_stop_check(state, sets, guard_front=None):
    from aki_amd import ops
    tokens, cache_len, start_len, done, done_at, stop_hit, row_set, _ = state
    want = sc.stop_step(tokens, cache_len, start_len, done, done_at, stop_hit, sets, row_set)
    flat, tok, d_len, d_start, d_done, d_at, _ = _upload(state, guard_front)
    keep = (flat.clone(), d_len.clone(), d_start.clone())
    st = _stops(sets, row_set)
    placed = st.row_set.clone()
    ops.stop_check(tok, d_len, d_start, d_done, d_at, st)
    got = (d_done.tolist(), d_at.tolist(), st.stop_hit.tolist())
    for name, g, w in zip(("done", "done_at", "stop_hit"), got, want):
        assert g == list(w), (name, g, list(w))
    assert torch.equal(flat, keep[0]) and torch.equal(d_len, keep[1]) and torch.equal(d_start, keep[2])
    assert torch.equal(st.row_set, placed)
    return got


@pytest.mark.parametrize("B", [1, 5, 16])
def test_stop_check_matches_the_reference_on_the_table(B):
    rows = [sc.ROWS[i] for i in sc.SUBSETS[B]]
    done, done_at, hit = _check_stop_check(sc.table_state(rows), sc.SETS)
    if B == 16:                                                 # the table's cases, spelled out
        assert hit == [-1, -1, -1, -1, 0, -1, 0, 63, 0, 1, -1, -1, -1, -1, -1, 0]
        assert done == [0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1]
        assert done_at == [-1, -1, -1, 2, 0, -1, 2, 5, 2, 1, 2, -1, -1, -1, -1, 5]


def test_stop_check_never_walks_out_of_row_0():
    """n = t + 2 in row 0: the ids right in front of the buffer would complete the match."""
    done, _, hit = _check_stop_check(sc.table_state([sc.ROWS[5]]), sc.SETS, guard_front=[2, 1, 0])
    assert done == [0] and hit == [-1]
    done, _, hit = _check_stop_check(sc.table_state([sc.ROWS[6]]), sc.SETS, guard_front=[2, 1, 0])      # n = t + 1 does match
    assert done == [1] and hit == [0]


def test_stop_check_a_32_id_sequence_at_t_31():
    done, done_at, hit = _check_stop_check(sc.table_state([sc.LONG_ROW]), sc.SETS)
    assert (done, done_at, hit) == ([1], [31], [0])
    short = dict(sc.LONG_ROW, t=30)                             # one token earlier the sequence is longer than the row's history
    assert _check_stop_check(sc.table_state([short]), sc.SETS)[0] == [0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_stop_check_matches_the_reference_on_random_rows(seed):
    """Whole rows walked token by token: the state after every launch equals the reference's, and the end equals first_stop."""
    from aki_amd import ops
    B = 16
    tokens, sets, row_set = sc.random_rows(seed, B)
    start = [5 + b for b in range(B)]
    st = _stops(sets, row_set)
    state = (tokens, list(start), start, [0] * B, [-1] * B, [-1] * B, row_set, [100] * B)
    _, tok, d_len, d_start, d_done, d_at, _ = _upload(state)
    done, done_at, hit = [0] * B, [-1] * B, [-1] * B
    for t in range(sc.LD):
        d_len.copy_(d_start + t)
        ops.stop_check(tok, d_len, d_start, d_done, d_at, st)
        done, done_at, hit = sc.stop_step(tokens, [s + t for s in start], start, done, done_at, hit, sets, row_set)
        assert (d_done.tolist(), d_at.tolist(), st.stop_hit.tolist()) == (done, done_at, hit), t
    for b in range(B):
        t, j = sc.first_stop(tokens[b], (), sets[row_set[b]])
        assert (done[b], done_at[b], hit[b]) == ((1, t, j) if t is not None else (0, -1, -1)), b
    assert 0 < sum(done) and any(h > 0 for h in hit)


@pytest.mark.parametrize("B", [1, 5, 16])
def test_fused_tick_equals_stop_check_then_slot_tick(B):
    from aki_amd import ops
    rows = [sc.ROWS[i] for i in sc.SUBSETS[B]]
    state = sc.table_state(rows)
    tokens, cache_len, start_len, done, done_at, stop_hit, row_set, limit = state
    # the reference of the pair, and the pair itself on the device
    w_done, w_at, w_hit = sc.stop_step(tokens, cache_len, start_len, done, done_at, stop_hit, sc.SETS, row_set)
    w_done, w_at, w_len = sc.tick_step(w_done, w_at, cache_len, start_len, limit)
    _, tok, a_len, a_start, a_done, a_at, a_limit = _upload(state)
    st_a = _stops(sc.SETS, row_set)
    ops.stop_check(tok, a_len, a_start, a_done, a_at, st_a)
    ops.slot_tick(a_done, a_at, a_len, a_start, a_limit)
    flat, tok, f_len, f_start, f_done, f_at, f_limit = _upload(state)
    keep = (flat.clone(), f_start.clone(), f_limit.clone())
    st_f = _stops(sc.SETS, row_set)
    ops.slot_tick(f_done, f_at, f_len, f_start, f_limit, stops=st_f, tokens=tok)
    fused = (f_done.tolist(), f_at.tolist(), f_len.tolist(), st_f.stop_hit.tolist())
    assert fused == (a_done.tolist(), a_at.tolist(), a_len.tolist(), st_a.stop_hit.tolist())
    assert fused == (w_done, w_at, w_len, w_hit)
    assert torch.equal(flat, keep[0]) and torch.equal(f_start, keep[1]) and torch.equal(f_limit, keep[2])
    by_row = dict(zip(sc.SUBSETS[B], zip(*fused)))
    assert by_row[6] == (1, 2, by_row[6][2], 0)                 # a stop and the budget at the same token is a stop
    if B > 1:
        i = sc.SUBSETS[B].index(3)
        assert by_row[3] == (1, 2, start_len[i] + 2, -1)        # the parked row: back on the cache row of the token it never fed
        assert by_row[11][0] == 1 and by_row[11][3] == -1       # the budget alone


def test_fused_tick_on_random_states():
    from aki_amd import ops
    for seed in range(4):
        B = (1, 5, 16, 16)[seed]
        tokens, sets, row_set = sc.random_rows(10 + seed, B)
        g = torch.Generator().manual_seed(seed)
        t = torch.randint(0, sc.LD, (B,), generator=g).tolist()
        limit = [int(x) for x in torch.randint(1, sc.LD + 2, (B,), generator=g)]
        done = [int(x) for x in torch.randint(0, 4, (B,), generator=g) == 0]
        done_at = [max(0, ti - 1) if d else -1 for d, ti in zip(done, t)]
        start = [9 + 2 * b for b in range(B)]
        state = (tokens, [s + ti for s, ti in zip(start, t)], start, done, done_at, [-1] * B, row_set, limit)
        w_done, w_at, w_hit = sc.stop_step(tokens, state[1], start, done, done_at, [-1] * B, sets, row_set)
        w_done, w_at, w_len = sc.tick_step(w_done, w_at, state[1], start, limit)
        _, tok, d_len, d_start, d_done, d_at, d_limit = _upload(state)
        st = _stops(sets, row_set)
        ops.slot_tick(d_done, d_at, d_len, d_start, d_limit, stops=st, tokens=tok)
        assert (d_done.tolist(), d_at.tolist(), d_len.tolist(), st.stop_hit.tolist()) == (w_done, w_at, w_len, w_hit), seed


def test_stop_sets_admit_and_row_views():
    from aki_amd import ops
    a, b = ((1,),), ((0, 1, 2),)
    st = ops.StopSets(DEV, [a, (), b, a], 3)
    assert st.keys == [(), a, b] and st.row_set.tolist() == [0, 0, 0] and st.stop_hit.tolist() == [-1, -1, -1]
    ptrs = (st.row_set.data_ptr(), st.stop_hit.data_ptr())
    st.stop_hit.fill_(5)
    st.admit(1, b)
    st.admit(2, ())
    assert st.row_set.tolist() == [0, 2, 0] and st.stop_hit.tolist() == [5, -1, -1]
    assert (st.row_set.data_ptr(), st.stop_hit.data_ptr()) == ptrs                 # in place: a captured step holds the addresses
    one = st.row(1)
    tok = torch.tensor([[0, 1, 2, 0]], dtype=torch.long, device=DEV)
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32, device=DEV)
    done, at = torch.zeros(1, dtype=torch.uint8, device=DEV), i32(-1)
    ops.stop_check(tok, i32(9), i32(7), done, at, one)
    assert done.tolist() == [1] and at.tolist() == [2] and st.stop_hit.tolist() == [5, 0, -1]      # the view writes the slot's own entry


def test_refusals():
    from aki_amd import ops

    def mk(n, ld=4):
        return dict(tokens=torch.zeros((n, ld), dtype=torch.long, device=DEV), cache_len=torch.ones(n, dtype=torch.int32, device=DEV),
                    start_len=torch.ones(n, dtype=torch.int32, device=DEV), done=torch.zeros(n, dtype=torch.uint8, device=DEV),
                    done_at=torch.full((n,), -1, dtype=torch.int32, device=DEV))

    st = lambda n: ops.StopSets(DEV, [((1,),)], n)
    ops.stop_check(stops=st(20), **mk(20))                      # stop_check takes any number of rows
    bad = []
    for name in ("tokens", "cache_len", "start_len", "done", "done_at"):
        a = mk(4)
        a[name] = a[name].cpu()
        bad.append((a, st(4)))                                  # CPU tensors
    for name, dt in (("tokens", torch.int32), ("cache_len", torch.int64), ("done", torch.bool), ("done_at", torch.int64)):
        a = mk(4)
        a[name] = a[name].to(dt)
        bad.append((a, st(4)))                                  # wrong dtypes
    a = mk(4)
    a["tokens"] = a["tokens"][:3]
    bad.append((a, st(4)))                                      # shapes
    a = mk(4, 8)
    a["tokens"] = a["tokens"][:, ::2]
    bad.append((a, st(4)))                                      # contiguity
    bad.append((mk(4), st(3)))                                  # a StopSets of another row count
    bad.append((mk(4), None))
    s = st(4)
    s.row_set = s.row_set.long()
    bad.append((mk(4), s))
    s = st(4)
    s.stop_hit = s.stop_hit.cpu()
    bad.append((mk(4), s))
    for i, (a, s) in enumerate(bad):
        with pytest.raises(ops.AkiError):
            ops.stop_check(stops=s, **a)
            pytest.fail(f"refusal {i} went through")
    # the fused form: the tick's own refusals, B above SLOT_MAX_ROWS, and tokens without stops
    lim = lambda n: torch.ones(n, dtype=torch.int32, device=DEV)
    a = mk(16)
    ops.slot_tick(a["done"], a["done_at"], a["cache_len"], a["start_len"], lim(16), stops=st(16), tokens=a["tokens"])
    a = mk(ops.SLOT_MAX_ROWS + 1)
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a["done"], a["done_at"], a["cache_len"], a["start_len"], lim(17), stops=st(17), tokens=a["tokens"])
    a = mk(4)
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a["done"], a["done_at"], a["cache_len"], a["start_len"], lim(4), stops=st(4), tokens=a["tokens"].int())
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a["done"], a["done_at"], a["cache_len"], a["start_len"], lim(4), stops=st(4), tokens=a["tokens"].cpu())
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a["done"], a["done_at"], a["cache_len"], a["start_len"], lim(4), stops=st(4))
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a["done"], a["done_at"], a["cache_len"], a["start_len"], lim(4), tokens=a["tokens"])
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a["done"], a["done_at"].long(), a["cache_len"], a["start_len"], lim(4), stops=st(4), tokens=a["tokens"])
