"""Stop sequences, the parts that need no GPU: stops.first_finish on CPU tensors against the pure-Python reference (stop_cases), the
refusals of check_stop_sequences, the None / () precedence, the StopPool layout, a SlotScheduler run whose rows end at their first stop, and
the keyword parsing."""
import random
import types

import pytest
import torch

import stop_cases as sc
from aki_amd.slots import RequestParams, SlotScheduler
from aki_amd.stops import STOP_MAX_LEN, STOP_MAX_SEQS, StopPool, check_stop_sequences, first_finish, resolve_stop_sequences


def _check_rows(tokens, eos, sets, row_set):
    eos_t = torch.tensor(sorted(eos), dtype=torch.long) if eos else None
    finished, index, hit = first_finish(torch.tensor(tokens, dtype=torch.long), eos_t, sets, row_set)
    assert finished.dtype == torch.bool and hit.dtype == torch.int32
    for b, row in enumerate(tokens):
        seqs = sets[row_set[b]] if 0 <= row_set[b] < len(sets) else ()
        t, j = sc.first_stop(row, eos, seqs)
        got = (bool(finished[b]), int(index[b]), int(hit[b]))
        assert got == (t is not None, 0 if t is None else t, j), (b, row, seqs, eos, got, (t, j))


@pytest.mark.parametrize("eos", [(), (1,), (0, 2)], ids=["no_eos", "eos_1", "eos_0_2"])
def test_first_finish_matches_the_reference_on_random_rows(eos):
    """A few hundred rows from the small alphabet: every tie between an EOS and a stop, and between two sequences, comes up."""
    for seed in range(12):
        tokens, sets, row_set = sc.random_rows(seed, 24)
        _check_rows(tokens, eos, sets, row_set)
        _check_rows([r[:5] for r in tokens], eos, sets, [0] * 24 if seed % 4 == 0 else [row_set[0]] * 24)     # one set for every row
    _check_rows([[], []], eos, [(), ((1,),)], [1, 0])                                                      # no tokens yet: nothing finished


def test_first_finish_on_the_hand_written_table():
    for rows in (sc.ROWS, [sc.LONG_ROW]):
        tokens = [r["tokens"] for r in rows]
        row_set = [r["row_set"] for r in rows]
        for eos in ((), (2,)):
            _check_rows(tokens, eos, sc.SETS, row_set)
    # the tie rules, spelled out: EOS wins at the same index, the lowest-numbered sequence among those that match there
    f, i, h = first_finish(torch.tensor([[0, 2, 1, 1]]), torch.tensor([1]), [((2, 1), (1,))], [0])
    assert (bool(f[0]), int(i[0]), int(h[0])) == (True, 2, -1)
    f, i, h = first_finish(torch.tensor([[0, 2, 1, 1]]), None, [((0, 2, 1), (2, 1), (1,))], [0])
    assert (bool(f[0]), int(i[0]), int(h[0])) == (True, 2, 0)
    f, i, h = first_finish(torch.tensor([[0, 2, 1, 1]]), None, [((1, 1), (2, 1, 1))], [0])
    assert (bool(f[0]), int(i[0]), int(h[0])) == (True, 3, 0)
    f, i, h = first_finish(torch.tensor([[1, 2]]), None, [((0, 1, 2),)], [0])                  # n = t + 2: the prompt never counts
    assert not bool(f[0]) and int(h[0]) == -1


def test_check_stop_sequences_normal_form_and_refusals():
    assert check_stop_sequences("x", []) == () and check_stop_sequences("x", ()) == ()
    assert check_stop_sequences("x", [[3, 4], (5,)], 6) == ((3, 4), (5,))
    assert check_stop_sequences("x", torch.tensor([[1, 2], [2, 1]])) == ((1, 2), (2, 1))
    assert check_stop_sequences("x", [[1.0]]) == ((1,),)
    assert len(check_stop_sequences("x", [[1]] * STOP_MAX_SEQS)) == STOP_MAX_SEQS
    assert len(check_stop_sequences("x", [[1] * STOP_MAX_LEN])[0]) == STOP_MAX_LEN
    bad = [None, 5, "ab", [[]], [3], [[1], []], ["ab"], [[1.5]], [[True]], [[-1]], [[1] * (STOP_MAX_LEN + 1)], [[1]] * (STOP_MAX_SEQS + 1)]
    for value in bad:
        with pytest.raises(ValueError, match="^request 4: "):
            check_stop_sequences("request 4", value)
    with pytest.raises(ValueError, match=r"^request 4: .*\[0, 6\)"):
        check_stop_sequences("request 4", [[5], [6]], 6)


def test_request_params_and_precedence():
    with pytest.raises(ValueError, match="^request 3: "):
        RequestParams(stop_sequences=[[]]).check(3, 8)
    with pytest.raises(ValueError, match=r"^request default \(params=\): "):
        RequestParams(stop_sequences=[[1] * 33]).check("default (params=)", 8)
    assert RequestParams().stop_sequences is None
    RequestParams(stop_sequences=()).check(0, 8)
    # only None passes a level on; () is a request without stops
    assert resolve_stop_sequences(None, None, None) is None
    assert resolve_stop_sequences(None, None, ((1,),)) == ((1,),)
    assert resolve_stop_sequences(None, [[2]], ((1,),)) == [[2]]
    assert resolve_stop_sequences((), [[2]], ((1,),)) == ()
    assert resolve_stop_sequences([[3]], [[2]], ((1,),)) == [[3]]
    assert resolve_stop_sequences(None, (), ((1,),)) == ()
    # through generate_many's own resolution: params=, the call-wide keyword, the request's own value, and the width
    from aki_amd.aki import _many_stop_sets, _parse_many_kwargs
    ids = torch.zeros((1, 2), dtype=torch.long)
    own, none = RequestParams(stop_sequences=[[4, 5], [6]]), RequestParams(stop_sequences=())
    reqs = [(None, ids, 4, RequestParams()), (None, ids, 4, own), (None, ids, 4, none)]
    opt = _parse_many_kwargs({"stop_sequences": [[1, 2]]}, 0, lambda: [])
    assert opt.stops == ((1, 2),) and opt.params.stop_sequences is None
    assert _many_stop_sets(reqs, opt, 10) == [((1, 2),), ((4, 5), (6,)), ()]
    opt = _parse_many_kwargs({"stop_sequences": [[1, 2]], "params": RequestParams(stop_sequences=[[7]])}, 0, lambda: [])
    reqs[0] = (None, ids, 4, opt.params)                       # what _many_requests hands a request that brings no RequestParams
    assert _many_stop_sets(reqs, opt, 10) == [((7,),), ((4, 5), (6,)), ()]
    opt = _parse_many_kwargs({}, 0, lambda: [])
    reqs[0] = (None, ids, 4, RequestParams())
    assert opt.stops is None and _many_stop_sets(reqs, opt) == [(), ((4, 5), (6,)), ()]
    with pytest.raises(ValueError, match="^request 1: "):
        _many_stop_sets(reqs, opt, 6)                          # id 6 is outside [0, 6)
    with pytest.raises(ValueError, match="generate_many"):
        _parse_many_kwargs({"stop_sequences": [[]]}, 0, lambda: [])


def test_stop_pool_layout_deduplicates_by_value_and_keeps_order():
    a, b, c = ((1, 2), (2,)), ((2,), (1, 2)), ((0, 0, 0),)
    pool = StopPool([a, (), [[1, 2], [2]], b, c, b])
    assert pool.keys == [(), a, b, c]                           # set 0 is the empty set; a list equal by value is one set; order is a difference
    assert pool.index == {(): 0, a: 1, b: 2, c: 3} and pool.n_sets == 4 and pool.n_seqs == 5
    assert pool.ids == [1, 2, 2, 2, 1, 2, 0, 0, 0]
    assert pool.seq_off == [0, 2, 3, 4, 6, 9]
    assert pool.set_first == [0, 0, 2, 4, 5]
    for k, key in enumerate(pool.keys):                        # the arrays give every set back, in its order
        seqs = tuple(tuple(pool.ids[pool.seq_off[s]:pool.seq_off[s + 1]]) for s in range(pool.set_first[k], pool.set_first[k + 1]))
        assert seqs == key
    empty = StopPool([])
    assert empty.keys == [()] and empty.ids == [] and empty.seq_off == [0] and empty.set_first == [0, 0]
    with pytest.raises(ValueError):
        StopPool([[[]]])


class StopRows:
    """test_slots_cpu.FakeRows with tokens: request r emits FREE[r] one token per step, a row is done from the first finish of the reference
    on (stop_cases.first_stop) or at its budget, and only a look shows it."""

    def __init__(self, free, seqs, slots):
        self.free, self.seqs, self.slots = free, seqs, slots
        self.request, self.generated, self.results, self.hits = [None] * slots, [0] * slots, {}, {}

    def _state(self, s):
        r = self.request[s]
        row = self.free[r][:self.generated[s]]
        t, j = sc.first_stop(row, (), self.seqs[r])
        if t is not None:
            return True, t, j
        return len(row) >= len(self.free[r]), len(row) - 1, -1

    def admit(self, req, slot):
        assert self.request[slot] is None
        self.request[slot], self.generated[slot] = req, 1
        return len(self.free[req]) == 1

    def step(self, n):
        for _ in range(n):
            for s in range(self.slots):
                if self.request[s] is not None and not self._state(s)[0]:
                    self.generated[s] += 1

    def look(self):
        st = [self._state(s) if self.request[s] is not None else (True, 0, -1) for s in range(self.slots)]
        self.seen = [j for _, _, j in st]
        return [d for d, _, _ in st], [at for _, at, _ in st]

    def retire(self, req, slot, n):
        self.results[req], self.hits[req] = self.free[req][:n], self.seen[slot]
        self.request[slot] = None


def test_scheduler_rows_end_at_their_first_stop():
    rng = random.Random(5)
    free = [[rng.randrange(sc.ALPHABET) for _ in range(n)] for n in (12, 1, 5, 12, 3, 9, 12, 30, 2, 17)]
    seqs = [sc.random_sets(rng, 1)[0] if r % 3 else () for r in range(len(free))]
    seqs[3] = ((free[3][0],),)                                  # a one-id stop that is the request's token 0
    for slots in (1, 3, 16):
        sched, rows = SlotScheduler(len(free), slots, 8), StopRows(free, seqs, slots)
        sched.run(rows.admit, rows.step, rows.look, rows.retire)
        out = sched.in_request_order(rows.results)
        assert out == [sc.cut(f, (), s) for f, s in zip(free, seqs)]
        assert sched.in_request_order(rows.hits) == [sc.first_stop(f, (), s)[1] for f, s in zip(free, seqs)]
        assert len(out[3]) == 1 and rows.hits[3] == 0
        assert sched.live_row_steps == sum(len(o) for o in out) - len(out)
    assert any(len(o) < len(f) for o, f in zip(out, free)) and any(len(o) == len(f) for o, f in zip(out, free))
    # without stops the same queue needs more steps
    plain = SlotScheduler(len(free), 3, 8)
    rows = StopRows(free, [()] * len(free), 3)
    plain.run(rows.admit, rows.step, rows.look, rows.retire)
    sched, rows = SlotScheduler(len(free), 3, 8), StopRows(free, seqs, 3)
    sched.run(rows.admit, rows.step, rows.look, rows.retire)
    assert sched.steps <= plain.steps and sched.live_row_steps < plain.live_row_steps


def _stub():
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: [7])


def test_keyword_parsing_needs_no_device():
    from aki_amd.aki import AKI, _parse_generate_kwargs
    opt = _parse_generate_kwargs({"stop_sequences": [[1, 2], [3]]}, 0, lambda: [7], False)
    assert opt.stops == ((1, 2), (3,))
    for none in (None, [], ()):
        assert _parse_generate_kwargs({"stop_sequences": none}, 0, lambda: [7], False).stops == ()
    assert _parse_generate_kwargs({}, 0, lambda: [7], False).stops == ()
    with pytest.raises(NotImplementedError, match="stop_sequences"):
        _parse_generate_kwargs({"stop_sequences": [[1]], "num_beams": 2}, 0, lambda: [7], False)
    _parse_generate_kwargs({"stop_sequences": [], "num_beams": 2}, 0, lambda: [7], False)               # no stops: beams as before
    with pytest.raises(NotImplementedError, match="stop_sequences"):
        AKI.generate(_stub(), None, None, num_beams=3, **{"stop_sequences": [[1]]})
    for kw in ("stopping_criteria", "stop_strings"):
        with pytest.raises(ValueError, match=kw) as e:
            _parse_generate_kwargs({kw: object()}, 0, lambda: [7], False)
        assert "stop_sequences" in str(e.value)                 # the error points to what is served
        with pytest.raises(ValueError, match=kw):
            AKI.generate(_stub(), None, None, **{kw: object()})
    with pytest.raises(ValueError, match="^generate: "):
        _parse_generate_kwargs({"stop_sequences": [[1] * 33]}, 0, lambda: [7], False)
    # generate_many: a request's bad set names the request, before any device work (the requests' tensors are never touched)
    ids = torch.zeros((1, 3), dtype=torch.long)
    with pytest.raises(ValueError, match="^request 1: "):
        AKI.generate_many(_stub(), [(None, ids), (None, ids, 4, RequestParams(stop_sequences=[[1], []]))], slots=2)
    with pytest.raises(ValueError, match="stop_sequences"):
        AKI.generate_many(_stub(), [(None, ids)], slots=2, stop_sequences=[[-1]])
