"""Per-request token constraints in generate_many, on the GPU: the per-row constrained picks (ops.greedy_pick / ops.sample_pick_rows with
slot_constraints=: aki_greedy_pick_constrained_rows / aki_sample_pick_rows_constrained) against the numpy reference of
tests/many_constraint_cases.py, and AKI.generate_many with RequestParams(constraint=...) end to end on the tiny bf16 model.  Every test
here needs the feature."""
import math

import numpy as np
import pytest
import torch

import constraint_cases as CC
import many_constraint_cases as MC
import many_sampling_cases as M
from test_many_sampling_gpu import call, seed_of, teacher_forced_logits, with_params
from test_slots_gpu import BUDGETS, generate_alone, tiny

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOTS = MC.SLOTS
WIDTHS = [8, 1000, 32067]          # no vector path; the vector path; an odd width with a padded row stride
SENTINEL = -7


# ---- the per-row picks at op level ----------------------------------------------------------------------------------------------------
def _pool_tensor(pool_np, V):
    ld = (V + 7) // 8 * 8
    t = torch.full((pool_np.shape[0], ld), -1, dtype=torch.int16)
    t[:, :V] = torch.from_numpy(pool_np.astype(np.int16))
    return t.to(DEV)


def _row_setup(V, order=(0, 1, 2)):
    """The six-row table on the device: (members, pool as numpy, (base, n) per row, bf16 logits, the same values as numpy, SlotConstraints
    with every state column at SENTINEL except the row's own)."""
    from aki_amd import ops
    mem = MC.members(V)
    pool_np, placed = MC.place([m.with_eos(MC.EOS) for m in mem], order)
    x = torch.from_numpy(MC.row_scores(V, pool_np, placed)).to(torch.bfloat16).to(DEV).contiguous()
    sc = ops.SlotConstraints(_pool_tensor(pool_np, V), len(MC.ROWS), MC.HISTORY - 1)
    sc.states.fill_(SENTINEL)
    for b, ((_, s, t, _), (base, n)) in enumerate(zip(MC.ROWS, placed)):
        sc.states[b, t] = s
        sc.row_base[b], sc.row_states[b] = base, n
    return mem, pool_np, placed, x, x.float().cpu().numpy(), sc


def _bookkeeping(advance):
    B = len(MC.ROWS)
    start = torch.tensor(MC.ROW_START, dtype=torch.int32, device=DEV)
    t = torch.tensor([r[2] for r in MC.ROWS], dtype=torch.int32, device=DEV)
    return dict(pad_token_id=MC.PAD, eos_ids=torch.tensor(MC.EOS, dtype=torch.long, device=DEV),
                done=torch.tensor([int(r[3]) for r in MC.ROWS], dtype=torch.uint8, device=DEV),
                tokens=torch.full((B, MC.HISTORY - 1), -5, dtype=torch.long, device=DEV), cache_len=(start + t - (1 if advance else 0)).contiguous(),
                start_len=start, advance=advance, done_at=torch.full((B,), -1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)], ids=["abc", "cba"])
@pytest.mark.parametrize("V", WIDTHS)
def test_greedy_rows_pick_inside_their_own_table(V, order):
    """Rows at different generated-token indices, each with its own place in the pool: tokens equal the numpy pick exactly, states[b, t + 1]
    is the LOCAL next state and no other column is written; the unconstrained row takes ops.greedy_pick's token and stores -1, the
    finished row pad and its own state.  Both pool orders: the result does not depend on where a table lies."""
    from aki_amd import ops
    mem, pool_np, placed, x, x_np, sc = _row_setup(V, order)
    proc = ops.LogitsProcessors(V, DEV, slot_constraints=True)
    assert proc.active
    B = len(MC.ROWS)
    ids = torch.full((B,), -1, dtype=torch.long, device=DEV)
    kw = _bookkeeping(True)
    before = kw["cache_len"].clone()
    ops.greedy_pick(x, ids, processors=proc, slot_constraints=sc, **kw)
    plain = torch.zeros(B, dtype=torch.long, device=DEV)
    ops.greedy_pick(x, plain)
    states, tokens = sc.states.cpu().numpy(), kw["tokens"].cpu().numpy()
    for b, ((kind, s, t, fin), (base, n)) in enumerate(zip(MC.ROWS, placed)):
        tok, ns = MC.pick(pool_np, base, n, s, x_np[b], fin, MC.PAD)
        want_states = np.full(MC.HISTORY, SENTINEL)
        want_states[t], want_states[t + 1] = s, ns
        want_tokens = np.full(MC.HISTORY - 1, -5)
        want_tokens[t] = tok
        assert int(ids[b]) == tok and np.array_equal(tokens[b], want_tokens) and np.array_equal(states[b], want_states), (b, int(ids[b]), tok, states[b])
        if kind is None:
            assert tok == int(plain[b]) and ns == -1
        elif fin:
            assert tok == MC.PAD and ns == s
        else:
            assert tok != int(plain[b]) and 0 <= ns < n, "the free argmax lies outside the allowed set"
            assert ns == int(mem[kind].with_eos(MC.EOS)[s, tok])
        hit = (not fin) and tok in MC.EOS
        assert bool(kw["done"][b]) == (fin or hit) and int(kw["done_at"][b]) == (t if hit else -1)
    assert torch.equal(kw["cache_len"], before + 1)


def test_a_table_above_row_32767_is_the_same_table():
    """V = 8, a pool of 33000 rows (528 KB): constraint B at pool row 0 and again at row 32900, past what an int16 state number could
    address.  The same states and scores give identical tokens and identical (local) next states; a slice that leaves the pool's end is
    a row left untouched."""
    from aki_amd import ops
    V, high = 8, 32900
    b_table = MC.members(V)[1].with_eos(MC.EOS)
    n = b_table.shape[0]
    pool_np = np.full((33000, V), -1, dtype=np.int32)
    pool_np[:n], pool_np[high:high + n] = b_table, b_table
    rows = [(0, n, s) for s in range(n)] + [(high, n, s) for s in range(n)] + [(33000 - 2, n, 2)]
    B = len(rows)
    sc = ops.SlotConstraints(_pool_tensor(pool_np, V), B, 1)
    rng = np.random.Generator(np.random.PCG64(5))
    x1 = rng.standard_normal((n, V)).astype(np.float32)
    x = torch.from_numpy(np.concatenate([x1, x1, x1[2:3]])).to(torch.bfloat16).to(DEV).contiguous()
    for b, (base, cnt, s) in enumerate(rows):
        sc.states[b, 0], sc.row_base[b], sc.row_states[b] = s, base, cnt
    ids = torch.zeros(B, dtype=torch.long, device=DEV)
    tokens = torch.full((B, 1), -5, dtype=torch.long, device=DEV)
    ops.greedy_pick(x, ids, tokens=tokens, processors=ops.LogitsProcessors(V, DEV, slot_constraints=True), slot_constraints=sc)
    got, st, x_np = ids.tolist(), sc.states.cpu().numpy(), x.float().cpu().numpy()
    for b, (base, cnt, s) in enumerate(rows):
        tok, ns = MC.pick(pool_np, base, cnt, s, x_np[b])
        assert (got[b], int(st[b, 1])) == (tok, ns), b
    assert got[:n] == got[n:2 * n] and np.array_equal(st[:n], st[n:2 * n])
    assert int(st[-1, 1]) == -1 and got[-1] == int(np.argmax(x_np[-1]))


@pytest.mark.parametrize("k,p", [(0, 1.0), (50, 1.0), (50, 0.9), (0, 0.5)])
@pytest.mark.parametrize("V", WIDTHS)
def test_sampled_rows_draw_inside_their_own_table(V, k, p):
    """probs_out is exactly 0 outside the row's allowed set, and row b is bit-equal - token and probabilities - to ops.sample_pick at
    B = 1 with that row's constraint bound alone, the row's seed and offset 0."""
    from aki_amd import ops
    mem, pool_np, placed, x, x_np, sc = _row_setup(V)
    B, Tm = len(MC.ROWS), 0.7
    seeds = [M.row_seed(40 + b) for b in range(B)]
    params = dict(temperature=torch.full((B,), Tm, dtype=torch.float32, device=DEV), top_k=torch.full((B,), k, dtype=torch.int32, device=DEV),
                  top_p=torch.full((B,), p, dtype=torch.float32, device=DEV),
                  seed=torch.from_numpy(np.array(seeds, np.uint64).view(np.int64)).to(DEV))
    probs = torch.full((B, V), -1.0, dtype=torch.float32, device=DEV)
    ids = torch.full((B,), -1, dtype=torch.long, device=DEV)
    kw = _bookkeeping(False)
    ops.sample_pick_rows(x, ids, processors=ops.LogitsProcessors(V, DEV, slot_constraints=True), slot_constraints=sc, probs_out=probs, **params, **kw)
    states = sc.states.cpu().numpy()
    for b, ((kind, s, t, fin), (base, n)) in enumerate(zip(MC.ROWS, placed)):
        tok = int(ids[b])
        assert int(kw["tokens"][b, t]) == tok
        if fin:
            assert tok == MC.PAD and bool((probs[b] == 0).all()) and int(states[b, t + 1]) == s
            continue
        p1 = torch.full((1, V), -1.0, dtype=torch.float32, device=DEV)
        i1 = torch.zeros(1, dtype=torch.long, device=DEV)
        one = dict(step=t, temperature=Tm, top_k=k, top_p=p, seed=seeds[b], offset=0, probs_out=p1,
                   tokens=torch.zeros((1, MC.HISTORY - 1), dtype=torch.long, device=DEV))
        if kind is None:
            ops.sample_pick(x[b:b + 1], i1, **one)
            assert int(states[b, t + 1]) == -1
        else:
            proc1 = ops.LogitsProcessors(V, DEV, constraint=mem[kind].bind(MC.EOS, DEV, rows_start=[0]))
            st1 = proc1.states(1, MC.HISTORY - 1)
            st1.fill_(-1)
            st1[0, t] = s
            ops.sample_pick(x[b:b + 1], i1, processors=proc1, **one)
            allowed = torch.from_numpy(MC.mask(pool_np, base, n, s)).to(DEV)
            assert bool((probs[b][~allowed] == 0).all()) and bool(allowed[tok]) and float(probs[b][allowed].sum()) > 0.999
            assert int(states[b, t + 1]) == int(pool_np[base + s, tok]) == int(st1[0, t + 1])
        assert tok == int(i1[0]) and torch.equal(probs[b], p1[0]), (b, tok, int(i1[0]))


def test_refusals_of_the_row_arrays():
    from aki_amd import ops
    V = 1000
    _, _, _, x, _, sc = _row_setup(V)
    B = x.shape[0]
    proc = ops.LogitsProcessors(V, DEV, slot_constraints=True)
    ids = torch.zeros(B, dtype=torch.long, device=DEV)
    rows = dict(temperature=torch.ones(B, dtype=torch.float32, device=DEV), top_k=torch.zeros(B, dtype=torch.int32, device=DEV),
                top_p=torch.ones(B, dtype=torch.float32, device=DEV), seed=torch.zeros(B, dtype=torch.long, device=DEV))
    picks = (lambda s, pr=proc: ops.greedy_pick(x, ids, processors=pr, slot_constraints=s),
             lambda s, pr=proc: ops.sample_pick_rows(x, ids, processors=pr, slot_constraints=s, **rows))
    for name in ("row_base", "row_states"):
        good = getattr(sc, name)
        for bad in (good.long(), good[:B - 1], good.cpu(), good.repeat(2)[::2], None):
            setattr(sc, name, bad)
            for pick in picks:
                with pytest.raises(ops.AkiError, match=name):
                    pick(sc)
        setattr(sc, name, good)
    for attr, bad in (("states", sc.states.long()), ("states", sc.states[:B - 1]), ("pool", sc.pool.int()), ("pool", sc.pool[:, :V - 8]),
                      ("pool", sc.pool.cpu())):
        good = getattr(sc, attr)
        setattr(sc, attr, bad)
        for pick in picks:
            with pytest.raises(ops.AkiError, match=attr):
                pick(sc)
        setattr(sc, attr, good)
    bound = MC.members(V)[0].bind(MC.EOS, DEV, rows_start=[0] * B)
    for pick in picks:
        with pytest.raises(ops.AkiError):                       # no scores scratch
            pick(sc, None)
        with pytest.raises(ops.AkiError):                       # a LogitsProcessors with a constraint of its own
            pick(sc, ops.LogitsProcessors(V, DEV, constraint=bound))
        with pytest.raises(ops.AkiError):
            pick(object())
    with pytest.raises(ops.AkiError):                           # ... which the per-row sampler refuses without slot_constraints too
        ops.sample_pick_rows(x, ids, processors=ops.LogitsProcessors(V, DEV, constraint=bound), **rows)
    for pick in picks:                                          # and the objects are intact
        pick(sc)


def test_admit_rewrites_a_slot_in_place():
    from aki_amd import ops
    V = 8
    pool = _pool_tensor(MC.members(V)[1].with_eos(MC.EOS), V)
    sc = ops.SlotConstraints(pool, 3, 4)
    ptrs = (sc.states.data_ptr(), sc.row_base.data_ptr(), sc.row_states.data_ptr())
    assert tuple(sc.states.shape) == (3, 5) and bool((sc.states == -1).all())
    sc.states.fill_(9)
    sc.admit(1, 0, 3, 2)
    sc.admit(2, 0, 0, -1)
    assert sc.states.tolist() == [[9] * 5, [2, -1, -1, -1, -1], [-1] * 5]
    assert sc.row_base.tolist() == [0, 0, 0] and sc.row_states.tolist() == [0, 3, 0]
    assert ptrs == (sc.states.data_ptr(), sc.row_base.data_ptr(), sc.row_states.data_ptr())
    one = sc.row(1)
    assert one.pool is sc.pool and one.states.data_ptr() == sc.states[1].data_ptr() and tuple(one.states.shape) == (1, 5)
    assert tuple(one.row_base.shape) == (1,) and one.row_states.tolist() == [3]


# ---- generate_many with RequestParams(constraint=...) on the tiny bf16 model ----------------------------------------------------------
def _width(m):
    head = m.lang_model.get_output_embeddings()
    return int(head.max_original_id) + 1 + int(head.additional_out_features) if hasattr(head, "max_original_id") else int(head.out_features)


_CONS = {}


def constraints():
    """The 7 requests' constraints (tests/many_constraint_cases.py's pattern), built once for the tiny model's logits width."""
    if "c" not in _CONS:
        m, _ = tiny(torch.bfloat16)
        _CONS["c"] = MC.request_constraints(_width(m))
    return _CONS["c"]


def constrained_params(**kw):
    import aki_amd
    return [aki_amd.RequestParams(constraint=c, **kw) for c in constraints()]


_RUNS = {}


def constrained_call():
    """The token lists of the greedy constrained call, made once."""
    if "c" not in _RUNS:
        m, reqs = tiny(torch.bfloat16)
        outs = m.generate_many(with_params(reqs, constrained_params()), slots=SLOTS, eos_token_id=[])
        _RUNS["c"] = ([o.tolist() for o in outs], dict(m.last_many_stats))
    return _RUNS["c"]


def _bar(full):
    return 0.05 * max(1.0, float(full.abs().max()))


def _check_walk(r, row, c, eos=(), top=1):
    """Request r's row is a legal walk of c, and every token's teacher-forced logit is at least the top-th best ALLOWED logit minus the bar."""
    table = c.with_eos(eos)
    states = CC.walk(table, c.starts[0], row)
    assert min(states) >= 0, (r, row, states)
    full = teacher_forced_logits(r, row)
    bar = _bar(full)
    for i, tok in enumerate(row):
        allowed = torch.from_numpy(table[states[i]] >= 0).to(DEV)
        if tok in eos:
            assert c.accepting[states[i]], (r, i, "an eos id outside an accepting state")
        vals = full[i][allowed]
        kth = vals.topk(min(top, vals.numel())).values[-1]
        assert float(full[i, tok]) >= float(kth) - bar, (r, i, tok, float(full[i, tok]), float(kth), bar)


def test_constrained_requests_walk_their_own_automaton():
    assert BUDGETS == MC.BUDGETS
    greedy, gstats = call("greedy")
    got, stats = constrained_call()
    assert [len(x) for x in got] == BUDGETS and stats["admits"] == 7 and stats["slots"] == SLOTS
    assert {k: stats[k] for k in ("steps", "admits", "looks")} == {k: gstats[k] for k in ("steps", "admits", "looks")}
    cons = constraints()
    for r, (row, c) in enumerate(zip(got, cons)):
        if c is None:
            assert row == greedy[r], f"request {r} is unconstrained: the all-greedy call's tokens"
        else:
            _check_walk(r, row, c)
    assert any(c is not None and row != greedy[r] for r, (row, c) in enumerate(zip(got, cons))), \
        "no constrained request differs from the greedy call: the tests here would show nothing"


def test_a_constrained_requests_tokens_do_not_depend_on_the_schedule():
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    got, _ = constrained_call()
    params = constrained_params()
    rev = m.generate_many(with_params(reqs, params)[::-1], slots=SLOTS, eos_token_id=[])[::-1]
    assert [o.tolist() for o in rev] == got
    # the neighbours change: request 0 takes another automaton, request 3 samples, request 5 takes a constraint - the others keep theirs
    cons = constraints()
    other = list(params)
    other[0] = aki_amd.RequestParams(constraint=cons[2])
    other[3] = aki_amd.RequestParams(do_sample=True, top_k=8, seed=seed_of(3))
    other[5] = aki_amd.RequestParams(constraint=cons[1], do_sample=True, temperature=1.3, seed=seed_of(5))
    outs = [o.tolist() for o in m.generate_many(with_params(reqs, other), slots=SLOTS, eos_token_id=[])]
    for r in (1, 2, 4, 6):
        assert outs[r] == got[r], r
    assert outs[0] != got[0] and CC.legal(cons[2].with_eos(()), 0, outs[0]) and CC.legal(cons[1].with_eos(()), 0, outs[5])


def test_choices_end_with_the_eos_and_retire_early():
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    eos = 2
    cons = MC.choice_constraints(_width(m))
    params = [aki_amd.RequestParams(constraint=c) for c in cons]
    outs = m.generate_many(with_params(reqs, params, [MC.CHOICE_BUDGET] * 7), slots=SLOTS, eos_token_id=[eos])
    assert m.last_many_stats["admits"] == 7
    for r, (o, c) in enumerate(zip(outs, cons)):
        row = o.tolist()
        assert row[-1] == eos and tuple(row[:-1]) in MC.CHOICES[r] and len(row) < MC.CHOICE_BUDGET, (r, row)
        _check_walk(r, row, c, eos=(eos,))


def test_sampled_and_constrained_requests_together():
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    cons = constraints()
    greedy, _ = call("greedy")
    params = [aki_amd.RequestParams() if c is None else aki_amd.RequestParams(do_sample=True, top_k=2, seed=seed_of(r), constraint=c)
              for r, c in enumerate(cons)]
    outs = [o.tolist() for o in m.generate_many(with_params(reqs, params), slots=SLOTS, eos_token_id=[])]
    assert [len(x) for x in outs] == BUDGETS
    for r, (row, c) in enumerate(zip(outs, cons)):
        if c is None:
            assert row == greedy[r], r
        else:
            _check_walk(r, row, c, top=2)                       # legal, and inside the top 2 of the allowed set
    assert any(c is not None and row != got for row, got, c in zip(outs, constrained_call()[0], cons)), "nothing was drawn"
    # log-probabilities compose: the same tokens, scored under the raw distribution
    lp = [aki_amd.RequestParams(do_sample=p.do_sample, top_k=p.top_k, seed=p.seed, constraint=p.constraint, logprobs=True, top_logprobs=2)
          for p in params]
    scored = m.generate_many(with_params(reqs, lp), slots=SLOTS, eos_token_id=[])
    for r, o in enumerate(scored):
        assert o.tokens.tolist() == outs[r] and o.logprobs.shape == (BUDGETS[r],) and bool((o.logprobs <= 0).all())
        assert bool((o.logprobs <= o.top_logprobs[:, 0]).all())


def test_one_slot_falls_back_to_generate_with_the_requests_constraint():
    m, reqs = tiny(torch.bfloat16)
    cons = constraints()
    outs = m.generate_many(with_params(reqs, constrained_params()), slots=1, eos_token_id=[])
    assert m.last_many_stats["per_request_generate"]
    for r, ((vx, lx), budget, c) in enumerate(zip(reqs, BUDGETS, cons)):
        kw = {} if c is None else dict(constraint=c)
        alone = generate_alone(m, vx, lx, max_new_tokens=budget, eos_token_id=[], **kw)
        assert outs[r].tolist() == alone.tolist(), r
        if c is not None:
            assert CC.legal(c.with_eos(()), 0, outs[r].tolist()), r


def test_a_constrained_call_captures_once_and_never_syncs_per_token(monkeypatch):
    from aki_amd import ops
    from aki_amd.phi3 import DecodeGraph
    m, reqs = tiny(torch.bfloat16)
    captures, picks = [], []
    real, real_pick = DecodeGraph._capture, ops.greedy_pick
    monkeypatch.setattr(DecodeGraph, "_capture", lambda self: (captures.append(1), real(self))[1])
    monkeypatch.setattr(ops, "greedy_pick", lambda *a, **kw: (picks.append((a[0].shape[0], kw.get("slot_constraints") is not None)),
                                                              real_pick(*a, **kw))[1])
    outs = m.generate_many(with_params(reqs, constrained_params()), slots=SLOTS, eos_token_id=[])
    st = m.last_many_stats
    assert [o.tolist() for o in outs] == constrained_call()[0]
    assert len(captures) == 1
    assert st["steps"] > 8 and st["looks"] <= math.ceil(st["steps"] / 8) + st["admits"] + 1, st
    assert sorted(picks) == [(1, True)] * 7 + [(SLOTS, True)]   # one pick per admit on row views, one inside the captured step


def test_a_call_without_a_constrained_request_never_reaches_the_new_entry_points(monkeypatch):
    import aki_amd
    from aki_amd import _lib, ops
    from test_slots_gpu import with_budgets

    def boom(*a, **kw):
        raise AssertionError("an unconstrained generate_many reached the per-row constrained picks")

    m, reqs = tiny(torch.bfloat16)
    lib = _lib.load()
    monkeypatch.setattr(lib, "aki_greedy_pick_constrained_rows", boom)
    monkeypatch.setattr(lib, "aki_sample_pick_rows_constrained", boom)
    monkeypatch.setattr(ops, "SlotConstraints", boom)
    outs = m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[])
    assert [o.tolist() for o in outs] == call("greedy")[0]
    outs = m.generate_many(with_params(reqs, [aki_amd.RequestParams(constraint=None)] * 7), slots=SLOTS, eos_token_id=[])
    assert [o.tolist() for o in outs] == call("greedy")[0]


def test_a_constrained_request_on_an_f32_model_is_refused_before_any_launch(monkeypatch):
    import aki_amd
    from aki_amd import ops
    m, reqs = tiny(torch.float32)

    def boom(*a, **kw):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(ops, "kv_slot_admit", boom)
    monkeypatch.setattr(type(m), "_prefill_request", boom)
    monkeypatch.setattr(type(m), "generate", boom)
    cons = MC.request_constraints(_width(m))
    for slots in (SLOTS, 1):
        with pytest.raises(ValueError, match="request 0.*bf16"):
            m.generate_many(with_params(reqs, [aki_amd.RequestParams(constraint=c) for c in cons]), slots=slots, eos_token_id=[])
