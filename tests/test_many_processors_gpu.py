"""Per-request logits processors in generate_many, on the GPU: the per-row entry points (ops.ProcessorSets.apply, ops.greedy_pick and
ops.sample_pick_rows with processor_sets=: aki_logits_process_rows / aki_greedy_pick_rows / aki_sample_pick_rows_processed) against the
installed transformers' processors run on each row alone with its own settings (tests/many_processor_cases.py holds the tables), and
AKI.generate_many with RequestParams' processor fields end to end on the tiny bf16 model.  Every test here needs the feature."""
import numpy as np
import pytest
import torch

import constraint_cases as CC
import many_processor_cases as P
import sampling_cases as S
from test_logits_processors_gpu import assert_scores_equal, hf_processors
from test_many_sampling_gpu import call, teacher_forced_logits, with_params
from test_slots_gpu import BUDGETS, generate_alone, tiny, with_budgets

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOTS = 3
B = 6


# ---- the per-row entry points at op level ------------------------------------------------------------------------------------------------
_HF = {}


def hf_rows(name, V):
    """transformers on every row alone with the row's own settings -> f32 [B, V] (a finished row: the plain copy).  Once per (table, V)."""
    if (name, V) not in _HF:
        table = P.TABLES[name]
        x, h = torch.from_numpy(P.logits(table, V, 11)), torch.from_numpy(P.histories(B, 12))
        rows = []
        for b, ((_, n, fin), key) in enumerate(zip(table, P.row_keys(table))):
            rows.append(x[b] if fin else hf_processors(**P.hf_kwargs(key))(h[b:b + 1, :n], x[b:b + 1].clone())[0])
        _HF[(name, V)] = torch.stack(rows)
    return _HF[(name, V)]


def setup(name, V, order):
    """The table on the device: bf16 logits with a row stride that is a multiple of 8 (V = 32066: a padded stride), the histories, the
    pool in `order` with every row's set index (the out-of-range row: past the pool in table a, negative in table b)."""
    from aki_amd import ops
    table = P.TABLES[name]
    x = P.logits(table, V, 11)
    buf = torch.zeros((B, (V + 7) // 8 * 8), dtype=torch.bfloat16, device=DEV)
    buf[:, :V] = torch.from_numpy(x).to(DEV)
    ps = ops.ProcessorSets(V, DEV, P.EOS, P.pool_keys(P.ORDERS[order]), B)
    outside = len(ps.keys) + 5 if name == "a" else -1
    ps.row_set.copy_(torch.tensor([outside if r[0] == P.OUT_OF_RANGE else ps.index[P.SETS[r[0]]] for r in table], dtype=torch.int32))
    return table, x, buf[:, :V], torch.from_numpy(P.histories(B, 12)).to(DEV), ps


def state(table, tokens, advance):
    n = torch.tensor([r[1] for r in table], dtype=torch.int32, device=DEV)
    return dict(pad_token_id=P.PAD, eos_ids=torch.tensor(P.EOS, dtype=torch.long, device=DEV),
                done=torch.tensor([int(r[2]) for r in table], dtype=torch.uint8, device=DEV), tokens=tokens.clone(),
                cache_len=(n + P.START - (1 if advance else 0)).contiguous(), start_len=torch.full((B,), P.START, dtype=torch.int32, device=DEV),
                advance=advance, done_at=torch.full((B,), -1, dtype=torch.int32, device=DEV))


def one_row(st, b):
    return {k: (v[b:b + 1] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in st.items()}


@pytest.mark.parametrize("order", [0, 1], ids=["order0", "order1"])
@pytest.mark.parametrize("V", P.WIDTHS)
@pytest.mark.parametrize("name", list(P.TABLES))
def test_rows_are_processed_and_picked_with_their_own_set(name, V, order):
    from aki_amd import ops
    table, x, logits, h, ps = setup(name, V, order)
    want = hf_rows(name, V)
    st = state(table, h, advance=False)
    got = ps.apply(logits, tokens=h, cache_len=st["cache_len"], start_len=st["start_len"], done=st["done"]).cpu()
    plain = torch.from_numpy(x)
    for b, (set_name, n, fin) in enumerate(table):
        if fin or set_name in ("neutral", P.OUT_OF_RANGE):
            assert torch.equal(got[b], plain[b]), f"row {b} ({set_name}): the plain bf16 -> f32 copy, bit for bit"
        else:
            assert_scores_equal(got[b], want[b], f"row {b} ({set_name}, n = {n})")
    assert_scores_equal(got, torch.from_numpy(P.reference(table, x, h.cpu().numpy())), "the numpy reference")
    # the greedy pick over the same rows, advance = True: t = cache_len + 1 - start_len
    st = state(table, h, advance=True)
    ids = torch.full((B,), -9, dtype=torch.long, device=DEV)
    ops.greedy_pick(logits, ids, processor_sets=ps, **st)
    # ... against the existing pick run on every row ALONE with the row's settings call-wide: token and bookkeeping, bit for bit
    for b, ((set_name, n, fin), key) in enumerate(zip(table, P.row_keys(table))):
        if not fin:
            assert int(ids[b]) == int(want[b].argmax()), f"row {b}: picked {int(ids[b])}, the processed argmax is {int(want[b].argmax())}"
        lone = one_row(state(table, h, advance=True), b)
        lone_id = torch.full((1,), -9, dtype=torch.long, device=DEV)
        proc = ops.LogitsProcessors(V, DEV, key[0], key[1], key[2], P.EOS, list(key[3]), list(key[4]), [list(w) for w in key[5]])
        ops.greedy_pick(logits[b:b + 1], lone_id, processors=proc if proc.active else None, **lone)
        assert proc.active == (key != P.NEUTRAL)                # the neutral and the out-of-range row: ops.greedy_pick's plain launch
        assert int(ids[b]) == int(lone_id[0]) and (int(ids[b]) == P.PAD) == fin, (b, set_name)
        for k in ("tokens", "cache_len", "done", "done_at"):
            assert torch.equal(st[k][b:b + 1], lone[k]), f"row {b} ({set_name}): {k} differs from what the existing pick writes"
        expect = h[b].clone()
        expect[n] = ids[b]
        assert torch.equal(st["tokens"][b], expect) and int(st["cache_len"][b]) == n + P.START
    if name == "a":                                            # the steered rows: an eos pick ends the row; a minimum length bans the eos
        assert int(ids[5]) == P.EOS[0] and int(st["done"][5]) == 1 and int(st["done_at"][5]) == 7
        assert int(ids[3]) != P.EOS[1] and float(plain[3].max()) == 60.0 and int(st["done"][3]) == 0 and int(st["done_at"][3]) == -1


@pytest.mark.parametrize("V", P.WIDTHS)
def test_sampling_rows_draw_from_their_own_processed_scores(V):
    """top_k = 1 rows take the greedy pick's token; one sampled row is checked against the float64 sampler reference over ITS processed scores."""
    from aki_amd import ops
    table, x, logits, h, ps = setup("a", V, 0)
    greedy = torch.full((B,), -9, dtype=torch.long, device=DEV)
    ops.greedy_pick(logits, greedy, processor_sets=ps, **state(table, h, advance=True))
    sampled, (set_name, n, _) = 4, table[4]
    T, k, p = 0.9, 50, 0.9
    rows = dict(temperature=torch.ones(B, device=DEV), top_k=torch.ones(B, dtype=torch.int32, device=DEV), top_p=torch.ones(B, device=DEV))
    rows["temperature"][sampled], rows["top_k"][sampled], rows["top_p"][sampled] = T, k, p
    ref = S.reference(S.Case("rows", V, 4.0, T, k, p), x=P.reference_row(x[sampled], h[sampled, :n].cpu().numpy(), P.SETS[set_name]))
    for seed in (1, 2, 3, 0xF234_5678_9ABC_DEF1 - (1 << 64), 5, 6):        # one key with its top bit set: the bits of a negative int64
        st = state(table, h, advance=True)
        ids = torch.full((B,), -9, dtype=torch.long, device=DEV)
        ops.sample_pick_rows(logits, ids, processor_sets=ps, seed=torch.full((B,), seed, dtype=torch.int64, device=DEV), **rows, **st)
        keep = torch.arange(B, device=DEV) != sampled
        assert torch.equal(ids[keep], greedy[keep]), "a top_k = 1 row takes the greedy pick's token"
        u = S.uniform(np.array([n]), 0, 0, seed=seed & 0xFFFFFFFFFFFFFFFF)
        tok = np.array([int(ids[sampled])])
        assert S.accepted(ref, tok, u).all(), (seed, tok, u)
        assert int(st["tokens"][sampled, n]) == int(ids[sampled]) and int(st["cache_len"][sampled]) == n + P.START


@pytest.mark.parametrize("V", P.WIDTHS)
def test_greedy_rows_compose_with_slot_constraints(V):
    """Table a with an automaton on row 5 (a repetition penalty only: the allowed set lies inside the histories' alphabet, so the penalty
    decides among allowed tokens) while row 4, unconstrained, keeps its bans."""
    from aki_amd import ops
    table, x, logits, h, ps = setup("a", V, 1)
    allowed = (np.arange(0, 12), np.arange(8, 24))              # state 0 -> 1 over [0, 12), state 1 -> 0 over [8, 24)
    tbl = torch.full((2, (V + 7) // 8 * 8), -1, dtype=torch.int16)
    tbl[0, allowed[0]], tbl[1, allowed[1]] = 1, 0
    sc = ops.SlotConstraints(tbl.to(DEV), B, P.HISTORY)
    row, n = 5, table[5][1]
    sc.row_states[row] = 2
    sc.states[row, n] = 1
    st = state(table, h, advance=True)
    ids = torch.full((B,), -9, dtype=torch.long, device=DEV)
    ops.greedy_pick(logits, ids, processor_sets=ps, slot_constraints=sc, **st)
    free = torch.full((B,), -9, dtype=torch.long, device=DEV)
    ops.greedy_pick(logits, free, processor_sets=ps, **state(table, h, advance=True))
    scores = P.reference_row(x[row], h[row, :n].cpu().numpy(), P.SETS["penalty"])
    masked = np.full(V, -np.inf, np.float32)
    masked[allowed[1]] = scores[allowed[1]]
    assert int(ids[row]) == int(masked.argmax()) != int(free[row]) == P.EOS[0]
    assert int(sc.states[row, n + 1]) == 0 and int(st["done"][row]) == 0
    keep = torch.arange(B, device=DEV) != row
    assert torch.equal(ids[keep], free[keep])                   # rows without a state: picked as without the constraint ...
    for b in range(B):
        if b != row and not table[b][2]:
            assert int(sc.states[b, table[b][1] + 1]) == -1     # ... and left without one
    st = state(table, h, advance=False)
    got = ps.apply(logits, tokens=h, cache_len=st["cache_len"], start_len=st["start_len"], done=st["done"], slot_constraints=sc).cpu()
    assert_scores_equal(got[row], torch.from_numpy(masked), "the constrained row's scores")
    assert_scores_equal(got[4], hf_rows("a", V)[4], "the unconstrained row keeps its bans")


def test_row_set_is_read_by_the_launch():
    """The same arguments launched twice with row_set rewritten in place in between: the rows follow their new sets."""
    from aki_amd import ops
    V = 32064
    table, x, logits, h, ps = setup("b", V, 0)
    st = state(table, h, advance=False)
    args = dict(tokens=h, cache_len=st["cache_len"], start_len=st["start_len"], done=st["done"])
    out = torch.empty((B, V), dtype=torch.float32, device=DEV)
    first = ps.apply(logits, out=out, **args).cpu()
    assert_scores_equal(first, torch.from_numpy(P.reference(table, x, h.cpu().numpy())), "before the rewrite")
    names = ["all", "neutral", "penalty", "bigram_words", "unigram", "all"]
    for b, name in enumerate(names):
        ps.admit(b, P.SETS[name])
    second = ps.apply(logits, out=out, **args).cpu()
    moved = tuple((name, n, fin) for name, (_, n, fin) in zip(names, table))
    assert_scores_equal(second, torch.from_numpy(P.reference(moved, x, h.cpu().numpy())), "after the rewrite")
    assert not torch.equal(first, second)
    ids = [torch.full((B,), -9, dtype=torch.long, device=DEV) for _ in range(2)]
    ops.greedy_pick(logits, ids[0], processor_sets=ps, **state(table, h, advance=True))
    ps.row_set.fill_(0)
    ops.greedy_pick(logits, ids[1], processor_sets=ps, **state(table, h, advance=True))
    want = torch.from_numpy(x).argmax(-1)
    live = torch.tensor([not r[2] for r in table])
    assert torch.equal(ids[1].cpu()[live], want[live]) and torch.equal(ids[0].cpu()[live], second.argmax(-1)[live])


# ---- generate_many on the tiny bf16 model ------------------------------------------------------------------------------------------------
def _width(m):
    head = m.lang_model.get_output_embeddings()
    return int(head.max_original_id) + 1 + int(head.additional_out_features) if hasattr(head, "max_original_id") else int(head.out_features)


def plain_tokens():
    return call("greedy")[0]                                    # the all-greedy call over the same 3 slots, eos-free: made once


def settings():
    return P.request_settings(plain_tokens())


def params_of(sets):
    import aki_amd
    return [aki_amd.RequestParams(**(s or {})) for s in sets]


def set_key(s, V, eos=()):
    from aki_amd.slots import RequestParams, processor_set_key, resolve_processors
    return processor_set_key("request", resolve_processors(RequestParams(**(s or {})), None, {}), eos, V)


def check_margin(r, row, key, eos=()):
    """The teacher-forced margin rule over the PROCESSED scores: every token is allowed by the request's own processors, and its processed
    logit is within 0.05 * max(1, max|logits|) of the best processed logit (bf16 at another batch size may flip a near-tie)."""
    full = teacher_forced_logits(r, row)
    bar = 0.05 * max(1.0, float(full.abs().max()))
    scores = full.cpu().numpy()
    for i, tok in enumerate(row):
        s = P.reference_row(scores[i], row[:i], key, eos)
        assert np.isfinite(s[tok]), (r, i, tok, "a token the request's processors ban")
        assert float(s.max() - s[tok]) <= bar, (r, i, tok, float(s.max() - s[tok]), bar)


_MIXED = {}


def mixed_call(use_graph):
    if use_graph not in _MIXED:
        m, reqs = tiny(torch.bfloat16)
        outs = m.generate_many(with_params(reqs, params_of(settings())), slots=SLOTS, eos_token_id=[], use_graph=use_graph)
        _MIXED[use_graph] = ([o.tolist() for o in outs], dict(m.last_many_stats))
    return _MIXED[use_graph]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_every_request_is_generated_with_its_own_processors(use_graph):
    assert BUDGETS == P.BUDGETS
    m, reqs = tiny(torch.bfloat16)
    plain, sets = plain_tokens(), settings()
    got, stats = mixed_call(use_graph)
    assert [len(x) for x in got] == BUDGETS and stats["admits"] == 7 and stats["slots"] == SLOTS
    V = _width(m)
    for r, (row, s) in enumerate(zip(got, sets)):
        check_margin(r, row, set_key(s, V))
    # a request that sets nothing, and one that sets a neutral value: the plain call's tokens (the same batch size: bit-identical rows)
    assert got[P.NOTHING] == plain[P.NOTHING] and got[P.EXPLICIT_NEUTRAL] == plain[P.EXPLICIT_NEUTRAL]
    # properties that hold whatever the numerics
    assert P.repeated_ngrams(got[P.NGRAM2], 2) == 0 and P.repeated_ngrams(got[P.WORDS], 2) == 0 and P.repeated_ngrams(got[P.HEAVY], 3) == 0
    assert not set(got[P.SUPPRESS]) & set(sets[P.SUPPRESS]["suppress_tokens"]) and set(plain[P.SUPPRESS]) & set(sets[P.SUPPRESS]["suppress_tokens"])
    assert got[P.BEGIN][0] != plain[P.BEGIN][0]
    word1, word2 = sets[P.WORDS]["bad_words_ids"]
    assert word1[0] not in got[P.WORDS] and tuple(word2) not in set(zip(got[P.WORDS], got[P.WORDS][1:]))
    assert sets[P.HEAVY]["suppress_tokens"][0] not in got[P.HEAVY]
    assert sum(g != q for g, q in zip(got, plain)) >= 4, "the processed requests do not differ from the plain call: the tests here would show nothing"


def test_one_slot_hands_each_request_to_generate_with_its_own_keywords():
    m, reqs = tiny(torch.bfloat16)
    sets = settings()
    outs = m.generate_many(with_params(reqs, params_of(sets)), slots=1, eos_token_id=[])
    assert m.last_many_stats["per_request_generate"]
    for r, ((vx, lx), budget, s) in enumerate(zip(reqs, BUDGETS, sets)):
        alone = generate_alone(m, vx, lx, max_new_tokens=budget, eos_token_id=[], **(s or {}))
        assert outs[r].tolist() == alone.tolist(), r


def test_an_f32_model_takes_the_per_row_scores():
    """The torch pick over aki_logits_process_rows' f32 scores: identical to generate() alone with the request's keywords."""
    m, reqs = tiny(torch.float32)
    plain = [generate_alone(m, vx, lx, max_new_tokens=b, eos_token_id=[]).tolist() for (vx, lx), b in zip(reqs, BUDGETS)]
    sets = P.request_settings(plain)
    outs = m.generate_many(with_params(reqs, params_of(sets)), slots=SLOTS, eos_token_id=[])
    for r, ((vx, lx), budget, s) in enumerate(zip(reqs, BUDGETS, sets)):
        alone = generate_alone(m, vx, lx, max_new_tokens=budget, eos_token_id=[], **(s or {}))
        assert outs[r].tolist() == alone.tolist(), r
    assert outs[P.BEGIN].tolist()[0] != plain[P.BEGIN][0]


def test_minimum_length_belongs_to_the_request():
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    for r in (0, 3, 6):                                         # the eos id: what the plain run of the prompt emits at index 2, so that it stops at three
        vx, lx = reqs[r]
        base = m.generate_many([(vx, lx, 12)] * 3, slots=SLOTS, eos_token_id=[])[0].tolist()
        if base[2] not in base[:2]:
            break
    else:
        raise AssertionError("no prompt whose third token differs from its first two")
    eos, plain = base[2], {r: base}
    params = [aki_amd.RequestParams(min_new_tokens=6), aki_amd.RequestParams(), aki_amd.RequestParams(min_new_tokens=0)]
    outs = [o.tolist() for o in m.generate_many([(vx, lx, 12, p) for p in params], slots=SLOTS, eos_token_id=[eos], min_new_tokens=0)]
    assert outs[1] == plain[r][:3] == outs[2]
    assert len(outs[0]) >= 6 and eos not in outs[0][:5] and outs[0][:2] == plain[r][:2] and outs[0][2] != eos
    check_margin(r, outs[0], set_key(dict(min_new_tokens=6), _width(m), (eos,)), (eos,))
    # the call-wide keyword as the default, a request's own neutral value over it
    outs = [o.tolist() for o in m.generate_many([(vx, lx, 12, p) for p in params[1:]], slots=SLOTS, eos_token_id=[eos], min_new_tokens=6)]
    assert len(outs[0]) >= 6 and outs[1] == plain[r][:3]


def test_a_refilled_slot_starts_with_its_own_set():
    """slots = 2, five requests: neutral requests are served right behind heavily processed ones and return the plain call's tokens.
    Eager steps (use_graph=False) in both calls: the comparison is between two calls of the same shape, so the rows are bit-identical."""
    import aki_amd
    m, reqs = tiny(torch.bfloat16)
    order, budgets = [0, 3, 6, 2, 4], [3, 4, 12, 5, 3]
    queue = [reqs[r] for r in order]
    plain = [o.tolist() for o in m.generate_many(with_budgets(queue, budgets), slots=2, eos_token_id=[], use_graph=False)]
    heavy = aki_amd.RequestParams(repetition_penalty=1.5, no_repeat_ngram_size=1, suppress_tokens=sorted({t for row in plain for t in row[:2]}))
    params = [heavy, heavy, aki_amd.RequestParams(), heavy, aki_amd.RequestParams(repetition_penalty=1.0)]
    outs = [o.tolist() for o in m.generate_many(with_params(queue, params, budgets), slots=2, eos_token_id=[], use_graph=False)]
    assert m.last_many_stats["admits"] == 5 and m.last_many_stats["slots"] == 2
    assert outs[2] == plain[2] and outs[4] == plain[4]
    for i in (0, 1, 3):
        assert outs[i] != plain[i] and len(set(outs[i])) == len(outs[i]) and not set(outs[i]) & set(heavy.suppress_tokens), i


def test_a_refilled_slot_follows_its_new_set_under_the_captured_step(monkeypatch):
    """The same queue with use_graph=True: row_set is rewritten in place under ONE capture.  The per-row pick is issued once for the capture
    and once per admit; every request's tokens pass the margin rule over the scores ITS OWN set gives (a heavy row's under the neutral set
    would repeat and emit suppressed ids, a neutral row's under the heavy set could not repeat a token), and the properties hold."""
    import aki_amd
    from aki_amd import _lib
    from aki_amd.phi3 import DecodeGraph
    m, reqs = tiny(torch.bfloat16)
    order, budgets = [0, 3, 6, 2, 4], [3, 4, 12, 5, 3]
    queue = [reqs[r] for r in order]
    plain = [o.tolist() for o in m.generate_many(with_budgets(queue, budgets), slots=2, eos_token_id=[])]
    assert P.repeated_ngrams(plain[2], 1) > 0, "the plain run repeats no token: a neutral row under the heavy set would go unnoticed"
    own = dict(repetition_penalty=1.5, no_repeat_ngram_size=1, suppress_tokens=sorted({t for row in plain for t in row[:2]}))
    sets = [own, own, None, own, dict(repetition_penalty=1.0)]
    lib, counts, captures = _lib.load(), [], []
    real, real_capture = lib.aki_greedy_pick_rows, DecodeGraph._capture
    monkeypatch.setattr(lib, "aki_greedy_pick_rows", lambda *a: (counts.append(a[1]), real(*a))[1])
    monkeypatch.setattr(DecodeGraph, "_capture", lambda self: (captures.append(1), real_capture(self))[1])
    outs = [o.tolist() for o in m.generate_many(with_params(queue, params_of(sets), budgets), slots=2, eos_token_id=[], use_graph=True)]
    st = m.last_many_stats
    assert st["admits"] == 5 and st["slots"] == 2 and [len(o) for o in outs] == budgets
    assert len(captures) == 1 and sorted(counts) == [1] * 5 + [2], counts      # B = 1 per admit, B = 2 once: inside the captured step
    V = _width(m)
    for i, (row, s) in enumerate(zip(outs, sets)):
        check_margin(order[i], row, set_key(s, V))
    for i in (0, 1, 3):
        assert len(set(outs[i])) == len(outs[i]) and not set(outs[i]) & set(own["suppress_tokens"]), i
    assert outs[2][:2] == plain[2][:2] and outs[4][0] == plain[4][0]       # what the heavy set suppresses, a neutral row still emits


def test_a_constrained_request_next_to_requests_with_bans():
    import aki_amd
    from test_many_constraint_gpu import constrained_call, constraints
    m, reqs = tiny(torch.bfloat16)
    cons, plain = constraints(), plain_tokens()
    assert cons[3] is None and cons[5] is None and cons[6] is not None
    own = {3: dict(no_repeat_ngram_size=2, bad_words_ids=[[plain[3][0]]]), 5: dict(suppress_tokens=sorted(set(plain[5][:2])))}
    params = [aki_amd.RequestParams(constraint=c, **own.get(r, {})) for r, c in enumerate(cons)]
    params[6] = aki_amd.RequestParams(constraint=cons[6], repetition_penalty=1.3)
    outs = [o.tolist() for o in m.generate_many(with_params(reqs, params), slots=SLOTS, eos_token_id=[])]
    assert [len(x) for x in outs] == BUDGETS
    alone = constrained_call()[0]
    for r in (0, 1, 2, 4):
        assert outs[r] == alone[r] and CC.legal(cons[r].with_eos(()), 0, outs[r]), r    # the constrained rows: walks of their automata
    assert CC.legal(cons[6].with_eos(()), 0, outs[6])
    V = _width(m)
    for r in (3, 5):
        check_margin(r, outs[r], set_key(own[r], V))
    assert plain[3][0] not in outs[3] and P.repeated_ngrams(outs[3], 2) == 0 and not set(outs[5]) & set(own[5]["suppress_tokens"])


NEW_ENTRY_POINTS = ("aki_logits_process_rows", "aki_greedy_pick_rows", "aki_sample_pick_rows_processed")
PICKS = ("aki_greedy_pick", "aki_greedy_pick_embed", "aki_greedy_pick_processed", "aki_greedy_pick_constrained",
         "aki_greedy_pick_constrained_rows", "aki_sample_pick", "aki_sample_pick_rows", "aki_sample_pick_rows_constrained")


def test_calls_with_one_set_launch_what_they_launched(monkeypatch):
    import aki_amd
    from aki_amd import _lib, ops

    def boom(*a, **kw):
        raise AssertionError("a generate_many call whose requests share one set reached the per-row entry points")

    m, reqs = tiny(torch.bfloat16)
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, boom)
    monkeypatch.setattr(ops, "ProcessorSets", boom)
    outs = m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[])
    assert [o.tolist() for o in outs] == plain_tokens()
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    wide = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=SLOTS, eos_token_id=[], **kw)]
    assert wide != plain_tokens()
    same = m.generate_many(with_params(reqs, [aki_amd.RequestParams(**kw)] * 7), slots=SLOTS, eos_token_id=[])
    assert [o.tolist() for o in same] == wide
    half = m.generate_many(with_params(reqs, [aki_amd.RequestParams(no_repeat_ngram_size=2)] * 7), slots=SLOTS, eos_token_id=[],
                           params=aki_amd.RequestParams(repetition_penalty=1.3), repetition_penalty=1.7)
    assert [o.tolist() for o in half] == wide


def test_a_mixed_call_issues_one_pick_launch_per_step(monkeypatch):
    from aki_amd import _lib
    m, reqs = tiny(torch.bfloat16)
    lib = _lib.load()
    counts = {}

    def spy(name):
        real = getattr(lib, name)

        def f(*a):
            counts[name] = counts.get(name, 0) + 1
            return real(*a)
        return f

    for name in NEW_ENTRY_POINTS + PICKS:
        monkeypatch.setattr(lib, name, spy(name))
    outs = m.generate_many(with_params(reqs, params_of(settings())), slots=SLOTS, eos_token_id=[], use_graph=False)
    st, seen = m.last_many_stats, dict(counts)
    assert seen == {"aki_greedy_pick_rows": st["steps"] + st["admits"]}, (seen, st)     # one per decode step, one per admit's token 0
