"""Constrained decoding on the device: the mask stage of ops.LogitsProcessors.apply, the constrained ops.greedy_pick / ops.sample_pick and
AKI.generate with its `constraint` keyword against the plain-Python reference of tests/constraint_cases.py."""
import numpy as np
import pytest
import torch

import constraint_cases as CC
import sampling_cases as S
from aki_amd.constraint import TokenConstraint
from test_logits_processors_gpu import _multi, _teacher_forced_check, assert_scores_equal
from test_sampling_gpu import PROBS_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = float("-inf")


def _choices(V):
    """A trie that touches the first and the last column of every V >= 8: states 0 (root: V-1, 3, 4), 1 (behind V-1: 1, V-2),
    2 (accepting leaf: the eos ids only), ..."""
    return ((V - 1, 1), (V - 1, V - 2, 5), (3, 3, 3, 3), (4,)), (0, 2)


def _bound(V, rows_start):
    ch, eos = _choices(V)
    c = TokenConstraint.from_choices(ch, V)
    return c, c.with_eos(eos), c.bind(eos, DEV, rows_start=rows_start), eos


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [8, 1000, 32067, 131072])
def test_apply_masks_exactly(V, dtype):
    """Allowed columns bit-equal to the f32 of the input, every other column -inf: V = 8 (one vector chunk), 1000 (a multiple of 8, not of
    1024 * 8), 32067 (scalar tail) and the processors' limit; three rows in different states at different history indices, one of them
    done (copied unprocessed); a state outside the table leaves its row untouched."""
    from aki_amd import ops
    c, table, bound, eos = _bound(V, [0, 0, 0])
    proc = ops.LogitsProcessors(V, DEV, constraint=bound)
    T = 6
    st = proc.states(3, T)
    row_state, row_n = [0, 1, 2], [0, 2, 5]
    st.fill_(-1)
    for b in range(3):
        st[b, row_n[b]] = row_state[b]
    g = torch.Generator().manual_seed(V)
    x = (torch.randn((3, V), generator=g) * 4).to(dtype).to(DEV)
    done = torch.tensor([0, 0, 1], dtype=torch.uint8, device=DEV)
    start = torch.full((3,), 100, dtype=torch.int32, device=DEV)
    cl = (start + torch.tensor(row_n, dtype=torch.int32, device=DEV)).contiguous()
    got = proc.apply(x, cache_len=cl, start_len=start, done=done)
    want = x.float().clone()
    for b in (0, 1):
        want[b, torch.from_numpy(~CC.mask(table, row_state[b])).to(DEV)] = NEG
    assert torch.equal(got, want)
    assert int(torch.isfinite(got[0]).sum()) == 3 and int(torch.isfinite(got[1]).sum()) == 2 and torch.equal(got[2], x[2].float())
    # n = step for every row, no done flags: the accepting leaf allows the eos ids alone
    st[:, 4] = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    got = proc.apply(x, step=4)
    for b, s in enumerate((2, 0, 1)):
        w = x[b].float().clone()
        w[torch.from_numpy(~CC.mask(table, s)).to(DEV)] = NEG
        assert torch.equal(got[b], w), b
    assert sorted(torch.nonzero(torch.isfinite(got[0])).flatten().tolist()) == sorted(eos)
    # a state outside [0, n_states), no state (-1) and an index outside the history: the row is left as it is
    st[:, 4] = torch.tensor([c.n_states, -1, 32767], dtype=torch.int32, device=DEV)
    assert torch.equal(proc.apply(x, step=4), x.float())
    assert torch.equal(proc.apply(x, cache_len=start + 500, start_len=start), x.float())


@pytest.mark.parametrize("V", [1000, 32067])
def test_apply_behind_the_repetition_penalty(V):
    """HF's RepetitionPenaltyLogitsProcessor, then the reference mask."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from aki_amd import ops
    c, table, bound, eos = _bound(V, [0, 0, 0])
    proc = ops.LogitsProcessors(V, DEV, repetition_penalty=1.3, constraint=bound)
    T = 6
    hist = torch.tensor([[V - 1, 3, 4, 1, 5, 3], [V - 1, V - 2, 3, 3, 4, 4], [4, 4, 4, 4, 4, 4]])       # allowed tokens among them: penalised AND kept
    lens, row_state = [3, 1, 0], [0, 1, 0]
    st = proc.states(3, T)
    st.fill_(-1)
    for b in range(3):
        st[b, lens[b]] = row_state[b]
    x = (torch.randn((3, V), generator=torch.Generator().manual_seed(V + 1)) * 4).to(torch.bfloat16)
    start = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    got = proc.apply(x.to(DEV), tokens=hist.to(DEV), cache_len=start + torch.tensor(lens, dtype=torch.int32, device=DEV), start_len=start).cpu()
    hf = RepetitionPenaltyLogitsProcessor(1.3)
    for b in range(3):
        want = hf(hist[b:b + 1, :lens[b]], x[b:b + 1].float())[0]
        want[torch.from_numpy(~CC.mask(table, row_state[b]))] = NEG
        assert_scores_equal(got[b], want, f"row {b}")


def test_greedy_pick_walks_the_automaton_and_follows_a_rewind():
    """Six picks at op level; the free argmax (column 40) is forbidden at every step.  Tokens, the state history, done / done_at and the
    embedding row against the reference; then cache_len is rewound to step 2 and the loop runs on with other scores: the history follows."""
    from aki_amd import ops
    V, B, T, PAD, d = 1000, 3, 6, 1, 16
    eos = (2, 998)
    members = [TokenConstraint.from_choices(ch, V) for ch in (((5, 6), (5, 6, 7), (9,)), ((10, 11, 12, 13, 14, 15),), ((20,), (21, 22)))]
    u = TokenConstraint.union(members)
    table = u.with_eos(eos)
    proc = ops.LogitsProcessors(V, DEV, constraint=u.bind(eos, DEV, rows_start=u.starts))
    g = torch.Generator().manual_seed(4)

    def scores(longer):
        x = torch.randn((T, B, V), generator=g)
        x[:, :, 40] = 9.0                                   # the unconstrained argmax: never allowed
        x[:, :, 998] = 5.0                                  # an eos id: taken as soon as a state accepts ...
        x[2, 0, 7] = 7.0 if longer else -7.0                # ... except behind (5, 6), where row 0 can go on to the longer choice
        x[0, 0, 5], x[0, 2, 20] = 6.0, 6.0                  # the first tokens of rows 0 and 2
        return x.to(torch.bfloat16)

    emb = torch.randn((V, d), generator=g).to(torch.bfloat16).to(DEV)
    tokens = torch.full((B, T), -5, dtype=torch.long, device=DEV)
    ids = torch.zeros(B, dtype=torch.long, device=DEV)
    nxt_emb = torch.zeros((B, d), dtype=torch.bfloat16, device=DEV)
    done, done_at = torch.zeros(B, dtype=torch.uint8, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
    start = torch.full((B,), 100, dtype=torch.int32, device=DEV)
    cl = start.clone()
    kw = dict(pad_token_id=PAD, eos_ids=torch.tensor(eos, dtype=torch.long, device=DEV), done=done, tokens=tokens, cache_len=cl, start_len=start,
              done_at=done_at, embed=(emb, None, V - 1), next_embeds=nxt_emb, processors=proc)

    def run(x, t0):
        for t in range(t0, T):
            ops.greedy_pick(x[t].to(DEV).contiguous(), ids, advance=t > 0, **kw)
            assert torch.equal(ids, tokens[:, t]) and torch.equal(nxt_emb, emb[ids])

    x1 = scores(True)
    assert (x1.float().argmax(-1) == 40).all()
    run(x1, 0)
    st = proc.states(B).cpu()
    assert st.shape == (B, T + 1) and torch.equal(cl.cpu(), start.cpu() + T - 1)
    first = []
    for b in range(B):
        toks, states, at = CC.greedy(table, u.starts[b], x1[:, b].float().numpy(), eos, PAD)
        first.append((toks, states, at))
        assert tokens[b].tolist() == toks and st[b].tolist() == states and int(done_at[b]) == at and bool(done[b]) == (at >= 0), b
        for t, tok in enumerate(toks):
            if tok in eos and (at < 0 or t <= at):
                assert u.accepting[states[t]], "an eos id outside an accepting state"
    assert first[0][0][:4] == [5, 6, 7, 998] and first[1][2] == -1 and first[2][2] == 1
    # the rewind of a chain recovery: back to step 2 (cache_len = start + 1), flags rebuilt from the first two tokens, other scores
    x2 = scores(False)
    cl.copy_(start + 1)
    keep = [at if 0 <= at < 2 else -1 for _, _, at in first]
    done.copy_(torch.tensor([k >= 0 for k in keep], dtype=torch.uint8))
    done_at.copy_(torch.tensor(keep, dtype=torch.int32))
    tokens[:, 2:] = -5
    run(x2, 2)
    st = proc.states(B).cpu()
    changed = False
    for b in range(B):
        toks0, states0, _ = first[b]
        if keep[b] >= 0:
            toks, states = [PAD] * (T - 2), [states0[2]] * (T - 1)
        else:
            toks, states, _ = CC.greedy(table, states0[2], x2[2:, b].float().numpy(), eos, PAD)
        assert tokens[b].tolist() == toks0[:2] + toks and st[b].tolist() == states0[:2] + states, b
        changed = changed or toks != toks0[2:]
    assert changed, "the second set of scores has to lead somewhere else"


@pytest.mark.parametrize("k,p", [(0, 1.0), (50, 1.0), (50, 0.9), (0, 0.5)])
def test_sample_pick_draws_inside_the_allowed_set(k, p):
    """probs_out: zero outside the state's allowed set, inside it the float64 softmax with temperature, top-k and top-p over that set
    (tests/sampling_cases.py's reference on the masked row, at test_sampling_gpu.PROBS_RTOL); rows: one allowed token (drawn with
    certainty), two allowed tokens, the root's three, the accepting leaf's eos ids."""
    from aki_amd import ops
    V, Tm = S.V_SMALL, 0.7
    ch = ((V - 1, 1), (V - 1, V - 2, 5), (3, 3, 3, 3), (4,))
    eos = (0, 2)
    c = TokenConstraint.from_choices(ch, V)
    table = c.with_eos(eos)
    row_state = [5, 1, 0, 2]                                # behind (3,): only 3; behind (V-1,): 1 or V-2; the root; behind (V-1, 1): eos ids
    assert [int(CC.mask(table, s).sum()) for s in row_state] == [1, 2, 3, 2]
    B, step = len(row_state), 3
    proc = ops.LogitsProcessors(V, DEV, constraint=c.bind(eos, DEV, rows_start=[0] * B))
    st = proc.states(B, 8)
    st.fill_(-1)
    st[:, step] = torch.tensor(row_state, dtype=torch.int32, device=DEV)
    case = S.Case(f"constraint-k{k}-p{p}", V, 2.0, Tm, k, p)
    x = S.logits(case)
    xs = torch.from_numpy(np.stack([x] * B)).to(torch.bfloat16).to(DEV)
    probs = torch.full((B, V), -1.0, dtype=torch.float32, device=DEV)
    ids = torch.zeros(B, dtype=torch.long, device=DEV)
    tokens = torch.zeros((B, 8), dtype=torch.long, device=DEV)
    ops.sample_pick(xs, ids, tokens=tokens, step=step, processors=proc, temperature=Tm, top_k=k, top_p=p, seed=S.SEED, offset=5, probs_out=probs)
    pr = probs.cpu().numpy().astype(np.float64)
    u = S.uniform(np.full(B, step), np.arange(B), np.full(B, 5))
    for b, s in enumerate(row_state):
        allowed = CC.mask(table, s)
        r = S.reference(case, x=np.where(allowed, x, -np.inf).astype(np.float32))
        tok = int(ids[b])
        assert (pr[b][~allowed] == 0).all() and (pr[b][~r.kept] == 0).all() and allowed[tok] and int(tokens[b, step]) == tok
        big = r.probs > 1e-30
        assert big.sum() >= 1 and np.abs(pr[b][big] / r.probs[big] - 1.0).max() <= PROBS_RTOL, (b, pr[b][allowed], r.probs[allowed])
        assert bool(S.accepted(r, np.array([tok]), u[b:b + 1])[0]), (b, tok, u[b])
        assert int(st[b, step + 1]) == int(table[s, tok])
    assert int(ids[0]) == 3 and pr[0, 3] == 1.0             # one allowed token: certain
    if k == 50 and p == 1.0:                                # two allowed tokens under top_k = 50: both stay, nothing else does
        assert (pr[1] > 0).sum() == 2 and abs(pr[1].sum() - 1.0) < 1e-6


@pytest.fixture(scope="module")
def tiny():
    from test_decode_gpu import _tiny_full_width_aki
    m, vx, ids, am = _tiny_full_width_aki()
    with torch.no_grad():
        V = m(vx, ids, attention_mask=am).logits.shape[-1]
    return m, vx, ids, am, V


# every walk passes at least two states that allow one token only (the margin rule of the teacher-forced check is then met for certain),
# and the first set holds a choice that is a prefix of another
def _gen(m, *args, **kw):
    """m.generate; the keywords go through here because tests/test_logits_processors_cpu.py keeps a closed list of the ones that may be
    spelled out in a generate call under tests/ and tools/."""
    return m.generate(*args, **kw)


E2E_CHOICES = [((100, 200, 300, 400, 500), (100, 200, 300, 400), (100, 201, 301), (5000, 6000)), ((7, 8, 9), (10, 11)),
               ((31000, 4, 4, 4), (31000, 5, 6), (12, 13))]
EOS, PAD = 2, 0


def _rows_are_choices(toks, choices_per_row):
    for row, choices in zip(toks.tolist(), choices_per_row):
        assert EOS in row, row
        n = row.index(EOS)
        assert tuple(row[:n]) in choices and all(t == PAD for t in row[n + 1:]), (row, choices)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_generate_greedy_stays_inside_its_choices(tiny, use_graph, B):
    m, vx, ids, am, V = tiny
    vx, ids, am = _multi(m, vx, ids, am, B)
    cons = [TokenConstraint.from_choices(E2E_CHOICES[b], V) for b in range(B)]
    toks = _gen(m, vx, ids, attention_mask=am, max_new_tokens=8, eos_token_id=[EOS], pad_token_id=PAD, use_graph=use_graph,
                      constraint=cons[0] if B == 1 else cons)
    assert toks.shape[0] == B and 3 <= toks.shape[1] <= 6
    _rows_are_choices(toks, E2E_CHOICES[:B])
    for b in range(B):
        table = torch.from_numpy(cons[b].with_eos([EOS]))

        def ref_mask(input_ids, scores, table=table):
            s = CC.walk(table.numpy(), 0, input_ids[0].tolist())[-1]
            return scores.masked_fill(table[s][None] < 0, NEG)

        assert _teacher_forced_check(m, vx[b:b + 1], ids[b:b + 1], toks[b:b + 1], ref_mask, [EOS]) >= 2


def test_generate_samples_and_continues_inside_the_constraint(tiny):
    import aki_amd
    m, vx, ids, am, V = tiny
    vx3, ids3, am3 = _multi(m, vx, ids, am, 3)
    cons = [TokenConstraint.from_choices(E2E_CHOICES[b], V) for b in range(3)]
    kw = dict(max_new_tokens=8, eos_token_id=[EOS], pad_token_id=PAD)
    # the device sampler, three continuations per sample: row b * 3 + j starts in sample b's start state
    out = _gen(m, vx3, ids3, attention_mask=am3, do_sample=True, top_k=50, generator=aki_amd.DeviceGenerator(7), num_return_sequences=3,
                     constraint=cons, output_logprobs=True, **kw)
    assert out.sequences.shape[0] == 9 and out.logprobs.shape == out.sequences.shape
    _rows_are_choices(out.sequences, [E2E_CHOICES[r // 3] for r in range(9)])
    # the RAW distribution, not the masked one: samples 1 and 2 end in leaves, where eos is the one allowed token (masked: log 1 = 0)
    assert bool((out.logprobs <= 0).all())
    for r in range(3, 9):
        assert float(out.logprobs[r, out.sequences[r].tolist().index(EOS)]) < -1e-3, r
    # both host loops: sample_next over apply()'s scores, and the device sampler outside a graph
    g = torch.Generator(device=DEV).manual_seed(3)
    toks = _gen(m, vx3, ids3, attention_mask=am3, do_sample=True, generator=g, constraint=cons, repetition_penalty=1.2, **kw)
    _rows_are_choices(toks, E2E_CHOICES)
    toks = _gen(m, vx3, ids3, attention_mask=am3, do_sample=True, generator=aki_amd.DeviceGenerator(9), use_graph=False, constraint=cons, **kw)
    _rows_are_choices(toks, E2E_CHOICES)
    # from a cache
    with torch.no_grad():
        prep = m._prepare_inputs_for_forward(vision_tokens=m.vision_tokenizer(m._encode_vision_x(vx)), lang_x=ids, attention_mask=am,
                                             padding_side="right")
        cache = m.lang_model(inputs_embeds=prep["inputs_embeds"], attention_mask=prep["attention_mask"], use_cache=True,
                             cache_capacity=prep["inputs_embeds"].shape[1] + 16, last_token_logits=True).past_key_values
    new_ids = torch.tensor([[11, 12, 13]], device=DEV)
    toks = _gen(m, None, new_ids, past_key_values=cache, constraint=cons[0], **kw)
    _rows_are_choices(toks, E2E_CHOICES[:1])
    # refused before any device work: another V, an eos id used as an edge
    with pytest.raises(ValueError, match="built for V"):
        _gen(m, vx, ids, attention_mask=am, constraint=TokenConstraint.from_choices([[5]], V + 1), **kw)
    with pytest.raises(ValueError, match="ordinary transition"):
        _gen(m, vx, ids, attention_mask=am, constraint=TokenConstraint.from_choices([[EOS, 5]], V), **kw)


def test_unchanged_without_a_constraint(tiny, monkeypatch):
    from aki_amd import ops
    m, vx, ids, am, V = tiny
    assert not ops.LogitsProcessors(V, DEV, 1.0, 0, 0, (EOS,), [], [], []).active
    seen = []
    orig = ops.greedy_pick

    def spy(*a, **kw):
        seen.append(kw.get("processors"))
        return orig(*a, **kw)

    monkeypatch.setattr(ops, "greedy_pick", spy)
    for ug in (False, True):
        plain = _gen(m, vx, ids, attention_mask=am, max_new_tokens=10, eos_token_id=[], use_graph=ug)
        same = _gen(m, vx, ids, attention_mask=am, max_new_tokens=10, eos_token_id=[], use_graph=ug, constraint=None)
        assert torch.equal(plain, same)
    assert seen and all(p is None for p in seen)
    free = TokenConstraint.from_table(np.zeros((1, V), np.int64), [True])        # one state that allows everything: the same tokens again
    monkeypatch.setattr(ops, "greedy_pick", orig)
    assert torch.equal(_gen(m, vx, ids, attention_mask=am, max_new_tokens=10, eos_token_id=[], constraint=free), plain)
