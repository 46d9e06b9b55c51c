"""Per-request logits processors in generate_many, the host half: the numpy reference of tests/many_processor_cases.py against the
installed transformers' processors, the pool of distinct sets (ops.ProcessorSets), the resolution precedence (request over params= over
the call-wide keyword), every validation error with the request's index, and the per-request constraint rule - all before any device
work.  Every test here needs the feature."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import many_constraint_cases as MC
import many_processor_cases as P
from conftest import ROOT
from aki_amd.slots import PROCESSOR_FIELDS, RequestParams, processor_set_key, resolve_processors


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.SETS))
def test_numpy_reference_matches_transformers(name):
    from test_logits_processors_gpu import assert_scores_equal, hf_processors
    V, key = 1000, P.SETS[name]
    hf = hf_processors(**P.hf_kwargs(key))
    h = P.histories(6, 7)
    x = P.bf16_round((np.random.default_rng(5).standard_normal((6, V)) * 4).astype(np.float32))
    x[:, list(P.EOS)] += 3.0
    for b, n in enumerate((0, 1, 7, 23, 39, 40)):
        want = hf(torch.from_numpy(h[b:b + 1, :n]), torch.from_numpy(x[b:b + 1].copy()))[0]
        got = torch.from_numpy(P.reference_row(x[b], h[b, :n], key))
        assert_scores_equal(got, want, f"{name}, n = {n}")
    if name == "neutral":
        assert np.array_equal(P.reference_row(x[0], h[0], key), x[0])


def test_the_tables_cover_what_they_claim():
    assert len(P.SETS) >= 5 and P.SETS["neutral"] == P.NEUTRAL and set(P.ORDERS[0]) == set(P.ORDERS[1]) == set(P.SETS) - {"neutral"}
    seen = set()
    for table in P.TABLES.values():
        assert len(table) == 6
        names = [r[0] for r in table]
        assert "neutral" in names and P.OUT_OF_RANGE in names and sum(r[2] for r in table) == 1
        seen |= {n for name, n, fin in table if not fin and name not in ("neutral", P.OUT_OF_RANGE)}
    assert seen >= {0, 7, 23, 39} and any(r[1] == 1 for t in P.TABLES.values() for r in t)
    x = P.logits(P.TABLES["a"], 1000, 3)
    assert np.array_equal(x, P.bf16_round(x)) and x[5, P.EOS[0]] == 60.0 and x[3, P.EOS[1]] == 60.0


# ---- the pool -----------------------------------------------------------------------------------------------------------------------------
def _pool(keys, V=64, rows=4, eos=P.EOS):
    from aki_amd import ops
    return ops.ProcessorSets(V, "cpu", eos, keys, rows)


def test_pool_deduplicates_by_value_and_keeps_set_0_neutral():
    a = (1.2, 3, 0, (1, 2), (), ((5, 6), (9,)))
    b = (1.0, 0, 4, (), (8,), ())
    ps = _pool([a, P.NEUTRAL, b, (1.2, 3, 0, (1, 2), (), ((5, 6), (9,))), b])
    assert ps.keys == [P.NEUTRAL, a, b] and ps.index == {P.NEUTRAL: 0, a: 1, b: 2}
    one = np.float32(1.0).view(np.int32)
    assert ps.sets.dtype == torch.int32 and ps.sets.tolist() == [
        [one, 0, 0, 0, 0, 0, 0, 0, 0],
        [int(np.float32(1.2).view(np.int32)), 3, 0, 0, 2, 2, 2, 0, 2],       # suppress ids[0:2], no begin ids, words 0 and 1
        [one, 0, 4, 2, 2, 2, 3, 2, 2]]                                       # begin ids[2:3], no words
    assert ps.ids.dtype == torch.int64 and ps.ids.tolist() == [1, 2, 8, 5, 6, 9]            # the plain lists of every set, then the words
    assert ps.bad_off.dtype == torch.int32 and ps.bad_off.tolist() == [3, 5, 6]             # ascending; the last word's end closes it
    words = [ps.ids[ps.bad_off[w]:ps.bad_off[w + 1]].tolist() for w in range(2)]
    assert words == [[5, 6], [9]]
    assert ps.row_set.dtype == torch.int32 and ps.row_set.tolist() == [0, 0, 0, 0]
    ps.admit(2, b)
    ps.admit(0, a)
    assert ps.row_set.tolist() == [1, 0, 2, 0]
    view = ps.row(2)
    assert view.row_set.tolist() == [2] and view.row_set.data_ptr() == ps.row_set[2:].data_ptr() and view.sets is ps.sets
    # a pool without any list: no ids, one closing offset
    bare = _pool([(1.5, 0, 0, (), (), ())])
    assert bare.ids.numel() == 0 and bare.bad_off.tolist() == [0] and bare.sets.shape == (2, 9)
    only = _pool([])
    assert only.keys == [P.NEUTRAL] and only.sets.shape == (1, 9)
    with pytest.raises(ValueError, match=r"\[0, 64\)"):
        _pool([(1.0, 0, 0, (64,), (), ())])


def test_set_key_is_equal_for_equal_behaviour():
    key = lambda eos=(7,), **kw: processor_set_key("request 0", resolve_processors(RequestParams(**kw), None, {}), eos, 64)
    assert key() == P.NEUTRAL == key(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=(), suppress_tokens=[])
    assert key(min_length=3, min_new_tokens=5)[2] == 5 and key(min_length=6, min_new_tokens=5)[2] == 6
    assert key(eos=(), min_new_tokens=5) == P.NEUTRAL                         # nothing to ban without an eos id
    assert key(bad_words_ids=[[7], [7, 8], [9]])[5] == ((7, 8), (9,))         # a one-token bad word equal to an eos id is dropped
    assert key(suppress_tokens=np.array([3, 4]), begin_suppress_tokens=torch.tensor([5])) == (1.0, 0, 0, (3, 4), (5,), ())
    assert key(repetition_penalty=1.2) == key(repetition_penalty=np.float32(1.2)) == key(repetition_penalty=torch.tensor(1.2))
    assert key(repetition_penalty=1.2)[0] == float(np.float32(1.2))           # the float32 the device reads
    for bad in (dict(repetition_penalty=1e39), dict(repetition_penalty=3.1e38), dict(suppress_tokens=torch.tensor([2.5])),
                dict(no_repeat_ngram_size=np.float32(1.5)), dict(bad_words_ids=[[1.25]])):
        with pytest.raises(ValueError, match=f"request 0.*{next(iter(bad))}"):
            key(**bad)
    assert key(repetition_penalty=3.0e38)[0] > 2.9e38 and key(no_repeat_ngram_size=np.int64(2), suppress_tokens=torch.tensor([2.0]))[1:4] == (2, 0, (2,))


# ---- resolution ---------------------------------------------------------------------------------------------------------------------------
def test_resolution_precedence_request_over_params_over_call():
    call = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=None, min_length=0, min_new_tokens=4, suppress_tokens=[9],
                begin_suppress_tokens=None)
    default = RequestParams(no_repeat_ngram_size=2, suppress_tokens=())
    own = RequestParams(repetition_penalty=1.0, min_new_tokens=0, begin_suppress_tokens=[5])
    r = resolve_processors(own, default, call)
    assert r == dict(repetition_penalty=1.0, no_repeat_ngram_size=2, bad_words_ids=(), min_length=0, min_new_tokens=0, suppress_tokens=(),
                     begin_suppress_tokens=[5])
    assert set(r) == set(PROCESSOR_FIELDS)
    # nothing of its own: params=, else the call; and with neither, the call's values as they are
    assert resolve_processors(RequestParams(), default, call)["no_repeat_ngram_size"] == 2
    plain = resolve_processors(RequestParams(), RequestParams(), call)
    assert plain["repetition_penalty"] == 1.2 and plain["no_repeat_ngram_size"] == 3 and plain["suppress_tokens"] == [9]
    assert plain["min_new_tokens"] == 4 and plain["bad_words_ids"] == ()
    assert all(getattr(RequestParams(), f) is None for f in PROCESSOR_FIELDS)


# ---- generate_many's host half --------------------------------------------------------------------------------------------------------------
V_STUB = 64


def _stub(dtype=torch.bfloat16, seen=None):
    """Just enough of a model for generate_many's host half; anything that would be device work raises.  With `seen`, generate() records the
    keywords of each request instead (the slots == 1 path)."""
    def boom(*a, **kw):
        raise AssertionError("device work before the refusal")

    def one(vx, lx, **kw):
        seen.append(kw)
        return torch.tensor([5, 6], dtype=torch.long)

    lm = types.SimpleNamespace(get_output_embeddings=lambda: types.SimpleNamespace(out_features=V_STUB),
                               get_input_embeddings=lambda: types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype)),
                               decode_step=boom, config=None, model=None)
    from aki_amd.aki import AKI
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: list(MC.EOS), lang_model=lm, _prefill_request=boom,
                                 _generate_one=boom if seen is None else one, generate=boom, media_token_id=63, num_tokens_per_vis=4,
                                 _cut_behind_eos=AKI._cut_behind_eos)


def _requests(params):
    ids = torch.tensor([[1, 5, 6]], dtype=torch.long)
    return [(None, ids, 4, p) for p in params]


BAD_VALUES = [(dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.0), "repetition_penalty"),
              (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
              (dict(repetition_penalty="x"), "repetition_penalty"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
              (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"), (dict(min_length=-2), "min_length"),
              (dict(min_new_tokens=-1), "min_new_tokens"), (dict(suppress_tokens=[-1]), "suppress_tokens"),
              (dict(suppress_tokens=5), "suppress_tokens"), (dict(begin_suppress_tokens=[1, -3]), "begin_suppress_tokens"),
              (dict(bad_words_ids=[5]), "bad_words_ids"), (dict(bad_words_ids=[[]]), "bad_words_ids"),
              (dict(bad_words_ids=[[1, -1]]), "bad_words_ids"), (dict(bad_words_ids=7), "bad_words_ids")]


@pytest.mark.parametrize("kw, what", BAD_VALUES, ids=[f"{w}-{i}" for i, (_, w) in enumerate(BAD_VALUES)])
def test_request_params_check_names_the_request(kw, what):
    with pytest.raises(ValueError, match=f"request 3.*{what}"):
        RequestParams(**kw).check(3, 5)


@pytest.mark.parametrize("slots", [3, 1])
def test_generate_many_validates_on_the_host_and_names_the_request(slots):
    from aki_amd.aki import AKI
    plain = RequestParams()
    many = lambda per_request, **kw: AKI.generate_many(_stub(), _requests(per_request), slots=slots, **kw)
    for kw, what in BAD_VALUES:
        with pytest.raises(ValueError, match=f"request 1.*{what}"):
            many([plain, RequestParams(**kw)])
        with pytest.raises(ValueError, match=f"params=.*{what}"):
            many([plain, plain], params=RequestParams(**kw))
    # the checks that need the logits' width
    for kw, what in ((dict(suppress_tokens=[V_STUB]), "suppress_tokens"), (dict(begin_suppress_tokens=[V_STUB + 5]), "begin_suppress_tokens"),
                     (dict(bad_words_ids=[[1, V_STUB]]), "bad_words_ids")):
        with pytest.raises(ValueError, match=rf"request 2.*{what}.*\[0, {V_STUB}\)"):
            many([plain, plain, RequestParams(**kw)])
    with pytest.raises(ValueError, match=rf"request 0.*suppress_tokens.*\[0, {V_STUB}\)"):
        many([plain, RequestParams(suppress_tokens=[1])], suppress_tokens=[V_STUB])        # a call-wide value the first request inherits


@pytest.mark.parametrize("slots", [3, 1])
def test_constraint_rule_is_per_request(slots):
    from aki_amd.aki import AKI
    a = MC.members(V_STUB)[0]
    plain, con = RequestParams(), RequestParams(constraint=a)
    many = lambda per_request, **kw: AKI.generate_many(_stub(), _requests(per_request), slots=slots, **kw)
    neutral = dict(no_repeat_ngram_size=0, bad_words_ids=(), min_length=0, min_new_tokens=0, suppress_tokens=(), begin_suppress_tokens=())
    banning = (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[7]]), dict(min_length=2), dict(min_new_tokens=2), dict(suppress_tokens=[9]),
               dict(begin_suppress_tokens=[9]))
    for ban in banning:
        name = next(iter(ban))
        # refused: its own, inherited from params=, inherited from the call
        with pytest.raises(ValueError, match=f"request 1.*{name}"):
            many([plain, RequestParams(constraint=a, **ban)])
        with pytest.raises(ValueError, match=f"request 2.*{name}"):
            many([RequestParams(**neutral), plain, RequestParams(constraint=a)], params=RequestParams(**ban))
        with pytest.raises(ValueError, match=f"request 1.*{name}"):
            many([plain, con], **ban)
        # legal up to the device: a constrained request next to a banning one, and one that overrides the call's keyword with the
        # neutral value - the stub's CPU tensors then stop the call at "needs bf16 logits on the GPU", behind every host check
        with pytest.raises(ValueError, match="request 0.*bf16"):
            many([con, RequestParams(**ban)])
        with pytest.raises(ValueError, match="request 1.*bf16"):
            many([plain, RequestParams(constraint=a, **{name: neutral[name]})], **ban)
    with pytest.raises(ValueError, match="request 0.*bf16"):
        many([RequestParams(constraint=a, repetition_penalty=1.3), plain], repetition_penalty=1.1)      # the penalty composes
    # the rule is judged on the normal form: arrays and tensors are lists, and what bans nothing after normalisation is no ban
    with pytest.raises(ValueError, match="request 1.*suppress_tokens"):
        many([plain, RequestParams(constraint=a, suppress_tokens=np.array([3, 4]))])
    with pytest.raises(ValueError, match="request 0.*begin_suppress_tokens"):
        many([RequestParams(constraint=a, begin_suppress_tokens=torch.tensor([3, 4])), plain])
    with pytest.raises(ValueError, match="request 0.*bf16"):
        many([RequestParams(constraint=a, bad_words_ids=[[MC.EOS[0]]]), plain])                         # a one-token bad word that is an eos id is dropped
    from aki_amd.slots import banning_keywords
    r = resolve_processors(RequestParams(min_new_tokens=4, min_length=2, bad_words_ids=[[7]], repetition_penalty=1.3), None, {})
    assert banning_keywords("request 0", r, (), V_STUB) == ["bad_words_ids"]                            # no eos id: a minimum length bans nothing
    assert banning_keywords("request 0", r, (7,), V_STUB) == ["min_length", "min_new_tokens"]           # ... and with one the word is dropped


def test_one_slot_hands_each_request_its_resolved_keywords():
    from aki_amd.aki import AKI
    seen = []
    params = [RequestParams(), RequestParams(repetition_penalty=1.0, suppress_tokens=[4]), RequestParams(min_new_tokens=0, bad_words_ids=[[8, 9]])]
    AKI.generate_many(_stub(seen=seen), _requests(params), slots=1, repetition_penalty=1.2, min_new_tokens=3,
                      params=RequestParams(no_repeat_ngram_size=2))
    pick = lambda kw: {f: kw[f] for f in PROCESSOR_FIELDS}
    base = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, bad_words_ids=(), min_length=0, min_new_tokens=3, suppress_tokens=(),
                begin_suppress_tokens=())
    assert [pick(kw) for kw in seen] == [base, dict(base, repetition_penalty=1.0, suppress_tokens=[4]),
                                         dict(base, min_new_tokens=0, bad_words_ids=[[8, 9]])]


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib as L
    lib = L.load()
    assert {"aki_logits_process_rows", "aki_greedy_pick_rows", "aki_sample_pick_rows_processed"} <= set(L.SIGNATURES)
    src = open(os.path.join(ROOT, "include", "aki_mi355x.h")).read()
    assert "AKI_PROCESSOR_SET_WORDS 9" in src and L.AKI_PROCESSOR_SET_WORDS == 9
    buf = C.create_string_buffer(256)
    Pp = C.cast(buf, C.c_void_p).value                          # 16-byte alignment is checked before any launch; nothing is dereferenced
    Pp = (Pp + 15) // 16 * 16

    def process(logits=Pp, B=2, V=64, sets=Pp, n_sets=3, row_set=Pp, ids=Pp, n_ids=4, off=Pp, n_words=2, table=None, states=None, base=None,
                dtype=L.AKI_DT_BF16):
        return lib.aki_logits_process_rows(logits, dtype, B, V, 64, Pp, 64, None, 0, None, None, 0, None, None, 0, sets, n_sets, row_set, ids,
                                           n_ids, off, n_words, table, 64, 5, states, 1, base, base, None)

    def greedy(logits=Pp, B=2, V=64, scores=Pp, sets=Pp, n_sets=3, row_set=Pp, ids=Pp, n_ids=4, off=Pp, n_words=2, table=None, states=None):
        return lib.aki_greedy_pick_rows(logits, B, V, 64, None, 0, 0, None, Pp, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, scores, 64,
                                        sets, n_sets, row_set, ids, n_ids, off, n_words, table, 64, 5, states, 1, Pp, Pp, None)

    def sample(logits=Pp, B=2, V=64, scores=Pp, sets=Pp, n_sets=3, row_set=Pp, ids=Pp, n_ids=4, off=Pp, n_words=2, T=Pp, seed=Pp, step=0,
               table=None, states=None):
        return lib.aki_sample_pick_rows_processed(logits, B, V, 64, None, 0, 0, None, Pp, None, 0, None, None, 0, None, None, None, 0, 0, 0, None,
                                                  scores, 64, sets, n_sets, row_set, ids, n_ids, off, n_words, step, T, Pp, Pp, seed, None, 0,
                                                  table, 64, 5, states, 1, Pp, Pp, None)

    bad = lib.aki_logits_process_rows(None, L.AKI_DT_BF16, 2, 64, 64, Pp, 64, None, 0, None, None, 0, None, None, 0, Pp, 3, Pp, Pp, 4, Pp, 2, None, 0, 0,
                                      None, 0, None, None, None)
    assert bad != 0
    for f in (process, greedy, sample):
        refused = [f(logits=None), f(B=0), f(V=L.AKI_LOGITS_PROCESS_MAX_V + 8), f(sets=None), f(n_sets=0), f(row_set=None),
                   f(ids=None), f(n_ids=-1), f(off=None), f(n_words=-1), f(n_words=1, ids=None, n_ids=0), f(table=Pp, states=None)]
        assert all(rc == bad for rc in refused), (f.__name__, refused)
    assert greedy(scores=None) == bad and sample(scores=None) == bad and sample(T=None) == bad and sample(seed=None) == bad
    assert sample(step=-1) == bad
    assert greedy(scores=Pp + 4) == sample(scores=Pp + 4) != bad and b"aligned" in lib.aki_strerror(greedy(scores=Pp + 4))
    assert process(dtype=77) not in (0, bad)
