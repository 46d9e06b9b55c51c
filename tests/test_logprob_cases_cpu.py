"""Per-token log-probabilities, the parts that need no GPU: the cases' float64 reference against a second formulation, the features every
case is meant to carry, the entry point's declaration / typing / export and its host-side validation, and the keyword parsing of
generate and the argument checks of score, which answer before any device is touched."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import logprob_cases as LC

AKI_ERR_INVALID_ARG, AKI_ERR_UNSUPPORTED, AKI_DT_BF16, AKI_DT_F32 = -1, -2, 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_reference_agrees_with_a_second_formulation(name):
    """log-softmax by pairwise logaddexp (and scipy's logsumexp where it is installed) against the reference's max-shifted sum; the ranking
    against a stable argsort; the inputs are bf16-exact and every row reaches the case's M."""
    x, ids = LC.make(name)
    V, rows, M, _ = LC.CASES[name]
    assert x.shape == (rows, V) and x.dtype == np.float32 and ids.shape == (rows,)
    assert np.array_equal(LC.bf16_exact(x), x) and not np.isnan(x).any() and np.isfinite(x).any(axis=1).all()
    assert np.abs(np.where(np.isfinite(x), x, 0)).max() == M
    for k in LC.TOP_KS:
        lp, top_ids, top_lp, bound = LC.reference(x, ids, k)
        x64 = x.astype(np.float64)
        lse = np.logaddexp.reduce(x64, axis=1)
        want = x64[np.arange(rows), ids] - lse
        same_inf = np.isinf(want) == np.isinf(lp)
        assert same_inf.all() and np.allclose(np.where(np.isinf(lp), 0, lp), np.where(np.isinf(want), 0, want), rtol=0, atol=1e-11)
        try:
            from scipy.special import logsumexp
            assert np.allclose(logsumexp(x64, axis=1), lse, rtol=0, atol=1e-11)
        except ImportError:
            pass
        n = min(k, V)
        order = np.argsort(-x64, axis=1, kind="stable")[:, :n]
        assert np.array_equal(top_ids[:, :n], order) and (top_ids[:, n:] == -1).all() and np.isneginf(top_lp[:, n:]).all()
        assert (bound > 0).all() and (bound < 1e-4).all()
        # a distribution: the probabilities of a whole row add up to one
        assert np.allclose(np.exp(x64 - lse[:, None]).sum(axis=1), 1.0, atol=1e-12)


def test_bound_is_the_beam_bound_plus_the_longer_thread_chain():
    import beam_cases
    for M, V in ((1.0, 2), (30.0, 1025), (80.0, 32013)):
        assert LC.logprob_bound(M, V) == pytest.approx(beam_cases.logprob_bound(M, V) + 8 * LC.U, rel=1e-12)


def test_cases_carry_their_features():
    assert {LC.CASES[n][0] for n in LC.CASES} >= {2, 1023, 1024, 1025, 32013}
    assert {LC.CASES[n][1] for n in LC.CASES} >= {1, 3, 33}
    assert {LC.CASES[n][2] for n in LC.CASES} >= {1.0, 30.0, 80.0}
    assert set(LC.TOP_KS) == {0, 1, 8}
    seen = set()
    for name in LC.CASES:
        x, ids = LC.make(name)
        V = x.shape[1]
        seen |= {"first" for r in range(len(ids)) if ids[r] == 0} | {"last" for r in range(len(ids)) if ids[r] == V - 1}
        seen |= {"neginf id" for r in range(len(ids)) if np.isneginf(x[r, ids[r]])}
    assert seen == {"first", "last", "neginf id"}
    x, _ = LC.make("ties_v1025")
    s = -np.sort(-x.astype(np.float64), axis=1)
    assert s[0, 0] == s[0, 1] and s[0, 7] == s[0, 8] and s[0, 9] > s[0, 10]        # row 0: ties across rank 1 | 2 and 8 | 9 and inside the top 8
    assert s[1, 2] == s[1, 3] and s[1, 7] == s[1, 8] and s[1, 0] > s[1, 1] > s[1, 2] and s[1, 3] > s[1, 4] and s[1, 8] > s[1, 9]
    assert (x[2] == x[2, 0]).all()                                                    # row 2: a constant row
    for name in ("neginf_v1024", "neginf_v32013"):
        x, ids = LC.make(name)
        V = x.shape[1]
        holes = np.isneginf(x).sum(axis=1)
        assert holes[0] == V // 10 and V - holes[1] == len(LC.NEGINF_FINITE) < max(LC.TOP_KS) and holes[2] == 2
        assert np.isneginf(x[2, [0, V - 1]]).all()
        _, top_ids, top_lp, _ = LC.reference(x, ids, 8)
        assert np.isneginf(top_lp[1, len(LC.NEGINF_FINITE):]).all() and np.isfinite(top_lp[1, :len(LC.NEGINF_FINITE)]).all()
        assert (top_ids[1, len(LC.NEGINF_FINITE):] == [0, 1, 2]).all()              # -inf columns last, the lower column first


def test_new_symbol_is_declared_typed_and_exported(lib):
    from aki_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aki_mi355x.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\baki_token_logprob\s*\(", src)
    assert "aki_token_logprob" in _lib.SIGNATURES
    assert re.search(r"\bT aki_token_logprob\b", exported)
    assert lib.aki_abi_version() == 17 and _lib.AKI_ABI_VERSION == 17
    assert re.search(r"#define AKI_LOGPROB_MAX_TOP 8\b", src) and _lib.AKI_LOGPROB_MAX_TOP == 8 == ops.LOGPROB_MAX_TOP
    assert re.search(r"#define AKI_LOGPROB_MAX_V 262144\b", src) and _lib.AKI_LOGPROB_MAX_V == 262144 >= 200000
    assert "logprob.hip" in __import__("aki_amd.build", fromlist=["SOURCES"]).SOURCES


def test_entry_point_validates_on_the_host_before_any_launch(lib):
    """Every call below is wrong in one argument and answers with an error code: no kernel is launched (there is no device here)."""
    buf = torch.zeros(64, dtype=torch.float32)
    p = buf.data_ptr()

    def call(logits=p, dtype=AKI_DT_F32, rows=1, V=4, ld=4, ids=p, tokens=None, tokens_ld=0, cache_len=None, start_len=None, step=0, skip=None,
             done_at=None, top_k=0, out=p, top_ids=None, top_lp=None, out_ld=1, out_cols=1):
        return lib.aki_token_logprob(logits, dtype, rows, V, ld, ids, tokens, tokens_ld, cache_len, start_len, step, skip, done_at, top_k, out,
                                     top_ids, top_lp, out_ld, out_cols, None)

    for bad in (dict(logits=None), dict(out=None), dict(ids=None), dict(rows=0), dict(rows=-1), dict(V=0), dict(V=-3), dict(ld=3), dict(step=-1),
                dict(out_cols=0), dict(out_ld=0), dict(cache_len=p), dict(start_len=p), dict(ids=None, tokens=p, tokens_ld=0),
                dict(top_k=1), dict(top_k=8, top_ids=p)):
        assert call(**bad) == AKI_ERR_INVALID_ARG, bad
    for bad in (dict(top_k=-1), dict(top_k=9, top_ids=p, top_lp=p), dict(dtype=2), dict(V=262145, ld=262145)):
        assert call(**bad) == AKI_ERR_UNSUPPORTED, bad


def test_ops_wrapper_rejects_cpu_tensors_dtypes_and_strides():
    from aki_amd import ops
    from aki_amd._lib import AkiError
    with pytest.raises(AkiError, match="CPU"):
        ops.token_logprob(torch.zeros(2, 8), ids=torch.zeros(2, dtype=torch.long))
    with pytest.raises(AkiError, match="unit column stride"):
        ops.token_logprob(torch.zeros(8, 2).t(), ids=torch.zeros(2, dtype=torch.long))
    with pytest.raises(AkiError, match="top_k"):
        ops.token_logprob(torch.zeros(2, 8), ids=torch.zeros(2, dtype=torch.long), top_k=9)


def _stub():
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: [])


def test_generate_parses_the_logprob_keywords():
    from aki_amd.aki import AKI
    lx = torch.zeros((1, 3), dtype=torch.long)
    for opts in (dict(output_logprobs=True), dict(output_logprobs=True, top_logprobs=8), dict(output_logprobs=False, top_logprobs=0),
                 dict(output_logprobs=True, top_logprobs=3, do_sample=True, num_return_sequences=2)):
        with pytest.raises(NotImplementedError, match="text-only"):                  # past the parser: the text-only check needs no device
            AKI.generate(_stub(), None, lx, max_new_tokens=4, **opts)
    for opts, what in ((dict(top_logprobs=2), "output_logprobs"), (dict(output_logprobs=True, top_logprobs=9), "0..8"),
                       (dict(output_logprobs=True, top_logprobs=-1), "0..8")):
        with pytest.raises(ValueError, match=what):
            AKI.generate(_stub(), None, lx, max_new_tokens=4, **opts)
    opts = dict(output_logprobs=True, num_beams=2)
    with pytest.raises(NotImplementedError, match="output_logprobs"):
        AKI.generate(_stub(), None, lx, max_new_tokens=4, **opts)
    for kw in ("return_dict_in_generate", "output_scores"):                          # HF's own names stay refused
        with pytest.raises(ValueError, match=kw):
            AKI.generate(_stub(), None, lx, max_new_tokens=4, **{kw: True})


def test_score_validates_before_touching_a_device():
    from aki_amd.aki import AKI
    import aki_amd
    assert aki_amd.AkiScoreOutput.__name__ == "AkiScoreOutput" and aki_amd.AkiGenerateOutput.__name__ == "AkiGenerateOutput"
    from transformers.utils import ModelOutput
    assert issubclass(aki_amd.AkiGenerateOutput, ModelOutput) and issubclass(aki_amd.AkiScoreOutput, ModelOutput)
    lx = torch.zeros((2, 3), dtype=torch.long)
    cont = torch.zeros((2, 2, 3), dtype=torch.long)
    bad = [dict(continuations=cont[0]), dict(continuations=cont.int()), dict(continuations=cont[:1]), dict(continuations=cont[:, :, :0]),
           dict(continuations=cont.tolist()), dict(continuations=cont, continuation_lengths=torch.ones(2, 3, dtype=torch.long)),
           dict(continuations=cont, continuation_lengths=torch.tensor([[3, 0], [1, 1]])),
           dict(continuations=cont, continuation_lengths=torch.tensor([[3, 4], [1, 1]])),
           dict(continuations=cont, continuation_lengths=torch.ones(2, 2)), dict(continuations=cont, top_logprobs=9),
           dict(continuations=cont, top_logprobs=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            AKI.score(_stub(), object(), lx, **kw)                                   # vision_x is never looked at
    with pytest.raises(NotImplementedError, match="text-only"):
        AKI.score(_stub(), None, lx, cont, continuation_lengths=torch.tensor([[3, 1], [2, 3]]), top_logprobs=8)
    from aki_amd.modeling_aki import AKI as Twin
    assert Twin.score is AKI.score
