"""Logits processors of AKI.generate, the parts that need no GPU: the two entry points are declared, typed and exported; host-side
validation answers before any launch; generate's keyword parsing names what it cannot honour instead of dropping it."""
import os
import re
import subprocess
import types

import pytest
import torch

from conftest import ROOT

NEW = ("aki_logits_process", "aki_greedy_pick_processed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_typed_and_exported(lib):
    from aki_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aki_mi355x.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\bT {name}\b", exported), name
    assert lib.aki_abi_version() == 17
    assert "AKI_LOGITS_PROCESS_MAX_V 131072" in src and _lib.AKI_LOGITS_PROCESS_MAX_V == 131072


FAKE = 1 << 20      # never dereferenced: every call below must be refused on the host


def _process(lib, **over):
    a = dict(logits=FAKE, dtype=0, B=2, V=100, ld=100, out=FAKE, ld_out=100, tokens=FAKE, tokens_ld=8, cache_len=None, start_len=None,
             step=0, done=None, penalty=1.2, ngram=2, min_len=0, eos=None, n_eos=0, sup=None, n_sup=0, bsup=None, n_bsup=0, bad=FAKE,
             off=FAKE, n_bad=1, n_bad_ids=2)
    a.update(over)
    return lib.aki_logits_process(*a.values(), None)


def test_logits_process_validates_on_the_host(lib):
    from aki_amd import _lib
    bad = -1                                            # AKI_ERR_INVALID_ARG
    assert _process(lib, logits=None) == bad
    assert _process(lib, out=None) == bad
    assert _process(lib, ngram=-1) == bad
    assert _process(lib, penalty=0.0) == bad
    assert _process(lib, penalty=-1.5) == bad
    assert _process(lib, penalty=float("inf")) == bad
    assert _process(lib, penalty=float("nan")) == bad
    assert _process(lib, min_len=-3) == bad
    assert _process(lib, n_bad_ids=0) == bad            # an offset table of one word cannot stay inside zero ids
    assert _process(lib, off=None) == bad
    assert _process(lib, bad=None) == bad
    assert _process(lib, n_bad=-1) == bad
    assert _process(lib, n_sup=2) == bad                # ids missing
    assert _process(lib, n_eos=1) == bad
    assert _process(lib, ld=99) == bad
    assert _process(lib, ld_out=50) == bad
    assert _process(lib, step=-1) == bad
    assert _process(lib, V=_lib.AKI_LOGITS_PROCESS_MAX_V + 1, ld=1 << 20, ld_out=1 << 20) == bad
    assert _process(lib, dtype=_lib.AKI_DT_FP8_E4M3) == -2                   # AKI_ERR_UNSUPPORTED


def _pick(lib, **over):
    a = dict(logits=FAKE, B=2, V=100, ld=100, eos=None, n_eos=0, pad=0, done=None, ids=FAKE, tokens=FAKE, tokens_ld=8, cache_len=FAKE,
             start_len=FAKE, advance=1, done_at=None, w=None, extra=None, max_orig=0, n_add=0, d=0, emb_out=None, scores=FAKE, ld_scores=100,
             penalty=1.2, ngram=2, min_len=0, sup=None, n_sup=0, bsup=None, n_bsup=0, bad=FAKE, off=FAKE, n_bad=1, n_bad_ids=2)
    a.update(over)
    return lib.aki_greedy_pick_processed(*a.values(), None)


def test_processed_pick_validates_on_the_host(lib):
    from aki_amd import _lib
    bad = -1                                            # AKI_ERR_INVALID_ARG
    assert _pick(lib, logits=None) == bad
    assert _pick(lib, scores=None) == bad
    assert _pick(lib, ngram=-2) == bad
    assert _pick(lib, penalty=0.0) == bad
    assert _pick(lib, n_bad_ids=0) == bad
    assert _pick(lib, ld_scores=99) == bad
    assert _pick(lib, cache_len=None) == bad            # advance without the counters
    assert _pick(lib, emb_out=FAKE) == bad              # an embedding output without a table
    assert _pick(lib, scores=FAKE + 4) == -3        # AKI_ERR_ALIGNMENT
    assert _pick(lib, ld_scores=102) == -3        # AKI_ERR_ALIGNMENT


def test_processor_object_rejects_bad_arguments():
    from aki_amd import ops
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1), dict(min_length=-1),
               dict(bad_words_ids=[[]]), dict(bad_words_ids=[5]), dict(bad_words_ids=[[3, 100]]), dict(bad_words_ids=[[-1]]),
               dict(suppress_tokens=[100]), dict(begin_suppress_tokens=[-2])):
        with pytest.raises(ValueError):
            ops.LogitsProcessors(100, "cpu", **kw)
    with pytest.raises(ValueError):
        ops.LogitsProcessors(0, "cpu")
    with pytest.raises(ValueError):
        ops.LogitsProcessors(200_000, "cpu", no_repeat_ngram_size=2)
    assert not ops.LogitsProcessors(200_000, "cpu").active                              # a plain generate is not limited by the kernel's V
    assert not ops.LogitsProcessors(100, "cpu", repetition_penalty=1.0, no_repeat_ngram_size=0).active
    assert not ops.LogitsProcessors(100, "cpu", min_length=5).active                   # no eos id: HF adds no min-length processor
    assert ops.LogitsProcessors(100, "cpu", min_length=5, eos_ids=[7]).active
    p = ops.LogitsProcessors(100, "cpu", bad_words_ids=[[7], [8], [7, 9]], eos_ids=[7])
    assert p.words == [[8], [7, 9]]                                                     # HF drops a one-token bad word that is an eos id


def _stub():
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: [])


@pytest.mark.parametrize("kw", ["logits_processor", "stopping_criteria", "return_dict_in_generate", "output_scores", "generation_config",
                                "forced_eos_token_id", "sequence_bias", "no_such_keyword"])
def test_generate_names_keywords_it_cannot_honour(kw):
    """Raised before any device work: vision_x / lang_x are never touched."""
    from aki_amd.aki import AKI
    with pytest.raises(ValueError, match=kw):
        AKI.generate(_stub(), None, None, max_new_tokens=4, **{kw: None})
    with pytest.raises(ValueError, match=kw):
        AKI.generate(_stub(), None, None, max_new_tokens=4, repetition_penalty=1.2, **{kw: 1})


def test_generate_consumes_every_known_keyword():
    """The keywords generate() honours get past the parser (they reach the text-only check, which needs no device)."""
    from aki_amd.aki import AKI
    kw = dict(attention_mask=None, max_new_tokens=4, do_sample=False, eos_token_id=[2], pad_token_id=0, num_beams=1, num_return_sequences=1,
              temperature=1.0, top_k=0, top_p=1.0, generator=None, use_graph=False, length_penalty=1.0, early_stopping=False,
              repetition_penalty=1.3, no_repeat_ngram_size=3, bad_words_ids=[[5]], min_length=2, min_new_tokens=4, suppress_tokens=[9],
              begin_suppress_tokens=[10])
    with pytest.raises(NotImplementedError, match="text-only"):
        AKI.generate(_stub(), None, torch.zeros((1, 3), dtype=torch.long), **kw)


def test_every_generate_caller_in_the_repository_passes_known_keywords():
    """The new ValueError breaks no caller: every keyword passed to .generate( in tests/ and tools/ is one generate() consumes."""
    from aki_amd.aki import PROCESSOR_KWARGS
    known = {"attention_mask", "max_new_tokens", "max_length", "do_sample", "eos_token_id", "pad_token_id", "num_beams", "num_return_sequences",
             "temperature", "top_k", "top_p", "generator", "use_graph", "length_penalty", "early_stopping", "image_size", "past_key_values",
             "past_media_locations", "past_vision_tokens"} | set(PROCESSOR_KWARGS)
    seen = set()
    for d in ("tests", "tools"):
        for root, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py") and f != os.path.basename(__file__):
                    src = open(os.path.join(root, f)).read()
                    for call in re.findall(r"\.generate\(([^()]*(?:\([^()]*\)[^()]*)*)\)", src):
                        seen |= set(re.findall(r"\b([a-z_]+)\s*=(?!=)", call))
    seen.discard("kw")
    assert seen and seen <= known, sorted(seen - known)
