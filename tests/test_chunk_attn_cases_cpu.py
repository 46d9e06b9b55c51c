"""The chunk attention case table checked on the host: every required corner is reached, every mutation of the float64 reference is
visible well above the tolerance in some case, the reference agrees with a dense masked softmax, and the ABI addition is in place."""
import os
import re

import numpy as np
import pytest

import chunk_attn_cases as C

SMALL = [c for c in C.CASES if c.id != C.LARGEST]            # the mutations are evaluated on the short cases: the issue's "short-cache cases"


def test_every_required_property_is_reached():
    reached = set()
    for c in C.CASES:
        reached |= C.properties(c)
    missing = [p for p in C.REQUIRED if p not in reached]
    assert not missing, f"no case reaches {missing}"


@pytest.fixture(scope="module")
def ratios():
    best = {}
    for c in SMALL:
        for fam in C.FAMILIES:
            for name, r in C.mutation_ratios(C.make_inputs(c, fam)).items():
                if r > best.get(name, (0.0,))[0]:
                    best[name] = (r, c.id, fam)
    return best


@pytest.mark.parametrize("mut", list(C.MUTATIONS))
def test_every_mutation_is_visible(ratios, mut):
    assert mut in ratios, f"{mut} applies to no row of any case"
    r, cid, fam = ratios[mut]
    print(f"{mut}: {r:.1f} tolerances in {cid} / {fam}")
    assert r >= C.MIN_RATIO, f"{mut}: at most {r:.2f} tolerances ({cid}, {fam}); the bar is {C.MIN_RATIO}"


def test_applies_follows_the_rules():
    c = C.CASE_BY_ID["b2-h4-cap128-lens40-30-T16-nnew16-0-prefix-masked"]
    assert not C.applies(c, "rope_at_chunk_index", (0, 3)), "a fully masked prefix hides a common rotation"
    assert not C.applies(c, "causal_one_short", (1, 0)), "sample 1 brings no token"
    assert C.applies(c, "causal_one_short", (0, 0)) and not C.applies(c, "sees_next", (0, 15)) and C.applies(c, "sees_next", (0, 14))
    c = C.CASE_BY_ID["b1-h2-cap256-len100-T65"]
    assert C.applies(c, "block_rows_swapped", (0, 0)) and C.applies(c, "block_rows_swapped", (0, 64)) and not C.applies(c, "next_sample_cache", (0, 0))


@pytest.mark.parametrize("cid", ["b2-h2-cap128-lens1-63-T31-nnew31-2-holes", "b1-h2-cap256-len100-T65"])
def test_reference_equals_a_dense_masked_softmax(cid):
    c = C.CASE_BY_ID[cid]
    for fam in C.FAMILIES:
        inp = C.make_inputs(c, fam)
        ref = C.reference(inp)
        for b in range(c.B):
            nn = c.n_new[b]
            dense = C.dense_reference(inp, b)
            assert np.allclose(ref[b, :nn], dense, rtol=1e-10, atol=1e-10), f"{cid} {fam} sample {b}"
            assert not ref[b, nn:].any()


def test_inputs_hold_nan_where_nothing_may_be_read():
    c = C.CASE_BY_ID["b2-h2-cap128-lens1-63-T31-nnew31-2-holes"]
    inp = C.make_inputs(c, "self")
    for b in range(c.B):
        assert inp.k[b, :, c.lens[b]:].isnan().all() and inp.v[b, :, c.lens[b]:].isnan().all()
        assert not inp.k[b, :, :c.lens[b]].isnan().any()
    q = inp.qkv.view(c.B, c.T, -1)
    assert q[1, 2:].isnan().all() and not q[1, :2].isnan().any() and np.isfinite(C.reference(inp)).all()


def test_abi_addition():
    from aki_amd import _lib
    assert "aki_chunk_attn_fwd" in _lib.SIGNATURES and "aki_chunk_attn_workspace_bytes" in _lib.SIGNATURES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "aki_mi355x.h")) as f:
        text = f.read()
    assert re.search(r"^#define\s+AKI_ABI_VERSION\s+17\b", text, re.M), "the addition is purely additive: the ABI version stays 17"
    assert "aki_chunk_attn_fwd(" in text and "aki_chunk_attn_workspace_bytes(" in text
