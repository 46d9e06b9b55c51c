"""The scripted beam-search cases (tests/beam_cases.py) are sound before any kernel sees them: every decision of the float64 reference
has a margin of at least four times the bound stated for the kernels' f32 arithmetic, every planted situation occurs, and the C ABI
declares the three launches without a version bump."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import beam_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", bc.NAMES)
def test_every_margin_is_four_bounds_and_every_planted_event_occurs(name):
    c = bc.case(name)
    s = c.spec
    print(f"{name}: M {c.M:.4g}, logprob bound {c.logprob_bound:.3g}, bound {c.bound:.3g}, smallest margin {c.min_margin:.3g}, "
          f"events {sorted(c.events)}")
    assert c.min_margin >= 4.0 * c.bound, f"{name}: margin {c.min_margin:.3g} < 4 * {c.bound:.3g}"
    assert s["expect"] <= c.events, f"{name}: {sorted(s['expect'] - c.events)} did not occur"
    assert len(c.ref.steps) == s["T"] and c.logits.shape == (s["T"], s["B"] * s["K"], s["V"])
    assert np.array_equal(c.logits, bc.round_bf16(c.logits)), "the logits are bf16 values"


def test_the_cases_cover_what_the_kernel_can_meet():
    specs = bc.SPECS
    assert {s["K"] for s in specs} == {1, 2, 3, 4, 8, 16} and {s["B"] for s in specs} == {1, 3}
    assert {s["V"] for s in specs} == {64, 1000, 32064 + 6} and max(s["T"] for s in specs) == 6
    assert {s["lp"] for s in specs} == {0.0, 1.0, 2.0} and {repr(s["es"]) for s in specs} == {"True", "False", "'never'"}
    events = set().union(*(bc.case(s["name"]).events for s in specs))
    assert {"eos_hyp", "eos_ignored", "slots_unfilled", "evicted", "closing", "done_at_2", "tie_in", "tie_k", "tie_2k"} <= events
    done2 = bc.case("k2_b3_v64_done_at_2").ref.steps
    assert done2[2]["done"].tolist() == [1, 0, 0] and done2[-1]["done"][1:].tolist() == [0, 0], "one sample done at step 2, the others run on"
    assert any(len(s["eos"]) == 2 and "slots_unfilled" in bc.case(s["name"]).events for s in specs)


def test_reference_ranks_exact_ties_by_the_lower_flat_index():
    ref = bc.RefSearch(1, 2, 1, [], 0, 1.0, False)
    ref.scores[:] = 0.0
    logits = np.zeros((2, 8), dtype=np.float32)
    logits[0, 5] = logits[0, 2] = logits[1, 1] = logits[1, 6] = 3.0          # two rows with the same log-sum-exp: four equal scores
    assert [(k, v) for _, k, v in ref.rank(logits, 0, 5)] == [(0, 2), (0, 5), (1, 1), (1, 6), (0, 0)]


def test_bounds_grow_with_magnitude_width_and_length():
    assert bc.logprob_bound(20.0, 32070) > bc.logprob_bound(20.0, 64) > bc.logprob_bound(10.0, 64) > 0
    assert bc.hyp_bound(20.0, 1000, 5) > bc.score_bound(20.0, 1000, 5) > bc.score_bound(20.0, 1000, 0) > bc.logprob_bound(20.0, 1000)
    assert 1e-5 < bc.hyp_bound(20.0, 32070, 5) < 1e-3, "six steps of f32 rounding at the real width: a few 1e-4"


def test_abi_declares_the_beam_launches_without_a_version_bump():
    from aki_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aki_mi355x.h")).read()
    assert re.search(r"#define\s+AKI_ABI_VERSION\s+17\b", header) and L.AKI_ABI_VERSION == 17
    want = {"aki_beam_logprob": 8, "aki_beam_step": 24, "aki_kv_beam_reorder": 13}
    for name, n_args in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/aki_mi355x.h"
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[-1] is C.c_void_p, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == n_args, f"{name}: the header and _lib.SIGNATURES disagree on the argument count"
    assert (L.AKI_BEAM_MAX_K, L.AKI_BEAM_MAX_EOS, L.AKI_KV_BEAM_REORDER_CHUNK) == (16, 8, 16)
    for macro, value in (("AKI_BEAM_MAX_K", 16), ("AKI_BEAM_MAX_EOS", 8), ("AKI_KV_BEAM_REORDER_CHUNK", 16)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", header)
    src = open(os.path.join(ROOT, "aki_amd", "csrc", "beam.hip")).read()
    assert re.search(r"BEAM_THREADS\s*=\s*%d\b" % bc.KERNEL_THREADS, src), "the bound counts the kernel's additions per thread"
