"""The case table of the grouped decode attention kernel checked against itself (no GPU): every REQUIRED corner of the launch plan is
reached, every mutation of the float64 reference moves an output element by at least MIN_RATIO (8) tolerances on at least one input
family, and the two new C symbols are declared, mirrored in ctypes and exported by the cross-compiled library.

Smallest ratio found over the mutation table, taking for every mutation its best case and family: 169.3, for
rows_past_16_dropped on n17-h2-p655-two-chunks (both families; the other mutations reach 278 - merge_without_rescaling on
n33-h2-p130-three-chunks, diffuse - to 3784).  test_every_mutation_is_visible prints every figure before it asserts."""
import os
import re
import subprocess

import pytest

import decode_group_cases as G

ROOT = G.__file__.rsplit(os.sep, 2)[0]
SMALL = [c for c in G.CASES if c.rows * c.H * (max(c.plens) + max(c.slens)) <= 300000]


def test_required_corners_are_covered():
    seen = set()
    for c in G.CASES:
        seen |= G.properties(c)
    missing = [p for p in G.REQUIRED if p not in seen]
    assert not missing, f"no case reaches {missing}"


def test_plan_keeps_the_key_cuts_of_eager_and_captured_steps():
    for c in G.CASES:
        eager, captured = c.key_bounds()
        a, b = G.plan(c.B0, c.N, c.H, c.pcap, c.scap, *eager), G.plan(c.B0, c.N, c.H, c.pcap, c.scap, *captured)
        assert a[1] == b[1] and a[3] == b[3], f"{c.id}: tiles per item differ between an eager and a captured step"
        assert a[0] <= b[0] and a[2] <= b[2]


@pytest.mark.parametrize("mut", G.MUTATIONS)
def test_every_mutation_is_visible(mut):
    best, where = 0.0, None
    for c in SMALL:
        for fam in G.FAMILIES:
            r = G.mutation_ratio(G.make_inputs(c, fam), mut)
            print(f"{mut:28s} {c.id:40s} {fam:9s} {r:10.1f}")
            if r > best:
                best, where = r, (c.id, fam)
    assert best >= G.MIN_RATIO, f"{mut}: largest error / tolerance {best:.2f} ({where}) is below {G.MIN_RATIO}"


def test_reference_of_a_fully_masked_prefix_is_the_suffix_alone():
    c = G.CASE_BY_ID["n3-h4-p65-s64-65-300-prefix-masked"]
    inp = G.make_inputs(c, "sentinel")
    import numpy as np
    for r in range(c.N, 2 * c.N):
        a = G.reference_row(inp, r)
        assert np.isfinite(a).all() and np.abs(a).max() < G.MASKED_V / 2, "a masked prefix column leaked into the reference"


def test_new_symbols_are_declared_mirrored_and_exported():
    from aki_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "aki_mi355x.h")).read()
    for sym in ("aki_decode_attn_group_workspace_bytes", "aki_decode_attn_group_fwd"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), f"{sym} is not declared in the header"
        assert sym in _lib.SIGNATURES, f"{sym} has no ctypes mirror"
    lib = build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for sym in ("aki_decode_attn_group_workspace_bytes", "aki_decode_attn_group_fwd"):
        assert re.search(r"\bT " + sym + r"\b", out), f"{sym} is not exported by {os.path.basename(lib)}"
