"""CPU-side check of the fixed-layout walk kernels as they compile for gfx950 (walk.cpp: k_walk_rows<W, C>, the probe-row layout compiled
in): all six are in the object, each fits a compute unit eight times as the generic kernel does (no private segment, 18,432 B of LDS, at
most 256 VGPRs), and folding the layout in really shrinks the kernel — k_walk_rows<2, 3> against k_walk<2, 64, false> OF THE SAME COMPILE:
fewer instructions, fewer spilled SGPRs, fewer 64-bit multiplies.  The counts are compared, not fixed: they move with the compiler.
Counted by tools/walk_isa.py.  Needs hipcc (cross-compiles, no GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS = "_ZN4ldbg11k_walk_rowsILi%dELi%dEEEvNS_8WalkArgsE"
GENERIC = "_ZN4ldbg6k_walkILi2ELi64ELb0EEEvNS_8WalkArgsE"
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import walk_isa
    if not any(c and os.path.exists(c) for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("rows_isa") / "walk.s")
    walk_isa.compile_walk(out)
    return walk_isa.kernels_of(open(out).read())


def test_all_six_fixed_kernels_are_in_the_object(kernels):
    have = {n for n in kernels if "k_walk_rows" in n}
    assert have == {ROWS % (w, c) for w in (1, 2) for c in (1, 2, 3)}, sorted(have)


def test_fixed_kernels_fit_a_cu_eight_times(kernels):
    for w in (1, 2):
        for c in (1, 2, 3):
            m = kernels[ROWS % (w, c)]["meta"]
            print("k_walk_rows<%d, %d>: %s, %s" % (w, c, m, kernels[ROWS % (w, c)]["all"]))
            assert m["private"] == 0, (w, c, m)
            assert m["lds"] == 18432 and 8 * m["lds"] <= CU_LDS, (w, c, m)
            assert m["vgpr"] <= 256, (w, c, m)


def test_folding_the_layout_in_shrinks_the_kernel(kernels):
    rows, gen = kernels[ROWS % (2, 3)], kernels[GENERIC]
    print("k_walk<2, 64, false>: %s, %s" % (gen["meta"], gen["all"]))
    print("k_walk_rows<2, 3>:    %s, %s" % (rows["meta"], rows["all"]))
    assert rows["all"]["instructions"] < gen["all"]["instructions"]
    assert rows["meta"]["sgpr_spill"] < gen["meta"]["sgpr_spill"]
    assert rows["all"]["mul64"] < gen["all"]["mul64"]
