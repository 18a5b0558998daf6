"""CPU-side check of the walk kernel as it compiles for gfx950: no resident k_walk instantiation keeps anything in private memory
(scratch).  A select chain over an array held in registers (a row's neighbour index, the words of a k-mer) is easily folded back by
the compiler into a load at a computed offset from a stack copy of the array: a private-memory round trip on the critical path of a
step, which shows up here as a non-zero private segment.  Needs hipcc (cross-compiles, no GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corticall_amd", "csrc")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def walk_kernels(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "walk.s")
    # the flags of the product build (csrc/Makefile: HIPFLAGS), device code only, as assembly
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                           "--offload-device-only", "-S", os.path.join(CSRC, "walk.cpp"), "-o", out], cwd=CSRC,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(_ZN4ldbg6k_walkILi(\d)ELi(\d+)ELb([01])EEEvNS_8WalkArgsE)\n((?:[ \t]+\..*\n)+)", text):
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(5))
        vgpr = re.search(r"\.vgpr_count:\s+(\d+)", m.group(5))
        kernels[(int(m.group(2)), int(m.group(3)), m.group(4) == "1")] = (int(priv.group(1)), int(vgpr.group(1)))
    return kernels


def test_resident_walk_kernels_have_no_private_segment(walk_kernels):
    resident = {key: v for key, v in walk_kernels.items() if not key[2]}
    # every instantiation the host dispatches to (walk.cpp: W = 1..4 words, 16 / 32 / 64 lanes per workgroup) is in the object
    assert set(resident) == {(w, bs, False) for w in (1, 2, 3, 4) for bs in (16, 32, 64)}, sorted(resident)
    bad = {key: priv for key, (priv, _) in resident.items() if priv != 0}
    assert not bad, "k_walk<W, BS, false> with a private segment (bytes): %s" % bad


def test_resident_walk_kernels_fit_two_wavefronts_per_simd(walk_kernels):
    # Engine::walk_prepare sizes the resident grid for 2 wavefronts per SIMD (512 VGPRs per lane and SIMD): at most 256 each
    for key, (_, vgpr) in walk_kernels.items():
        if not key[2]:
            assert vgpr <= 256, (key, vgpr)
