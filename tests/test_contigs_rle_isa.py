"""CPU-side check of the contig kernels as they compile for gfx950: k_contigs_rle<W> and k_contigs_repeat<W> (csrc/walk.cpp), W = 1..4, keep
at most 64 VGPRs and nothing in private memory.  k_contigs_rle runs beside the other engine's resident k_walk launch, whose wavefronts
take 240 of a SIMD's 512 VGPRs each: at 64 registers four contig wavefronts fit beside one walk wavefront, at 80 three did.
Reads only the compiler's resource remarks (-Rpass-analysis=kernel-resource-usage).  Needs hipcc (cross-compiles, no GPU)."""
import os
import re
import subprocess

import pytest

from tests.test_walk_isa import CSRC, _hipcc

KERNELS = ("k_contigs_rle", "k_contigs_repeat")


@pytest.fixture(scope="module")
def contig_kernels(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "walk.o")
    # the flags of the product build (csrc/Makefile: HIPFLAGS), device code only, as tests/test_walk_isa.py compiles it; the remarks go to stderr
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                        "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "walk.cpp"), "-o", out],
                       cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: _ZN4ldbg\d+(k_contigs_rle|k_contigs_repeat)ILi(\d)EEEvNS_13ContigRleArgsE", line)
        if m:
            name = (m.group(1), int(m.group(2)))
            found[name] = {}
            continue
        if "remark: Function Name:" in line:
            name = None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and name is not None:
            found[name][m.group(1)] = int(m.group(2))
    return found


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_contig_kernel_registers(contig_kernels, kernel, W):
    assert (kernel, W) in contig_kernels, sorted(contig_kernels)
    r = contig_kernels[(kernel, W)]
    print("%s<%d>: %d VGPRs, %d AGPRs, %d SGPRs, private segment %d B, %d waves/SIMD" % (
        kernel, W, r["VGPRs"], r["AGPRs"], r["TotalSGPRs"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"]))
    assert r["VGPRs"] + r["AGPRs"] <= 64, r
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
