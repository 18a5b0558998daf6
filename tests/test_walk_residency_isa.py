"""CPU-side check of what the host asks the runtime about (rt.h: blocks_per_cu): the resident walk and dfs kernels as they compile for
gfx950 fit a compute unit EIGHT times — two wavefronts per SIMD.  Read from the code object's metadata: the LDS of a workgroup
(LDBG_LS_FAST x lanes x 24 B, strand.h) must fit eight times into the CU's 160 KB, and k_walk<W, BS, false> must need at most 256 VGPRs
and no private segment.  k_dfs<W, false> is checked for LDS only: some of its instantiations need more than 256 VGPRs today and run one
wavefront per SIMD (the host takes that from the runtime, dfs.cpp); their counts are printed with a failure.  Needs hipcc (cross-compiles,
no GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corticall_amd", "csrc")
CU_LDS = 160 * 1024           # bytes of LDS per compute unit of an MI355X (gfx950)
WALK = re.compile(r"^_ZN4ldbg6k_walkILi(\d)ELi(\d+)ELb0EEEvNS_8WalkArgsE$")
DFS = re.compile(r"^_ZN4ldbg5k_dfsILi(\d)ELb0EEEvNS_7DfsArgsE$")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _kernels(text):
    """name -> {lds, vgpr, priv} of every kernel in the assembly's amdhsa.kernels metadata"""
    out = {}
    meta = text[text.index("amdhsa.kernels:"):]
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1))
        out[name.group(1)] = {"lds": field("group_segment_fixed_size"), "vgpr": field("vgpr_count"), "priv": field("private_segment_fixed_size")}
    return out


@pytest.fixture(scope="module")
def resident(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("residency_isa")
    # the flags of the product build (csrc/Makefile: HIPFLAGS), device code only, as assembly; both sources at once
    procs = [(src, subprocess.Popen([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                                     "--offload-device-only", "-S", os.path.join(CSRC, src + ".cpp"), "-o", str(d / (src + ".s"))], cwd=CSRC,
                                    stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)) for src in ("walk", "dfs")]
    walk, dfs = {}, {}
    for src, p in procs:
        assert p.wait() == 0, src
        for name, r in _kernels(open(str(d / (src + ".s"))).read()).items():
            if WALK.match(name):
                walk[tuple(int(x) for x in WALK.match(name).groups())] = r
            elif DFS.match(name):
                dfs[int(DFS.match(name).group(1))] = r
    return walk, dfs


def test_every_resident_instantiation_is_there(resident):
    walk, dfs = resident
    assert set(walk) == {(w, bs) for w in (1, 2, 3, 4) for bs in (16, 32, 64)}, sorted(walk)
    assert set(dfs) == {1, 2, 3, 4}, sorted(dfs)


def test_eight_walk_workgroups_fit_a_cu(resident):
    walk, _ = resident
    for key, r in sorted(walk.items()):
        assert 8 * r["lds"] <= CU_LDS, ("k_walk<%d, %d, false>" % key, r)
        assert r["vgpr"] <= 256, ("k_walk<%d, %d, false>" % key, r)
        assert r["priv"] == 0, ("k_walk<%d, %d, false>" % key, r)


def test_eight_dfs_workgroups_fit_a_cu_by_lds(resident):
    _, dfs = resident
    regs = {"k_dfs<%d, false>" % w: (r["vgpr"], r["priv"]) for w, r in sorted(dfs.items())}
    for w, r in sorted(dfs.items()):
        assert 8 * r["lds"] <= CU_LDS, ("k_dfs<%d, false>" % w, r, "(VGPRs, private segment) of all of them: %s" % regs)
