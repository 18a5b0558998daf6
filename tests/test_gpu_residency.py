"""The resident grid of k_walk on a real MI355X: with 12 link-store elements per lane in LDS (18 KB per workgroup) and at most 256 VGPRs
the runtime grants eight wavefronts per CU, and the host sizes the launch by that answer (rt.h: blocks_per_cu).  One batch of
refill_cases.BEYOND_N seeds — more strands than 8 x 256 x 64 lanes — takes every slot; the same batch under LDBG_WG_PER_CU=6 (the
residency this kernel had with 16 elements in LDS), in a fresh process, gives the same contigs.  Run with `pytest -m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run_batch(ctx, ctp, seeds):
    """-> (arena, offsets, walk lengths, walk_wavefronts, walk_refills, CUs of the device)"""
    import torch
    import corticall_amd as ca
    from corticall_amd import ContigStopper, CortexGraph, CortexLinks, TraversalEngineFactory
    lib = ca.default_lib()
    assert lib.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    g = CortexGraph(ctx, lib=lib)
    e = TraversalEngineFactory(lib=lib).traversalColors(0).graph(g).maxBranchLength(100).stoppingRule(ContigStopper).links(CortexLinks(ctp, g)).make()
    ca.profile_reset(lib=lib)
    arena, offs, wl = e.walk_batch_arrays(seeds)
    return (np.array(arena), np.array(offs), np.array(wl), int(ca.profile_get("walk_wavefronts", lib=lib)[0]), int(ca.profile_get("walk_refills", lib=lib)[0]),
            int(torch.cuda.get_device_properties(0).multi_processor_count))


def test_eight_wavefronts_per_cu_and_the_same_contigs_as_six(orc, tmp_path):
    import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)
    import corticall_amd as ca
    from tests import refill_cases as rc
    cs, distinct, which = rc._beyond_cap_graph(orc, ca.default_lib(), tmp_path, "res")
    ctp = str(tmp_path / "res.kid.ctp.gz")
    seeds = np.ascontiguousarray(np.frombuffer("".join(distinct).encode(), dtype=np.uint8).reshape(len(distinct), cs.k)[which])
    assert len(seeds) == rc.BEYOND_N
    arena, offs, wl, waves, refills, cus = _run_batch(cs.path, ctp, seeds)
    print("walk_wavefronts %d = %.2f x %d CUs, walk_refills %d" % (waves, waves / cus, cus, refills))
    assert 2 * rc.BEYOND_N > 8 * cus * 64
    assert waves == 8 * cus, (waves, cus)
    assert refills > 0
    # the same batch at six wavefronts per CU, in a process of its own (the knob is read per batch, the process keeps nothing of this one)
    np.save(str(tmp_path / "seeds.npy"), seeds)
    env = dict(os.environ, LDBG_WG_PER_CU="6")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), cs.path, ctp, str(tmp_path / "seeds.npy"), str(tmp_path / "six.npz")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    six = np.load(str(tmp_path / "six.npz"))
    assert int(six["waves"]) == 6 * cus and int(six["refills"]) > refills
    assert (six["offs"] == offs).all() and (six["wl"] == wl).all() and six["arena"].tobytes() == arena.tobytes()
    assert len(set(np.diff(offs).tolist())) > 5         # contigs of many lengths


if __name__ == "__main__":      # the child: the batch as the environment says, results to an .npz
    sys.path.insert(0, ROOT)
    a, o, w, nw, nr, _ = _run_batch(sys.argv[1], sys.argv[2], np.load(sys.argv[3]))
    np.savez(sys.argv[4], arena=a, offs=o, wl=w, waves=nw, refills=nr)
