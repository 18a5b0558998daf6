"""Link stores on either side of the LDS / HBM split (csrc/strand.h: LDBG_LS_FAST = 12 elements per lane in LDS, the rest in the lane's HBM
tail).  The graph of parity_cases.case_big_link_stores (k = 5, a 9-base unit repeated, 241 bp, the first 40 k-mers as seeds) with the reads
taken from every `stride`-th position: the fewer reads, the fewer live links a walk carries.  Over the strides below the walk of seed
number PROBE peaks at 9, 11, 12, 13, 14, 16 and 18 elements (PEAKS; measured with the host simulation built at the header's own split,
tests/test_ls_boundary.py::test_probe_walk_peaks_on_either_side_of_the_split), so its store ends exactly at the split, one element
beyond it, inside a 16-lane group that reaches across it, and beyond the groups; the other walks of the batch carry from a handful to
several hundred elements.  Shared by the host simulation (tests/test_ls_boundary.py) and the device (tests/test_gpu_ls_boundary.py)."""
import random

from tests import parity_cases as pc

PROBE = 14                      # index of the probe walk's seed among the case's seeds
PEAKS = {27: 9, 23: 11, 21: 12, 19: 13, 17: 14, 15: 16, 11: 18}       # read stride -> peak number of elements in the probe walk's link store
STRIDES = tuple(PEAKS)


def boundary_case(orc, lib, tmp, stride):
    """-> (case, its 40 seeds)"""
    rng = random.Random(50)
    unit = pc.rand_seq(rng, 9)
    g1 = pc.rand_seq(rng, 60) + unit * 6 + pc.rand_seq(rng, 60) + unit * 3 + pc.rand_seq(rng, 40)
    reads = {"a": [g1[i:] for i in range(0, len(g1) - 30, stride)]}
    cs = pc.Case(orc, tmp, lib, [("a", [g1])], 5, link_samples=["a"], reads=reads, name="split%d" % stride)
    return cs, cs.all_kmers()[:40]


# The lock-step simulation costs a fibre switch per lane and primitive, and a walk that circles the tandem repeat carries hundreds of links:
# the whole batch takes it 1.5 to 3.5 minutes per stride at 64 lanes.  There the case runs the 24 walks whose store stays below 100
# elements at maxLength 40 (the probe among them, with the same peaks: PEAKS does not depend on maxLength from 40 on) and four searches
# around the probe: a few seconds.
LOCKSTEP_SEEDS = (1, 4, 6, 7, 8, 10, 12, 14, 15, 19, 21, 23, 24, 25, 26, 27, 28, 30, 32, 33, 34, 35, 36, 39)


def case_across_the_split(orc, lib, tmp, stride, lockstep=False):
    """walks (ContigStopper, BOTH) of the 40 seeds and ExplorationStopper searches from ten of them, the probe among them, bit for bit
    against the oracle; lockstep: the smaller form for the host simulation with more than one lane per wavefront"""
    cs, seeds = boundary_case(orc, lib, tmp, stride)
    if lockstep:
        pc.compare_walks(cs, [seeds[i] for i in LOCKSTEP_SEEDS], trav=[0], links=["a"], max_len=40)
        pc.compare_dfs(cs, seeds[PROBE - 2:PROBE + 2], trav=[0], stopper="ExplorationStopper", links=["a"], max_len=20)
        return
    pc.compare_walks(cs, seeds, trav=[0], links=["a"], max_len=400)
    pc.compare_dfs(cs, seeds[PROBE - 5:PROBE + 5], trav=[0], stopper="ExplorationStopper", links=["a"], max_len=200)
