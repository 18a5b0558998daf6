"""Walks and searches whose link stores end on either side of the LDS / HBM split, on the CPU: the host simulation built with the header's
own LDBG_LS_FAST (make hostsimdev), at 1, 16 and 64 lanes per wavefront — at 64 lanes the 8- and 16-lane group operations of lscoop.h
run with a store that reaches from the simulated LDS into the HBM tail, as they do on the device; the test asks the simulation's count of
such accesses (ldbg_hostsim_group_tail) that they did.  At 16 and 64 lanes the batch is the reduced one of ls_boundary_cases.LOCKSTEP_SEEDS.

Which inputs sit at the split (tests/ls_boundary_cases.py): the walk of seed number 14 (PROBE) of the 241 bp graph.  With reads from every
21st position its link store peaks at exactly 12 elements (the last one that is in LDS), from every 19th position at 13 (one element in
the tail); strides 27 / 23 / 17 / 15 / 11 give 9 / 11 / 14 / 16 / 18.  Checked by test_probe_walk_peaks_on_either_side_of_the_split: the
simulation records the highest element index any link store has written (engine.h: LDBG_LS_PEAK, read through ldbg_hostsim_ls_peak), and
the probe seed is walked in a batch of its own."""
import ctypes as C
import os

import pytest

from tests import ls_boundary_cases as bc


def _load(lanes):
    from corticall_amd import NativeLib
    from tests import hostsim
    hostsim.build("hostsimdev")
    lib = NativeLib(os.path.join(hostsim.ROOT, "tests", "hostsim", "_builddev", "libldbg_hostsim.so"))
    lib.dll.ldbg_hostsim_set_lanes(int(lanes))
    return lib


@pytest.fixture(scope="module", params=[1, 16, 64])
def lanes_lib(request):
    return request.param, _load(request.param)


@pytest.mark.parametrize("stride", bc.STRIDES)
def test_walks_and_searches_across_the_split(orc, lanes_lib, tmp_path, stride):
    lanes, lib = lanes_lib
    lib.dll.ldbg_hostsim_group_tail.restype = C.c_ulonglong
    lib.dll.ldbg_hostsim_group_tail()                  # (reading the hook resets it)
    bc.case_across_the_split(orc, lib, tmp_path, stride, lockstep=lanes > 1)
    # the 8- and 16-lane group forms exist at 64 lanes only; there, at every stride, some store of 13..16 elements must have been worked on
    # by a group whose last lanes read or wrote the HBM tail (lscoop.h: LDBG_GROUP_TAIL counts those accesses)
    n = lib.dll.ldbg_hostsim_group_tail()
    assert (n > 0) == (lanes == 64), (lanes, stride, n)


def test_probe_walk_peaks_on_either_side_of_the_split(orc, tmp_path):
    lib = _load(1)
    fast = lib.dll.ldbg_hostsim_ls_fast()
    peaks = {}
    for stride in bc.STRIDES:
        cs, seeds = bc.boundary_case(orc, lib, tmp_path, stride)
        at = []
        for max_len in (400, 40):                      # (the two lengths case_across_the_split walks at)
            e = cs.engines(trav=[0], links=["a"], max_len=max_len)[1]
            lib.dll.ldbg_hostsim_ls_peak()             # (reading the hook resets it)
            e.walk_batch([seeds[bc.PROBE]])
            at.append(lib.dll.ldbg_hostsim_ls_peak())
        assert at[0] == at[1] == bc.PEAKS[stride], (stride, at)
        peaks[stride] = at[0]
    assert peaks[21] == 12 and peaks[19] == 13
    assert min(peaks.values()) < 12 and max(peaks.values()) > 16
    assert min(peaks.values()) < fast < max(peaks.values()), "the sweep does not cross this build's split (LDBG_LS_FAST = %d)" % fast
