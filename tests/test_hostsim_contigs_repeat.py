"""k_contigs_rle files a strand's REPEAT descriptor in a per-batch list and k_contigs_repeat, behind it on the stream, copies its bases
(csrc/walk.cpp).  The cases of tests/contigs_repeat_cases.py on the host simulation: one lane, and 64 and 16 lanes in lock step.  Every
contig is compared with the oracle's and with the dense path of the same build; the simulation's hook (ldbg_hostsim_contig_seen) says
whether the descriptors a case is about were met."""
import ctypes as C
import os

import pytest

from tests import contigs_repeat_cases as rc

SEEN = ("repeats repeats_rev repeats_fwd both_strands next_group past_block short_period len_below_8 len_off_8 min_period "
        "runs runs_asc runs_desc runs_mirrored run_lens_1_to_8 runs_512 runs_513").split()


@pytest.fixture(scope="module", params=[1, 64, 16])
def sim(request):
    from tests import hostsim
    lanes = request.param
    os.environ.pop("LDBG_EAGER_PATHS", None)
    lib = hostsim.load() if lanes == 1 else hostsim.load_wavefront(lanes)
    yield lib, lanes
    lib.dll.ldbg_hostsim_set_lanes(1)


def seen(lib):
    """what k_contigs_rle has met since the last call"""
    out = (C.c_ulonglong * len(SEEN))()
    lib.dll.ldbg_hostsim_contig_seen(out)
    return dict(zip(SEEN, list(out)))


def test_batch_without_repeat(orc, sim, tmp_path):
    lib, _ = sim
    seen(lib)
    rc.case_no_repeat(orc, lib, tmp_path)
    s = seen(lib)
    assert s["repeats"] == 0 and s["runs"] > 0, s


def test_every_walk_ends_in_a_repeat(orc, sim, tmp_path):
    lib, lanes = sim
    seen(lib)
    n = rc.case_every_walk_repeats(orc, lib, tmp_path, n=7 if lanes == 1 else 4)
    s = seen(lib)
    # the first batch, walked with host and with device seeds (parity_cases.compare_walks): both strands of every seed, every time;
    # the second (ten seeds): some of them
    assert s["repeats_rev"] == s["repeats_fwd"] == s["both_strands"], s
    assert 2 * n < s["both_strands"] < 2 * n + 2 * 10 and s["min_period"] == 12 and s["runs"] > 0, s


def test_short_period_and_every_len(orc, sim, tmp_path):
    lib, lanes = sim
    seen(lib)
    rc.case_short_period_and_len(orc, lib, tmp_path, n=6 if lanes == 1 else 2)
    s = seen(lib)
    assert s["min_period"] == 5 and s["short_period"] == s["repeats"] > 0, s
    assert s["len_below_8"] > 0 and s["len_off_8"] > 0 and s["len_off_8"] < s["repeats"], s


def test_repeat_after_long_flank(orc, sim, tmp_path):
    lib, lanes = sim
    seen(lib)
    rc.case_repeat_after_long_flank(orc, lib, tmp_path, n=66 if lanes != 16 else 20)
    s = seen(lib)
    assert s["past_block"] > 0, s                     # the strand's stored entries cross a path block before its REPEAT
    if lanes == 64:
        assert 0 < s["next_group"] < s["repeats"], s  # a head in the last lane of its group of 64: the payload is read from the next group


def test_run_lengths(orc, sim, tmp_path):
    lib, lanes = sim
    seen(lib)
    rc.case_run_lengths(orc, lib, tmp_path)
    s = seen(lib)
    assert s["run_lens_1_to_8"] == 0x1FE and s["runs_512"] > 0 and s["runs_513"] > 0, s
    assert s["runs_asc"] > 0 and s["runs_desc"] > 0 and 0 < s["runs_mirrored"] < s["runs"], s
