"""The cases of tests/contigs_repeat_cases.py on the MI355X: contigs spelled by k_contigs_rle and k_contigs_repeat (csrc/walk.cpp) against
the oracle's and against the dense path of the same build, byte for byte.  tests/test_hostsim_contigs_repeat.py runs the same graphs on
the host simulation and checks there, through the simulation's hook, that they hold the descriptors each case is about.
Run with `pytest -m gpu`."""
import pytest

import corticall_amd as ca
from tests import contigs_repeat_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    l = ca.default_lib()
    assert l.device_count() >= 1, "needs an MI355X"
    return l


def test_batch_without_repeat(orc, lib, tmp_path):
    rc.case_no_repeat(orc, lib, tmp_path)


def test_every_walk_ends_in_a_repeat(orc, lib, tmp_path):
    rc.case_every_walk_repeats(orc, lib, tmp_path)


def test_short_period_and_every_len(orc, lib, tmp_path):
    rc.case_short_period_and_len(orc, lib, tmp_path)


def test_repeat_after_long_flank(orc, lib, tmp_path):
    rc.case_repeat_after_long_flank(orc, lib, tmp_path)


def test_run_lengths(orc, lib, tmp_path):
    rc.case_run_lengths(orc, lib, tmp_path)
