"""The fixed-layout walk kernels on the CPU: the cases of tests/walk_rows_cases.py through the TEST-ONLY host simulation (tests/hostsim),
which builds and runs the same dispatch as the device (walk.cpp: walk_rows_fit, launch_k_walk).  Every case in the one-lane simulation;
the shape of the reference pipeline (k = 47, three colours), a one-colour graph and the run steps also with 16 and 64 lanes in LOCK STEP.
The same cases run on the device in tests/test_gpu_walk_rows.py."""
import pytest

from tests import parity_cases as pc
from tests import refill_cases as rc
from tests import walk_rows_cases as wr


@pytest.fixture(scope="module")
def lib():
    from tests import hostsim
    return hostsim.load()


@pytest.fixture(scope="module", params=[16, 64])
def lib_lanes(request):
    from tests import hostsim
    return hostsim.load_wavefront(request.param)


@pytest.mark.parametrize("case", wr.FIXED, ids=wr.case_id)
def test_fixed_kernel_equals_generic(orc, lib, tmp_path, monkeypatch, case):
    wr.both_kernels(monkeypatch, lib, True, case[0], orc, lib, tmp_path, *case[1])


@pytest.mark.parametrize("case", wr.GENERIC, ids=wr.case_id)
def test_generic_kernel_keeps_what_is_not_built(orc, lib, tmp_path, monkeypatch, case):
    wr.both_kernels(monkeypatch, lib, False, case[0], orc, lib, tmp_path, *case[1])


def test_lanes_refill(orc, lib, tmp_path, monkeypatch):
    """64 lanes for every launch: each lane of the fixed kernel goes back to the queue"""
    rc.few_slots(monkeypatch, 64)
    wr.both_kernels(monkeypatch, lib, True, pc.case_random_walks, orc, lib, tmp_path, 47, 5, True)
    assert rc.refills(lib, "walk_refills") > 0


def test_second_launch_takes_the_fixed_kernel(orc, lib, tmp_path, monkeypatch):
    wr.second_launch(monkeypatch, lib, pc.case_random_walks, orc, lib, tmp_path, 47, 5, True)


def test_second_launch_takes_the_fixed_kernel_run_steps(orc, lib, tmp_path, monkeypatch):
    """(run steps and REPEAT descriptors in the first launch, none in the second)"""
    wr.second_launch(monkeypatch, lib, pc.case_run_steps, orc, lib, tmp_path, 0)


# ---- lock step, 16 and 64 lanes
def test_lockstep_run_steps(orc, lib_lanes, tmp_path, monkeypatch):
    wr.both_kernels(monkeypatch, lib_lanes, True, pc.case_run_steps, orc, lib_lanes, tmp_path, 0)


def test_lockstep_second_launch(orc, lib_lanes, tmp_path, monkeypatch):
    wr.second_launch(monkeypatch, lib_lanes, pc.case_random_walks, orc, lib_lanes, tmp_path, 47, 5, True)


def test_lockstep_reference_shape(orc, lib_lanes, tmp_path, monkeypatch):
    wr.both_kernels(monkeypatch, lib_lanes, True, pc.case_random_walks, orc, lib_lanes, tmp_path, 47, 5, True)


def test_lockstep_one_colour(orc, lib_lanes, tmp_path, monkeypatch):
    wr.both_kernels(monkeypatch, lib_lanes, True, wr.case_one_colour, orc, lib_lanes, tmp_path, 31, 0)


def test_lockstep_generic_even_k(orc, lib_lanes, tmp_path, monkeypatch):
    wr.both_kernels(monkeypatch, lib_lanes, False, pc.case_random_walks, orc, lib_lanes, tmp_path, 46, 8, True)
