"""Lanes that take a second strand or search, on the CPU: the cases of tests/refill_cases.py with 64 lanes for every launch, through the
TEST-ONLY host simulation (tests/hostsim).  The same cases run on the device in tests/test_gpu_refill.py.

Every case runs in the one-lane simulation, where the wavefronts of a launch run one after the other: the first lane takes the whole
queue, strand after strand, so each strand but the first begins in registers, a link store (simulated LDS and HBM tail), snapshots, a
frame stack and a visited table that another strand has just used.  The dense cases run in LOCK STEP as well (load_wavefront: 64 fibres,
the device's 16 link-store elements per lane in LDS, and the detector for lanes that reach different primitives), and so does
case_run_steps(0): there the 64 lanes of one wavefront refill at different iterations, beside lanes that regrow tables or take
cooperative link-store steps.  (The lock-step
simulation costs a fibre switch per lane and primitive: the whole list would take more than an hour in it.)"""
import pytest

from tests import parity_cases as pc
from tests import refill_cases as rc


@pytest.fixture(scope="module")
def lib():
    from tests import hostsim
    return hostsim.load()


@pytest.fixture(scope="module")
def lib64():
    from tests import hostsim
    return hostsim.load_wavefront(64)


@pytest.mark.parametrize("case", rc.WALK_CASES, ids=rc.case_id)
def test_walks_refill(orc, lib, tmp_path, monkeypatch, case):
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib, "walk_refills", case[0], orc, lib, tmp_path, *case[1])


@pytest.mark.parametrize("knob,value", rc.WALK_KNOBS)
def test_walks_refill_with_knobs(orc, lib, tmp_path, monkeypatch, knob, value): rc.case_walk_knobs(orc, lib, tmp_path, monkeypatch, knob, value)


@pytest.mark.parametrize("case", rc.DFS_CASES, ids=rc.case_id)
def test_dfs_refill(orc, lib, tmp_path, monkeypatch, case):
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib, "dfs_refills", case[0], orc, lib, tmp_path, *case[1])


def test_dfs_second_launch_refills(orc, lib, tmp_path, monkeypatch): rc.case_dfs_second_launch(orc, lib, tmp_path, monkeypatch)


def test_step_counts_unchanged(orc, lib, tmp_path, monkeypatch):
    rc.case_step_counts_unchanged(orc, lib, tmp_path, monkeypatch, pc.case_run_steps, 0)


@pytest.mark.parametrize("seed,env", rc.STEPS_ALONE, ids=lambda x: str(x) if isinstance(x, int) else "-".join("%s=%s" % kv for kv in x.items()) or "plain")
def test_steps_alone_and_in_a_batch(orc, lib, tmp_path, monkeypatch, seed, env):
    """(seeds 1 and 3 fail when the refill branch of k_walk leaves `anchor_at` / `period` as the previous strand had them)"""
    rc.case_steps_alone_and_in_a_batch(orc, lib, tmp_path, monkeypatch, seed, **env)


# ---- lock step, 64 lanes
@pytest.mark.parametrize("seed", [0, 2])
def test_lockstep_dense_cycles_refill(orc, lib64, tmp_path, monkeypatch, seed):
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib64, "walk_refills", pc.case_dense_cycles, orc, lib64, tmp_path, seed)


@pytest.mark.parametrize("knob,value", rc.WALK_KNOBS)
def test_lockstep_dense_cycles_refill_with_knobs(orc, lib64, tmp_path, monkeypatch, knob, value):
    rc.case_walk_knobs(orc, lib64, tmp_path, monkeypatch, knob, value, random_walks=False)


def test_lockstep_run_steps_refill(orc, lib64, tmp_path, monkeypatch):
    """run steps and REPEAT descriptors in lanes that refill beside lanes in cooperative steps.  (The k_dfs counterpart,
    case_dfs_run_steps(0), takes 3.5 minutes in lock step, as much as the rest of this module: it runs in the one-lane simulation above
    and on the device.)"""
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib64, "walk_refills", pc.case_run_steps, orc, lib64, tmp_path, 0)


def test_lockstep_dfs_dense_refill(orc, lib64, tmp_path, monkeypatch):
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib64, "dfs_refills", pc.case_dfs_dense, orc, lib64, tmp_path, 0)
