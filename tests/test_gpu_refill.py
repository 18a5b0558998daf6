"""Lanes that take a second strand or search, on a real MI355X: the cases of tests/refill_cases.py through the HIP library with 64 lanes
for every launch of k_walk and k_dfs (resident table and image kernels), and two batches beyond the residency cap with no knob set.
Run with `pytest -m gpu`; the host simulation runs the same cases in tests/test_hostsim_refill.py."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import parity_cases as pc
from tests import refill_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


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


@pytest.mark.parametrize("seed,env", rc.STEPS_ALONE, ids=lambda x: str(x) if isinstance(x, int) else "-".join("%s=%s" % kv for kv in x.items()) or "plain")
def test_steps_alone_and_in_a_batch(orc, lib, tmp_path, monkeypatch, seed, env):
    """(in the one-lane host simulation seeds 1 and 3 fail when the refill branch of k_walk leaves `anchor_at` / `period` as the previous strand had them)"""
    rc.case_steps_alone_and_in_a_batch(orc, lib, tmp_path, monkeypatch, seed, **env)


@pytest.mark.parametrize("k,with_links,ncol", rc.SHARDED_WALKS)
def test_sharded_walks_refill_one_rank_rccl(orc, lib, tmp_path, monkeypatch, k, with_links, ncol):
    """k_walk<W, 64, true>: a lane saved at the end of a round, restored, finishes and begins another strand"""
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib, "walk_refills", pc.case_sharded_walks_one_rank_rccl, orc, lib, tmp_path, k, with_links, ncol)


@pytest.mark.parametrize("k,ncol", rc.SHARDED_DFS)
def test_sharded_dfs_refill_one_rank_rccl(orc, lib, tmp_path, monkeypatch, k, ncol):
    """k_dfs<W, true>, both directions"""
    rc.few_slots(monkeypatch, 64)
    rc.refilled(lib, "dfs_refills", pc.case_sharded_dfs_one_rank_rccl, orc, lib, tmp_path, k, ncol)


def test_walks_beyond_the_residency_cap(orc, lib, tmp_path): rc.case_beyond_cap_walks(orc, lib, tmp_path)
def test_dfs_beyond_the_residency_cap(orc, lib, tmp_path): rc.case_beyond_cap_dfs(orc, lib, tmp_path)
