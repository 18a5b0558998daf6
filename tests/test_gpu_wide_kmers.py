"""Wide k-mers (W = 3 and 4 words, k 65..128) and sorts past one record per chunk owner through the HIP library on an MI355X:
the W = 4 instances are the default arm of every kernel's W switch, and only the device build shows what the gfx950 compiler makes
of them.  The same cases, over the same lists of tests/parity_cases.py, run through the host simulation in
tests/test_hostsim_wide_kmers.py.  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import parity_cases as pc
from tests import unitig_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("k,ncol", pc.WIDE_FIND)
def test_random_find(orc, lib, tmp_path, k, ncol): pc.case_random_find(orc, lib, tmp_path, k, ncol)


@pytest.mark.parametrize("k", pc.WIDE_ALL_BITS)
def test_all_bits_kmers(orc, lib, tmp_path, k): pc.case_all_bits_kmers(orc, lib, tmp_path, k)


@pytest.mark.parametrize("k,seed,links", pc.WIDE_WALKS)
def test_random_walks(orc, lib, tmp_path, k, seed, links): pc.case_random_walks(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed,links", pc.WIDE_DFS_RULES)
def test_dfs_rules(orc, lib, tmp_path, k, seed, links): pc.case_dfs_rules(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed", pc.WIDE_RUN_STEPS)
def test_run_steps(orc, lib, tmp_path, k, seed): pc.case_run_steps(orc, lib, tmp_path, seed, k=k)


@pytest.mark.parametrize("k,seed", pc.WIDE_RUN_STEPS)
def test_dfs_run_steps(orc, lib, tmp_path, k, seed): pc.case_dfs_run_steps(orc, lib, tmp_path, seed, k=k)


@pytest.mark.parametrize("k,seed,links", pc.WIDE_GRAPH_TOOLS)
def test_partition(orc, lib, tmp_path, k, seed, links): pc.case_partition(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed,links", pc.WIDE_GRAPH_TOOLS)
def test_findtips(orc, lib, tmp_path, k, seed, links): pc.case_findtips(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed,links", pc.WIDE_GRAPH_TOOLS)
def test_facade(orc, lib, tmp_path, k, seed, links): pc.case_facade(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed,ncol,kind", pc.WIDE_UNITIGS)
def test_unitigs(orc, lib, tmp_path, k, seed, ncol, kind): uc.case_random(orc, lib, tmp_path, k, seed, ncol, kind)


@pytest.mark.parametrize("k", pc.WIDE_LINK_FORMATS)
def test_link_formats(orc, lib, tmp_path, k): pc.case_link_formats(orc, lib, tmp_path, k)


@pytest.mark.parametrize("k,n_bp,ncol", pc.SORT_LARGE_CASES)
def test_sort_large(orc, lib, tmp_path, k, n_bp, ncol): pc.case_sort_large(orc, lib, tmp_path, k, n_bp, ncol)


def test_join_large(orc, lib, tmp_path): pc.case_join_large(orc, lib, tmp_path)


@pytest.mark.parametrize("block,k,seed,links", pc.WALK_BLOCKS)
def test_walk_blocks(orc, lib, tmp_path, monkeypatch, block, k, seed, links):
    """the walk kernel in workgroups of 16 and 32 lanes (LDBG_WALK_BLOCK is read on every run)"""
    monkeypatch.setenv("LDBG_WALK_BLOCK", str(block))
    pc.case_random_walks(orc, lib, tmp_path, k, seed, links)
