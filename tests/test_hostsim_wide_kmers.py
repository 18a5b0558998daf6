"""Wide k-mers (W = 3 and 4 words, k 65..128) and sorts past one record per chunk owner through the TEST-ONLY host simulation of
the kernels (tests/hostsim).  The same cases, over the same lists of tests/parity_cases.py, run on the device in
tests/test_gpu_wide_kmers.py: the host build cannot see what the gfx950 compiler makes of the W = 4 instances."""
import pytest

from tests import parity_cases as pc
from tests import unitig_cases as uc


@pytest.fixture(scope="module")
def lib():
    from tests import hostsim
    return hostsim.load()


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
