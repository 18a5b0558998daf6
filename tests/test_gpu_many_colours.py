"""Graphs of 4 to 32 colours through the HIP library on an MI355X: colours beyond the packed word of colours 0..3 (csrc/engine.h: the
`more` loop of node_fill_bytes), rows that are never the packed layout (row_is_packed: the unpacked loads of node_from_entry), colour
masks up to their top bit, records of up to 8 W + 160 bytes through upload, sort and join.  The same cases, over the same lists of
tests/parity_cases.py, run through the host simulation in tests/test_hostsim_many_colours.py.  Run with `pytest -m gpu`."""
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


@pytest.mark.parametrize("k,ncol", pc.MANY_FIND)
def test_random_find(orc, lib, tmp_path, k, ncol): pc.case_random_find(orc, lib, tmp_path, k, ncol)


@pytest.mark.parametrize("ncol,k", pc.MANY_COLOURS + [(32, 64)])
def test_records(orc, lib, tmp_path, ncol, k): pc.case_many_records(orc, lib, tmp_path, ncol, k)


@pytest.mark.parametrize("ncol,k,links", pc.MANY_WALKS)
def test_walks(orc, lib, tmp_path, ncol, k, links): pc.case_many_walks(orc, lib, tmp_path, ncol, k, links)


@pytest.mark.parametrize("ncol,k,seed", pc.MANY_RUN_STEPS)
def test_run_steps(orc, lib, tmp_path, ncol, k, seed): pc.case_run_steps(orc, lib, tmp_path, seed, k=k, ncol=ncol)


@pytest.mark.parametrize("ncol,k,links", pc.MANY_DFS)
def test_dfs_rules(orc, lib, tmp_path, ncol, k, links): pc.case_many_dfs(orc, lib, tmp_path, ncol, k, links)


@pytest.mark.parametrize("ncol,k,seed,links", pc.MANY_FACADE)
def test_facade(orc, lib, tmp_path, ncol, k, seed, links): pc.case_facade(orc, lib, tmp_path, k, seed, links, ncol=ncol)


@pytest.mark.parametrize("k,seed,ncol,kind", pc.MANY_UNITIGS)
def test_unitigs(orc, lib, tmp_path, k, seed, ncol, kind):
    uc.case_random(orc, lib, tmp_path, k, seed, ncol, kind, sets=uc.many_color_sets(ncol), gfa_colors=[ncol - 1])


def test_sort(orc, lib, tmp_path): pc.case_sort(orc, lib, tmp_path, cases=pc.MANY_SORT)


@pytest.mark.parametrize("k,n_bp,ncol", pc.MANY_SORT_LARGE)
def test_sort_large(orc, lib, tmp_path, k, n_bp, ncol): pc.case_sort_large(orc, lib, tmp_path, k, n_bp, ncol)


def test_join_32_colours(orc, lib, tmp_path): pc.case_many_join(orc, lib, tmp_path)


def test_beyond_32_colours(orc, lib, tmp_path):
    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    pc.case_beyond_32_colours(orc, lib, tmp_path, free_bytes=free_bytes)


def test_collection_engine(orc, lib, tmp_path): pc.case_collection_engine_many(orc, lib, tmp_path)
def test_factory_validation(orc, lib, tmp_path): pc.case_factory_validation_many(orc, lib, tmp_path)
