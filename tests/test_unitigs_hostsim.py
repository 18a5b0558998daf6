"""Unitigs (ldbg_graph_unitigs) through the TEST-ONLY host simulation of the kernels, against the yardstick of
tests/unitig_cases.py.  The same cases run on the device in tests/test_gpu_unitigs.py."""
import pytest

from tests import unitig_cases as uc


@pytest.fixture(scope="module")
def lib():
    from tests import hostsim
    return hostsim.load()


def test_fixture_known_answer(orc, lib, tmp_path): uc.case_fixture(orc, lib, tmp_path)


@pytest.mark.parametrize("k,seed,ncol,kind", uc.RANDOM_CASES)
def test_random_graphs(orc, lib, tmp_path, k, seed, ncol, kind): uc.case_random(orc, lib, tmp_path, k, seed, ncol, kind)


def test_hash_collisions(orc, lib, tmp_path): uc.case_hash_collisions(orc, lib, tmp_path)
def test_tiny_table(orc, lib, tmp_path): uc.case_tiny(orc, lib, tmp_path)
def test_collection_and_shard(orc, lib, tmp_path): uc.case_collection_and_shard(orc, lib, tmp_path)
def test_bad_arguments(orc, lib, tmp_path): uc.case_bad_arguments(orc, lib, tmp_path)
