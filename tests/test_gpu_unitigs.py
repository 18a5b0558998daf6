"""Unitigs (ldbg_graph_unitigs) through the HIP library on an MI355X: the cases of tests/unitig_cases.py (also run
through the host simulation by tests/test_unitigs_hostsim.py) and a synthetic graph.  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import unitig_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


def test_fixture_known_answer(orc, lib, tmp_path): uc.case_fixture(orc, lib, tmp_path)


@pytest.mark.parametrize("k,seed,ncol,kind", uc.RANDOM_CASES)
def test_random_graphs(orc, lib, tmp_path, k, seed, ncol, kind): uc.case_random(orc, lib, tmp_path, k, seed, ncol, kind)


def test_hash_collisions(orc, lib, tmp_path): uc.case_hash_collisions(orc, lib, tmp_path)
def test_tiny_table(orc, lib, tmp_path): uc.case_tiny(orc, lib, tmp_path)
def test_collection_and_shard(orc, lib, tmp_path): uc.case_collection_and_shard(orc, lib, tmp_path)
def test_bad_arguments(orc, lib, tmp_path): uc.case_bad_arguments(orc, lib, tmp_path)
def test_synthetic_graph(orc, lib, tmp_path): uc.case_synth(orc, lib, tmp_path)
