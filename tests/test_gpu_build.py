"""Graph construction (ldbg_graph_build) through the HIP library on an MI355X: the cases of tests/build_cases.py (also
run through the host simulation by tests/test_build_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import build_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("M", bc.SHAPE_WINDOWS)
def test_shapes(orc, lib, tmp_path, M): bc.case_shapes(orc, lib, tmp_path, M)


@pytest.mark.parametrize("k", bc.KMER_SIZES)
def test_kmer_sizes(orc, lib, tmp_path, k): bc.case_kmer_sizes(orc, lib, tmp_path, k)


@pytest.mark.parametrize("variant", bc.EDGE_VARIANTS)
def test_sequence_edges(orc, lib, tmp_path, variant): bc.case_sequence_edges(orc, lib, tmp_path, variant)


@pytest.mark.parametrize("C", bc.COLOURS)
def test_colours(orc, lib, tmp_path, C): bc.case_colours(orc, lib, tmp_path, C)


@pytest.mark.parametrize("variant", bc.HEAVY)
def test_heavy_kmers(orc, lib, tmp_path, variant): bc.case_heavy_kmers(orc, lib, tmp_path, variant)


@pytest.mark.parametrize("bad", bc.NON_ACGT_BYTES, ids=["N", "dot", "newline", "high"])
def test_non_acgt(orc, lib, tmp_path, bad): bc.case_non_acgt(orc, lib, tmp_path, bad)


def test_reference_shapes(orc, lib, tmp_path): bc.case_reference_shapes(orc, lib, tmp_path)
def test_resident(orc, lib, tmp_path): bc.case_resident(orc, lib, tmp_path)
def test_deterministic(orc, lib, tmp_path): bc.case_deterministic(orc, lib, tmp_path)
def test_bad_arguments(orc, lib, tmp_path): bc.case_bad_arguments(orc, lib, tmp_path)
