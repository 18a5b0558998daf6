"""Link construction (ldbg_links_build) through the HIP library on an MI355X: the cases of tests/links_build_cases.py
(also run through the host simulation by tests/test_links_build_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import links_build_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("nw", lc.SHAPE_WINDOWS)
def test_shapes(orc, lib, tmp_path, nw): lc.case_shapes(orc, lib, tmp_path, nw)


@pytest.mark.parametrize("k", lc.KMER_SIZES)
def test_kmer_sizes(orc, lib, tmp_path, k): lc.case_kmer_sizes(orc, lib, tmp_path, k)


@pytest.mark.parametrize("C", [8, 32])
def test_many_colours(orc, lib, tmp_path, C): lc.case_many_colours(orc, lib, tmp_path, C)


def test_reference_vectors(orc, lib, tmp_path): lc.case_reference_vectors(orc, lib, tmp_path)
def test_short_reads(orc, lib, tmp_path): lc.case_short_reads(orc, lib, tmp_path)
def test_colours(orc, lib, tmp_path): lc.case_colours(orc, lib, tmp_path)
def test_orders(orc, lib, tmp_path): lc.case_orders(orc, lib, tmp_path)
def test_one_sided_edges(orc, lib, tmp_path): lc.case_one_sided_edges(orc, lib, tmp_path)
def test_errors(orc, lib, tmp_path): lc.case_errors(orc, lib, tmp_path)
def test_bad_arguments(orc, lib, tmp_path): lc.case_bad_arguments(orc, lib, tmp_path)
def test_resident(orc, lib, tmp_path): lc.case_resident(orc, lib, tmp_path)
def test_end_to_end(orc, lib, tmp_path): lc.case_end_to_end(orc, lib, tmp_path)
def test_deterministic(orc, lib, tmp_path): lc.case_deterministic(orc, lib, tmp_path)
