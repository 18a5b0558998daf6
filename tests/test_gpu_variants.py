"""callVariant in batches (ldbg_engine_variant_batch) and ComputeInheritance.call_variants through the HIP library on an
MI355X: the cases of tests/variant_cases.py (also run through the host simulation by tests/test_variants_hostsim.py).  Run with
`pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import variant_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("k", vc.WIDTH_K)
def test_variant_widths(orc, lib, tmp_path, k): vc.case_widths(orc, lib, tmp_path, k)


def test_variant_boundaries(orc, lib, tmp_path):
    lengths = set()
    for k in vc.BOUNDARY_K:
        lengths |= vc.case_boundaries(orc, lib, tmp_path, k)
    assert {63, 64, 65, 127, 128, 129} <= lengths


@pytest.mark.parametrize("n", vc.SEED_COUNTS)
def test_variant_seed_counts(orc, lib, tmp_path, n): vc.case_counts(orc, lib, tmp_path, n)


def test_variant_pool_of_three(orc, lib, tmp_path, monkeypatch): vc.case_counts(orc, lib, tmp_path, 65, monkeypatch, slots=3)
def test_variant_family(orc, lib, tmp_path): vc.case_family(orc, lib, tmp_path)
def test_variant_tables(orc, lib, tmp_path): vc.case_tables(orc, lib, tmp_path)
def test_variant_sums(orc, lib, tmp_path): vc.case_sums(orc, lib, tmp_path, vc.package_mean)
def test_variant_refused(orc, lib, tmp_path): vc.case_refused(orc, lib, tmp_path)
def test_call_variants_command(orc, lib, tmp_path): vc.case_command(orc, lib, tmp_path)
