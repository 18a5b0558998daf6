"""callVariant in batches (ldbg_engine_variant_batch) and ComputeInheritance.call_variants through the TEST-ONLY host
simulation of the kernels, one lane per wavefront and 64 lanes in lock step, against the yardstick of tests/variant_cases.py (the
reference's loops over the CPU oracle's cursor, trimToAlleles and TableWriter on strings).  The same cases run on the device in
tests/test_gpu_variants.py."""
import pytest

from tests import variant_cases as vc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


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
