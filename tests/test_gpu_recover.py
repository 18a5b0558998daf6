"""RecoverExcludedKmers on the device (ldbg_graph_recover) through the HIP library on an MI355X: the cases of
tests/recover_cases.py (also run through the host simulation by tests/test_recover_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import recover_cases as rv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("N", rv.SHAPE_SIZES)
def test_recover_shapes(orc, lib, tmp_path, N): rv.case_recover_shapes(orc, lib, tmp_path, N)


@pytest.mark.parametrize("C,child", rv.COLOUR_CASES)
def test_recover_colours(orc, lib, tmp_path, C, child): rv.case_recover_colours(orc, lib, tmp_path, C, child)


@pytest.mark.parametrize("k", rv.WIDTH_K)
def test_recover_widths(orc, lib, tmp_path, k): rv.case_recover_widths(orc, lib, tmp_path, k)


def test_recover_tiny_dirty(orc, lib, tmp_path): rv.case_recover_tiny_dirty(orc, lib, tmp_path)
def test_recover_dirty_colours(orc, lib, tmp_path): rv.case_recover_dirty_colours(orc, lib, tmp_path)
def test_recover_end_to_end(orc, lib, tmp_path): rv.case_recover_end_to_end(orc, lib, tmp_path)
def test_recover_bad_arguments(orc, lib, tmp_path): rv.case_recover_bad_arguments(orc, lib, tmp_path)
