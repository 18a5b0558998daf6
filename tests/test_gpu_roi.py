"""Record selection (ldbg_graph_select, DESIGN.md §11: FindROIs, the prefilters, Remove) through the HIP library on an MI355X: the
cases of tests/roi_cases.py (also run through the host simulation by tests/test_roi_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import roi_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("N", rc.SHAPE_SIZES)
def test_select_shapes(orc, lib, tmp_path, N): rc.case_select_shapes(orc, lib, tmp_path, N)


@pytest.mark.parametrize("C", rc.CLAUSE_COLOURS)
def test_filter_clauses(orc, lib, tmp_path, C): rc.case_filter_clauses(orc, lib, tmp_path, C)


@pytest.mark.parametrize("k", rc.PACK_K)
def test_pack_layouts(orc, lib, tmp_path, k): rc.case_pack_layouts(orc, lib, tmp_path, k)


def test_find_rois(orc, lib, tmp_path): rc.case_find_rois(orc, lib, tmp_path)
def test_prefilters(orc, lib, tmp_path): rc.case_prefilters(orc, lib, tmp_path)
def test_remove(orc, lib, tmp_path): rc.case_remove(orc, lib, tmp_path)
def test_resident_roi(orc, lib, tmp_path): rc.case_resident_roi(orc, lib, tmp_path)
def test_bad_arguments(orc, lib, tmp_path): rc.case_bad_arguments(orc, lib, tmp_path)
