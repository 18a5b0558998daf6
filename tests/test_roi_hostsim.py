"""Record selection (ldbg_graph_select, DESIGN.md §11: FindROIs, the prefilters, Remove) through the TEST-ONLY host simulation of the
kernels, one lane per wavefront and 64 lanes in lock step, against the numpy yardstick of tests/roi_cases.py.  The same cases run on
the device in tests/test_gpu_roi.py."""
import pytest

from tests import roi_cases as rc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


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
