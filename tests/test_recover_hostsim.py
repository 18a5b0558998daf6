"""RecoverExcludedKmers on the device (ldbg_graph_recover) through the TEST-ONLY host simulation of the kernels, one lane
per wavefront and 64 lanes in lock step, against the numpy / dict yardstick of tests/recover_cases.py.  The same cases run on the
device in tests/test_gpu_recover.py."""
import pytest

from tests import recover_cases as rv


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


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
