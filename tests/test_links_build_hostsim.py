"""Link construction (ldbg_links_build) through the TEST-ONLY host simulation of the kernels, one lane per wavefront
and 64 lanes in lock step, against the oracle's TempLinksAssembler restatement (tests/links_build_cases.py).  The same cases run on
the device in tests/test_gpu_links_build.py."""
import pytest

from tests import links_build_cases as lc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


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
