"""Graph construction (ldbg_graph_build) through the TEST-ONLY host simulation of the kernels, one lane per wavefront
and 64 lanes in lock step, against the oracle's TempGraphAssembler restatement (tests/build_cases.py).  The same cases run on the
device in tests/test_gpu_build.py."""
import pytest

from tests import build_cases as bc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


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
