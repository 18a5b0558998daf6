"""Sequences threaded through a graph on the device (ldbg_graph_thread) and the commands over it through the TEST-ONLY
host simulation of the kernels, one lane per wavefront and 64 lanes in lock step, against the string / dict / set yardstick of
tests/thread_cases.py.  The same cases run on the device in tests/test_gpu_thread.py."""
import pytest

from tests import thread_cases as tc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


@pytest.mark.parametrize("k", tc.WIDTH_K)
def test_thread_widths(orc, lib, tmp_path, k): tc.case_widths(orc, lib, tmp_path, k)


@pytest.mark.parametrize("n", tc.CHUNK_WINDOWS)
def test_thread_chunk_single(orc, lib, tmp_path, n): tc.case_chunk_single(orc, lib, tmp_path, n)


@pytest.mark.parametrize("n", tc.MANY_SEQS)
def test_thread_many_sequences(orc, lib, tmp_path, n): tc.case_many_sequences(orc, lib, tmp_path, n)


def test_thread_lengths(orc, lib, tmp_path): tc.case_lengths(orc, lib, tmp_path)
def test_thread_chunk_batch(orc, lib, tmp_path): tc.case_chunk_batch(orc, lib, tmp_path)
def test_thread_non_bases(orc, lib, tmp_path): tc.case_non_bases(orc, lib, tmp_path)
def test_thread_table_sizes(orc, lib, tmp_path): tc.case_table_sizes(orc, lib, tmp_path)
def test_thread_repeats(orc, lib, tmp_path): tc.case_repeats(orc, lib, tmp_path)
def test_thread_regions(orc, lib, tmp_path): tc.case_regions(orc, lib, tmp_path)
def test_trim_partitions(orc, lib, tmp_path): tc.case_trim(orc, lib, tmp_path)
def test_filter_and_count_partitions(orc, lib, tmp_path): tc.case_filter_and_count(orc, lib, tmp_path)
def test_coverage(orc, lib, tmp_path): tc.case_coverage(orc, lib, tmp_path)
def test_thread_end_to_end(orc, lib, tmp_path): tc.case_end_to_end(orc, lib, tmp_path)
def test_thread_bad_arguments(orc, lib, tmp_path): tc.case_bad_arguments(orc, lib, tmp_path)
def test_thread_too_many_windows(orc, lib, tmp_path): tc.case_too_many_windows(orc, lib, tmp_path)
