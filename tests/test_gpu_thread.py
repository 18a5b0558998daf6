"""Sequences threaded through a graph on the device (ldbg_graph_thread) and the commands over it through the HIP library
on an MI355X: the cases of tests/thread_cases.py (also run through the host simulation by tests/test_thread_hostsim.py).  Run with
`pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import thread_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


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
