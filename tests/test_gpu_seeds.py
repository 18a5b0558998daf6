"""The variant seeds (ldbg_graph_variant_seeds), the occurrences of a threading (ldbg_threading_occurrences) and the commands
over them through the HIP library on an MI355X: the cases of tests/seed_cases.py (also run through the host simulation by
tests/test_seeds_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import seed_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("strand", [1, -1], ids=["forward", "reverse"])
@pytest.mark.parametrize("j", [1, 2, 3])
def test_seed_chain(orc, lib, tmp_path, j, strand): sc.case_chain(orc, lib, tmp_path, j, strand)


@pytest.mark.parametrize("k", sc.WIDTH_K)
def test_seed_widths(orc, lib, tmp_path, k): sc.case_widths(orc, lib, tmp_path, k)


@pytest.mark.parametrize("n", sc.CHUNK_N)
def test_seed_chunks(orc, lib, tmp_path, n): sc.case_chunks(orc, lib, tmp_path, n)


@pytest.mark.parametrize("c,children", sc.INHERITANCE)
def test_seed_inheritance_clauses(orc, lib, tmp_path, c, children): sc.case_inheritance_clauses(orc, lib, tmp_path, c, children)


def test_seed_chain_no_start(orc, lib, tmp_path): sc.case_chain_no_start(orc, lib, tmp_path)
def test_seed_asymmetric(orc, lib, tmp_path): sc.case_asymmetric(orc, lib, tmp_path)
def test_seed_out_two(orc, lib, tmp_path): sc.case_out_two(orc, lib, tmp_path)
def test_seed_repeats(orc, lib, tmp_path): sc.case_repeats(orc, lib, tmp_path)
def test_seed_clauses(orc, lib, tmp_path): sc.case_clauses(orc, lib, tmp_path)
def test_occurrences(orc, lib, tmp_path): sc.case_occurrences(orc, lib, tmp_path)
def test_compute_assembly_quality(orc, lib, tmp_path): sc.case_quality(orc, lib, tmp_path)
def test_compute_inheritance_seeds(orc, lib, tmp_path): sc.case_inheritance_command(orc, lib, tmp_path)
def test_seed_refused(orc, lib, tmp_path): sc.case_refused(orc, lib, tmp_path)
