"""Smith-Waterman in batches (ldbg_sw_align_batch) through the HIP library on an MI355X: the cases of tests/sw_cases.py
(also run through the host simulation by tests/test_sw_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import sw_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


def test_sw_table(lib): sc.case_table(lib)
def test_sw_lengths(lib): sc.case_lengths(lib)
def test_sw_lds_limit(lib, monkeypatch): sc.case_lds_limit(lib, monkeypatch)
def test_sw_random_inputs_have_gaps(): sc.case_random_inputs_have_gaps()
def test_sw_random(lib): sc.case_random(lib)
def test_sw_ties(lib): sc.case_ties(lib)
def test_sw_long_gaps(lib): sc.case_long_gaps(lib)
def test_sw_letters(lib): sc.case_letters(lib)


@pytest.mark.parametrize("n", [1, 63, 64])
def test_sw_batch(lib, n): sc.case_batch(lib, n)


def test_sw_batch_slices_and_singles(lib, monkeypatch): sc.case_batch(lib, 65, monkeypatch)
def test_sw_refusals(lib, monkeypatch): sc.case_refusals(lib, monkeypatch)
def test_sw_helpers(lib): sc.case_helpers(lib)
