"""Tesserae in batches (ldbg_mosaic_align_batch) through the HIP library on an MI355X: the cases of tests/mosaic_cases.py
(also run through the host simulation by tests/test_mosaic_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import mosaic_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


def test_mosaic_small_tests(lib): mc.case_small_tests(lib)
def test_mosaic_alignment(lib): mc.case_mosaic_alignment(lib)
def test_mosaic_lengths(lib): mc.case_lengths(lib)
def test_mosaic_hbm_columns(lib, monkeypatch): mc.case_hbm_columns(lib, monkeypatch)


@pytest.mark.parametrize("n", [1, 63, 64])
def test_mosaic_batch(lib, n): mc.case_batch(lib, n)


def test_mosaic_batch_slices_and_singles(lib, monkeypatch): mc.case_batch(lib, 65, monkeypatch)
def test_mosaic_ties(lib): mc.case_ties(lib)
def test_mosaic_non_bases(lib): mc.case_non_bases(lib)
def test_mosaic_long_gaps(lib): mc.case_long_gaps(lib)
def test_mosaic_quirk(lib): mc.case_quirk(lib)
def test_mosaic_roundtrip(lib): mc.case_roundtrip(lib)
def test_mosaic_refusals(lib, monkeypatch): mc.case_refusals(lib, monkeypatch)
