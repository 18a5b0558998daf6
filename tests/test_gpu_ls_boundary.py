"""Walks and searches whose link stores end on either side of the LDS / HBM split (tests/ls_boundary_cases.py), on a real MI355X: the probe
walk's store peaks at 9, 11, 12 (the last element in LDS), 13 (the first in the HBM tail), 14, 16 and 18 elements.  Run with
`pytest -m gpu`; tests/test_ls_boundary.py runs the same cases in the host simulation and checks the peaks."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import ls_boundary_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("stride", bc.STRIDES)
def test_walks_and_searches_across_the_split(orc, lib, tmp_path, stride): bc.case_across_the_split(orc, lib, tmp_path, stride)
