"""FindOrphans through the HIP library on an MI355X: the cases of tests/orphan_cases.py (also run through the host simulation by
tests/test_orphans_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import orphan_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("k", oc.ORPHAN_K)
def test_find_orphans(orc, lib, tmp_path, k): oc.case_find_orphans(orc, lib, tmp_path, k)


@pytest.mark.parametrize("stopper", oc.LOOP_RULES)
@pytest.mark.parametrize("k", oc.ORPHAN_K)
def test_orphan_loop(orc, lib, tmp_path, k, stopper): oc.case_orphan_loop(orc, lib, tmp_path, k, stopper)


def test_orphans_null_record(orc, lib, tmp_path): oc.case_orphans_null_record(orc, lib, tmp_path)
