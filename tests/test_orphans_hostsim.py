"""FindOrphans (corticall_amd.partition.FindOrphans: neighbour batches and one dfs batch on the device, the order-dependent loop replayed
on the host) through the TEST-ONLY host simulation, against the restatement over the oracle engine in tests/orphan_cases.py.  The same
cases run on the device in tests/test_gpu_orphans.py."""
import pytest

from tests import orphan_cases as oc


@pytest.fixture(scope="module")
def lib():
    from tests import hostsim
    return hostsim.load()


@pytest.mark.parametrize("k", oc.ORPHAN_K)
def test_find_orphans(orc, lib, tmp_path, k): oc.case_find_orphans(orc, lib, tmp_path, k)


@pytest.mark.parametrize("stopper", oc.LOOP_RULES)
@pytest.mark.parametrize("k", oc.ORPHAN_K)
def test_orphan_loop(orc, lib, tmp_path, k, stopper): oc.case_orphan_loop(orc, lib, tmp_path, k, stopper)


def test_orphans_null_record(orc, lib, tmp_path): oc.case_orphans_null_record(orc, lib, tmp_path)
