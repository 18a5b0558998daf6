"""The fixed-layout walk kernels (k_walk_rows<W, C>) on a real MI355X: the cases of tests/walk_rows_cases.py through the HIP library, each
on the generic kernel and under LDBG_WALK_ROWS, against the oracle and against each other byte for byte; and one batch beyond the residency
cap, which shows that the runtime grants the new symbol eight wavefronts per CU as it does the generic kernel.  Run with `pytest -m gpu`;
the host simulation runs the same cases in tests/test_hostsim_walk_rows.py."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import parity_cases as pc
from tests import refill_cases as rc
from tests import walk_rows_cases as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


@pytest.mark.parametrize("case", wr.FIXED_DEVICE, ids=wr.case_id)
def test_fixed_kernel_equals_generic(orc, lib, tmp_path, monkeypatch, case):
    wr.both_kernels(monkeypatch, lib, True, case[0], orc, lib, tmp_path, *case[1])


@pytest.mark.parametrize("case", wr.GENERIC, ids=wr.case_id)
def test_generic_kernel_keeps_what_is_not_built(orc, lib, tmp_path, monkeypatch, case):
    wr.both_kernels(monkeypatch, lib, False, case[0], orc, lib, tmp_path, *case[1])


def test_lanes_refill(orc, lib, tmp_path, monkeypatch):
    rc.few_slots(monkeypatch, 64)
    wr.both_kernels(monkeypatch, lib, True, pc.case_random_walks, orc, lib, tmp_path, 47, 5, True)
    assert rc.refills(lib, "walk_refills") > 0


def test_second_launch_takes_the_fixed_kernel(orc, lib, tmp_path, monkeypatch):
    wr.second_launch(monkeypatch, lib, pc.case_random_walks, orc, lib, tmp_path, 47, 5, True)


def test_second_launch_takes_the_fixed_kernel_one_word(orc, lib, tmp_path, monkeypatch):
    wr.second_launch(monkeypatch, lib, wr.case_one_colour, orc, lib, tmp_path, 31, 0)


def test_eight_wavefronts_per_cu_beyond_the_residency_cap(orc, lib, tmp_path, monkeypatch):
    """refill_cases.BEYOND_N seeds in one batch (k = 31, three colours: k_walk_rows<1, 3>): more strands than 8 x CUs x 64 lanes, so the
    grid is what rt::blocks_per_cu answers for the kernel that is launched.  The same batch on the generic kernel: the same bytes.  (Against
    the oracle this batch is checked by tests/test_gpu_refill.py::test_walks_beyond_the_residency_cap, which takes the fixed kernel too.)"""
    import corticall_amd as ca
    from corticall_amd import ContigStopper, TraversalEngineFactory
    cs, distinct, which = rc._beyond_cap_graph(orc, lib, tmp_path, "rows_cap")
    seeds = np.ascontiguousarray(np.frombuffer("".join(distinct).encode(), dtype=np.uint8).reshape(len(distinct), cs.k)[which])
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert 2 * rc.BEYOND_N > 8 * cus * 64
    e = TraversalEngineFactory(lib=lib).traversalColors(0).graph(cs.g).maxBranchLength(100).stoppingRule(ContigStopper).links(cs.links["kid"]).make()

    def batch():
        ca.profile_reset(lib=lib)
        arena, offs, wl = e.walk_batch_arrays(seeds)
        return (arena.tobytes(), offs.tobytes(), wl.tobytes(), e.kmers_traversed), int(ca.profile_get("walk_wavefronts", lib=lib)[0]), wr.fixed_rows(lib)
    generic, waves_g, n_generic = batch()
    assert n_generic == 0 and waves_g == 8 * cus, (n_generic, waves_g, cus)
    monkeypatch.setenv(wr.KNOB, "1")
    fixed, waves, n_fixed = batch()
    print("k_walk_rows<1, 3>: walk_wavefronts %d = %.2f x %d CUs, walk_fixed_rows %d" % (waves, waves / cus, cus, n_fixed))
    assert n_fixed > 0 and waves == 8 * cus, (n_fixed, waves, cus)
    assert generic == fixed
    assert len(set(np.diff(np.frombuffer(fixed[1], dtype=np.int64)).tolist())) > 5         # contigs of many lengths
