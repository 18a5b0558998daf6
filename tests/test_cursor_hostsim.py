"""Cursors advanced in batches (ldbg_engine_cursor_batch) through the TEST-ONLY host simulation of the kernels, one lane
per wavefront and 64 lanes in lock step, against the yardstick of tests/cursor_cases.py (the reference's loops over the CPU oracle's
cursor).  The same cases run on the device in tests/test_gpu_cursor.py."""
import pytest

from tests import cursor_cases as cc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


@pytest.mark.parametrize("with_links", [False, True], ids=["plain", "links"])
@pytest.mark.parametrize("k", cc.WIDTH_K)
def test_cursor_widths(orc, lib, tmp_path, k, with_links): cc.case_widths(orc, lib, tmp_path, k, with_links)


@pytest.mark.parametrize("n", cc.BATCH_SIZES)
def test_cursor_batch_sizes(orc, lib, tmp_path, n): cc.case_batch_size(orc, lib, tmp_path, n)


@pytest.mark.parametrize("with_links", [False, True], ids=["plain", "links"])
@pytest.mark.parametrize("slots", [1, 3, 64])
def test_cursor_slot_reuse(orc, lib, tmp_path, monkeypatch, slots, with_links): cc.case_slot_reuse(orc, lib, tmp_path, monkeypatch, slots, with_links)


@pytest.mark.parametrize("slots", [1, 3])
def test_cursor_epoch_wrap(orc, lib, tmp_path, monkeypatch, slots): cc.case_slot_reuse(orc, lib, tmp_path, monkeypatch, slots, True, epoch0=0x3FFF - 3)


def test_cursor_reference_vectors(orc, lib, tmp_path): cc.case_reference_vectors(orc, lib, tmp_path)
def test_cursor_limits(orc, lib, tmp_path): cc.case_limits(orc, lib, tmp_path)
def test_cursor_stop_rules(orc, lib, tmp_path): cc.case_stop_rules(orc, lib, tmp_path)
def test_cursor_null_records(orc, lib, tmp_path): cc.case_null_records(orc, lib, tmp_path)
def test_cursor_refused(orc, lib, tmp_path): cc.case_refused(orc, lib, tmp_path)
def test_cursor_agrees_with_assemble(orc, lib, tmp_path): cc.case_agrees_with_assemble(orc, lib, tmp_path)
