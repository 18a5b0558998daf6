"""Cursors advanced in batches (ldbg_engine_cursor_batch) through the HIP library on an MI355X: the cases of
tests/cursor_cases.py (also run through the host simulation by tests/test_cursor_hostsim.py).  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import cursor_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


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
