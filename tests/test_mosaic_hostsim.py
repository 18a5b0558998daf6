"""Tesserae in batches (ldbg_mosaic_align_batch) through the TEST-ONLY host simulation of the kernel, one lane per
wavefront and 64 lanes in lock step, against the literal yardstick of tests/mosaic_cases.py.  The same cases run on the device in
tests/test_gpu_mosaic.py.  Also here, because they need no library: the yardstick against the reference's smallTest, sectionContig /
trimQuery against string restatements, and the sanitizer build's stand-alone program."""
import os
import subprocess

import pytest

from tests import mosaic_cases as mc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


def test_yardstick_small_test(): mc.case_yardstick_small_test()
def test_section_contig_and_trim_query(): mc.case_section_and_trim()
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


def test_mosaic_sanitizer_program():
    """hostsim-san-mosaic builds, and its program (ASan + UBSan over the host simulation, a process of its own) exits clean on the
    boundary-length cases"""
    csrc = os.path.join(mc.ROOT, "corticall_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "hostsim-san-mosaic", "-j8"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(mc.ROOT, "tests", "hostsim", "_build_asan", "mosaic_san_main")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "mosaic_san_main: ok" in out.stdout
