"""Smith-Waterman in batches (ldbg_sw_align_batch) through the TEST-ONLY host simulation of the kernel, one lane per
wavefront and 64 lanes in lock step, against the literal yardstick of tests/sw_cases.py.  The same cases run on the device in
tests/test_gpu_sw.py.  Also here, because they need no library: the yardstick against the values derived by hand, the condition on
the random inputs, the callers' arithmetic against string restatements, and the sanitizer build's stand-alone program."""
import os
import subprocess

import pytest

from tests import sw_cases as sc


@pytest.fixture(scope="module", params=[1, 64], ids=["lane1", "lanes64"])
def lib(request):
    from tests import hostsim
    l = hostsim.load()
    l.dll.ldbg_hostsim_set_lanes(request.param)
    yield l
    l.dll.ldbg_hostsim_set_lanes(1)


def test_yardstick_table(): sc.case_yardstick_table()
def test_random_inputs_have_gaps(): sc.case_random_inputs_have_gaps()
def test_helpers_no_library(): sc.case_helpers_no_library()
def test_sw_table(lib): sc.case_table(lib)
def test_sw_lengths(lib): sc.case_lengths(lib)
def test_sw_lds_limit(lib, monkeypatch): sc.case_lds_limit(lib, monkeypatch)
def test_sw_random(lib): sc.case_random(lib)
def test_sw_ties(lib): sc.case_ties(lib)
def test_sw_long_gaps(lib): sc.case_long_gaps(lib)
def test_sw_letters(lib): sc.case_letters(lib)


@pytest.mark.parametrize("n", [1, 63, 64])
def test_sw_batch(lib, n): sc.case_batch(lib, n)


def test_sw_batch_slices_and_singles(lib, monkeypatch): sc.case_batch(lib, 65, monkeypatch)
def test_sw_refusals(lib, monkeypatch): sc.case_refusals(lib, monkeypatch)
def test_sw_helpers(lib): sc.case_helpers(lib)


def test_sw_sanitizer_program():
    """hostsim-san-sw builds, and its program (ASan + UBSan over the host simulation, a process of its own) exits clean on the
    boundary-length cases"""
    csrc = os.path.join(sc.ROOT, "corticall_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "hostsim-san-sw", "-j8"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(sc.ROOT, "tests", "hostsim", "_build_asan", "sw_san_main")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "sw_san_main: ok" in out.stdout
