"""FindLowComplexity (corticall_amd.prefilter.FindLowComplexity, host only): a ROI record is excluded when
(float) gzipLength / (float) k < threshold (J/commands/prefilter/FindLowComplexity.java:35-100, SequenceUtils.java:794-813).  The
expected exclusions come from an independent route to the same number — gzip.compress(b, 6, mtime=0), the whole gzip member — and
float32 arithmetic.  The ROI is opened through the host simulation; nothing here needs a GPU."""
import gzip
import random

import numpy as np
import pytest

from corticall_amd import CortexGraph, FindLowComplexity
from corticall_amd.prefilter import gzip_length
from tests import recover_cases as rv
from tests import roi_cases as rc
from tests.parity_cases import rand_seq

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def lib():
    from tests import hostsim
    return hostsim.load()


def canonical(s):
    r = s.encode().translate(_COMP)[::-1].decode()
    return min(s, r)


def roi_of(tmp, k):
    """homopolymers, dinucleotide and trinucleotide repeats, random k-mers -> (path, the canonical k-mers in record order)"""
    rng = random.Random(k)
    kmers = {canonical(b * k) for b in "ACGT"}
    kmers |= {canonical((a + b) * k)[:k] for a in "ACGT" for b in "ACGT" if a != b}
    kmers |= {canonical(((u * k)[:k])) for u in ("ACG", "AAT", "CCG", "ACGT", "AACCGGTT")}
    kmers |= {canonical(rand_seq(rng, k)) for _ in range(40)}
    kmers = sorted(kmers)
    asc = np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(len(kmers), k)
    n = len(kmers)
    cov = np.arange(1, n + 1, dtype=np.uint32).reshape(n, 1)
    edges = (np.arange(n) % 256).astype(np.uint8).reshape(n, 1)
    return rc.write_ctx(tmp / ("roi%d.ctx" % k), k, ["kid"], rv.pack_kmers(asc, k), cov, edges), kmers


def ratio(kmer):
    return np.float32(len(gzip.compress(kmer.encode(), 6, mtime=0))) / np.float32(len(kmer))


@pytest.mark.parametrize("k", [31, 47])
def test_low_complexity(lib, tmp_path, k):
    path, kmers = roi_of(tmp_path, k)
    roi = CortexGraph(path, lib=lib)
    assert roi.getNumRecords() == len(kmers)
    assert all(gzip_length(s.encode()) == len(gzip.compress(s.encode(), 6, mtime=0)) for s in kmers)
    ratios = np.array([ratio(s) for s in kmers], dtype=np.float32)
    on = np.sort(np.unique(ratios))[len(np.unique(ratios)) // 2]                 # a threshold that sits exactly on a ratio
    for tag, thr in (("default", 0.70), ("on", on), ("above", np.nextafter(on, np.float32(2)))):
        exp = [i for i in range(len(kmers)) if ratios[i] < np.float32(thr)]
        f = FindLowComplexity(None, [], roi, thr) if tag != "default" else FindLowComplexity(None, [], roi)
        out = tmp_path / ("low_%s.ctx" % tag)
        kept, excluded = f.execute(out)
        assert f.excluded == exp and (kept, excluded) == (len(kmers) - len(exp), len(exp)), (k, tag)
        assert out.read_bytes() == rc.expected_excluded(path, exp, lib, tmp_path, "low_%s" % tag)
        if tag == "default" and k == 47:
            assert 0 < len(exp) < len(kmers)                                     # at least one excluded and one kept
            assert kmers.index("A" * k) in exp                                   # a homopolymer compresses
        if tag == "on":                                                          # the strict <: the k-mers on the ratio are kept
            assert any(ratios[i] == on for i in range(len(kmers))) and all(ratios[i] != on for i in exp)
            n_on = len(exp)
        if tag == "above":
            assert len(exp) > n_on
    assert FindLowComplexity(None, [], roi).execute() == FindLowComplexity(None, [], roi, 0.70).execute()
    roi.close()
