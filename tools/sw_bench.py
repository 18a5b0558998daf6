"""Smith-Waterman in batches (ldbg_sw_align_batch): cell updates per second on the device, beside one host thread running
the same kernel body.

Two shapes: 1,000 x 1,000 bases in batches of 1, 64 and 4,096 pairs (the inversion test of Call), and 150 x 150 bases in a batch of
65,536 (VerifyCalls).  The subject is a copy of the query with a substitution every ~25 bases and a few short insertions and deletions.
A cell update is one (MATCH, GAPINCOL, GAPINROW) triple: query length x subject length per pair.  Per batch: the device time of the
"sw" profile family (HIP events around the launches), cell updates per second from it, and the wall time of the whole call (filter,
upload, launches, traceback, download).

The number set against it: tools/_build/libsw_cpu.so, the kernel body of corticall_amd/csrc/sw.cpp compiled as plain C++ at -O2 and run
by one thread on this machine's host, on --cpu-pairs pairs of each shape; its arrays must equal the device's."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libldbg: torch's HIP runtime initialises first)

import corticall_amd as ca  # noqa: E402
from corticall_amd import _native  # noqa: E402


def make_pairs(rng, n, length):
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for _ in range(n):
        q = rng.integers(0, 4, size=length)
        s = np.where(rng.random(size=length) < 0.04, rng.integers(0, 4, size=length), q)
        s = s.tolist()
        for _ in range(max(1, length // 250)):
            at = int(rng.integers(0, len(s)))
            if rng.random() < 0.5:
                del s[at:at + int(rng.integers(1, 7))]
            else:
                s[at:at] = rng.integers(0, 4, size=int(rng.integers(1, 7))).tolist()
        s = (s + q.tolist())[:length]
        out.append((bases[q].tobytes().decode(), bases[np.asarray(s)].tobytes().decode()))
    return out


def cpu_run(cpu, pairs):
    n = len(pairs)
    q = b"".join(a.encode() for a, _ in pairs)
    s = b"".join(b.encode() for _, b in pairs)
    qoff = np.zeros(n + 1, np.int64)
    soff = np.zeros(n + 1, np.int64)
    qoff[1:] = np.cumsum([len(a) for a, _ in pairs])
    soff[1:] = np.cumsum([len(b) for _, b in pairs])
    score = np.zeros(n, np.float64)
    out6 = np.zeros((n, 6), np.int32)
    sec = C.c_double()
    rc = cpu.sw_cpu_align(C.c_int64(n), q, qoff.ctypes.data_as(C.c_void_p), s, soff.ctypes.data_as(C.c_void_p), score.ctypes.data_as(C.c_void_p),
                          out6.ctypes.data_as(C.c_void_p), C.byref(sec))
    assert rc == 0
    return score, out6, sec.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000:1,64,4096;150:65536", help="length:batches;...")
    ap.add_argument("--cpu-pairs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    lib = ca.default_lib()
    print("library:", lib.dll.ldbg_version().decode(), flush=True)
    cpu = C.CDLL(os.path.join(ROOT, "tools", "_build", "libsw_cpu.so"))
    rng = np.random.default_rng(20)
    sw = ca.SmithWaterman(lib=lib)
    for shape in args.shapes.split(";"):
        length, batches = shape.split(":")
        length = int(length)
        cells_each = length * length
        ps = make_pairs(rng, args.cpu_pairs, length)
        score, out6, sec = cpu_run(cpu, ps)
        dev = sw.align_arrays(ps)
        dev6 = np.stack([dev.end_q, dev.end_s, dev.begin_q, dev.begin_s, dev.aligned_len, dev.edits], axis=1)
        assert dev.score.tobytes() == score.tobytes() and (dev6 == out6).all(), "the host build and the device disagree"
        print("shape=%dx%d host-one-thread n=%d wall_s=%.3f cells_per_s=%.3e (arrays equal to the device's)" % (length, length, len(ps), sec, len(ps) * cells_each / sec),
              flush=True)
        for n in [int(x) for x in batches.split(",")]:
            ps = make_pairs(rng, min(n, 256), length)
            ps = (ps * ((n + len(ps) - 1) // len(ps)))[:n]
            for rep in range(args.repeats):
                ms0 = ca.profile_get("sw", lib)[0]
                t0 = time.perf_counter()
                r = sw.align_arrays(ps)
                wall = time.perf_counter() - t0
                ms = ca.profile_get("sw", lib)[0] - ms0
                assert (r.status == _native.LDBG_OK).all()
                print("shape=%dx%d device n=%d repeat=%d device_ms=%.2f cells_per_s=%.3e wall_s=%.3f" % (length, length, n, rep, ms, n * cells_each / (ms / 1e3), wall),
                      flush=True)


if __name__ == "__main__":
    main()
