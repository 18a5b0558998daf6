"""Tesserae in batches (ldbg_mosaic_align_batch): cell updates per second on the device, beside one host thread running
the same kernel body.

The shape: a query of --query-len bases against 2, then 8, targets of --target-len bases (each target a copy of a random haplotype
with a substitution every ~50 bases; the query switches haplotype every 250 bases), in batches of 1, 64 and 4,096 problems.  A cell
update is one (M, I, D) triple: query length x sum of target lengths per problem.  Per batch: the device time of the "mosaic" profile
family (HIP events around the launches), cell updates per second from it, and the wall time of the whole call (conversion, upload,
launches, traceback, download).

The number set against it: tools/_build/libmosaic_cpu.so, the kernel body of corticall_amd/csrc/mosaic.cpp compiled as plain C++ at
-O2 and run by one thread on this machine's host, on --cpu-problems problems of each shape; its log likelihoods must carry the
device's bits."""
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


def make_problems(rng, n, n_targets, qlen, tlen):
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for _ in range(n):
        hap = rng.integers(0, 4, size=(n_targets, tlen))
        flip = rng.random(size=hap.shape) < 0.02
        base = rng.integers(0, 4, size=tlen)
        hap = np.where(flip, hap, base[None, :])
        at = np.arange(min(qlen, tlen))
        q = hap[(at // 250) % n_targets, at]
        out.append((bases[q].tobytes().decode(), [("h%d" % t, bases[hap[t]].tobytes().decode()) for t in range(n_targets)]))
    return out


def pack(problems):
    qoff, tfirst, toff = [0], [0], [0]
    qs, ts = [], []
    for q, t in problems:
        qs.append(q.encode())
        qoff.append(qoff[-1] + len(q))
        for _, s in t:
            ts.append(s.encode())
            toff.append(toff[-1] + len(s))
        tfirst.append(len(toff) - 1)
    return b"".join(qs), np.asarray(qoff, np.int64), np.asarray(tfirst, np.int64), b"".join(ts), np.asarray(toff, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--targets", default="2,8")
    ap.add_argument("--query-len", type=int, default=1000)
    ap.add_argument("--target-len", type=int, default=1000)
    ap.add_argument("--cpu-problems", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    lib = ca.default_lib()
    print("library:", lib.dll.ldbg_version().decode(), flush=True)
    cpu = C.CDLL(os.path.join(ROOT, "tools", "_build", "libmosaic_cpu.so"))
    rng = np.random.default_rng(19)
    t = ca.Tesserae(lib=lib)
    for nt in [int(x) for x in args.targets.split(",")]:
        cells_each = args.query_len * nt * args.target_len
        ps = make_problems(rng, args.cpu_problems, nt, args.query_len, args.target_len)
        q, qoff, tfirst, tb, toff = pack(ps)
        llk = np.zeros(len(ps), np.float64)
        sec = C.c_double()
        rc = cpu.mosaic_cpu_align(C.byref(t.params), C.c_int64(len(ps)), q, qoff.ctypes.data_as(C.c_void_p), tfirst.ctypes.data_as(C.c_void_p), tb,
                                  toff.ctypes.data_as(C.c_void_p), llk.ctypes.data_as(C.c_void_p), C.byref(sec))
        assert rc == 0
        dev = t.align_arrays(ps)
        assert dev[1].tobytes() == llk.tobytes(), "the host build and the device disagree"
        print("targets=%d host-one-thread n=%d wall_s=%.3f cells_per_s=%.3e (llk bits equal to the device's)" % (nt, len(ps), sec.value, len(ps) * cells_each / sec.value),
              flush=True)
        for n in [int(x) for x in args.batches.split(",")]:
            ps = make_problems(rng, n, nt, args.query_len, args.target_len)
            for rep in range(args.repeats):
                ms0 = ca.profile_get("mosaic", lib)[0]
                t0 = time.perf_counter()
                status = t.align_arrays(ps)[0]
                wall = time.perf_counter() - t0
                ms = ca.profile_get("mosaic", lib)[0] - ms0
                assert (status == _native.LDBG_OK).all()
                print("targets=%d device n=%d repeat=%d device_ms=%.2f cells_per_s=%.3e wall_s=%.3f" % (nt, n, rep, ms, n * cells_each / (ms / 1e3), wall), flush=True)


if __name__ == "__main__":
    main()
