"""Cursors advanced in batches (ldbg_engine_cursor_batch) against the only route there was before: one
ldbg_engine_assemble call per seed, each of which seeks twice and launches two kernels in which one thread works.

The input is made here, as tools/thread_scale.py makes it: a random genome (--genome-len), its graph built on the device (one colour,
k = --k).  The seeds are k-mers of the genome at random places; every cursor runs --max-len vertices in each direction at the most
(maxBranchLength), which on a random genome it does unless it meets an end of the genome first.  Prints
  (a) the wall time of n = 64 ldbg_engine_assemble calls, as C calls and through assemble() (which builds a vertex object per vertex),
  (b) the wall time of one batch of the same 64 seeds, as arrays and through assemble_batch(), and whether both name the same vertices,
  (c) one batch of 4,096 and of 50,000 seeds: wall time, the kernel time of the "cursor" family, k-mers stepped per second (of the
      result; the count pass steps every cursor a second time), the longest cursor's step count."""
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
from corticall_amd.traversal import profile_get, profile_reset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=47)
    ap.add_argument("--max-len", type=int, default=5000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 50000])
    args = ap.parse_args()
    rng = np.random.default_rng(16)
    k = args.k
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=args.genome_len)].tobytes()
    lib = ca.default_lib()
    g = ca.CortexGraph.build([("s", [genome])], k)
    e = ca.TraversalEngineFactory(lib=lib).traversalColors(0).graph(g).maxBranchLength(args.max_len).stoppingRule(ca.ContigStopper).make()
    print("graph %d records, k %d, maxBranchLength %d; %s" % (g.getNumRecords(), k, args.max_len, lib.dll.ldbg_version().decode()))

    def seeds_of(n):
        return [genome[p:p + k] for p in rng.integers(0, args.genome_len - k, size=n)]

    flat = lambda vs: [(v.getKmerAsString(), v.getCortexRecord().index if v.getCortexRecord() is not None else -1) for v in vs]
    seeds = seeds_of(64)
    e.assemble(seeds[0]); e.assemble_batch_arrays(seeds[:2])          # both routes warm (code objects loaded, pools made)
    # the C calls alone (no vertex objects on either side): what a host pays at the ABI
    cap = 2 * args.max_len + 1
    words, rec, ln = np.zeros((cap, g.getKmerBits()), dtype=np.uint64), np.zeros(cap, dtype=np.int64), C.c_int64()
    t = time.time()
    for s in seeds:
        lib.check(lib.dll.ldbg_engine_assemble(e._h, s, C.c_int64(cap), C.byref(ln), words.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)))
    t_a_raw = time.time() - t
    t = time.time()
    one = [e.assemble(s) for s in seeds]
    t_a = time.time() - t
    t = time.time()
    many = e.assemble_batch(seeds)
    t_b = time.time() - t
    t = time.time()
    e.assemble_batch_arrays(seeds)
    t_b2 = time.time() - t
    same = [flat(v) for v in one] == [flat(v) for v in many]
    nv = sum(len(v) for v in one)
    print("(a) 64 ldbg_engine_assemble calls: %.1f ms wall as C calls, %.1f ms through assemble() with vertex objects; %d vertices" % (t_a_raw * 1e3, t_a * 1e3, nv))
    print("(b) one batch of the same 64 seeds: %.1f ms wall as arrays, %.1f ms through assemble_batch() with vertex objects; the same vertices: %s; "
          "(a) / (b) = %.1f as C calls and arrays, %.2f with vertex objects" % (t_b2 * 1e3, t_b * 1e3, same, t_a_raw / t_b2, t_a / t_b))
    for n in args.sizes:
        sd = np.frombuffer(b"".join(seeds_of(n)), dtype=np.uint8).reshape(n, k)
        profile_reset(lib)
        t = time.time()
        r = e.assemble_batch_arrays(sd)
        wall = time.time() - t
        ms, _ = profile_get("cursor", lib)
        longest, _ = profile_get("cursor_longest", lib)
        steps, _ = profile_get("cursor_steps", lib)
        print("(c) one batch of %d seeds: %.1f ms wall, kernels %.1f ms; %d steps in the result (%d vertices), %.1f M k-mers stepped per second of "
              "kernel time; the longest cursor: %d steps; statuses ok: %s"
              % (n, wall * 1e3, ms, int(steps), int(r["offsets"][-1]), steps / max(ms, 1e-9) / 1e3, int(longest), bool((r["status"] == 0).all())))
    e.close()
    g.close()
    return 0 if (same and t_b < t_a and t_b2 < t_a_raw) else 1


if __name__ == "__main__":
    sys.exit(main())
