"""The variant seeds and the occurrence table (ldbg_graph_variant_seeds, ldbg_threading_occurrences) at a size where
per-call costs no longer hide per-record ones: an SNV family of about --genome-len records.

The input is made here: a random parent, a child with one substitution every 97 bases, their two-colour graph built on the device
(colour 0 the child, k = --k).  The child is threaded through the graph, its occurrences counted, and the seeds taken with
ComputeAssemblyQuality's filter.  Prints the HIP-event times of the occurrence kernel and of the seed pass, the three counts and what
the family predicts for them (m substitutions: m k records in S, 2 m starts, 2 m good seeds)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libldbg: torch's HIP runtime initialises first)

import corticall_amd as ca  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--launches", type=int, default=7)
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    k, L = args.k, args.genome_len
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = rng.integers(0, 4, size=L)
    sites = np.arange(100, L - 100, 97)
    child = codes.copy()
    child[sites] = (codes[sites] + rng.integers(1, 4, size=len(sites))) % 4
    parent, child = alphabet[codes].tobytes(), alphabet[child].tobytes()
    lib = ca.default_lib()
    g = ca.CortexGraph.build([("child", [child]), ("parent", [parent])], k)
    m = len(sites)
    print("graph %d records, 2 colours, k %d; %d substitutions; %s" % (g.getNumRecords(), k, m, lib.dll.ldbg_version().decode()))
    occ_ms, seed_ms, wall = [], [], []
    counts = None
    for _ in range(args.launches):
        with g.thread([child]) as th:
            t = time.time()
            with th.occurrences() as occ:
                occ_ms.append(occ.device_ms)
                with g.variant_seeds(all_zero=(1,), covered=[((0,), 1, 1)], unique=[(-1, occ)]) as sel:
                    wall.append(time.time() - t)
                    seed_ms.append(sel.device_ms)
                    got = (sel.n_seeds, sel.n_unique, sel.n_good)
                    assert counts in (None, got), (counts, got)
                    counts = got
    print("ldbg_threading_occurrences over %d windows: kernel median %.3f ms (min %.3f)" % (th.n_windows, statistics.median(occ_ms), min(occ_ms)))
    print("ldbg_graph_variant_seeds: kernels median %.3f ms (min %.3f); both calls, wall median %.1f ms" % (statistics.median(seed_ms), min(seed_ms), statistics.median(wall) * 1e3))
    print("seeds %d (m k = %d), starts %d (2 m = %d), good %d" % (counts[0], m * k, counts[1], 2 * m, counts[2]))
    g.close()
    return 0 if counts[2] > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
