"""Contigs threaded through a graph at a size where the per-call costs no longer hide the per-window ones: ldbg_graph_thread (DESIGN.md
§15) against the only route there was before it — every contig cut into its k-mer strings on the host, n x k ASCII bytes handed to
ldbg_graph_find_ascii once for the graph and once for the ROI graph, the per-contig values left to the caller.

The input is made here: a random genome (--genome-len), its graph built on the device (one colour, k = --k), a ROI graph of the
k-mers of random stretches that cover about a tenth of it, and --contigs substrings of --contig-len bases as the contigs.  Prints the
wall time and the HIP-event time of the threading kernels without and with copy indices, the wall time of the host-cut route, whether
both routes name the same records, and the bytes either route sends over the bus."""
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
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=47)
    ap.add_argument("--contigs", type=int, default=2000)
    ap.add_argument("--contig-len", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=7)
    args = ap.parse_args()
    rng = np.random.default_rng(15)
    k = args.k
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=args.genome_len)].tobytes()
    lib = ca.default_lib()
    g = ca.CortexGraph.build([("s", [genome])], k)
    stretches = [genome[p:p + 200] for p in rng.integers(0, args.genome_len - 200, size=args.genome_len // 2000)]
    roi = ca.CortexGraph.build([("s", stretches)], k)
    starts = rng.integers(0, args.genome_len - args.contig_len, size=args.contigs)
    contigs = [genome[p:p + args.contig_len] for p in starts]
    n_win = args.contigs * (args.contig_len - k + 1)
    print("graph %d records, ROI graph %d records, k %d; %d contigs of %d bases, %d windows; %s"
          % (g.getNumRecords(), roi.getNumRecords(), k, args.contigs, args.contig_len, n_win, lib.dll.ldbg_version().decode()))

    for name, copy in (("without copy indices (one sort: distinct ROI k-mers)", False), ("with copy indices (two sorts)", True)):
        wall, dev = [], []
        for _ in range(args.launches):
            t = time.time()
            with g.thread(contigs, rois=roi, copy_index=copy) as th:
                rec, info, _ = th.windows()
                sm = th.summary()
            wall.append(time.time() - t)
            dev.append(th.device_ms)
        print("ldbg_graph_thread %s: wall median %.1f ms (min %.1f), kernels median %.2f ms; %d hits, %d distinct, %d regions"
              % (name, statistics.median(wall) * 1e3, min(wall) * 1e3, statistics.median(dev), int(sm["n_hits"].sum()), int(sm["n_distinct"].sum()), th.n_regions))

    host = []
    for _ in range(3):
        t = time.time()
        cut = np.ascontiguousarray(np.concatenate([np.lib.stride_tricks.sliding_window_view(np.frombuffer(c, dtype=np.uint8), k) for c in contigs]))
        t_cut = time.time() - t
        gi, _, _ = g.find_batch(cut, with_payload=False)
        ri, _, _ = roi.find_batch(cut, with_payload=False)
        host.append((time.time() - t, t_cut))
    h_all, h_cut = sorted(host)[1]
    same = bool((gi == rec).all()) and bool(((ri >= 0) == ((info & 8) != 0)).all())
    print("host-cut route: %d x %d ASCII bytes cut in %.1f ms, two ldbg_graph_find_ascii batches: %.1f ms in all (median of 3); records and ROI membership the same: %s"
          % (n_win, k, h_cut * 1e3, h_all * 1e3, same))
    print("bytes over the bus, host to device: threading %.1f MB (the text and the offsets), host-cut route %.1f MB (twice n x k)"
          % ((args.contigs * args.contig_len + 8 * (args.contigs + 1)) / 1e6, 2.0 * n_win * k / 1e6))
    roi.close()
    g.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
