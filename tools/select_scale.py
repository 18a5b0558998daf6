"""FindROIs at the bench's size: the device selection (ldbg_graph_select + the pack of ldbg_selection_open_graph) against the only
route there was before it — ldbg_graph_records of all N records into host memory, then the predicate in numpy.

The graph is bench.py's own (23.3 Mb, 3 colours, k = 47; colour 0 = the child = the traversal colour).  Prints the kernel times from
the profile families "select" and "select_pack" (median of --launches after --warmup), the achieved GB/s against the byte model of
DESIGN.md §11 (12 B per record read from the three coverage planes, 4 B per selected index and 8W + 5 B per packed record written)
and the fraction of the 8 TB/s HBM peak; then the wall time of both routes and whether they agree."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libldbg: torch's HIP runtime initialises first)

import bench  # noqa: E402
import corticall_amd as ca  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=bench.GENOME_LEN)
    ap.add_argument("--k", type=int, default=bench.K)
    ap.add_argument("--seeds", type=int, default=bench.N_SEEDS)
    ap.add_argument("--repeat-families", type=int, default=4000)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    prefix, _ = bench.workload_files(args, 0)
    g = ca.CortexGraph(prefix + ".ctx")
    N, W, C = g.getNumRecords(), g.getKmerBits(), g.getNumColors()
    child, parents = 0, [1, 2]
    print("graph %s: %d records, W %d, %d colours; %s" % (prefix + ".ctx", N, W, C, ca.default_lib().dll.ldbg_version().decode()))

    sel_ms, pack_ms, wall = [], [], []
    n_sel = 0
    for i in range(args.warmup + args.launches):
        ca.profile_reset()
        t = time.time()
        with g.select(all_positive=[child], all_zero=parents) as sel:
            n_sel = sel.count
            roi = sel.graph([child])
        dt = time.time() - t
        roi.close()
        if i >= args.warmup:
            sel_ms.append(ca.profile_get("select")[0])
            pack_ms.append(ca.profile_get("select_pack")[0])
            wall.append(dt)
    s_ms, p_ms = statistics.median(sel_ms), statistics.median(pack_ms)
    sel_bytes = 12 * N + 4 * n_sel                       # three coverage planes in, the indices out
    pack_bytes = (8 * W + 5) * n_sel
    for name, ms, nbytes in (("select", s_ms, sel_bytes), ("select_pack", p_ms, pack_bytes), ("both", s_ms + p_ms, sel_bytes + pack_bytes)):
        gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        print("%-12s median %.4f ms over %d launches (min %.4f, max %.4f)  byte model %.1f MB  %.1f GB/s  %.2f %% of %.0f GB/s"
              % (name, ms, args.launches, min(sel_ms if name == "select" else pack_ms if name == "select_pack" else [a + b for a, b in zip(sel_ms, pack_ms)]),
                 max(sel_ms if name == "select" else pack_ms if name == "select_pack" else [a + b for a, b in zip(sel_ms, pack_ms)]),
                 nbytes / 1e6, gbs, 100.0 * gbs / bench.HBM_PEAK_GBS, bench.HBM_PEAK_GBS))
    print("device route, wall (select + resident ROI graph of %d records, opened and closed): median %.2f ms" % (n_sel, statistics.median(wall) * 1e3))
    with g.select(all_positive=[child], all_zero=parents) as sel:
        t = time.time()
        dev_idx = sel.indices()
        t_idx = time.time() - t

    # the route of the parent commit: every record over the bus, the predicate on the host
    host = []
    for _ in range(3):
        t = time.time()
        _, cov, _ = g.records(0, N)
        t_fetch = time.time() - t
        v = np.asarray(cov)
        host_idx = np.nonzero((v[:, child] > 0) & (v[:, parents[0]] == 0) & (v[:, parents[1]] == 0))[0]
        host.append((time.time() - t, t_fetch))
    h_all, h_fetch = sorted(host)[1]
    same = len(host_idx) == len(dev_idx) and bool((host_idx == dev_idx).all())
    d_wall = statistics.median(wall) + t_idx
    print("host route: ldbg_graph_records of %d records (%d B each) %.1f ms + numpy predicate %.1f ms = %.1f ms (median of 3)"
          % (N, 8 * W + 5 * C, h_fetch * 1e3, (h_all - h_fetch) * 1e3, h_all * 1e3))
    print("device route incl. the download of the %d indices: %.2f ms; kernels alone %.4f ms" % (n_sel, d_wall * 1e3, s_ms + p_ms))
    print("same indices: %s; host / device wall %.1fx; host wall / device kernels %.0fx" % (same, h_all / d_wall, h_all * 1e3 / (s_ms + p_ms)))
    g.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
