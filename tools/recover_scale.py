"""RecoverExcludedKmers at the bench's size: ldbg_graph_recover against the only route there was before it —
ldbg_graph_records of all N records into host memory, one ldbg_graph_find batch of the candidates' k-mers into DIRTY, the loop in numpy.

GRAPH is bench.py's own graph (23.3 Mb, 3 colours, k = 47; colour 0 = the child).  DIRTY is made from it: every record the child
covers plus every record only a parent covers, one colour under the child's name, coverage 1 — so every candidate is found and
recovered, the most lookups the graph can ask for.  Prints the HIP-event medians of the recover kernels (profile family "recover":
classify, the two scans, the candidate scatter and key gather, merge, the final scatter), of the findRecord launch into DIRTY ("find")
and of the pack ("select_pack"), the achieved GB/s against the byte model of §14 and the fraction of the 8 TB/s HBM peak; then the wall
time of both routes and whether the two files hold the same bytes."""
import argparse
import ctypes as C
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libldbg: torch's HIP runtime initialises first)

import bench  # noqa: E402
import corticall_amd as ca  # noqa: E402
from corticall_amd.distributed import ctx_header  # noqa: E402
from corticall_amd.prefilter import Selection  # noqa: E402

LOOKUP_BYTES = 64 + 2 * 64        # the model of one findRecord: a line of the radix index, two probe rows of DIRTY (64 B each at W = 2, C = 1)


def fresh_header(k, W, name):
    """CortexGraphWriter.initialize for one colour with an empty block"""
    n = name.encode()
    return (b"CORTEX" + struct.pack("<IIII", 6, k, W, 1) + struct.pack("<I", 0) + struct.pack("<Q", 0) + struct.pack("<I", len(n)) + n
            + bytes([0, 0xd8, 0xa3, 0x70, 0x3d, 0x0a, 0xd7, 0xa3, 0xf8, 0x3f, 0, 0, 0, 0, 0, 0]) + bytes(16) + b"CORTEX")


def record_bytes(words, cov0, edges0):
    n = words.shape[0]
    return np.concatenate([np.ascontiguousarray(words, dtype="<u8").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(cov0, dtype="<u4").view(np.uint8).reshape(n, 4),
                           np.ascontiguousarray(edges0, dtype=np.uint8).reshape(n, 1)], axis=1)


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
    lib = ca.default_lib()
    g = ca.CortexGraph(prefix + ".ctx")
    N, W, Cn, k = g.getNumRecords(), g.getKmerBits(), g.getNumColors(), g.getKmerSize()
    child = 0
    print("graph %s: %d records, W %d, %d colours; %s" % (prefix + ".ctx", N, W, Cn, lib.dll.ldbg_version().decode()))

    words, cov, edges = g.records(0, N)
    cov = np.asarray(cov).view(np.int32)                    # CortexRecord.getCoverage: the Java int
    in_dirty = (cov > 0).any(axis=1)
    dpath = prefix + ".recover_dirty.ctx"
    with open(dpath, "wb") as f:
        f.write(fresh_header(k, W, g.getSampleName(child)))
        f.write(record_bytes(words[in_dirty], np.ones(int(in_dirty.sum()), dtype=np.uint32), edges[in_dirty][:, child]).tobytes())
    dirty = ca.CortexGraph(dpath)
    print("dirty %s: %d records, 1 colour" % (dpath, dirty.getNumRecords()))

    rec_ms, find_ms, wall = [], [], []
    for i in range(args.warmup + args.launches):
        ca.profile_reset()
        t = time.time()
        sel, n_rec = Selection.recover(g, child, dirty)
        dt = time.time() - t
        n_sel = sel.count
        sel.close()
        if i >= args.warmup:
            rec_ms.append(ca.profile_get("recover")[0])
            find_ms.append(ca.profile_get("find")[0])
            wall.append(dt)
    n_cand = n_rec                                          # every candidate is in DIRTY with coverage 1
    # the C planes once; the two ballot arrays, written three times and read five (N / 8 bytes each); index, coverage column and the child's
    # plane again per written record; per candidate its number (written, read), its k-mer (gathered, written) and DIRTY's coverage (read twice)
    scan_bytes = 4 * Cn * N + N + 12 * n_sel + n_cand * (8 + 16 * W + 8)
    lookup_bytes = n_cand * (8 * W + LOOKUP_BYTES + 8 + 4)
    r_ms, f_ms = statistics.median(rec_ms), statistics.median(find_ms)
    both = [a + b for a, b in zip(rec_ms, find_ms)]
    for name, ms, xs, nbytes in (("recover", r_ms, rec_ms, scan_bytes), ("find (DIRTY)", f_ms, find_ms, lookup_bytes),
                                 ("both", statistics.median(both), both, scan_bytes + lookup_bytes)):
        gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        print("%-12s median %.4f ms over %d launches (min %.4f, max %.4f)  byte model %.1f MB  %.1f GB/s  %.2f %% of %.0f GB/s"
              % (name, ms, args.launches, min(xs), max(xs), nbytes / 1e6, gbs, 100.0 * gbs / bench.HBM_PEAK_GBS, bench.HBM_PEAK_GBS))
    print("ldbg_graph_recover, wall: median %.2f ms; %d records written, %d of them recovered (= candidates looked up)"
          % (statistics.median(wall) * 1e3, n_sel, n_rec))

    out_dev = prefix + ".recovered_dev.ctx"
    ca.profile_reset()
    t = time.time()
    sel, n_rec = Selection.recover(g, child, dirty)
    sel.write_recovered(out_dev)
    sel.close()
    d_all = time.time() - t
    print("device route incl. packing (%.4f ms of kernels) and writing the %.0f MB file: %.1f ms"
          % (ca.profile_get("select_pack")[0], os.path.getsize(out_dev) / 1e6, d_all * 1e3))

    # the route of the parent commit: every record over the bus, one find batch into DIRTY, the loop on the host
    host = []
    for _ in range(3):
        t = time.time()
        w, c, e = g.records(0, N)
        t_fetch = time.time() - t
        c = np.asarray(c).view(np.int32)
        kept = c[:, child] > 0
        cand = np.nonzero(~kept & (np.delete(c, child, axis=1) > 0).any(axis=1))[0]
        q = np.ascontiguousarray(w[cand])
        idx = np.empty(len(cand), dtype=np.int64)
        dcov = np.zeros((max(len(cand), 1), 1), dtype=np.uint32)
        t1 = time.time()
        lib.check(lib.dll.ldbg_graph_find(dirty._h, q.ctypes.data_as(C.c_void_p), C.c_int64(len(cand)), idx.ctypes.data_as(C.c_void_p),
                                          dcov.ctypes.data_as(C.c_void_p), None))
        t_find = time.time() - t1
        got = (idx >= 0) & (dcov[:len(cand), 0].view(np.int32) > 0)
        c0 = c[:, 0].copy()
        if child == 0:
            c0[cand[got]] = dcov[:len(cand), 0].view(np.int32)[got]
        keep = kept.copy()
        keep[cand[got]] = True
        body = record_bytes(w[keep], c0[keep].view(np.uint32), e[keep][:, 0])
        host.append((time.time() - t, t_fetch, t_find, int(got.sum())))
    h_all, h_fetch, h_find, h_rec = sorted(host)[1]
    raw = np.fromfile(out_dev, dtype=np.uint8)
    off = ctx_header(raw[:1 << 20])["data_offset"]
    same = h_rec == n_rec and raw.size - off == body.size and bool((raw[off:] == body.reshape(-1)).all())
    print("host route (the file is not written): ldbg_graph_records of %d records (%d B each) %.1f ms + ldbg_graph_find of %d k-mers %.1f ms + numpy loop %.1f ms = %.1f ms (median of 3)"
          % (N, 8 * W + 5 * Cn, h_fetch * 1e3, len(cand), h_find * 1e3, (h_all - h_fetch - h_find) * 1e3, h_all * 1e3))
    print("same records in the file (%d bytes after a %d-byte header): %s; host / device wall %.1fx; host wall / device kernels %.0fx"
          % (raw.size - off, off, same, h_all / d_all, h_all * 1e3 / (r_ms + f_ms)))
    dirty.close()
    g.close()
    for p in (dpath, out_dev):
        os.remove(p)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
