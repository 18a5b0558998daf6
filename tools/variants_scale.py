"""callVariant of n seeds (ldbg_engine_variant_batch) against what a caller could do before it existed.

The input is made here: a random parent of --genome-len bases, a second parent with one substitution every ~500 bases, a child made of
alternating halves of the two, their three-colour graph built on the device (k = --k).  The seeds are the child's records the first
parent does not have (selected on the device), so the stop colour is the first parent's.

  --route host    three assemble_batch_arrays calls chained on the host (backwards and forwards on the child's engine until a vertex the
                  parent covers, then the parent's engine from source to destination), the three results downloaded, the contigs, the
                  coverage sums and trimToAlleles in numpy.  Needs nothing of the variant batch: it runs on a library built from the commit
                  before it (LDBG_DIAG_LIB=variantNAME picks corticall_amd/_build_variantNAME/libldbg.so).
  --route device  one variant_batch.

Per size and repeat: wall time, kernel time of the "cursor" and "variants" families, bytes that cross the bus in each direction, and a
digest of (status, st, s0end, s1end, sums, alleles) of every seed.  The seeds of a size are the same on both routes (one seeded
generator), so the routes agree when their lines "n=... digest ..." carry the same digest: each route runs in a process of its own, and
`grep -o "n=[0-9]* .*digest.*" LOG | sed "s/repeat.*digest//" | sort -u` over a log of both leaves one line per size when they do."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libldbg: torch's HIP runtime initialises first)

from corticall_amd import _native  # noqa: E402


def genomes(rng, n):
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = rng.integers(0, 4, size=n)
    p1 = bases[code]
    at = np.arange(250, n - 250, 500) + rng.integers(-100, 100, size=len(range(250, n - 250, 500)))
    code2 = code.copy()
    code2[at] = (code2[at] + rng.integers(1, 4, size=len(at))) % 4
    p2 = bases[code2]
    kid = np.concatenate([p1[:n // 2], p2[n // 2:]])
    return p1.tobytes(), p2.tobytes(), kid.tobytes()


def _kmer_ascii(words, k):
    """packed k-mers u64[n, W] -> their text as u8[n, k]"""
    n, W = words.shape
    out = np.empty((n, k), dtype=np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    for p in range(k):
        off = 2 * (k - 1 - p)
        out[:, p] = bases[((words[:, W - 1 - off // 64] >> np.uint64(off % 64)) & np.uint64(3)).astype(np.int64)]
    return out


def digest(status, st, e0, e1, csum, psum, alleles):
    h = hashlib.sha1()
    for a in (status, st, e0, e1, csum, psum):
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
    h.update(alleles)
    return h.hexdigest()[:16]


def host_route(ec, ep, g, seeds, cov, k):
    """-> (digest, bytes up, bytes down)"""
    from corticall_amd import FORWARD, REVERSE
    n = seeds.shape[0]
    rv = ec.assemble_batch_arrays(seeds, REVERSE, until_colour=1)
    fw = ec.assemble_batch_arrays(seeds, FORWARD, until_colour=1)
    both = (rv["end_reverse"] == 2) & (fw["end_forward"] == 2) & (rv["status"] == 0) & (fw["status"] == 0)
    src = np.full((n, k), ord("N"), dtype=np.uint8)
    dst = np.full((n, k), ord("N"), dtype=np.uint8)
    ok = np.nonzero(both)[0]
    src[ok] = _kmer_ascii(rv["words"][rv["offsets"][ok]], k)
    dst[ok] = _kmer_ascii(fw["words"][fw["offsets"][ok + 1] - 1], k)
    pa = ep.assemble_batch_arrays(src, FORWARD, targets=dst)
    up = 4 * n * k
    down = sum(a.nbytes for r in (rv, fw, pa) for a in r.values())
    W = rv["words"].shape[1]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    last = [bases[(r["words"][:, W - 1] & np.uint64(3)).astype(np.int64)] for r in (rv, fw, pa)]
    seed_rec = fw["seed_rec"]
    status = np.zeros(n, dtype=np.int64); st = np.zeros(n, dtype=np.int64); e0 = np.zeros(n, dtype=np.int64); e1 = np.zeros(n, dtype=np.int64)
    csum = np.zeros(n, dtype=np.int64); psum = np.zeros(n, dtype=np.int64)
    alleles = []
    for i in range(n):
        if rv["status"][i] or fw["status"][i]:
            status[i] = 4 if 1 in (rv["status"][i], fw["status"][i]) else 5
        elif rv["end_reverse"][i] == 1 or fw["end_forward"][i] == 1:
            status[i] = 6
        elif rv["end_reverse"][i] != 2:
            status[i] = 1
        elif fw["end_forward"][i] != 2:
            status[i] = 2
        elif pa["status"][i]:
            status[i] = 4 if pa["status"][i] == 1 else 5
        elif pa["end_forward"][i] == 1:
            status[i] = 6
        elif pa["end_forward"][i] != 2:
            status[i] = 3
        if status[i]:
            continue
        r0, r1, f0, f1, p0, p1 = rv["offsets"][i], rv["offsets"][i + 1], fw["offsets"][i], fw["offsets"][i + 1], pa["offsets"][i], pa["offsets"][i + 1]
        s0 = np.concatenate([src[i], last[0][r0 + 1:r1], seeds[i][-1:], last[1][f0:f1]])
        s1 = np.concatenate([src[i], last[2][p0:p1]])
        crec = np.concatenate([rv["rec"][r0:r1], seed_rec[i:i + 1], fw["rec"][f0:f1]])
        prec = np.concatenate([rv["rec"][r0:r0 + 1], pa["rec"][p0:p1]])
        csum[i], psum[i] = cov[crec, 0].sum(dtype=np.int64), cov[prec, 1].sum(dtype=np.int64)
        m = min(len(s0), len(s1))
        ne = np.nonzero(s0[:m] != s1[:m])[0]
        a = int(ne[0]) if len(ne) else 0
        stop = (s0[::-1][:m] != s1[::-1][:m])
        if a > 0:
            q = np.arange(m)
            stop |= (len(s0) - 1 - q == a - 1) | (len(s1) - 1 - q == a - 1)
        hit = np.nonzero(stop)[0]
        b0, b1 = (len(s0) - int(hit[0]), len(s1) - int(hit[0])) if len(hit) else (len(s0), len(s1))
        st[i], e0[i], e1[i] = a, b0, b1
        alleles.append(s0[a:b0].tobytes() + s1[a:b1].tobytes())
    return digest(status, st, e0, e1, csum, psum, b"".join(alleles)), up, down


def device_route(ec, ep, seeds, k):
    r = ec.variant_batch(ep, seeds, 1, (0,))
    down = sum(a.nbytes for a in r.values() if isinstance(a, np.ndarray) and a is not r["type"])
    return digest(r["status"], r["st"], r["s0end"], r["s1end"], r["child_sum"][:, 0], r["parent_sum"], r["alleles"].tobytes()), seeds.shape[0] * k, down


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["host", "device"], required=True)
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=47)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 4096, 50000])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.route == "host":      # a library from before the variant batch does not export it
        _native.EXPORTS = [e for e in _native.EXPORTS if "variant_batch" not in e and "variant_result" not in e]
    import corticall_amd as ca
    from corticall_amd.traversal import profile_get, profile_reset
    rng = np.random.default_rng(18)
    k = args.k
    p1, p2, kid = genomes(rng, args.genome_len)
    lib = ca.default_lib()
    g = ca.CortexGraph.build([("kid", [kid]), ("mom", [p1]), ("dad", [p2])], k)
    with g.select(all_positive=(0,), all_zero=(1,)) as sel:
        idx = np.asarray(sel.indices(), dtype=np.int64)
    words, cov, _ = g.records(0, g.getNumRecords())
    every = _kmer_ascii(words[idx], k)
    make = lambda c: ca.TraversalEngineFactory(lib=lib).traversalColors(c).graph(g).stoppingRule(ca.ContigStopper).make()
    ec, ep = make(0), make(1)
    print("route %s: graph %d records, k %d, %d child-specific seeds; %s" % (args.route, g.getNumRecords(), k, len(idx), lib.dll.ldbg_version().decode()))
    for n in args.sizes:
        pick = rng.permutation(len(idx))[:n] if n <= len(idx) else rng.integers(0, len(idx), size=n)
        seeds = np.ascontiguousarray(every[np.sort(pick)])
        run = (lambda: host_route(ec, ep, g, seeds, cov, k)) if args.route == "host" else (lambda: device_route(ec, ep, seeds, k))
        run()                                            # warm: code objects loaded, pools made at this size
        for rep in range(args.repeats):
            profile_reset(lib)
            t = time.time()
            dg, up, down = run()
            wall = time.time() - t
            print("%s n=%d repeat %d: %.1f ms wall; kernels: cursor %.1f ms, variants %.2f ms; bus: %d bytes up, %d bytes down; digest %s"
                  % (args.route, n, rep, wall * 1e3, profile_get("cursor", lib)[0], profile_get("variants", lib)[0], up, down, dg))
            sys.stdout.flush()
    ec.close(); ep.close(); g.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
