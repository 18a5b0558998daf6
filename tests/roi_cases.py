"""Record selection cases (ldbg_graph_select, DESIGN.md §11: FindROIs, FindLowCoverage, FindDust, FindShared, Remove) shared by the
host-simulation run (tests/test_roi_hostsim.py) and the GPU run (tests/test_gpu_roi.py).

Nothing expected here comes from the code under test: every input .ctx is parsed with numpy (header, 8W + 5C-byte records), the
reference's predicate is applied in Python on the Java int view of the coverages, and the expected file is built here — the kept
header through ldbg_ctx_write_records (CortexGraphWriter over chosen records, present before the selection existed) or a Python
restatement of the writer (parity_cases.java_write_header, CortexGraphWriter.java:36-98), the records by slicing."""
import ctypes as C
import os
import random
import struct

import numpy as np

import corticall_amd as ca
from corticall_amd import (CortexGraph, FindDust, FindLowCoverage, FindROIs, FindShared, Partition, Remove, TraversalEngineFactory,
                           ContigStopper, BOTH, OR)
from corticall_amd.partition import unpack_kmers
from tests.parity_cases import genome_with_repeats, java_read_header, java_rewritten_header, java_write_header, mutate, rand_seq

CHUNK = 4096                    # select.h: LDBG_SELECT_CHUNK, the records one entry of the scanned counts covers
TOP = 64 * CHUNK                # the records one step of the scan over those counts covers (64 lanes)
NEG = 0x80000000                # a stored coverage the reference reads as Integer.MIN_VALUE
COV_VALUES = np.array([0, 1, 0x7FFFFFFF, NEG, 0xFFFFFFFF], dtype=np.uint32)


# ---------------------------------------------------------------- .ctx files with numpy
def fresh_col(name):
    return dict(mrl=0, tot=0, name=name.encode() if isinstance(name, str) else name, flags=b"\0\0\0\0", t1=0, t2=0, cleaned=b"")


def header_len(raw):
    """offset of the first record"""
    C_ = struct.unpack_from("<I", raw, 18)[0]
    p = 22 + 12 * C_
    for _ in range(C_):
        p += 4 + struct.unpack_from("<I", raw, p)[0]
    p += 16 * C_
    for _ in range(C_):
        p += 16 + struct.unpack_from("<I", raw, p + 12)[0]
    assert raw[p:p + 6] == b"CORTEX"
    return p + 6


def read_ctx(path):
    """-> dict(k, W, C, names, header (bytes), words u64[N, W], cov u32[N, C], edges u8[N, C])"""
    raw = open(path, "rb").read()
    k, W, cols = java_read_header(raw)
    C_ = len(cols)
    h = header_len(raw)
    R = 8 * W + 5 * C_
    assert (len(raw) - h) % R == 0
    rec = np.frombuffer(raw, dtype=np.uint8, offset=h).reshape(-1, R)
    N = rec.shape[0]
    words = np.ascontiguousarray(rec[:, :8 * W]).view("<u8").reshape(N, W)
    cov = np.ascontiguousarray(rec[:, 8 * W:8 * W + 4 * C_]).view("<u4").reshape(N, C_)
    edges = np.ascontiguousarray(rec[:, 8 * W + 4 * C_:]).reshape(N, C_)
    return dict(k=k, W=W, C=C_, N=N, names=[c["name"] for c in cols], header=raw[:h], words=words, cov=cov, edges=edges)


def record_bytes(words, cov, edges):
    """CortexGraphWriter.addRecord (:115-138) of every row: the k-mer words, the coverages (LE), the edges"""
    n = words.shape[0]
    if n == 0:
        return b""
    return np.concatenate([np.ascontiguousarray(words, dtype="<u8").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(cov, dtype="<u4").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(edges, dtype=np.uint8).reshape(n, -1)], axis=1).tobytes()


def write_ctx(path, k, names, words, cov, edges, header=None):
    W = (k + 31) // 32
    hdr = header if header is not None else java_write_header(k, W, [fresh_col(n) for n in names])
    with open(path, "wb") as f:
        f.write(hdr + record_bytes(words, cov, edges))
    return str(path)


def random_keys(rng, n, k):
    """n distinct k-mers as packed words u64[n, W], ascending"""
    W = (k + 31) // 32
    top = 2 * k - 64 * (W - 1)
    seen = {}
    while len(seen) < n:
        w = rng.integers(0, 1 << 62, size=(2 * (n - len(seen)) + 8, W), dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, size=(2 * (n - len(seen)) + 8, W), dtype=np.uint64)
        if top < 64:
            w[:, 0] &= np.uint64((1 << top) - 1)
        for row in w:
            seen.setdefault(tuple(int(x) for x in row), None)
            if len(seen) == n:
                break
    keys = np.array(sorted(seen), dtype=np.uint64).reshape(n, W)
    return keys


def sequential_keys(n, k):
    """n ascending one-word k-mers, cheap at any n"""
    assert k <= 32 and n < (1 << (2 * k - 1))
    return (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)).reshape(n, 1)


# ---------------------------------------------------------------- the reference's predicate
def java_cov(cov):
    return np.asarray(cov, dtype=np.uint32).view(np.int32)


def ref_pass(cov, edges, all_zero=(), all_positive=(), any_positive=(), none_positive=(), cov_below=None, degree_above=None):
    """the filter as the reference's loops state it, on CortexRecord.getCoverage's int and the edge byte's set bits"""
    v = java_cov(cov)
    ok = np.ones(v.shape[0], dtype=bool)
    for c in all_zero:
        ok &= v[:, c] == 0
    for c in all_positive:
        ok &= v[:, c] > 0
    if len(any_positive):
        ok &= (v[:, list(any_positive)] > 0).any(axis=1)
    for c in none_positive:
        ok &= ~(v[:, c] > 0)
    if cov_below is not None:
        ok &= v[:, cov_below[0]] < cov_below[1]
    if degree_above is not None:
        e = edges[:, degree_above[0]]
        deg = np.array([bin(int(x) >> 4).count("1") + bin(int(x) & 0xF).count("1") for x in range(256)])[e]     # getInDegree + getOutDegree
        ok &= deg > degree_above[1]
    return np.nonzero(ok)[0].astype(np.int64)


def fetch_dev(lib, sel, n):
    """ldbg_selection_indices_dev into device memory, copied back"""
    if lib.is_hostsim:                               # the simulation's device memory is host memory
        buf = np.full(max(n, 1), -7, dtype=np.int64)
        sel.indices_dev(buf.ctypes.data, 0, n)
        return buf[:n]
    import torch
    t = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sel.indices_dev(t.data_ptr(), 0, n)
    return t.cpu().numpy()[:n]


def check_select(lib, g, d, **flt):
    exp = ref_pass(d["cov"], d["edges"], **flt)
    with g.select(**flt) as sel:
        assert sel.count == len(exp), (flt, sel.count, len(exp))
        assert (sel.indices() == exp).all(), flt
        assert (fetch_dev(lib, sel, sel.count) == exp).all(), flt
        if len(exp) > 2:
            assert (sel.indices(1, len(exp) - 2) == exp[1:-1]).all()
    return exp


# ---------------------------------------------------------------- cases
SHAPE_SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, CHUNK + 1, 70001, TOP + 65]


def case_select_shapes(orc, lib, tmp, N):
    """table sizes around a ballot word, a chunk and a scan step; per colour a density: none, all, ~1 %, ~50 %, a cluster at the very
    start, a cluster at the very end"""
    rng = np.random.default_rng(N)
    cov = np.zeros((N, 6), dtype=np.uint32)
    cov[:, 1] = 1
    cov[:, 2] = rng.random(N) < 0.01
    cov[:, 3] = rng.random(N) < 0.5
    cov[:min(N, 70), 4] = 7
    cov[max(0, N - 70):, 5] = 9
    if N > 2:
        cov[N - 1, 2] = 1
    edges = np.zeros((N, 6), dtype=np.uint8)
    p = write_ctx(tmp / ("shape%d.ctx" % N), 21, ["c%d" % c for c in range(6)], sequential_keys(N, 21), cov, edges)
    d = read_ctx(p)
    g = CortexGraph(p, lib=lib)
    assert g.getNumRecords() == N
    for c in range(6):
        exp = check_select(lib, g, d, all_positive=[c])
        assert len(exp) == int((cov[:, c] > 0).sum())
    assert len(check_select(lib, g, d)) == N                      # the empty filter selects everything
    g.close()


CLAUSE_COLOURS = [1, 3, 5, 32]


def clause_graph(tmp, C_, n=1500, k=31, seed=0):
    rng = np.random.default_rng(1000 * C_ + seed)
    cov = COV_VALUES[rng.integers(0, len(COV_VALUES), size=(n, C_))]
    edges = rng.integers(0, 256, size=(n, C_), dtype=np.uint8)
    m = min(n, 256)
    edges[:m, 0] = np.arange(256)[:m]                               # every edge byte, so every degree 0..8
    edges[:m, C_ - 1] = np.arange(256)[::-1][:m]
    return write_ctx(tmp / ("clause%d_%d.ctx" % (C_, seed)), k, ["s%d" % c for c in range(C_)], random_keys(rng, n, k), cov, edges)


def case_filter_clauses(orc, lib, tmp, C_):
    p = clause_graph(tmp, C_)
    d = read_ctx(p)
    g = CortexGraph(p, lib=lib)
    top = C_ - 1                                                    # bit 31 of the masks with 32 colours
    mid = C_ // 2
    n = d["N"]
    singles = [dict(all_zero=[top]), dict(all_positive=[top]), dict(any_positive=[top]), dict(none_positive=[top]),
               dict(any_positive=sorted({0, top})), dict(all_zero=sorted({0, mid})), dict(all_positive=sorted({mid, top})),
               dict(none_positive=sorted({0, top}))]
    singles += [dict(cov_below=(top, m)) for m in (0, 1, 5, -(1 << 31))]
    singles += [dict(degree_above=(c, a)) for c in sorted({0, top}) for a in (0, 4, 7, 8)]
    for flt in singles:
        exp = check_select(lib, g, d, **flt)
        if flt.get("degree_above", (0, 0))[1] != 8 and flt.get("cov_below", (0, 0))[1] != -(1 << 31):
            assert 0 < len(exp) < n, (flt, len(exp))                # the clause separates the records
        else:
            assert len(exp) == 0                                    # no byte has 9 bits; nothing is below Integer.MIN_VALUE
    # a stored 0x80000000 is neither == 0 nor > 0, and is < MIN for any MIN
    neg = np.nonzero(d["cov"][:, top] == NEG)[0]
    assert len(neg) > 0
    for flt, inside in ((dict(all_zero=[top]), False), (dict(all_positive=[top]), False), (dict(cov_below=(top, -5)), True), (dict(none_positive=[top]), True)):
        with g.select(**flt) as sel:
            assert np.isin(neg, sel.indices()).all() == inside and np.isin(neg, sel.indices()).any() == inside, flt
    # all clauses together
    others = [c for c in range(C_) if c not in (0, top)]
    both = dict(all_zero=others[:1], all_positive=[top], any_positive=sorted({0, top}), none_positive=others[1:2], cov_below=(top, 5), degree_above=(0, 4))
    exp = check_select(lib, g, d, **both)
    assert len(exp) > 0
    assert len(check_select(lib, g, d)) == n
    g.close()


def sliced_file(d, idx, colours, header):
    return header + record_bytes(d["words"][idx], d["cov"][idx][:, colours], d["edges"][idx][:, colours])


def fresh_header(d, colours):
    return java_write_header(d["k"], d["W"], [fresh_col(d["names"][c]) for c in colours])


def compare_graph_with_slice(g, d, idx, colours):
    n = g.getNumRecords()
    assert n == len(idx) and g.getNumColors() == len(colours) and g.getKmerSize() == d["k"]
    if n:
        w, c, e = g.records(0, n)
        assert (w == d["words"][idx]).all() and (c.view(np.uint32) == d["cov"][idx][:, colours]).all() and (e == d["edges"][idx][:, colours]).all()
    for j, col in enumerate(colours):
        assert g.getSampleName(j).encode() == d["names"][col]


PACK_K = [21, 47, 65, 97]


def case_pack_layouts(orc, lib, tmp, k):
    rng = np.random.default_rng(k)
    n, C_ = 300, 3
    cov = rng.integers(0, 4, size=(n, C_)).astype(np.uint32) * np.uint32(0x40000001)
    edges = rng.integers(0, 256, size=(n, C_), dtype=np.uint8)
    p = write_ctx(tmp / ("pack%d.ctx" % k), k, ["a", "bb", "ccc"], random_keys(rng, n, k), cov, edges)
    d = read_ctx(p)
    assert d["W"] == (k + 31) // 32 == PACK_K.index(k) + 1
    g = CortexGraph(p, lib=lib)
    for flt in (dict(all_positive=[0]), dict(), dict(all_zero=[1], all_positive=[2])):
        exp = ref_pass(d["cov"], d["edges"], **flt)
        assert len(exp) > 64 or flt.get("all_zero")
        with g.select(**flt) as sel:
            for colours in ([1], [2, 0], [0, 1, 2]):
                out = tmp / ("pack%d_%s.ctx" % (k, "".join(map(str, colours))))
                sel.write_ctx(out, colours)
                assert out.read_bytes() == sliced_file(d, exp, colours, fresh_header(d, colours)), (k, flt, colours)
                ro = CortexGraph(out, lib=lib)                     # the packed file is a graph: ldbg_graph_open takes it
                compare_graph_with_slice(ro, d, exp, colours)
                ro.close()
                rg = sel.graph(colours)                            # and the same without the file
                compare_graph_with_slice(rg, d, exp, colours)
                rg.close()
            kept = tmp / ("pack%d_kept.ctx" % k)
            sel.write_ctx(kept, [0, 1, 2], header_path=p)
            want = tmp / ("pack%d_want.ctx" % k)
            lib.check(lib.dll.ldbg_ctx_write_records(p.encode(), exp.ctypes.data_as(C.c_void_p), C.c_int64(len(exp)), str(want).encode()))
            assert kept.read_bytes() == want.read_bytes()
    g.close()


def synth_trio(tmp, k=31):
    from tools import synth
    prefix = str(tmp / "trio")
    synth.generate(prefix, 30000, k, colours=3, with_links=False, seed=0xC0FFEE11, n_chrom=1, n_indels=5, n_dnm=6, n_tandem=1,
                   n_repeat_families=3, repeat_copies=2, repeat_len=(40, 80), n_seeds=10, threads=2)
    return prefix + ".ctx"


def check_find_rois(lib, tmp, path, child, parents, tag):
    d = read_ctx(path)
    g = CortexGraph(path, lib=lib)
    names = [n.decode() for n in d["names"]]
    v = java_cov(d["cov"])
    novel = v[:, child] > 0                                        # FindROIs.isNovel :72-82
    for c in parents:
        novel &= v[:, c] == 0
    exp = np.nonzero(novel)[0]
    out = tmp / ("roi_%s.ctx" % tag)
    f = FindROIs(g, [names[c] for c in parents], names[child])
    assert f.execute(out) == len(exp)
    assert out.read_bytes() == sliced_file(d, exp, [child], fresh_header(d, [child])), tag
    g.close()
    return exp, str(out)


def case_find_rois(orc, lib, tmp):
    path = synth_trio(tmp)
    exp, _ = check_find_rois(lib, tmp, path, 0, [1, 2], "child0")
    assert len(exp) > 0, "the synthetic trio has no novel k-mers"
    d = read_ctx(path)
    perm = [1, 2, 0]                                               # the child as colour 2
    p2 = write_ctx(tmp / "trio_c2.ctx", d["k"], [d["names"][c] for c in perm], d["words"], d["cov"][:, perm], d["edges"][:, perm])
    exp2, _ = check_find_rois(lib, tmp, p2, 2, [0, 1], "child2")
    assert (exp2 == exp).all()
    # a hand-made table: (child, mom, dad) coverages as stored
    rows = [(1, 0, 0), (NEG, 0, 0), (1, NEG, 0), (1, 0, 1), (0, 0, 0), (0x7FFFFFFF, 0, 0), (0xFFFFFFFF, 0, 0), (3, 0, NEG), (2, 0, 0)]
    cov = np.array(rows, dtype=np.uint32)
    edges = np.arange(27, dtype=np.uint8).reshape(9, 3)
    p3 = write_ctx(tmp / "hand.ctx", 5, ["kid", "mom", "dad"], sequential_keys(9, 5), cov, edges)
    exp3, _ = check_find_rois(lib, tmp, p3, 0, [1, 2], "hand")
    # 0x80000000 in the child is not coverage (not > 0); in a parent it is coverage (not == 0)
    assert list(exp3) == [0, 5, 8]
    # no novel k-mer: the header alone (CortexGraphWriter.close initialises the file, :140-142)
    p4 = write_ctx(tmp / "nonovel.ctx", 5, ["kid", "mom", "dad"], sequential_keys(9, 5), np.ones((9, 3), dtype=np.uint32), edges)
    exp4, out4 = check_find_rois(lib, tmp, p4, 0, [1, 2], "nonovel")
    assert len(exp4) == 0 and open(out4, "rb").read() == java_write_header(5, 1, [fresh_col("kid")])
    ro = CortexGraph(out4, lib=lib)
    assert ro.getNumRecords() == 0
    ro.close()


def family_graph(orc, tmp, k=21, seed=5):
    """child, two parents and two further samples that share some of the child's novel k-mers"""
    rng = random.Random(seed)
    base = genome_with_repeats(rng, 900, n_rep=2)
    mom, dad = base, mutate(rng, base, snv=0.01, indel=0.0)
    kid = mutate(rng, base, snv=0.03, indel=0.002)
    u1 = kid[:len(kid) // 2] + rand_seq(rng, 100)
    u2 = rand_seq(rng, 60) + kid[len(kid) // 3:2 * len(kid) // 3]
    p = str(tmp / "family.ctx")
    orc.build_graph(p, [("kid", [kid]), ("mom", [mom]), ("dad", [dad]), ("u1", [u1]), ("u2", [u2])], k)
    return p


def expected_excluded(roi_path, excluded_idx, lib, tmp, tag):
    """cgw.setHeader(ROI.getHeader()); the excluded records: what ldbg_ctx_write_records writes for them"""
    want = tmp / ("want_%s.ctx" % tag)
    idx = np.ascontiguousarray(excluded_idx, dtype=np.int64)
    lib.check(lib.dll.ldbg_ctx_write_records(str(roi_path).encode(), idx.ctypes.data_as(C.c_void_p), C.c_int64(len(idx)), str(want).encode()))
    return want.read_bytes()


def case_prefilters(orc, lib, tmp):
    gp = family_graph(orc, tmp)
    gd = read_ctx(gp)
    g = CortexGraph(gp, lib=lib)
    roi0 = tmp / "roi0.ctx"
    assert FindROIs(g, ["mom", "dad"], "kid").execute(roi0) > 20
    r0 = read_ctx(roi0)
    rng = np.random.default_rng(9)
    n = r0["N"]
    cov = rng.integers(0, 9, size=(n, 1)).astype(np.uint32)          # coverages around the thresholds, edges of every degree
    cov[::7, 0] = NEG
    edges = rng.integers(0, 256, size=(n, 1), dtype=np.uint8)
    rp = write_ctx(tmp / "roi.ctx", r0["k"], None, r0["words"], cov, edges, header=r0["header"])
    rd = read_ctx(rp)
    roi = CortexGraph(rp, lib=lib)
    for m in (0, 1, 5):                                               # FindLowCoverage.java:46: kept iff getCoverage(0) >= MIN
        exc = np.nonzero(java_cov(rd["cov"])[:, 0] < m)[0]
        out = tmp / ("low%d.ctx" % m)
        kept, excluded = FindLowCoverage(roi, m).execute(out)
        assert (kept, excluded) == (n - len(exc), len(exc)) and kept + excluded == n
        assert out.read_bytes() == expected_excluded(rp, exc, lib, tmp, "low%d" % m)
        assert len(exc) > 0                                           # (0x80000000 is below every MIN)
    exc = ref_pass(rd["cov"], rd["edges"], degree_above=(0, 4))       # FindDust.isDust :133-135
    out = tmp / "dust.ctx"
    kept, excluded = FindDust(g, ["mom", "dad"], roi).execute(out)
    assert (kept, excluded) == (n - len(exc), len(exc)) and 0 < len(exc) < n
    assert out.read_bytes() == expected_excluded(rp, exc, lib, tmp, "dust")
    # FindShared: the record of every ROI k-mer in the graph, coverage > 0 in a colour that is not child, parent or ignored
    where = {tuple(int(x) for x in row): i for i, row in enumerate(gd["words"])}
    gi = np.array([where[tuple(int(x) for x in row)] for row in rd["words"]])
    gv = java_cov(gd["cov"])[gi]
    for ignore, others, tag in (((), [3, 4], "shared"), (("u2",), [3], "shared_ign"), (("u1", "u2"), [], "shared_none")):
        exc = np.nonzero((gv[:, others] > 0).any(axis=1))[0] if others else np.zeros(0, dtype=np.int64)
        out = tmp / (tag + ".ctx")
        kept, excluded = FindShared(g, ["mom", "dad"], roi, ignore=ignore).execute(out)
        assert (kept, excluded) == (n - len(exc), len(exc)), tag
        assert out.read_bytes() == expected_excluded(rp, exc, lib, tmp, tag)
        if others:
            assert 0 < len(exc) < n
    a = np.nonzero((gv[:, [3, 4]] > 0).any(axis=1))[0]
    b = np.nonzero((gv[:, [3]] > 0).any(axis=1))[0]
    assert len(a) != len(b), "ignoring a colour changes nothing"
    # a ROI k-mer without a record in the graph: the reference dereferences the null (FindShared.java:63-68)
    rng2 = random.Random(77)
    sp = str(tmp / "stranger.ctx")
    orc.build_graph(sp, [("kid", [rand_seq(rng2, 80)])], 21)
    stranger = CortexGraph(sp, lib=lib)
    try:
        FindShared(g, ["mom", "dad"], stranger).execute(tmp / "never.ctx")
        raise AssertionError("a ROI k-mer without a record did not raise")
    except ca.JavaNullPointerException:
        pass
    stranger.close()
    roi.close()
    g.close()
    # a graph of two records never finds anything
    tp = str(tmp / "tiny2.ctx")
    orc.build_graph(tp, [("s", ["ACGTT"]), ("t", ["ACGTT"])], 4)
    td = read_ctx(tp)
    assert td["N"] == 2
    trp = write_ctx(tmp / "tiny2roi.ctx", 4, ["s"], td["words"], td["cov"][:, :1], td["edges"][:, :1])
    tg, troi = CortexGraph(tp, lib=lib), CortexGraph(trp, lib=lib)
    try:
        FindShared(tg, [], troi).execute()
        raise AssertionError("a graph of two records answered findRecord")
    except ca.JavaNullPointerException:
        pass
    tg.close()
    troi.close()


def case_remove(orc, lib, tmp):
    rng = random.Random(21)
    k = 21
    a, b = genome_with_repeats(rng, 500, n_rep=2), genome_with_repeats(rng, 300, n_rep=1)
    pp, s1 = str(tmp / "prim.ctx"), str(tmp / "sec1_raw.ctx")
    orc.build_graph(pp, [("p0", [a]), ("p1", [mutate(rng, a, snv=0.02, indel=0.0)])], k)
    orc.build_graph(s1, [("x", [a[100:220], b])], k)               # k-mers of the primary and k-mers of its own
    d1 = read_ctx(s1)
    cov1 = d1["cov"].copy()
    cov1[::3, 0] = 0                                               # present in the secondary with coverage 0: not "found"
    cov1[1::9, 0] = NEG                                            # nor is a negative coverage (> 0 is the test, Remove.java:51)
    s1 = write_ctx(tmp / "sec1.ctx", k, None, d1["words"], cov1, d1["edges"], header=d1["header"])
    dp = read_ctx(pp)
    # a member of two records: one k-mer of the primary (removed), one of its own with coverage 0
    own = read_ctx(orc.build_graph(str(tmp / "own.ctx"), [("y", [rand_seq(rng, k)])], k))
    w2 = np.concatenate([dp["words"][5:6], own["words"][:1]])
    order = np.lexsort(w2.T[::-1])
    s2 = write_ctx(tmp / "sec2.ctx", k, ["y"], w2[order], np.array([[4], [0]], dtype=np.uint32)[order], np.array([[3], [9]], dtype=np.uint8)[order])
    # the collection's iterator: the union of the k-mers, every member's colours side by side (CortexCollection.java:218-293)
    union = {}
    first = 0
    total_c = dp["C"] + 2
    for d in (dp, read_ctx(s1), read_ctx(s2)):
        for i in range(d["N"]):
            key = tuple(int(x) for x in d["words"][i])
            row = union.setdefault(key, (np.zeros(total_c, dtype=np.uint32), np.zeros(total_c, dtype=np.uint8)))
            row[0][first:first + d["C"]] = d["cov"][i]
            row[1][first:first + d["C"]] = d["edges"][i]
        first += d["C"]
    keys = sorted(union)
    cov = np.array([union[x][0] for x in keys])
    edges = np.array([union[x][1] for x in keys])
    words = np.array(keys, dtype=np.uint64).reshape(len(keys), -1)
    P = dp["C"]
    keep = np.nonzero(~(java_cov(cov)[:, P:] > 0).any(axis=1))[0]   # Remove.java:49-56
    want = java_rewritten_header(open(pp, "rb").read()) + record_bytes(words[keep], cov[keep][:, :P], edges[keep][:, :P])
    out = tmp / "removed.ctx"
    kept, removed = Remove(CortexGraph(pp, lib=lib), [s1, s2], out).execute()
    assert (kept, removed) == (len(keep), len(keys) - len(keep)) and kept + removed == len(keys)
    assert out.read_bytes() == want
    in_primary = {tuple(int(x) for x in row) for row in dp["words"]}
    kept_keys = [keys[i] for i in keep]
    assert any(x not in in_primary for x in kept_keys), "no k-mer known to a secondary only (coverage 0) was written"
    assert tuple(int(x) for x in own["words"][0]) in kept_keys       # the record of the two-record member arrives through the iterator view
    assert tuple(int(x) for x in dp["words"][5]) not in kept_keys
    assert 0 < kept < len(keys)


def roi_hits(e, seeds):
    e.walk_batch_arrays(seeds)
    n = len(seeds)
    off = np.zeros(n + 1, dtype=np.int64)
    has_null = np.zeros(n, dtype=np.uint8)
    hits = np.zeros(1, dtype=np.uint32)
    st = e._d.ldbg_engine_walk_roi_hits(e._h, off.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.c_int64(0), has_null.ctypes.data_as(C.c_void_p))
    assert st in (0, 7)
    hits = np.zeros(max(1, int(off[n])), dtype=np.uint32)
    e._lib.check(e._d.ldbg_engine_walk_roi_hits(e._h, off.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.c_int64(len(hits)),
                                                has_null.ctypes.data_as(C.c_void_p)))
    return [sorted(int(x) for x in hits[off[i]:off[i + 1]]) for i in range(n)], list(has_null)


def case_resident_roi(orc, lib, tmp):
    """FindROIs(...).graph() — the ROI graph that never left the device — against the ROI opened from the file FindROIs wrote"""
    gp = family_graph(orc, tmp, k=21, seed=6)
    g = CortexGraph(gp, lib=lib)
    f = FindROIs(g, ["mom", "dad"], "kid")
    out = tmp / "roi.ctx"
    n = f.execute(out)
    assert n > 20
    res, fil = f.graph(), CortexGraph(out, lib=lib)
    assert res.getNumRecords() == fil.getNumRecords() == n and res.getSampleName(0) == fil.getSampleName(0) == "kid"
    a, b = res.records(0, n), fil.records(0, n)
    assert all((x == y).all() for x, y in zip(a, b))
    seeds = unpack_kmers(a[0], 21)
    ia, ib = res.find_batch(seeds), fil.find_batch(seeds)
    assert (ia[0] == np.arange(n)).all() and all((x == y).all() for x, y in zip(ia, ib))
    assert res.findRecord(seeds[3].tobytes()) == fil.findRecord(seeds[3].tobytes())
    ta, tb = Partition(g, res).execute(), Partition(g, fil).execute()
    assert ta == tb and ta.startswith(">partition0")
    hits = []
    for roi in (res, fil):
        e = (TraversalEngineFactory(lib=lib).traversalColors(0).traversalDirection(BOTH).combinationOperator(OR).graph(g).rois(roi)
             .stoppingRule(ContigStopper).make())
        hits.append(roi_hits(e, seeds))
        e.close()
    assert hits[0] == hits[1] and any(len(h) > 1 for h in hits[0][0])
    res.close()
    fil.close()
    g.close()


def _refused(fn, status):
    try:
        fn()
    except ca.LdbgError as e:
        assert e.status == status, e
        return
    raise AssertionError("not refused")


def case_bad_arguments(orc, lib, tmp):
    p = clause_graph(tmp, 3, n=100, seed=1)
    g = CortexGraph(p, lib=lib)
    for flt in (dict(all_zero=[3]), dict(all_positive=[40]), dict(any_positive=[63]), dict(none_positive=[3]),      # a mask bit at or above C
                dict(cov_below=(3, 1)), dict(cov_below=(-2, 1)), dict(degree_above=(3, 1))):
        _refused(lambda: g.select(**flt), 6)
    other = CortexGraph(write_ctx(tmp / "k5.ctx", 5, ["s0", "s1", "s2"], sequential_keys(4, 5), np.ones((4, 3), np.uint32), np.zeros((4, 3), np.uint8)), lib=lib)
    two = write_ctx(tmp / "two.ctx", 31, ["a", "b"], sequential_keys(4, 31), np.ones((4, 2), np.uint32), np.zeros((4, 2), np.uint8))
    with g.select(all_positive=[0]) as sel:
        assert sel.count > 0
        for cols in ([3], [-1], [], [0, 5]):                                                                        # a projection colour out of range
            _refused(lambda: sel.write_ctx(tmp / "bad.ctx", cols), 6)
            _refused(lambda: sel.graph(cols), 6)
        _refused(lambda: sel.write_ctx(tmp / "bad.ctx", [0, 1, 2], header_path=two), 6)                              # the header has 2 colours
        _refused(lambda: sel.write_ctx(tmp / "bad.ctx", [0, 1, 2], header_path=other.path), 6)                       # the header has another k
        _refused(lambda: sel.graph([0, 1], header_path=other.path), 6)
        _refused(lambda: sel.indices(0, sel.count + 1), 6)
        try:
            sel.write_ctx(tmp / "bad.ctx", [0], header_path=tmp / "missing.ctx")
            raise AssertionError("a missing header file")
        except ca.CortexJDKException:
            pass
    _refused(lambda: g.select(all_positive=[0], lookup=other), 6)                                                   # another k
    # one rank's part of a hash-sharded table, and its image
    lib.check(lib.dll.ldbg_graph_set_shard(g._h, 1))
    _refused(lambda: g.select(all_positive=[0]), 4)
    _refused(lambda: other.select(lookup=g), 4)
    img = C.c_void_p()
    lib.check(lib.dll.ldbg_image_create(g._h, C.c_int64(64), C.c_int64(100), C.byref(img)))
    ig = C.c_void_p()
    lib.check(lib.dll.ldbg_image_graph(img, C.byref(ig)))
    image_graph = CortexGraph._from_handle(ig, lib, "#image")
    _refused(lambda: image_graph.select(all_positive=[0]), 4)
    lib.check(lib.dll.ldbg_image_destroy(img))
    lib.check(lib.dll.ldbg_graph_set_shard(g._h, 0))
    g.close()
    other.close()
