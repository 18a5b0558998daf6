"""Cases for sequences threaded through a graph (ldbg_graph_thread) and the commands built on it, shared by the
host-simulation run (tests/test_thread_hostsim.py) and the GPU run (tests/test_gpu_thread.py).

Nothing expected here comes from the code under test.  The yardstick restates the reference's loops on strings, dicts and sets:
TrimPartitions.java:41-67, FilterPartitions.java:56-125, CountNovelKmersInPartitions.java:36-46, Coverage.java:32-46,
Call.loadChildWalk (Call.java:2358-2381) and Call.getRegions (:2425-2451).  The .ctx files are parsed with roi_cases.read_ctx; a graph
is a dict from k-mer string to record number (empty under findRecord's quirk Q1 when the file has two records or fewer), a ROI graph
the same without the quirk (a HashSet filled by iteration).  Every record written here is canonical.  Bytes other than upper-case ACGT:
the window is invalid, has no record, is in no ROI set and gets copy index 0 (the entry's documented definition)."""
import random

import numpy as np

import corticall_amd as ca
from corticall_amd import (CortexGraph, CountNovelKmersInPartitions, Coverage, FilterPartitions, FindROIs, Partition, Threading,
                           TrimPartitions, traversal_utils)
from corticall_amd.partition import unpack_kmers
from tests import roi_cases as rc
from tests.orphan_cases import family
from tests.parity_cases import rand_seq
from tests.recover_cases import pack_kmers

_COMP = str.maketrans("ACGT", "TGCA")
VALID, FLIP, PAL, ROI = 1, 2, 4, 8


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canonical(s):
    r = revcomp(s)
    return r if r < s else s


def is_bases(s):
    return all(c in "ACGT" for c in s)


# ---------------------------------------------------------------- tables
def make_ctx(tmp, name, k, kmers, cov=None, colours=1):
    """the canonical forms of `kmers`, sorted, as a .ctx of `colours` colours -> (path, sorted list of k-mer strings)"""
    ks = sorted({canonical(x) for x in kmers})
    asc = np.frombuffer("".join(ks).encode(), dtype=np.uint8).reshape(len(ks), k) if ks else np.zeros((0, k), dtype=np.uint8)
    words = pack_kmers(asc, k)
    if cov is None:
        cov = np.ones((len(ks), colours), dtype=np.uint32)
    edges = np.zeros((len(ks), colours), dtype=np.uint8)
    p = rc.write_ctx(tmp / (name + ".ctx"), k, ["s%d" % c for c in range(colours)], words, np.asarray(cov, dtype=np.uint32).reshape(len(ks), colours), edges)
    return p, ks


def table_of(path):
    """-> (k, dict k-mer string -> record number, cov u32[N, C])"""
    d = rc.read_ctx(path)
    strs = [bytes(row).decode() for row in unpack_kmers(d["words"], d["k"])] if d["N"] else []
    return d["k"], {s: i for i, s in enumerate(strs)}, d["cov"]


# ---------------------------------------------------------------- the yardstick
def get_regions(hits):
    """Call.getRegions :2425-2451 over a list of booleans"""
    regions, start, stop = [], -1, 0
    for i, h in enumerate(hits):
        if h:
            if start == -1:
                start = i
            stop = i
        elif start > -1:
            regions.append((start, stop))
            start, stop = -1, 0
    if start > -1:
        regions.append((start, stop))
    return regions


def yardstick(seqs, k, gpath=None, rpath=None, quirk=False):
    seqs = [s.decode() if isinstance(s, bytes) else s for s in seqs]
    gmap, rmap = None, None
    if gpath is not None:
        _, gmap, _ = table_of(gpath)
        if quirk and len(gmap) <= 2:
            gmap = {}                                                      # Q1: findRecord's loop never runs
    if rpath is not None:
        _, rmap, _ = table_of(rpath)
    rec, info, copy, win_start = [], [], [], [0]
    first, last, n_hits, n_distinct, ends, regions = [], [], [], [], [], []
    for s in seqs:
        seen, hits, used = {}, [], set()
        for i in range(len(s) - k + 1):
            sk = s[i:i + k]
            if not is_bases(sk):
                rec.append(-1); info.append(0); copy.append(0); hits.append(False)
                continue
            r = revcomp(sk)
            ck = r if r < sk else sk
            seen[sk] = seen[sk] + 1 if sk in seen else 0                  # loadChildWalk :2368-2372
            hit = rmap is not None and ck in rmap
            if hit:
                used.add(ck)
            rec.append(gmap.get(ck, -1) if gmap is not None else -1)
            info.append(VALID | (FLIP if r < sk else 0) | (PAL if r == sk else 0) | (ROI if hit else 0))
            copy.append(seen[sk])
            hits.append(hit)
        win_start.append(win_start[-1] + len(hits))
        idx = [i for i, h in enumerate(hits) if h]
        first.append(idx[0] if idx else -1)
        last.append(idx[-1] if idx else -1)
        n_hits.append(len(idx))
        n_distinct.append(len(used))
        ends.append((1 if hits and hits[0] else 0) | (2 if hits and hits[-1] else 0))
        regions.append(get_regions(hits))
    return dict(rec=np.array(rec, dtype=np.int64), info=np.array(info, dtype=np.uint8), copy=np.array(copy, dtype=np.int32),
                win_start=np.array(win_start, dtype=np.int64), first_hit=np.array(first, dtype=np.int32), last_hit=np.array(last, dtype=np.int32),
                n_hits=np.array(n_hits, dtype=np.int32), n_distinct=np.array(n_distinct, dtype=np.int32), ends=np.array(ends, dtype=np.uint8),
                regions=regions)


def compare(t, exp, tag, copy=True):
    assert (t.n_seqs, t.n_windows) == (len(exp["first_hit"]), len(exp["rec"])), tag
    rec, info, ci = t.windows()
    assert (rec == exp["rec"]).all(), (tag, np.nonzero(rec != exp["rec"])[0][:5])
    assert (info == exp["info"]).all(), (tag, np.nonzero(info != exp["info"])[0][:5])
    if copy:
        assert (ci == exp["copy"]).all(), (tag, np.nonzero(ci != exp["copy"])[0][:5])
    sm = t.summary()
    for key in ("win_start", "first_hit", "last_hit", "n_hits", "n_distinct", "ends"):
        assert (sm[key] == exp[key]).all(), (tag, key, sm[key][:8], exp[key][:8])
    offs, start, stop = t.regions()
    flat = [r for rs in exp["regions"] for r in rs]
    assert t.n_regions == len(flat), tag
    assert list(offs) == list(np.cumsum([0] + [len(rs) for rs in exp["regions"]])), tag
    assert list(zip(start.tolist(), stop.tolist())) == flat, tag


def check(lib, seqs, k, gpath=None, rpath=None, quirk=False, copy=True, tag=""):
    """one threading against the yardstick -> the expected values"""
    exp = yardstick(seqs, k, gpath, rpath, quirk)
    g = CortexGraph(gpath, lib=lib) if gpath is not None else None
    r = CortexGraph(rpath, lib=lib) if rpath is not None else None
    with Threading(g, r, seqs, find_quirk=quirk, copy_index=copy) as t:
        compare(t, exp, tag, copy)
    for x in (g, r):
        if x is not None:
            x.close()
    return exp


def upload(lib, arr):
    """-> (holder, device pointer): the simulation's device memory is host memory"""
    if lib.is_hostsim:
        a = np.ascontiguousarray(arr).copy()
        return a, a.ctypes.data
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr).copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def pick_kmers(rng, seqs, k, frac):
    """the valid windows of the sequences, each with probability frac"""
    out = []
    for s in seqs:
        for i in range(len(s) - k + 1):
            if is_bases(s[i:i + k]) and rng.random() < frac:
                out.append(s[i:i + k])
    return out


# ---------------------------------------------------------------- cases
WIDTH_K = [5, 31, 32, 33, 47, 63, 65, 97]


def case_widths(orc, lib, tmp, k):
    """W = 1..4; three sequences whose first bytes fall at offsets 0, 1 and 31 modulo 32 of the uploaded text; with an even k a
    planted palindrome that the graph and the ROI graph hold"""
    rng = random.Random(k)
    base = 32 * ((k + 40) // 32 + 1)
    s0, s1, s2 = rand_seq(rng, base + 1), rand_seq(rng, base + 30), rand_seq(rng, k + 25)
    planted = []
    if k % 2 == 0:
        half = rand_seq(rng, k // 2)
        pal = half + revcomp(half)
        s2 = s2[:7] + pal + s2[7:]
        planted.append(pal)
    seqs = [s0, s1, s2]
    assert [sum(len(x) for x in seqs[:i]) % 32 for i in range(3)] == [0, 1, 31]
    gp, _ = make_ctx(tmp, "g%d" % k, k, pick_kmers(rng, seqs, k, 0.7) + planted + [rand_seq(rng, k) for _ in range(20)])
    rp, _ = make_ctx(tmp, "r%d" % k, k, pick_kmers(rng, seqs, k, 0.3) + planted + [rand_seq(rng, k) for _ in range(20)])
    exp = check(lib, seqs, k, gp, rp, tag="k%d" % k)
    assert (exp["rec"] >= 0).sum() > 10 and (exp["rec"] < 0).sum() > 10 and (exp["info"] & FLIP).any() and (~exp["info"] & FLIP).any()
    assert exp["n_hits"].min() > 0 and table_of(gp)[0] == k
    if k % 2 == 0:
        w = exp["win_start"][2] + 7
        assert exp["info"][w] == VALID | PAL | ROI and exp["rec"][w] >= 0


def case_lengths(orc, lib, tmp):
    k = 31
    rng = random.Random(1)
    body = rand_seq(rng, k + 1)
    seqs = ["", body[:k - 1], body[:k], body]
    rp, _ = make_ctx(tmp, "len_r", k, [body[:k], body[1:]])
    exp = check(lib, seqs, k, rp, rp, tag="lengths")
    assert list(np.diff(exp["win_start"])) == [0, 0, 1, 2] and list(exp["n_hits"]) == [0, 0, 1, 2] and list(exp["ends"]) == [0, 0, 3, 3]
    check(lib, [], k, rp, rp, tag="empty batch")
    check(lib, ["", "ACGT"], k, None, rp, tag="no windows")


CHUNK_WINDOWS = [4095, 4096, 4097]


def case_chunk_single(orc, lib, tmp, n):
    k = 21
    rng = random.Random(n)
    s = rand_seq(rng, n + k - 1)
    s = s[:300] + s[100:200] + s[300:]                                      # a repeat: copy indices above 0
    s = s[:n + k - 1]
    rp, _ = make_ctx(tmp, "chunk_r%d" % n, k, pick_kmers(rng, [s], k, 0.4) + [s[-k:]])
    exp = check(lib, [s], k, rp, rp, tag="chunk%d" % n)
    assert len(exp["rec"]) == n and exp["copy"].max() == 1 and exp["info"][-1] & ROI and len(exp["regions"][0]) > 100


def case_chunk_batch(orc, lib, tmp):
    """a batch whose windows cross 4096 and 2 x 4096: at each boundary a run of equal k-mers (poly-A, in the ROI graph), which is
    one region, lies across it inside one sequence"""
    k = 21
    rng = random.Random(77)
    a = rand_seq(rng, 4000 + k - 1)                                         # windows 0 .. 3999
    b = rand_seq(rng, 79) + "C" + "A" * (k + 39) + "C" + rand_seq(rng, 4040) + "C" + "A" * (k + 49) + "C" + rand_seq(rng, 500)
    seqs = [a, b]
    rp, _ = make_ctx(tmp, "batch_r", k, ["A" * k] + pick_kmers(rng, seqs, k, 0.05))
    exp = check(lib, seqs, k, rp, rp, tag="chunk batch")
    p1, p2 = 4000 + b.index("A" * k), 4000 + b.index("A" * (k + 49))
    assert p1 < 4096 < p1 + 39 and p2 < 8192 < p2 + 49 and len(exp["rec"]) > 8192
    assert list(exp["copy"][p1:p1 + 40]) == list(range(40)) and list(exp["copy"][p2:p2 + 50]) == list(range(40, 90))
    for lo, n in ((p1 - 4000, 40), (p2 - 4000, 50)):
        assert any(r[0] <= lo and r[1] >= lo + n - 1 for r in exp["regions"][1])


MANY_SEQS = [1, 64, 65, 1000]


def case_many_sequences(orc, lib, tmp, n):
    k = 11
    rng = random.Random(n)
    seqs = [rand_seq(rng, rng.choice([0, 3, k - 1, k, k + 1, 17, 30])) for _ in range(n)]
    seqs[-1] = rand_seq(rng, 30)
    seqs[0] = seqs[-1][5:25] if n > 1 else seqs[0]                          # k-mers shared between sequences
    rp, _ = make_ctx(tmp, "many_r%d" % n, k, pick_kmers(rng, seqs, k, 0.5) + [seqs[-1][-k:]])
    exp = check(lib, seqs, k, rp, rp, tag="many%d" % n)
    assert exp["ends"][-1] & 2 and exp["n_hits"].sum() > 0


def case_non_bases(orc, lib, tmp):
    """N as the first / last byte of a window; a lower-case stretch; a window that would hit if upper-cased must miss"""
    k = 31
    rng = random.Random(3)
    x = rand_seq(rng, 120)
    with_n = x[:50] + "N" + x[51:]                                          # windows 20 .. 50 hold it: 20 as the last byte, 50 as the first
    lower = x[:40] + x[40:75].lower() + x[75:]                              # window 42 is all lower case
    rp, _ = make_ctx(tmp, "nb_r", k, [x[i:i + k] for i in range(0, 90, 3)])
    exp = check(lib, [x, with_n, lower, "N" * 40, x.lower()], k, rp, rp, tag="non bases")
    w = exp["win_start"]
    assert exp["info"][w[0] + 42] & ROI and exp["info"][w[2] + 42] == 0 and exp["rec"][w[2] + 42] == -1
    assert list(exp["info"][w[1] + 20:w[1] + 51]) == [0] * 31 and exp["info"][w[1] + 19] & VALID and exp["info"][w[1] + 51] & VALID
    assert not exp["info"][w[3]:].any() and exp["n_hits"][3] == exp["n_hits"][4] == 0


def case_table_sizes(orc, lib, tmp):
    """ROI graphs of 0, 1, 2 and 3 records: membership holds for all.  Graphs of 2 and 3 records with and without
    LDBG_THREAD_FIND_QUIRK: Q1."""
    k = 31
    rng = random.Random(4)
    s = rand_seq(rng, 80)
    kmers = [s[3:3 + k], s[20:20 + k], s[44:44 + k]]
    for m in (0, 1, 2, 3):
        rp, _ = make_ctx(tmp, "ts_r%d" % m, k, kmers[:m])
        exp = check(lib, [s], k, None, rp, copy=False, tag="rois%d" % m)
        assert exp["n_hits"][0] == m and (exp["rec"] == -1).all()
    for m in (2, 3):
        gp, _ = make_ctx(tmp, "ts_g%d" % m, k, kmers[:m])
        for quirk in (False, True):
            exp = check(lib, [s], k, gp, None, quirk=quirk, copy=False, tag="g%d quirk %s" % (m, quirk))
            assert (exp["rec"] >= 0).sum() == (0 if quirk and m == 2 else m) and exp["n_hits"][0] == 0


def case_repeats(orc, lib, tmp):
    """a k-mer three times forward and once as its reverse complement in one sequence, and again in a second sequence"""
    k = 31
    rng = random.Random(5)
    x = rand_seq(rng, k)
    if revcomp(x) < x:
        x = revcomp(x)
    sp = [rand_seq(rng, 9) for _ in range(6)]
    s0 = sp[0] + x + sp[1] + x + sp[2] + revcomp(x) + sp[3] + x + sp[4]
    s1 = sp[5] + x + sp[0]
    rp, _ = make_ctx(tmp, "rep_r", k, [x])
    gp, _ = make_ctx(tmp, "rep_g", k, [x, s0[1:1 + k], s1[2:2 + k]])
    exp = check(lib, [s0, s1], k, gp, rp, tag="repeats")
    pos = [9, 9 + k + 9, 9 + 2 * (k + 9), 9 + 3 * (k + 9)]
    assert [int(exp["copy"][p]) for p in pos] == [0, 1, 0, 2]               # in order of appearance: forward, forward, reverse complement, forward
    assert sorted(int(exp["copy"][p]) for p in (pos[0], pos[1], pos[3])) == [0, 1, 2] and exp["copy"][pos[2]] == 0
    assert list(exp["n_hits"]) == [4, 1] and list(exp["n_distinct"]) == [1, 1]
    assert exp["copy"][exp["win_start"][1] + 9] == 0                        # counts do not leak between sequences
    rec, ci = traversal_utils.load_child_walk(s0, CortexGraph(gp, lib=lib))
    assert (rec == exp["rec"][:len(rec)]).all() and (ci == exp["copy"][:len(ci)]).all()


def case_regions(orc, lib, tmp):
    """a hit in the first window; in the last window; two regions separated by one miss; alternating hit / miss; only hits; none.
    The windows of random sequences at k = 31 do not collide, so the hit pattern is exactly the planted one (asserted)."""
    k = 31
    rng = random.Random(8)
    pats = ["1" + "0" * 20, "0" * 20 + "1", "0001101100", "10" * 12, "1" * 15, "0" * 15, "01" * 10 + "1"]
    seqs = [rand_seq(rng, len(p) + k - 1) for p in pats]
    chosen = [s[i:i + k] for s, p in zip(seqs, pats) for i, c in enumerate(p) if c == "1"]
    rp, _ = make_ctx(tmp, "regx_r", k, chosen)
    exp = check(lib, seqs, k, None, rp, copy=False, tag="regions exact")
    assert exp["regions"][0] == [(0, 0)] and exp["regions"][1] == [(20, 20)] and exp["regions"][2] == [(3, 4), (6, 7)]
    assert exp["regions"][3] == [(i, i) for i in range(0, 24, 2)] and exp["regions"][4] == [(0, 14)] and exp["regions"][5] == []
    assert list(exp["ends"]) == [1, 2, 0, 1, 3, 0, 2] and list(exp["first_hit"]) == [0, 20, 3, 0, 0, -1, 1]
    with Threading(None, CortexGraph(rp, lib=lib), seqs) as th:
        assert [traversal_utils.get_regions(th, i) for i in range(len(seqs))] == exp["regions"]


# ---------------------------------------------------------------- the commands
def write_fasta(path, recs, width=None):
    with open(path, "w") as f:
        for name, seq in recs:
            f.write(">" + name + "\n")
            if width:
                for i in range(0, len(seq), width):
                    f.write(seq[i:i + width] + "\n")
            else:
                f.write(seq + "\n")
    return str(path)


def ref_trim(recs, k, rset, margin):
    """TrimPartitions.java:41-67 -> (text, raised): raised when subList(start, stop) throws, the text then ends before that record"""
    out = []
    for name, seq in recs:
        w = []
        start, stop = len(seq) - k, 0
        for i in range(len(seq) - k + 1):
            sk = seq[i:i + k]
            if is_bases(sk) and canonical(sk) in rset:
                if i < start:
                    start = i
                if i > stop:
                    stop = i
            w.append(sk)
        start = start - margin if start - margin >= 0 else 0
        stop = stop + margin if stop + margin < len(w) - 1 else len(w) - 1
        if len(w) > 0:
            if start > stop:
                return "".join(out), True
            sub = w[start:stop]
            out.append(">" + name + "\n")
            out.append((sub[0] + "".join(x[-1] for x in sub[1:]) if sub else "") + "\n")        # TraversalUtils.toContig
    return "".join(out), False


def ref_used(seq, k, rset):
    return {canonical(seq[i:i + k]) for i in range(len(seq) - k + 1) if is_bases(seq[i:i + k]) and canonical(seq[i:i + k]) in rset}


def ref_filter(recs, k, rset, threshold):
    """FilterPartitions.java:56-125; ties in input order (the reference's HashMap order is not pinned) -> (text, raised)"""
    kept = []
    for name, seq in recs:
        if len(seq) < k:
            return "", True                                                  # substring(0, k): StringIndexOutOfBoundsException
        cks = ref_used(seq, k, rset)
        ck0, ck1 = seq[:k], seq[len(seq) - k:]
        in0 = is_bases(ck0) and canonical(ck0) in rset
        in1 = is_bases(ck1) and canonical(ck1) in rset
        if len(cks) > threshold and not in0 and not in1:
            kept.append((name, seq, len(cks)))
    kept.sort(key=lambda x: -x[2])
    return "".join(">%s\n%s\n" % (n, s) for n, s, _ in kept), False


def ref_count(recs, k, rset):
    return "partitionName\tpartitionLength\tnovelKmers\n" + "".join("%s\t%d\t%d\n" % (n.split(" ")[0], len(s), len(ref_used(s, k, rset))) for n, s in recs)


def ref_coverage(recs, k, gmap, cov, colour):
    """Coverage.java:32-46 -> (text, raised): raised at the first window without a record, after the lines before it"""
    out = ["contig\tkmer\tindex\tcoverage\n"]
    if len(gmap) <= 2:
        gmap = {}
    for name, seq in recs:
        for i in range(len(seq) - k + 1):
            sk = seq[i:i + k]
            r = gmap.get(canonical(sk)) if is_bases(sk) else None
            if r is None:
                return "".join(out), True
            out.append("%s\t%s\t%d\t%d\n" % (name.split(" ")[0], sk, i, int(np.int32(np.uint32(cov[r, colour])))))
    return "".join(out), False


def run_command(cmd, out, exc):
    """-> (text written to out, raised)"""
    try:
        text = cmd.execute(out)
        raised = False
    except exc as e:
        text, raised = e.printed, True
    assert open(out).read() == text
    return text, raised


def case_trim(orc, lib, tmp):
    k, M = 11, 3
    rng = random.Random(9)
    mid = rand_seq(rng, 60)            # hits at windows 20 and 30: neither clamp
    edge = rand_seq(rng, 40)           # hits at windows 1 and 28 of 30: both clamps
    one = rand_seq(rng, k)             # a single window: stop == start, the empty body
    short = rand_seq(rng, k - 2)       # no window: nothing printed
    nohit_small = rand_seq(rng, k + 5)  # no hit, n - 1 <= 2 M: start <= stop
    nohit_big = rand_seq(rng, k + 30)  # no hit, n - 1 > 2 M: start > stop
    rp, ks = make_ctx(tmp, "trim_r", k, [mid[20:20 + k], mid[30:30 + k], edge[1:1 + k], edge[28:28 + k]])
    rset = set(ks)
    roi = CortexGraph(rp, lib=lib)
    good = [("mid one", mid), ("edge", edge), ("one", one), ("short", short), ("small", nohit_small)]
    fa = write_fasta(tmp / "trim.fa", good, width=25)
    want, raised = ref_trim(good, k, rset, M)
    assert not raised and want.count(">") == 4 and ">one\n\n" in want and ">mid one\n" + mid[17:33 + k - 1] + "\n" in want and ">edge\n" + edge[:29 + k - 1] + "\n" in want
    assert run_command(TrimPartitions(fa, roi, M), tmp / "trim.out", ca.CortexJDKException) == (want, False)
    bad = good[:2] + [("big", nohit_big), ("after", mid)]
    fb = write_fasta(tmp / "trim_bad.fa", bad)
    want, raised = ref_trim(bad, k, rset, M)
    assert raised and want.count(">") == 2
    assert run_command(TrimPartitions(fb, roi, M), tmp / "trim_bad.out", ca.CortexJDKException) == (want, True)
    assert TrimPartitions(good, roi).MARGIN == 500
    roi.close()


def case_filter_and_count(orc, lib, tmp):
    k = 11
    rng = random.Random(10)
    contigs, chosen = [], []
    for name, n_roi, end in (("five", 5, False), ("six x=1", 6, False), ("seven end", 7, True), ("eight a", 8, False), ("eight b", 8, False), ("nine", 9, False)):
        s = rand_seq(rng, 70)
        chosen += [s[10 + 4 * j:10 + 4 * j + k] for j in range(n_roi - (1 if end else 0))]
        if end:
            chosen.append(s[-k:])
        contigs.append((name, s))
    rp, ks = make_ctx(tmp, "flt_r", k, chosen)
    rset = set(ks)
    assert [len(ref_used(s, k, rset)) for _, s in contigs] == [5, 6, 7, 8, 8, 9]
    roi = CortexGraph(rp, lib=lib)
    fa = write_fasta(tmp / "flt.fa", contigs)
    want, raised = ref_filter(contigs, k, rset, 5)
    assert not raised and [l[1:] for l in want.split("\n") if l.startswith(">")] == ["nine", "eight a", "eight b", "six x=1"]
    assert run_command(FilterPartitions(fa, roi), tmp / "flt.out", ca.CortexJDKException) == (want, False)
    assert FilterPartitions(fa, roi, 8).execute() == ref_filter(contigs, k, rset, 8)[0]
    want = ref_count(contigs, k, rset)
    assert "six\t70\t6\n" in want and "eight\t70\t8\n" in want
    assert run_command(CountNovelKmersInPartitions(fa, roi), tmp / "cnt.out", ca.CortexJDKException) == (want, False)
    short = contigs[:3] + [("short", rand_seq(rng, k - 1))]
    assert ref_filter(short, k, rset, 5) == ("", True)
    try:
        FilterPartitions(short, roi).execute()
        raise AssertionError("a contig shorter than k was accepted")
    except ca.CortexJDKException:
        pass
    roi.close()


def case_coverage(orc, lib, tmp):
    k = 11
    rng = random.Random(11)
    a, b = rand_seq(rng, 40), rand_seq(rng, 30)
    kmers = sorted({canonical(s[i:i + k]) for s in (a, b) for i in range(len(s) - k + 1)})
    cov = rc.COV_VALUES[np.arange(2 * len(kmers)) % len(rc.COV_VALUES)].reshape(len(kmers), 2)
    cov[kmers.index(canonical(a[5:5 + k])), 1] = rc.NEG
    gp, ks = make_ctx(tmp, "cov_g", k, kmers, cov=cov, colours=2)
    _, gmap, gcov = table_of(gp)
    g = CortexGraph(gp, lib=lib)
    recs = [("a first", a), ("b", b), ("tiny", "ACG")]
    fa = write_fasta(tmp / "cov.fa", recs)
    want, raised = ref_coverage(recs, k, gmap, gcov, 1)
    assert not raised and "a\t%s\t5\t-2147483648\n" % a[5:5 + k] in want and want.count("\n") == 1 + 30 + 20
    assert run_command(Coverage(g, fa, "s1"), tmp / "cov.out", ca.JavaNullPointerException) == (want, False)
    stranger = b[:15] + rand_seq(rng, 20)                                   # windows from 5 on are not in the graph
    recs = [("a first", a), ("gap", stranger), ("b", b)]
    want, raised = ref_coverage(recs, k, gmap, gcov, 0)
    assert raised and want.count("\n") == 1 + 30 + 5
    assert run_command(Coverage(g, recs, 0), tmp / "cov_bad.out", ca.JavaNullPointerException) == (want, True)
    with g.thread([a]) as t:
        rc._refused(lambda: t.coverage(2), 6)
        rc._refused(lambda: t.coverage(-1), 6)
    g.close()
    tp, _ = make_ctx(tmp, "cov_tiny", k, kmers[:2])                         # Q1: findRecord finds nothing in two records
    tiny = CortexGraph(tp, lib=lib)
    two = [("t", kmers[0])]
    assert run_command(Coverage(tiny, two, 0), tmp / "cov_tiny.out", ca.JavaNullPointerException) == ("contig\tkmer\tindex\tcoverage\n", True)
    tiny.close()


def case_end_to_end(orc, lib, tmp):
    """Build -> FindROIs -> Partition on the small family of the orphan cases, then the three post-filters over Partition's FASTA;
    and the device form over the same bytes: identical arrays"""
    k = 21
    haps = family(orc, k, 1)
    gp = str(tmp / "family.ctx")
    g = CortexGraph.build(haps, k, path=gp, lib=lib)
    rp = tmp / "roi.ctx"
    assert FindROIs(g, ["mom", "dad"], "kid").execute(rp) > 0
    roi = CortexGraph(str(rp), lib=lib)
    text = Partition(g, roi).execute()
    fa = tmp / "partitions.fa"
    fa.write_text(text)
    recs = [(l[1:], s) for l, s in zip(text.split("\n")[0::2], text.split("\n")[1::2])]
    assert len(recs) >= 3 and all(len(s) >= k for _, s in recs)
    _, rmap, _ = table_of(str(rp))
    rset = set(rmap)
    want, raised = ref_trim(recs, k, rset, 10)
    assert run_command(TrimPartitions(str(fa), roi, 10), tmp / "trim.out", ca.CortexJDKException) == (want, raised)
    want, raised = ref_filter(recs, k, rset, 5)
    assert not raised and run_command(FilterPartitions(str(fa), roi), tmp / "flt.out", ca.CortexJDKException) == (want, False)
    want = ref_count(recs, k, rset)
    assert run_command(CountNovelKmersInPartitions(str(fa), roi), tmp / "cnt.out", ca.CortexJDKException) == (want, False)
    # host form against the yardstick, device form against the host form
    seqs = [s for _, s in recs]
    exp = yardstick(seqs, k, gp, str(rp))
    bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    hb, pb = upload(lib, bases)
    ho, po = upload(lib, offs)
    with g.thread(seqs, rois=roi, copy_index=True) as th, g.thread_device(pb, po, len(seqs), rois=roi, copy_index=True) as td:
        compare(th, exp, "e2e host")
        compare(td, exp, "e2e device")
        n = th.n_windows
        hr, pr = upload(lib, np.full(n, -7, dtype=np.int64))
        hi, pi = upload(lib, np.full(n, 0xEE, dtype=np.uint8))
        hc, pc = upload(lib, np.full(n, -7, dtype=np.int32))
        td.windows_dev(pr, pi, pc)
        back = [x if lib.is_hostsim else x.cpu().numpy() for x in (hr, hi, hc)]
        assert (back[0] == exp["rec"]).all() and (back[1] == exp["info"]).all() and (back[2] == exp["copy"]).all()
        assert (exp["rec"] >= 0).all() and exp["n_hits"].sum() > 0         # Partition's contigs are walks of the graph
    del hb, ho
    roi.close()
    g.close()


def case_bad_arguments(orc, lib, tmp):
    import ctypes as C
    k = 31
    rng = random.Random(12)
    s = rand_seq(rng, 60)
    gp, _ = make_ctx(tmp, "bad_g", k, [s[i:i + k] for i in range(10)])
    k5, _ = make_ctx(tmp, "bad_k5", 5, ["AACGT", "AAGGT", "ACCGA", "AACCA"])
    g, other = CortexGraph(gp, lib=lib), CortexGraph(k5, lib=lib)
    rc._refused(lambda: Threading(None, None, [s]), 6)
    text = np.frombuffer(s.encode(), dtype=np.uint8)
    h = C.c_void_p()

    def raw(gh, rh, offsets, flags=0):
        offs = np.array(offsets, dtype=np.int64)
        st = lib.dll.ldbg_graph_thread(gh, rh, C.c_void_p(text.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_int64(len(offs) - 1), flags, C.byref(h))
        assert h.value is None or st == 0
        return st
    assert raw(None, None, [0, 60]) == 6                                    # both graphs NULL
    assert raw(g._h, other._h, [0, 60]) == 6                                # differing k
    assert raw(g._h, None, [0, 40, 30]) == 6                                # decreasing offsets
    assert raw(g._h, None, [-1, 40]) == 6
    assert raw(g._h, None, [0, 60], flags=4) == 6
    lib.check(lib.dll.ldbg_graph_set_shard(g._h, 1))
    assert raw(g._h, None, [0, 60]) == 4                                    # one rank's part of a sharded table
    assert raw(None, g._h, [0, 60]) == 4
    lib.check(lib.dll.ldbg_graph_set_shard(g._h, 0))
    with g.thread([s]) as t:
        rc._refused(lambda: t.windows(0, t.n_windows + 1), 6)
        rc._refused(lambda: t.summary(1, 1), 6)
        ci = np.zeros(t.n_windows, dtype=np.int32)
        assert lib.dll.ldbg_threading_windows(t._h, C.c_int64(0), C.c_int64(t.n_windows), None, None, C.c_void_p(ci.ctypes.data)) == 6   # made without copy indices
    other.close()
    g.close()


def case_too_many_windows(orc, lib, tmp):
    """offsets that claim 2^31 windows over a one-byte buffer: refused from the offsets alone, nothing is read"""
    import ctypes as C
    gp, _ = make_ctx(tmp, "big_g", 5, ["AACGT", "AAGGT", "ACCGA"])
    g = CortexGraph(gp, lib=lib)
    text = np.zeros(1, dtype=np.uint8)
    offs = np.array([0, (1 << 31) + 4], dtype=np.int64)
    h = C.c_void_p()
    assert lib.dll.ldbg_graph_thread(g._h, None, C.c_void_p(text.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_int64(1), 0, C.byref(h)) == 4
    offs = np.array([0, 1 << 30, 1 << 31, (1 << 31) + 20], dtype=np.int64)  # the sum crosses it in the last sequence
    assert lib.dll.ldbg_graph_thread(g._h, None, C.c_void_p(text.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_int64(3), 0, C.byref(h)) == 4
    assert h.value is None
    g.close()
