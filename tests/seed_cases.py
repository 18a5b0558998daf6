"""Cases for the variant seeds (ldbg_graph_variant_seeds) and the occurrences of a threading (ldbg_threading_occurrences),
shared by the host-simulation run (tests/test_seeds_hostsim.py) and the GPU run (tests/test_gpu_seeds.py).

Nothing expected here comes from the code under test.  The yardstick restates getVariantSeeds (ComputeAssemblyQuality.java:204-286, with
its LinkedHashSet guard; ComputeInheritance.java:238-322 is the same loop without it) on strings, dicts and sets over a .ctx parsed with
roi_cases.read_ctx: the filter on CortexRecord.getCoverage's int, the string graph as two dicts of sets (no parallel edges, loops
allowed), the walk from every vertex of in-degree 0 and out-degree 1.  Occurrences are counted by a plain loop over the sequences.
Hand-written tables choose their edge bytes through Tab, which only produces inputs: what they mean is decided by the yardstick."""
import ctypes as C
import math
import random

import numpy as np

import corticall_amd as ca
from corticall_amd import ComputeAssemblyQuality, ComputeInheritance, CortexCollection, CortexGraph, Threading, _native
from corticall_amd.partition import unpack_kmers
from tests import roi_cases as rc
from tests.parity_cases import rand_seq
from tests.recover_cases import pack_kmers
from tests.thread_cases import canonical, is_bases, revcomp, upload, write_fasta

NEG = rc.NEG
_COMP1 = {"A": "T", "C": "G", "G": "C", "T": "A"}


# ---------------------------------------------------------------- the yardstick
def table(path):
    """-> dict(k, C, N, strs: the stored k-mers, index: k-mer -> record, cov: Java ints [N, C], edges u8[N, C])"""
    d = rc.read_ctx(path)
    strs = [bytes(row).decode() for row in unpack_kmers(d["words"], d["k"])] if d["N"] else []
    return dict(k=d["k"], C=d["C"], N=d["N"], strs=strs, index={s: i for i, s in enumerate(strs)}, cov=rc.java_cov(d["cov"]).reshape(d["N"], d["C"]),
                edges=d["edges"].reshape(d["N"], d["C"]))


def in_edges(e):
    """CortexRecord.getInEdgesAsBytes :214-237"""
    return [b for i, b in enumerate("ACGT") if (e >> 4) & (1 << (3 - i))]


def out_edges(e):
    """CortexRecord.getOutEdgesAsBytes :251-273"""
    return [b for i, b in enumerate("ACGT") if (e & 0xF) & (1 << i)]


def singly_connected(t, r):
    """isSinglyConnected :288-299"""
    return all(len(in_edges(int(t["edges"][r, c]))) == 1 and len(out_edges(int(t["edges"][r, c]))) == 1 for c in range(t["C"]) if t["cov"][r, c] > 0)


def filter_pass(t, r, all_zero=(), covered=(), unique=()):
    """the conjunction of the entry point's clauses; unique: (colour or -1, bool per record)"""
    v = t["cov"][r]
    if not singly_connected(t, r) or any(v[c] != 0 for c in all_zero):
        return False
    for colours, lo, hi in covered:
        if len(colours) and not lo <= sum(1 for c in colours if v[c] > 0) <= hi:
            return False
    return all(bool(u[r]) for c, u in unique if c < 0 or v[c] > 0)


def variant_seeds(t, S):
    """getVariantSeeds over the records S -> (sorted good records, |S|, starts, good)"""
    succ, pred, verts = {}, {}, []

    def vertex(x):
        if x not in succ:
            succ[x], pred[x] = set(), set()
            verts.append(x)

    def edge(a, b):
        vertex(a); vertex(b)
        succ[a].add(b); pred[b].add(a)
    for r in S:
        fw = t["strs"][r]
        rv = revcomp(fw)
        vertex(fw); vertex(rv)
        for c in range(t["C"]):
            if t["cov"][r, c] > 0:
                for ie in in_edges(int(t["edges"][r, c])):
                    p = ie + fw[:-1]
                    edge(p, fw); edge(rv, revcomp(p))
                for oe in out_edges(int(t["edges"][r, c])):
                    n = fw[1:] + oe
                    edge(fw, n); edge(revcomp(n), rv)
    starts, good = 0, set()
    for sk in verts:
        if len(pred[sk]) == 0 and len(succ[sk]) == 1:
            starts += 1
            contig, v = [sk], sk
            while len(succ[v]) == 1:
                v = next(iter(succ[v]))
                if v in contig:
                    break
                contig.append(v)
            if len(contig) > 3:
                good.add(canonical(contig[1]))
    recs = sorted(t["index"][g] for g in good)              # (a KeyError here: a good seed that is no record)
    return recs, len(S), starts, len(recs)


def count_occurrences(t, seqs, quirk=False):
    """per record the windows of the sequences whose canonical k-mer it is, and the first of them (-1: none); windows are numbered
    through all sequences, the invalid ones included"""
    k = t["k"]
    count, first = np.zeros(t["N"], dtype=np.uint32), np.full(t["N"], -1, dtype=np.int64)
    index = {} if quirk and t["N"] <= 2 else t["index"]
    w = 0
    for s in seqs:
        for i in range(len(s) - k + 1):
            sk = s[i:i + k]
            if is_bases(sk):
                r = index.get(canonical(sk))
                if r is not None:
                    count[r] += 1
                    if first[r] < 0:
                        first[r] = w
            w += 1
    return count, first


def expect(t, all_zero=(), covered=(), unique=()):
    S = [r for r in range(t["N"]) if filter_pass(t, r, all_zero, covered, unique)]
    return variant_seeds(t, S) + (S,)


def compare(sel, exp, tag):
    recs, n_seeds, starts, n_good, _ = exp
    assert (sel.n_seeds, sel.n_unique, sel.n_good, sel.count) == (n_seeds, starts, n_good, n_good), (tag, sel.n_seeds, sel.n_unique, sel.n_good, exp[1:4])
    assert sel.indices().tolist() == recs, tag


def check(lib, path, all_zero=(), covered=(), unique=(), unique_lib=None, tag=""):
    """one seed pass against the yardstick -> the expected values.  unique: what the yardstick takes; unique_lib (path -> graph -> list):
    what the library takes, made once the graph is open"""
    t = table(path)
    exp = expect(t, all_zero, covered, unique)
    g = CortexGraph(path, lib=lib)
    held = []
    try:
        ul = unique_lib(g, held) if unique_lib else ()
        with g.variant_seeds(all_zero=all_zero, covered=covered, unique=ul) as sel:
            compare(sel, exp, tag)
            if sel.count:
                assert rc.fetch_dev(lib, sel, sel.count).tolist() == exp[0], tag
    finally:
        for x in reversed(held):
            x.close() if hasattr(x, "close") else None
        g.close()
    return t, exp


# ---------------------------------------------------------------- hand-written tables
class Tab:
    """records with chosen coverages and edge bytes.  edge(a, b, colours, declare): the edge a -> b between oriented k-mers, written
    into a's record (as a successor of the stored k-mer or a predecessor of its reverse complement) and / or into b's record."""

    def __init__(self, k, colours=1):
        self.k, self.C, self.rec = k, colours, {}

    def add(self, v, cov):
        cov = [cov] * self.C if isinstance(cov, int) else list(cov)
        self.rec.setdefault(canonical(v), [cov, [0] * self.C])[0] = cov

    def _in(self, key, base, cols):
        for c in cols:
            self.rec[key][1][c] |= 1 << (4 + 3 - "ACGT".index(base))

    def _out(self, key, base, cols):
        for c in cols:
            self.rec[key][1][c] |= 1 << "ACGT".index(base)

    def edge(self, a, b, colours=None, declare="ab"):
        cols = range(self.C) if colours is None else colours
        assert a[1:] == b[:-1]
        ka, kb = canonical(a), canonical(b)
        if "a" in declare and ka in self.rec:
            if a == ka:
                self._out(ka, b[-1], cols)
            else:
                self._in(ka, _COMP1[b[-1]], cols)
        if "b" in declare and kb in self.rec:
            if b == kb:
                self._in(kb, a[0], cols)
            else:
                self._out(kb, _COMP1[a[0]], cols)

    def path(self, vs, colours=None):
        for a, b in zip(vs, vs[1:]):
            self.edge(a, b, colours)

    def write(self, tmp, name):
        ks = sorted(self.rec)
        asc = np.frombuffer("".join(ks).encode(), dtype=np.uint8).reshape(len(ks), self.k)
        cov = np.array([self.rec[x][0] for x in ks], dtype=np.uint32).reshape(len(ks), self.C)
        edges = np.array([self.rec[x][1] for x in ks], dtype=np.uint8).reshape(len(ks), self.C)
        return rc.write_ctx(tmp / (name + ".ctx"), self.k, ["s%d" % c for c in range(self.C)], pack_kmers(asc, self.k), cov, edges)


def windows(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def strand_path(rng, k, n, strand):
    """n consecutive k-mers that are all canonical as given (strand +1) or all the reverse complement of their record (-1)"""
    while True:
        s = rand_seq(rng, k + n - 1)
        ws = windows(s, k)
        if len({canonical(w) for w in ws}) == n and all((canonical(w) == w) == (strand > 0) and w != revcomp(w) for w in ws):
            return ws


COV0 = [((0,), 1, 1)]           # coverage in colour 0


# ---------------------------------------------------------------- chains at the boundary
def case_chain(orc, lib, tmp, j, strand):
    """v0 -> ... -> v_{j+1} with v1 .. vj in S: j + 2 vertices, so j = 1 is rejected and j = 2 is the shortest accepted"""
    k = 11
    vs = strand_path(random.Random(100 * j + strand), k, j + 2, strand)
    tb = Tab(k)
    for i, v in enumerate(vs):
        tb.add(v, 1 if 1 <= i <= j else 0)
    tb.path(vs)
    t, exp = check(lib, tb.write(tmp, "chain%d_%d" % (j, strand)), covered=COV0, tag="chain %d %d" % (j, strand))
    want = sorted({t["index"][canonical(vs[1])], t["index"][canonical(vs[j])]}) if j >= 2 else []
    assert exp[:4] == (want, j, 2, len(want)), exp


def case_chain_no_start(orc, lib, tmp):
    """v0 is itself declared as a successor by another record u of S: its in-degree is 1, it is no start; the chain now starts before u"""
    k, j = 11, 3
    vs = strand_path(random.Random(7), k, j + 4, 1)            # t, u, v0 .. v4
    tb = Tab(k)
    for i, v in enumerate(vs):
        tb.add(v, 1 if i == 1 or 3 <= i <= 5 else 0)           # u and v1 .. v3 in S; t, v0 and v4 are records without coverage
    tb.path(vs)
    t, exp = check(lib, tb.write(tmp, "nostart"), covered=COV0, tag="no start")
    assert exp[:4] == (sorted([t["index"][vs[1]], t["index"][vs[5]]]), 4, 2, 2), exp      # good: u (forward) and v3 (reverse strand), not v1


# ---------------------------------------------------------------- asymmetric and multi-colour edges
def case_asymmetric(orc, lib, tmp):
    k = 11
    rng = random.Random(21)
    # (a) a successor that does not declare the edge back: v2 names another predecessor, so its in-degree is 2
    vs = strand_path(rng, k, 5, 1)
    x = next(b for b in "ACGT" if b != vs[1][0]) + vs[2][:-1]
    tb = Tab(k)
    for i, v in enumerate(vs):
        tb.add(v, 1 if 1 <= i <= 3 else 0)
    tb.edge(vs[0], vs[1]); tb.edge(vs[1], vs[2], declare="a"); tb.edge(x, vs[2], declare="b"); tb.edge(vs[2], vs[3]); tb.edge(vs[3], vs[4])
    t, exp = check(lib, tb.write(tmp, "asym_a"), covered=COV0, tag="asym a")
    assert exp[:4] == (sorted([t["index"][vs[1]], t["index"][vs[2]]]), 3, 3, 2), exp      # starts: v0, x and rc(v4), whose chain ends at rc(v2): two successors
    # (b) a predecessor edge declared only by the neighbour: v1 names v0 while v0 (in S) names another successor, so v0's out-degree is 2
    vs = strand_path(rng, k, 6, 1)
    y = vs[1][1:] + next(b for b in "ACGT" if b != vs[2][-1])
    tb = Tab(k)
    for i, v in enumerate(vs):
        tb.add(v, 1 if 1 <= i <= 4 else 0)
    tb.edge(vs[0], vs[1]); tb.edge(vs[1], y, declare="a"); tb.edge(vs[1], vs[2], declare="b"); tb.path(vs[2:])
    t, exp = check(lib, tb.write(tmp, "asym_b"), covered=COV0, tag="asym b")
    assert t["index"][vs[1]] not in exp[0], exp               # the chain from v0 ends at v1: two vertices
    # (c) two covered colours with different single in-edges: the union is 2, the vertex's in-degree is 2
    vs = strand_path(rng, k, 5, 1)
    z = next(b for b in "ACGT" if b != vs[0][0]) + vs[1][:-1]
    tb = Tab(k, 2)
    for i, v in enumerate(vs):
        tb.add(v, [1, 1] if 1 <= i <= 3 else [0, 0])
    tb.edge(vs[0], vs[1], colours=[0]); tb.edge(z, vs[1], colours=[1]); tb.path(vs[1:])
    t, exp = check(lib, tb.write(tmp, "asym_c"), tag="asym c")
    # every clause off: v0 and v4, records without coverage, are in S and declare nothing.  v0 and z start chains of 5 through v1; rc(v4)
    # starts one that ends at rc(v1), which has two successors: 4 vertices
    assert singly_connected(t, t["index"][vs[1]]) and exp[:4] == (sorted([t["index"][vs[1]], t["index"][vs[3]]]), 5, 3, 2), exp


def case_out_two(orc, lib, tmp):
    """an out-set of 2 ends a chain after exactly 3 vertices (no seed) and after exactly 4 (a seed)"""
    k = 11
    rng = random.Random(22)
    for n, good in ((3, False), (4, True)):
        vs = strand_path(rng, k, n + 2, 1)                     # v0 .. v_{n-1} is the chain; v_{n-1} has a second successor w
        w = vs[n - 1][1:] + next(b for b in "ACGT" if b != vs[n][-1])
        tb = Tab(k)
        for i, v in enumerate(vs):
            tb.add(v, 1 if 1 <= i <= n else 0)
        tb.add(w, 1)
        tb.path(vs)
        tb.edge(vs[n - 1], w, declare="b"); tb.edge(w, w[1:] + "A", declare="a")
        t, exp = check(lib, tb.write(tmp, "out2_%d" % n), covered=COV0, tag="out two %d" % n)
        assert (t["index"][vs[1]] in exp[0]) == good, exp


# ---------------------------------------------------------------- repeats
def case_repeats(orc, lib, tmp):
    k = 11
    # a homopolymer self loop reached from a start: s -> x -> x
    x = "A" * k
    tb = Tab(k)
    tb.add(x, 1); tb.add("C" + x[:-1], 0)
    tb.edge("C" + x[:-1], x); tb.edge(x, x, declare="a")
    t, exp = check(lib, tb.write(tmp, "loop"), covered=COV0, tag="self loop")
    assert exp[:4] == ([], 1, 1, 0), exp                       # (the reverse strand's vertex T..T has two successors)
    # a two-vertex cycle of out-degree-one vertices entered after 1, 2 and 3 steps: 3, 4 and 5 vertices before the guard stops the walk;
    # and the self loop above entered after 1, 2 and 3 steps: 2, 3 and 4 vertices
    c0, c1 = "AC" * (k // 2) + "A", "CA" * (k // 2) + "C"
    for cyc, name in (([c0, c1], "cycle2"), ([x], "cycle1")):
        for steps in (1, 2, 3):
            tail = [cyc[0]]
            for _ in range(steps):
                tail.insert(0, next(b for b in "GT" if b + tail[0][:-1] not in cyc) + tail[0][:-1])
            tb = Tab(k)
            for v in tail[1:] + cyc:
                tb.add(v, 1)
            tb.add(tail[0], 0)
            tb.path(tail)
            for a, b in zip(cyc, cyc[1:]):
                tb.edge(a, b)
            tb.edge(cyc[-1], cyc[0], declare="a")              # (the cycle's first vertex names the tail as its one predecessor)
            t, exp = check(lib, tb.write(tmp, "%s_%d" % (name, steps)), covered=COV0, tag="%s %d" % (name, steps))
            fwd_good = t["index"][canonical(tail[1])] in exp[0]
            assert fwd_good == (steps + len(cyc) > 3), (name, steps, exp)
    # even-k palindromes (one vertex for both strands): as a start's neighbour, and inside a chain
    k = 32
    rng = random.Random(23)
    half = rand_seq(rng, k // 2)
    q = half + revcomp(half)
    for lead in (1, 2):
        s = rand_seq(rng, lead) + q + rand_seq(rng, 3)
        vs = windows(s, k)
        assert vs[lead] == q and len({canonical(v) for v in vs}) == len(vs)
        tb = Tab(k)
        for i, v in enumerate(vs):
            tb.add(v, 1 if 1 <= i < len(vs) - 1 else 0)
        tb.path(vs)
        t, exp = check(lib, tb.write(tmp, "pal_%d" % lead), covered=COV0, tag="palindrome %d" % lead)
        assert singly_connected(t, t["index"][q]) and exp[2] >= 1, exp


# ---------------------------------------------------------------- widths: an SNV family under ComputeAssemblyQuality's filter
WIDTH_K = [5, 31, 32, 33, 47, 63, 65, 97]
QUALITY = dict(all_zero=(1,), covered=[((0,), 1, 1)])


def snv_family(k, L=None, seed=None):
    """a random parent and a child with one substitution every 97 bases, at least 100 from either end -> (parent, child, substitutions)"""
    # k = 97: the substituted windows of neighbouring sites touch, one chain per strand is all there is, so 2 m - 8 <= 2 needs m <= 5;
    # k = 5: the 512 canonical 5-mers leave a child no k-mer of its own in a long parent, so the sequence is kept short (one site), and
    # drawn so that the yardstick finds the site's two seeds (it finds none in the first draw: a neighbour occurs twice)
    L = L or {5: 240, 97: 600}.get(k, 1200)
    seed = {5: 6}.get(k, 0) if seed is None else seed
    rng = random.Random(1000 + k + seed)
    parent = rand_seq(rng, L)
    child = list(parent)
    sites = list(range(100, L - 100 + 1, 97))
    for p in sites:
        child[p] = rng.choice([b for b in "ACGT" if b != parent[p]])
    return parent, "".join(child), len(sites)


def family_ctx(orc, tmp, k, name, parent, child):
    """colour 0: the child (the evaluated assembly), colour 1: the parent"""
    p = str(tmp / (name + ".ctx"))
    orc.build_graph(p, [("child", [child]), ("parent", [parent])], k)
    return p


def occ_unique(seqs, colour=-1):
    def make(g, held):
        th = g.thread(seqs)
        held.append(th)
        occ = th.occurrences()
        held.append(occ)
        return [(colour, occ)]
    return make


def case_widths(orc, lib, tmp, k):
    parent, child, m = snv_family(k)
    p = family_ctx(orc, tmp, k, "snv%d" % k, parent, child)
    t = table(p)
    count, _ = count_occurrences(t, [child])
    t, exp = check(lib, p, unique=[(-1, count == 1)], unique_lib=occ_unique([child]), tag="widths k%d" % k, **QUALITY)
    assert exp[3] >= max(2, 2 * m - 8), (k, m, exp[1:4])      # an input that yields no seed cannot pass silently
    assert exp[1] >= k or k == 5, (k, exp[1:4])


# ---------------------------------------------------------------- chunk edges
CHUNK_N = [1, 2, 3, 63, 64, 65, 4095, 4096, 4097]


def case_chunks(orc, lib, tmp, N):
    """tables of N records, every record on one path, two of every 37 without coverage (the chains end there), S reaching into the last
    record.  N <= 2 still produces seeds: membership is by value, findRecord's quirk Q1 has no part in it"""
    k = 21
    for seed in range(50):
        rng = random.Random(N * 100 + seed)
        vs = windows(rand_seq(rng, N + k + 1), k)              # w0 and w_{N+1} are no records
        tb = Tab(k)
        for i, v in enumerate(vs[1:-1]):
            tb.add(v, 0 if i % 37 >= 35 else 1)
        if len(tb.rec) != N or tb.rec[max(tb.rec)][0][0] == 0:
            continue
        tb.path(vs)
        break
    t, exp = check(lib, tb.write(tmp, "chunk%d" % N), covered=COV0, tag="chunk %d" % N)
    assert t["N"] == N and N - 1 in exp[4] and exp[1] == sum(1 for i in range(N) if i % 37 < 35) and exp[2] >= 2, exp[1:4]
    if N == 2:
        assert exp[3] == 2, exp
    if N >= 63:
        assert exp[3] >= 2 * (N // 37), exp[1:4]


# ---------------------------------------------------------------- filter clauses
CLAUSE_K = 15


def clause_seq(n, seed):
    return rand_seq(random.Random(seed), n + CLAUSE_K + 1)


def clause_table(tmp, name, C, n, seed):
    """n records along one sequence, the path's edges in every colour, coverages drawn per colour from 0, 1, 5 and 0x80000000"""
    k = CLAUSE_K
    rng = random.Random(seed + 1000)
    vs = windows(clause_seq(n, seed), k)
    tb = Tab(k, C)
    vals = [0, 1, 1, 5, NEG]
    for v in vs[1:-1]:
        tb.add(v, [rng.choice(vals) for _ in range(C)])
    tb.path(vs)
    return tb.write(tmp, name)


def inheritance_sets(C, num_children):
    """(ref, parents, drafts, children) colours of a C-colour graph with that many children"""
    sets = {(2, 0): (0, [0], [1]), (3, 1): (1, [0], [1]), (9, 2): (4, [0, 1, 5], [2, 3, 6]), (9, 4): (4, [0, 1], [2, 3]),
            (3, 0): (2, [0], [1]), (9, 1): (4, [0, 1, 5], [2, 3, 6, 7]), (9, 0): (4, [0, 1, 5, 7], [2, 3, 6, 8])}
    ref, parents, drafts = sets[(C, num_children)]
    children = [c for c in range(C) if c not in parents and c not in drafts and c != ref]
    assert len(children) == num_children
    return ref, parents, drafts, children


def java_inheritance_pass(t, r, ref, parents, drafts, uniq):
    """isSinglyConnected && isSharedWithOnlyOneParent && isSharedWithSomeChildren && hasUniqueCoordinates (ComputeInheritance.java:338-404)"""
    v = t["cov"][r]
    if not singly_connected(t, r):
        return False
    if sum(1 for c in parents if v[c] > 0) != 1 or sum(1 for c in drafts if v[c] > 0) != 1:
        return False
    ignore = set(parents) | set(drafts) | {ref}
    num_children = sum(1 for c in range(t["C"]) if c not in ignore)
    with_cov = sum(1 for c in range(t["C"]) if c not in ignore and v[c] > 0)
    if not (num_children == 1 or 1 < with_cov < num_children):
        return False
    draft = [c for c in drafts if v[c] > 0]
    return len(draft) == 1 and bool(uniq[draft[0]][r])


INHERITANCE = [(2, 0), (3, 1), (9, 2), (9, 4), (3, 0), (9, 1)]


def case_inheritance_clauses(orc, lib, tmp, C, num_children):
    """ComputeInheritance's mapping onto the clauses, unique by a caller's byte per record"""
    ref, parents, drafts, children = inheritance_sets(C, num_children)
    p = clause_table(tmp, "inh%d_%d" % (C, num_children), C, 600, 31 * C + num_children)
    t = table(p)
    rng = np.random.default_rng(C + num_children)
    uniq = {c: (rng.random(t["N"]) < 0.8).astype(np.uint8) * np.uint8(7) for c in drafts}
    S = [r for r in range(t["N"]) if java_inheritance_pass(t, r, ref, parents, drafts, uniq)]
    want = variant_seeds(t, S)
    covered = [(parents, 1, 1), (drafts, 1, 1)]
    if num_children != 1:
        covered.append((children, 2, num_children - 1) if children else ((0,), 1, 0))
    held = [upload(lib, uniq[c]) for c in drafts]
    g = CortexGraph(p, lib=lib)
    with g.variant_seeds(covered=covered, unique=[(c, h[1]) for c, h in zip(drafts, held)]) as sel:
        compare(sel, want + (S,), "inheritance %d %d" % (C, num_children))
    g.close()
    del held
    assert (len(S) > 0) == (num_children in (1, 4)), (C, num_children, len(S))      # 0 and 2 children: 1 < n < numChildren has no solution
    # the same sets through the command's own derivation
    names = ["s%d" % c for c in range(C)]
    cmd = ComputeInheritance(None, {names[c]: [] for c in drafts}, [names[c] for c in parents], [names[c] for c in children], names[ref])
    cmd.GRAPH = g2 = CortexGraph(p, lib=lib)
    assert cmd.colours() == (ref, parents, drafts, children)
    g2.close()


def case_clauses(orc, lib, tmp):
    """a stored 0x80000000 in a clause colour and in an all_zero colour; at_least > at_most; unique by occurrences with k-mers that
    occur 0, 1 and 2 times, once per strand and across two sequences; unique by bytes; an entry whose colour is not covered"""
    p = clause_table(tmp, "clauses", 3, 900, 5)
    t = table(p)
    neg_zero = [r for r in range(t["N"]) if np.uint32(t["cov"][r, 2]) == NEG and filter_pass(t, r, covered=[((0, 1), 1, 2)])]
    neg_clause = [r for r in range(t["N"]) if np.uint32(t["cov"][r, 1]) == NEG and t["cov"][r, 0] > 0 and singly_connected(t, r)]
    assert len(neg_zero) > 5 and len(neg_clause) > 5
    _, exp = check(lib, p, all_zero=(2,), covered=[((0, 1), 1, 2)], tag="0x80000000 is neither > 0 nor == 0")
    assert not set(neg_zero) & set(exp[4]) and exp[1] > 20
    _, exp = check(lib, p, covered=[((0, 1), 2, 2)], tag="covered twice")
    assert not set(neg_clause) & set(exp[4]) and exp[1] > 20
    _, exp = check(lib, p, covered=[((0,), 1, 1), ((1,), 2, 1)], tag="at_least > at_most")
    assert exp[:4] == ([], 0, 0, 0)
    _, exp = check(lib, p, tag="every clause off")
    assert exp[1] > 100
    # occurrences: the records' own sequence once; a stretch again forward, a stretch as its reverse complement, a stretch in a second sequence
    k = t["k"]
    rng = random.Random(6)
    walk = clause_seq(900, 5)
    seqs = [walk[:700] + "N" + walk[100:160], revcomp(walk[300:360]), walk[500:540] + rand_seq(rng, 30)]
    count, first = count_occurrences(t, seqs)
    assert {0, 1, 2} <= set(count.tolist()) and count.max() == 2
    for colour in (-1, 0, 2):
        _, exp = check(lib, p, covered=[((0, 1), 1, 2)], unique=[(colour, count == 1)], unique_lib=occ_unique(seqs, colour), tag="unique by occurrences %d" % colour)
        assert 5 < exp[1]
    everything = expect(t, covered=[((0, 1), 1, 2)])
    only0 = expect(t, covered=[((0, 1), 1, 2)], unique=[(0, count == 1)])
    always = expect(t, covered=[((0, 1), 1, 2)], unique=[(-1, count == 1)])
    assert always[1] < only0[1] < everything[1]                # an entry whose colour is not covered is ignored
    bytes_ = (np.arange(t["N"]) % 3 != 0).astype(np.uint8) * np.uint8(0x80)
    held = upload(lib, bytes_)
    _, exp = check(lib, p, covered=[((0, 1), 1, 2)], unique=[(1, bytes_)], unique_lib=lambda g, h: [(1, held[1])], tag="unique by bytes")
    assert exp[1] < everything[1]
    del held


# ---------------------------------------------------------------- occurrences
def check_occurrences(lib, path, seqs, quirk=False, tag=""):
    t = table(path)
    count, first = count_occurrences(t, seqs, quirk)
    g = CortexGraph(path, lib=lib)
    with Threading(g, None, seqs, find_quirk=quirk) as th, th.occurrences() as occ:
        assert occ.n_records == t["N"]
        got_c, got_f = occ.get()
        assert (got_c == count).all() and (got_f == first).all(), (tag, np.nonzero(got_c != count)[0][:5], np.nonzero(got_f != first)[0][:5])
        assert (occ.count == count).all() and (occ.first == first).all()
        if t["N"] > 2:
            c2, f2 = occ.get(1, t["N"] - 2)
            assert (c2 == count[1:-1]).all() and (f2 == first[1:-1]).all()
            hc, pc = upload(lib, np.full(t["N"], 77, dtype=np.uint32))
            hf, pf = upload(lib, np.full(t["N"], 77, dtype=np.int64))
            occ.get_dev(pc, pf)
            back = [x if lib.is_hostsim else x.cpu().numpy() for x in (hc, hf)]
            assert (back[0] == count).all() and (back[1] == first).all(), tag
        hit = [r for r in range(t["N"]) if count[r]][:40] + [r for r in range(t["N"]) if not count[r]][:3]
        win_start = np.cumsum([0] + [max(0, len(s) - t["k"] + 1) for s in seqs])
        for r, (si, off, flipped) in zip(hit, occ.positions(hit)):
            if count[r] == 0:
                assert (si, off, flipped) == (-1, -1, False)
                continue
            assert win_start[si] + off == first[r], tag
            sk = seqs[si][off:off + t["k"]]
            assert canonical(sk) == t["strs"][r] and flipped == (sk != t["strs"][r])
    g.close()
    return count, first


def case_occurrences(orc, lib, tmp):
    k = 21
    rng = random.Random(31)
    a = rand_seq(rng, 300)
    b = a[40:140] + rand_seq(rng, 50) + revcomp(a[60:120])     # a's k-mers again forward and on the other strand
    c = a[:120] + "N" + a[121:200] + a[150:180].lower()        # invalid windows in front of and behind valid ones
    t = Tab(k)
    for w in windows(a, k)[::2] + windows(rand_seq(rng, 80), k):
        t.add(w, 1)
    p = t.write(tmp, "occ")
    count, first = check_occurrences(lib, p, [a, b, c, "", "ACGT"], tag="occurrences")
    assert count.max() >= 4 and (count == 0).any() and (first[count > 0] < 300).all()
    # a 4097-window sequence
    s = rand_seq(rng, 4097 + k - 1)
    s = s[:4000] + s[100:200] + s[4100:]
    t = Tab(k)
    for w in windows(s, k)[::3] + [s[-k:]]:
        t.add(w, 1)
    count, first = check_occurrences(lib, t.write(tmp, "occ4097"), [s], tag="4097 windows")
    assert first.max() == 4096 and count.max() == 2
    # the quirk flag on a graph of two records: rec is taken as the threading has it
    t = Tab(k)
    t.add(a[:k], 1); t.add(a[5:5 + k], 1)
    p2 = t.write(tmp, "occ2")
    count, _ = check_occurrences(lib, p2, [a], quirk=True, tag="quirk")
    assert count.sum() == 0
    count, _ = check_occurrences(lib, p2, [a], quirk=False, tag="no quirk")
    assert count.tolist() == [1, 1]


# ---------------------------------------------------------------- the commands
def case_quality(orc, lib, tmp):
    k = 31
    parent, child, m = snv_family(k)
    pe, pc = str(tmp / "eval.ctx"), str(tmp / "comp.ctx")
    orc.build_graph(pe, [("child", [child])], k)
    orc.build_graph(pc, [("parent", [parent])], k)
    t = table(family_ctx(orc, tmp, k, "joined_by_hand", parent, child))
    count, _ = count_occurrences(t, [child[:700], child[650:]])
    exp = expect(t, unique=[(-1, count == 1)], **QUALITY)
    fa = write_fasta(tmp / "eval.fa", [("chr1 first", child[:700]), ("chr2", child[650:])], width=60)
    cmd = ComputeAssemblyQuality(pe, pc, fa, out=tmp / "q.txt", lib=lib)
    q = cmd.execute()
    bases = 700 + len(child) - 650
    assert (cmd.n_seeds, cmd.n_unique, cmd.n_good, cmd.numBases) == (exp[1], exp[2], exp[3], bases)
    assert exp[3] >= 2 * m - 8 - 4                             # (the 50 bases both sequences hold occur twice: the sites there are no seeds)
    want = -10 * math.log10(exp[3] / bases)
    assert q == want and (tmp / "q.txt").read_text() == repr(want) + "\n"
    # no seed: the assembly against itself
    cmd = ComputeAssemblyQuality(pe, pe, [("c", child)], out=tmp / "inf.txt", lib=lib)
    assert cmd.execute() == math.inf and cmd.n_good == 0 and (tmp / "inf.txt").read_text() == "Infinity\n"


def case_inheritance_command(orc, lib, tmp):
    """two parents, their two draft assemblies, three children, a reference sample: the seeds against the yardstick run with the Java
    predicate written out"""
    k = 21
    rng = random.Random(41)
    p1 = rand_seq(rng, 1600)
    p2 = list(p1)
    for s in range(120, 1500, 110):
        p2[s] = rng.choice([b for b in "ACGT" if b != p1[s]])
    p2 = "".join(p2)
    h = 800
    kids = [p1[:h] + p2[h:], p2[:h] + p1[h:], p1]
    samples = [("ref", [p1]), ("mom", [p1]), ("dad", [p2]), ("mom_asm", [p1]), ("dad_asm", [p2]), ("k1", [kids[0]]), ("k2", [kids[1]]), ("k3", [kids[2]])]
    p = str(tmp / "pedigree.ctx")
    orc.build_graph(p, samples, k)
    t = table(p)
    ref, parents, drafts = 0, [1, 2], [3, 4]
    uniq = {3: count_occurrences(t, [p1])[0] == 1, 4: count_occurrences(t, [p2])[0] == 1}
    S = [r for r in range(t["N"]) if java_inheritance_pass(t, r, ref, parents, drafts, uniq)]
    want = variant_seeds(t, S)
    assert want[3] >= 10, want[1:]
    g = CortexGraph(p, lib=lib)
    cmd = ComputeInheritance(g, {"mom_asm": [("m", p1)], "dad_asm": write_fasta(tmp / "dad.fa", [("d", p2)], width=70)}, {"mother": "mom", "father": "dad"}, {"k1", "k2", "k3"}, "ref")
    assert cmd.colours() == (ref, parents, drafts, [5, 6, 7])
    with cmd.variant_seeds() as sel:
        compare(sel, want + (S,), "pedigree")
    try:
        cmd.execute()
        raise AssertionError("execute() ran")
    except NotImplementedError as e:
        assert "callVariants" in str(e)
    g.close()


# ---------------------------------------------------------------- refused inputs
def _refused(fn, status, word):
    try:
        fn()
    except ca.LdbgError as e:
        assert e.status == status and word in str(e), e
        return
    raise AssertionError("not refused")


def case_refused(orc, lib, tmp):
    p = clause_table(tmp, "refused", 3, 50, 1)
    q = clause_table(tmp, "refused_other", 3, 50, 2)
    g, other = CortexGraph(p, lib=lib), CortexGraph(q, lib=lib)
    _refused(lambda: g.variant_seeds(all_zero=(3,)), 6, "colour")
    _refused(lambda: g.variant_seeds(covered=[((0, 40), 1, 1)]), 6, "colour")
    bytes_ = upload(lib, np.ones(50, dtype=np.uint8))
    _refused(lambda: g.variant_seeds(unique=[(3, bytes_[1])]), 6, "colour")
    _refused(lambda: g.variant_seeds(unique=[(-2, bytes_[1])]), 6, "colour")
    _refused(lambda: g.variant_seeds(covered=[((0,), 1, 1)] * 4), 6, "more clauses")
    _refused(lambda: g.variant_seeds(unique=[(-1, bytes_[1])] * 9), 6, "more clauses")
    with other.thread(["ACGT" * 20]) as th, th.occurrences() as occ:
        _refused(lambda: g.variant_seeds(unique=[(-1, occ)]), 6, "another graph")
    with Threading(None, other, ["ACGT" * 20]) as th:          # a threading made without a graph
        _refused(lambda: th.occurrences(), 6, "without a graph")
    # the raw entry: a NULL filter, counts beyond the arrays, an entry with neither input and with both
    h, cn = C.c_void_p(), _native.SeedCounts()

    def raw(f):
        st = lib.dll.ldbg_graph_variant_seeds(g._h, C.byref(f) if f is not None else None, C.byref(h), C.byref(cn))
        assert h.value is None
        return st, lib.dll.ldbg_last_error().decode()
    assert raw(None)[0] == 6 and "null filter" in raw(None)[1]
    f = _native.SeedFilter()
    f.n_covered = 4
    assert raw(f)[0] == 6 and "covered" in raw(f)[1]
    f.n_covered, f.n_unique = 0, 9
    assert raw(f)[0] == 6 and "unique" in raw(f)[1]
    f.n_unique = 1
    f.unique[0].colour = -1
    assert raw(f)[0] == 6 and "neither or both" in raw(f)[1]
    with g.thread(["ACGT" * 20]) as th, th.occurrences() as occ:
        f.unique[0].occurrences, f.unique[0].d_unique = occ._h, bytes_[1]
        assert raw(f)[0] == 6 and "neither or both" in raw(f)[1]
        rc._refused(lambda: occ.get(0, 51), 6)
        rc._refused(lambda: occ.get(-1, 2), 6)
    # a collection; one rank's part of a hash-sharded table, and its image
    cc = CortexCollection(p, q, lib=lib)
    _refused(lambda: cc.variant_seeds(), 4, "collection")
    cc.close()
    lib.check(lib.dll.ldbg_graph_set_shard(g._h, 1))
    _refused(lambda: g.variant_seeds(), 4, "hash-sharded")
    img, ig = C.c_void_p(), C.c_void_p()
    lib.check(lib.dll.ldbg_image_create(g._h, C.c_int64(64), C.c_int64(100), C.byref(img)))
    lib.check(lib.dll.ldbg_image_graph(img, C.byref(ig)))
    _refused(lambda: CortexGraph._from_handle(ig, lib, "#image").variant_seeds(), 4, "image")
    lib.check(lib.dll.ldbg_image_destroy(img))
    lib.check(lib.dll.ldbg_graph_set_shard(g._h, 0))
    # an empty S and an empty table are no errors
    with g.variant_seeds(covered=[((0,), 1, 0)]) as sel:
        assert (sel.count, sel.n_seeds, sel.n_unique, sel.n_good) == (0, 0, 0, 0) and sel.indices().tolist() == []
    del bytes_
    other.close()
    g.close()
