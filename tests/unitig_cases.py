"""Unitig cases shared by the host-simulation run (tests/test_unitigs_hostsim.py) and the GPU run (tests/test_gpu_unitigs.py).

The yardstick is written here in plain Python from the definition in DESIGN.md §10, over the records as the CPU oracle reads them
(Graph.record_string); its ToGfa1 restates J/commands/utils/ToGfa1.java:37-145 line by line.  The product (ldbg_graph_unitigs and
the writers behind it) must match it byte for byte."""
import os
import random

import numpy as np

import corticall_amd as ca
from corticall_amd import CortexCollection, CortexGraph, ToGfa1
from tests.parity_cases import GOLDEN, genome_with_repeats, mutate, rand_seq

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    return min(s, rc(s))


def java_int(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def java_hash(s):
    """java.util.Arrays.hashCode(byte[]) as a Java int"""
    h = 1
    for ch in s.encode():
        h = (31 * h + ch) & 0xFFFFFFFF
    return java_int(h)


def java_float_to_int(f):
    f = np.float32(f)
    if np.isnan(f):
        return 0
    if f >= np.float32(2 ** 31):
        return 2 ** 31 - 1
    if f <= np.float32(-2 ** 31):
        return -2 ** 31
    return int(f)


class Yardstick:
    """the records of a graph as the oracle reads them: k-mer -> (record number, coverages (Java int), in bases, out bases per colour)"""

    def __init__(self, og):
        self.k, self.C = og.k, og.C
        self.recs = {}
        self.kmers = []
        for i in range(og.N):
            parts = og.record_string(i).split()
            kmer, cov, ed = parts[0], [int(x) for x in parts[1:1 + og.C]], parts[1 + og.C:]
            ins = [{b.upper() for b in e[:4] if b != "."} for e in ed]
            outs = [{b for b in e[4:] if b != "."} for e in ed]
            self.recs[kmer] = (i, cov, ins, outs)
            self.kmers.append(kmer)

    def rec(self, ck):
        """crs.get(canonical k-mer): (record number, coverages, in bases, out bases per colour) or None"""
        return self.recs.get(ck)

    # ---- the definition
    def is_vertex(self, s, S):
        r = self.rec(canon(s))
        return r is not None and any(r[1][c] != 0 for c in S)

    def adj(self, s, S, forward):
        """out(s) / in(s): the k-mers the edge bytes of s's record, ORed over S, name from s as it reads (present or not)"""
        _, _, ins, outs = self.rec(canon(s))
        I = set().union(*[ins[c] for c in S])
        O = set().union(*[outs[c] for c in S])
        flipped = s != canon(s)
        if forward:
            bases = {b.translate(_COMP) for b in I} if flipped else O
            return {s[1:] + b for b in bases}
        bases = {b.translate(_COMP) for b in O} if flipped else I
        return {b + s[:-1] for b in bases}

    def unitig_edge(self, x, S):
        o = self.adj(x, S, True)
        if len(o) != 1:
            return None
        y = next(iter(o))
        if not self.is_vertex(y, S) or self.adj(y, S, False) != {x}:
            return None
        if canon(x) == canon(y) or x == rc(x) or y == rc(y):
            return None
        return y

    def unitigs(self, S):
        verts = [s for kmer in self.kmers for s in (kmer, rc(kmer)) if self.is_vertex(s, S)]
        succ = {x: self.unitig_edge(x, S) for x in verts}
        pred = {y: x for x, y in succ.items() if y is not None}
        out, done = set(), set()
        for x in verts:                                    # maximal paths: from every vertex without a predecessor
            if x in pred:
                continue
            path = [x]
            while succ[path[-1]] is not None:
                path.append(succ[path[-1]])
            done.update(path)
            seq = path[0] + "".join(p[-1] for p in path[1:])
            out.add(min(seq, rc(seq)))
        for x in verts:                                    # pure cycles
            if x in done:
                continue
            cyc = [x]
            while succ[cyc[-1]] != x:
                cyc.append(succ[cyc[-1]])
            done.update(cyc)
            m = min(canon(c) for c in cyc)
            if m not in cyc:
                continue                                   # the mirror copy holds it
            i = cyc.index(m)
            path = cyc[i:] + cyc[:i]
            seq = path[0] + "".join(p[-1] for p in path[1:])
            assert seq <= rc(seq)
            out.add(seq)
        return sorted(out, key=lambda s: self.rec(canon(s[:self.k]))[0])

    def coverage(self, seq):
        k = self.k
        return [sum(self.rec(canon(seq[i:i + k]))[1][c] for i in range(len(seq) - k + 1)) & 0xFFFFFFFF for c in range(self.C)]

    # ---- ToGfa1.execute, J/commands/utils/ToGfa1.java:37-145
    def to_gfa1(self, seqs, sample_color=0, plus=":"):
        k = self.k
        g_vertices, g_edges = {}, {}                       # DefaultDirectedGraph: LinkedHashMap-backed vertex and edge sets
        beginning, ending, seq_names, positive = {}, {}, {}, {}
        for index, rseq in enumerate(seqs):                # :52-69
            for v in (rseq, rc(rseq)):
                g_vertices.setdefault(v, None)
                beginning[v[:k]] = v
                ending[v[len(v) - k:]] = v
                seq_names[v] = index
            positive[rseq] = True
            positive[rc(rseq)] = False
        averages = {}
        for v in list(g_vertices):                         # :75-126
            cov = 0
            for i in range(len(v) - k + 1):
                r = self.rec(canon(v[i:i + k]))
                if r is not None:
                    cov = java_int(cov + r[1][sample_color])
            averages[v] = java_float_to_int(np.float32(cov) / np.float32(len(v) - k + 1))
            bsk = v[:k]
            for x in self.hashset(self.prev_kmers(bsk, sample_color)):
                if x in ending:
                    g_edges.setdefault((ending[x], v), None)
            esk = v[len(v) - k:]
            for x in self.hashset(self.next_kmers(esk, sample_color)):
                if x in beginning:
                    g_edges.setdefault((v, beginning[x]), None)
        lines = ["H\tVN:Z:1.0"]
        seen = set()
        for v in g_vertices:                               # :130-141
            vid = seq_names[v]
            if vid not in seen:
                av = averages[v]
                lines.append("S\t%d\t%s\tRC:i:%d\tAC:i:%d" % (vid, v, java_int(av * len(v)), av))
                seen.add(vid)
        for vs, vt in g_edges:                             # :143-154
            lines.append("L\t%d\t%s\t%d\t%s\t%dM" % (seq_names[vs], plus if positive[vs] else "-", seq_names[vt], plus if positive[vt] else "-", k))
        return "".join(x + "\n" for x in lines)

    def _edges(self, sk, c):
        _, _, ins, outs = self.rec(canon(sk))              # crs.get: a missing k-mer is a NullPointerException in ToGfa1
        return sk != canon(sk), ins[c], outs[c]

    @staticmethod
    def _byte_set(bases):
        """new HashSet<>(Collection<Byte>): 16 buckets by the byte value, A C T G"""
        return sorted(bases, key=lambda b: (ord(b) ^ (ord(b) >> 16)) & 15)

    def prev_kmers(self, sk, c):                           # TraversalUtils.getAllPrevKmers :510-531 with getInEdges :560-574
        flipped, ins, outs = self._edges(sk, c)
        bases = {b.translate(_COMP) for b in outs} if flipped else ins
        return [b + sk[:-1] for b in self._byte_set(bases)]

    def next_kmers(self, sk, c):                           # getAllNextKmers :533-557 with getOutEdges :576-590
        flipped, ins, outs = self._edges(sk, c)
        bases = {b.translate(_COMP) for b in ins} if flipped else outs
        return [sk[1:] + b for b in self._byte_set(bases)]

    @staticmethod
    def hashset(kmers):
        """iteration order of a HashSet<CortexByteKmer> of at most 12 keys filled in this order"""
        def bucket(s):
            h = java_hash(s) & 0xFFFFFFFF
            return (h ^ (h >> 16)) & 15
        return sorted(kmers, key=bucket)



class LazyYardstick(Yardstick):
    """the yardstick over a large graph: records looked up one by one with the oracle's findRecord, for a sample of unitigs"""

    def __init__(self, og):
        self.og, self.k, self.C, self.cache = og, og.k, og.C, {}

    def rec(self, ck):
        if ck not in self.cache:
            i, cov, ed = self.og.find(ck)
            self.cache[ck] = None if i < 0 else (i, cov, [{b for j, b in enumerate("ACGT") if (e >> 4) & (1 << (3 - j))} for e in ed],
                                                 [{b for j, b in enumerate("ACGT") if e & (1 << j)} for e in ed])
        return self.cache[ck]


def check_unitig(y, s, S):
    """one unitig against the definition: every k-mer a vertex, consecutive k-mers joined by unitig edges, both ends maximal (or a
    pure cycle cut at its smallest canonical k-mer), the lowest orientation"""
    k = y.k
    kms = [s[i:i + k] for i in range(len(s) - k + 1)]
    assert all(y.is_vertex(x, S) for x in kms)
    for a, b in zip(kms, kms[1:]):
        assert y.unitig_edge(a, S) == b, (s, a, b)
    nxt = y.unitig_edge(kms[-1], S)
    prv = [x for x in y.adj(kms[0], S, False) if y.is_vertex(x, S) and y.unitig_edge(x, S) == kms[0]]
    if nxt is None:
        assert not prv, s
        assert s <= rc(s)
    else:                                                  # a pure cycle: closes on itself, cut at its smallest canonical k-mer
        assert nxt == kms[0] and prv == [kms[-1]], s
        assert kms[0] == min(canon(x) for x in kms), s

def fasta_text(seqs):
    return "".join(">%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def check_graph(orc, lib, tmp, path, color_sets, og=None, gfa_colors=None):
    """the product against the yardstick for every colour set: sequences, FASTA, GFA (sample colour: each colour of the graph),
    coverage, labels, determinism, and ToGfa1 over the product's own FASTA"""
    og = og or orc.Graph(path)
    y = Yardstick(og)
    g = CortexGraph(path, lib=lib)
    k = g.getKmerSize()
    for S in color_sets:
        exp = y.unitigs(S)
        u = g.unitigs(S)
        got = u.sequences()
        assert got == exp, (S, len(got), len(exp), [s for s in got if s not in exp][:3], [s for s in exp if s not in got][:3])
        assert list(u) == exp and len(u) == len(exp)
        assert u.total_bases == sum(len(s) for s in exp) and u.longest == max([len(s) for s in exp], default=0)
        # coverage, every colour
        cov = u.coverages()
        assert cov.tolist() == [y.coverage(s) for s in exp]
        # every member record in exactly one unitig at one position; non-members -1; the spelled k-mers round-trip
        uid, pos, ori = u.of_records(np.arange(og.N))
        for r, kmer in enumerate(y.kmers):
            if not y.is_vertex(kmer, S):
                assert uid[r] == -1 and pos[r] == -1 and ori[r] == -1, (r, kmer)
                continue
            s = exp[uid[r]][pos[r]:pos[r] + k]
            assert s == (rc(kmer) if ori[r] else kmer), (r, kmer, s)
        n_members = sum(1 for kmer in y.kmers if y.is_vertex(kmer, S))
        assert sum(len(s) - k + 1 for s in exp) == n_members
        # FASTA and GFA byte for byte
        fa = tmp / ("u_%s.fa" % "_".join(map(str, S)))
        u.write_fasta(fa)
        assert fa.read_text() == fasta_text(exp)
        for sc in (gfa_colors if gfa_colors is not None else range(og.C)):
            gp = tmp / ("u_%s_%d.gfa" % ("_".join(map(str, S)), sc))
            u.write_gfa1(gp, sc)
            assert gp.read_text() == y.to_gfa1(exp, sc), (S, sc)
            u.write_gfa1(gp, sc, plus_strand=True)
            assert gp.read_text() == y.to_gfa1(exp, sc, plus="+"), (S, sc)
        # ToGfa1 given the product's FASTA (the reference semantics over find_batch) writes what the device path writes
        tp, gp = tmp / "togfa1_fasta.gfa", tmp / "u0.gfa"
        ToGfa1(g, tp, FASTA=fa).execute()
        u.write_gfa1(gp, 0)
        assert tp.read_text() == gp.read_text(), S
        # two builds are identical
        u2 = g.unitigs(S)
        assert u2.sequences() == got and (u2.coverages() == cov).all() and all((a == b).all() for a, b in zip(u2.of_records(np.arange(og.N)), (uid, pos, ori)))
        u2.close()
        u.close()
    # ToGfa1 without a FASTA: the sample colour's unitigs built on the device
    tp = tmp / "togfa1.gfa"
    ToGfa1(g, tp).execute()
    assert tp.read_text() == y.to_gfa1(y.unitigs([0]), 0)
    g.close()
    return y


# ------------------------------------------------------------------ cases
CONTIG1 = "ACTATACGAAATAGGGCCACGATTTTTATTCAGAGCATACGATACAGAA"
CONTIG2 = "ACTGGGGGGCCACGACACTACGACTACAGCAACTACATGACCAGTACTCAGAGAGAAGCCCATAATAGGCGCGGCCC"


def case_fixture(orc, lib, tmp):
    """known answer: the reference's two_short_contigs.ctx (k = 31, two contigs without a shared k-mer, one per colour)"""
    path = os.path.join(GOLDEN, "two_short_contigs.ctx")
    g = CortexGraph(path, lib=lib)
    with g.unitigs([0]) as u:
        assert u.sequences() == [CONTIG1]
        gp = tmp / "c0.gfa"
        u.write_gfa1(gp, 0)
        assert gp.read_text() == "H\tVN:Z:1.0\nS\t0\t%s\tRC:i:49\tAC:i:1\n" % CONTIG1
    with g.unitigs([1]) as u:
        assert u.sequences() == [CONTIG2]
        gp = tmp / "c1.gfa"
        u.write_gfa1(gp, 1)
        assert gp.read_text() == "H\tVN:Z:1.0\nS\t0\t%s\tRC:i:77\tAC:i:1\n" % CONTIG2
    with g.unitigs([0, 1]) as u:
        assert sorted(u.sequences()) == sorted([CONTIG1, CONTIG2]) and len(u) == 2
    # ToGfa1 of colour 0 without a FASTA, and by sample name
    tp = tmp / "t.gfa"
    ToGfa1(g, tp).execute()
    assert tp.read_text() == "H\tVN:Z:1.0\nS\t0\t%s\tRC:i:49\tAC:i:1\n" % CONTIG1
    g.close()
    check_graph(orc, lib, tmp, path, [[0], [1], [0, 1]])


def _palindrome(rng, k):
    h = rand_seq(rng, k // 2)
    return h + rc(h)


def random_graph(orc, tmp, k, seed, ncol, kind):
    rng = random.Random(seed * 1000 + k)
    base = genome_with_repeats(rng, 260 + 6 * k, n_rep=3)
    haps = [[base]]
    if kind == "dense":                                    # many branches: haplotypes with many SNVs
        haps[0] += [mutate(rng, base, snv=0.05, indel=0.01) for _ in range(2)]
    if kind == "tandem":                                   # pure cycles: short units repeated, alone in a haplotype
        for _ in range(2):
            unit = rand_seq(rng, rng.randint(k // 2, k - 1))
            haps[0].append(unit * (3 + (2 * k) // len(unit)))
        haps[0][0] += unit * 3
    if k % 2 == 0:                                         # palindromes: alone and inside a haplotype
        p = _palindrome(rng, k)
        haps[0] += [rand_seq(rng, k) + p + rand_seq(rng, k), p]
    for _ in range(1, ncol):
        haps.append([mutate(rng, base, snv=0.02, indel=0.005)] + haps[0][1:2])
    path = str(tmp / ("r%d_%d_%s.ctx" % (k, seed, kind)))
    orc.build_graph(path, [("s%d" % i, h) for i, h in enumerate(haps)], k)
    return path


# (k, seed, colours, kind): even k for palindromes, tandem repeats for pure cycles, dense for branches
RANDOM_CASES = [(21, 1, 1, "tandem"), (21, 7, 3, "plain"), (31, 2, 2, "plain"), (31, 8, 1, "tandem"), (32, 3, 3, "dense"), (32, 9, 2, "tandem"),
                (47, 4, 2, "tandem"), (47, 10, 3, "dense"), (63, 5, 1, "dense"), (63, 11, 2, "tandem"), (64, 6, 3, "tandem"), (64, 12, 1, "dense")]


def color_sets(ncol):
    sets = [[c] for c in range(ncol)]
    if ncol > 1:
        sets += [list(range(ncol)), [ncol - 1, 0]]
    return sets


def many_color_sets(ncol):
    """the colour sets of a many-colour graph: the top colour alone, a pair that straddles the packed word of colours 0..3, every
    colour, and the top colour with colour 0 in that order"""
    return [[ncol - 1], [3, 4] if ncol > 4 else [2, 3], list(range(ncol)), [ncol - 1, 0]]


def case_random(orc, lib, tmp, k, seed, ncol, kind, sets=None, gfa_colors=None):
    """sets=None: color_sets(ncol), GFA for every colour of the graph"""
    path = random_graph(orc, tmp, k, seed, ncol, kind)
    y = check_graph(orc, lib, tmp, path, sets if sets is not None else color_sets(ncol), gfa_colors=gfa_colors)
    if sets is not None:      # the colours of the sets differ, or a build that took one for another would pass
        u = [y.unitigs(S) for S in sets]
        assert all(u[i] != u[j] for i in range(len(u)) for j in range(i)), "two colour sets with the same unitigs"
        assert max(len(s) for s in u[0]) > 3 * k


def case_hash_collisions(orc, lib, tmp):
    """graphs around the quirk-Q6 k-mers (tests/golden/hash_collisions.txt, built as parity_cases.case_hash_collision builds them):
    unitigs orient by string comparison, never by the Java hash"""
    rng = random.Random(5)
    for x in open(os.path.join(GOLDEN, "hash_collisions.txt")).read().split():
        k = len(x)
        xo = x if rng.random() < 0.5 else rc(x)
        h1 = rand_seq(rng, 3 * k) + xo + rand_seq(rng, 3 * k)
        h2 = rand_seq(rng, 2 * k) + h1[2 * k: 5 * k + 5] + rand_seq(rng, 2 * k)
        h3 = rand_seq(rng, k) + rc(xo) + rand_seq(rng, k)
        path = str(tmp / ("coll%d_%s.ctx" % (k, x[:6])))
        orc.build_graph(path, [("a", [h1, h2, h3]), ("b", [h1])], k)
        check_graph(orc, lib, tmp, path, [[0], [1], [0, 1]])


def case_tiny(orc, lib, tmp):
    """a table of two records: findRecord's quirk Q1 does not apply (ToGfa1 looks records up in a HashMap)"""
    p = str(tmp / "tiny.ctx")
    orc.build_graph(p, [("s", ["ACGTT"])], 4)
    check_graph(orc, lib, tmp, p, [[0]])


def case_collection_and_shard(orc, lib, tmp):
    """a collection answers like the joined table; one rank's part of a hash-sharded table is refused"""
    rng = random.Random(77)
    a, b = genome_with_repeats(rng, 400), genome_with_repeats(rng, 400)
    pa, pb = str(tmp / "ca.ctx"), str(tmp / "cb.ctx")
    orc.build_graph(pa, [("a", [a])], 31)
    orc.build_graph(pb, [("b", [b, a[50:200]])], 31)
    joined = str(tmp / "cab.ctx")
    ca.Join([pa, pb], joined, lib=lib).execute()
    gj = CortexGraph(joined, lib=lib)
    gc = CortexCollection(CortexGraph(pa, lib=lib), CortexGraph(pb, lib=lib), lib=lib)
    for S in ([0], [1], [0, 1]):
        with gj.unitigs(S) as uj, gc.unitigs(S) as uc:
            assert uc.sequences() == uj.sequences() and (uc.coverages() == uj.coverages()).all()
    y = Yardstick(orc.Graph(joined))
    with gc.unitigs([0, 1]) as uc:
        assert uc.sequences() == y.unitigs([0, 1])
    gc.close()
    lib.check(lib.dll.ldbg_graph_set_shard(gj._h, 1))
    try:
        gj.unitigs([0])
        raise AssertionError("a shard built unitigs")
    except ca.LdbgError as e:
        assert e.status == 4, e
    lib.check(lib.dll.ldbg_graph_set_shard(gj._h, 0))
    gj.close()


def case_bad_arguments(orc, lib, tmp):
    g = CortexGraph(os.path.join(GOLDEN, "two_short_contigs.ctx"), lib=lib)
    for cols in ([], [2], [-1]):
        try:
            g.unitigs(cols)
            raise AssertionError(cols)
        except ca.LdbgError as e:
            assert e.status == 6, e
    with g.unitigs([0]) as u:
        try:
            u.write_gfa1(tmp / "x.gfa", 5)
            raise AssertionError("colour 5")
        except ca.LdbgError as e:
            assert e.status == 6
        try:
            u.sequences(0, 2)
            raise AssertionError("range")
        except ca.LdbgError as e:
            assert e.status == 6
    g.close()


def _ascii_of_words(words, k):
    """packed k-mer words [n, W] -> ASCII [n, k]"""
    W = words.shape[1]
    out = np.empty((words.shape[0], k), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(k):
        bit = 2 * (k - 1 - i)
        out[:, i] = lut[((words[:, W - 1 - (bit >> 6)] >> np.uint64(bit & 63)) & np.uint64(3)).astype(np.int64)]
    return out


def case_synth(orc, lib, tmp, genome_len=2_000_000, k=47, budget_s=15.0):
    """a synthetic 3-colour graph (tools/synth.generate): the invariants on every unitig, the yardstick on a sample; prints the times"""
    import time
    from tools import synth
    prefix = str(tmp / "synth")
    synth.generate(prefix, genome_len, k, colours=3, with_links=False, seed=0xC0FFEE05, n_chrom=4, n_repeat_families=100,
                   repeat_copies=4, repeat_len=(50, 300), n_seeds=10, threads=min(16, os.cpu_count() or 1))
    path = prefix + ".ctx"
    g = CortexGraph(path, lib=lib)
    N = g.getNumRecords()
    words, cov, _ = g.records(0, N)
    cov = np.asarray(cov).view(np.uint32).reshape(N, -1)
    kmers = _ascii_of_words(np.asarray(words, dtype=np.uint64).reshape(N, -1), k)
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    y = LazyYardstick(orc.Graph(path))
    rng = random.Random(3)
    for S in ([0], [0, 1, 2]):
        t = time.time()
        u = g.unitigs(S)
        wall_ms = (time.time() - t) * 1e3
        seqs = u.sequences()
        U = len(seqs)
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)])
        allb = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        assert u.total_bases == allb.size and u.longest == lens.max() and (lens >= k).all()
        assert np.isin(allb, np.frombuffer(b"ACGT", np.uint8)).all()
        # members: exactly the records with coverage in S, each at one (unitig, position); the spelled k-mers round-trip
        uid, pos, ori = u.of_records(np.arange(N))
        member = (cov[:, S] != 0).any(axis=1)
        assert ((uid >= 0) == member).all()
        m = np.nonzero(member)[0]
        assert m.size == int((lens - k + 1).sum())
        key = uid[m] * (1 << 32) + pos[m]
        assert np.unique(key).size == m.size and (pos[m] <= lens[uid[m]] - k).all()
        start = off[uid[m]] + pos[m]
        got = allb[start[:, None] + np.arange(k)[None, :]]
        exp = kmers[m]
        fl = ori[m] == 1
        exp[fl] = comp[exp[fl][:, ::-1]]
        assert (got == exp).all()
        # coverage per unitig and colour
        csum = np.zeros((U, g.getNumColors()), dtype=np.uint64)
        np.add.at(csum, uid[m], cov[m].astype(np.uint64))
        assert ((csum & np.uint64(0xFFFFFFFF)).astype(np.uint32) == u.coverages()).all()
        # the lowest orientation, ids in record order of the first k-mer
        assert all(s <= rc(s) for s in seqs)
        first = [r for r in m[pos[m] == 0]]
        assert sorted(first, key=lambda r: uid[r]) == sorted(first)
        # the yardstick on a sample
        t_end, n_checked = time.time() + budget_s, 0
        for i in rng.sample(range(U), min(U, 400)):
            if time.time() > t_end and n_checked >= 50:
                break
            check_unitig(y, seqs[i], S)
            n_checked += 1
        t = time.time()
        u.write_gfa1(tmp / "synth.gfa", S[0])
        gfa_ms = (time.time() - t) * 1e3
        lines = (tmp / "synth.gfa").read_text().split("\n")
        assert lines[0] == "H\tVN:Z:1.0" and sum(1 for x in lines if x.startswith("S\t")) == U
        assert u.sequences() == g.unitigs(S).sequences()
        print("unitigs of %s: %d records, %d unitigs, %d bases, longest %d; build %.2f ms on the device (%.1f ms wall), GFA %.0f ms; "
              "%d checked against the yardstick" % (S, N, U, u.total_bases, u.longest, u.build_ms, wall_ms, gfa_ms, n_checked))
        u.close()
    g.close()
