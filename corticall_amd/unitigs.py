"""Unitigs of a colour set, built on the device (ldbg_graph_unitigs), and ToGfa1 over them.

Unitigs   the handle: every unitig's bases, coverage per colour, record -> (unitig, position, orientation), FASTA and GFA1 writers
          (the text is formatted in the library, on the host, in C++).
ToGfa1    J/commands/utils/ToGfa1.java:37-145.  Without a FASTA the unitigs of the sample colour are built on the device and written
          by the library; with a FASTA the reference's semantics are applied to that file, its k-mers looked up with find_batch.
"""
import ctypes as C

import numpy as np

from . import _native

LDBG_GFA_PLUS_STRAND = 1
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def _revcomp(s):
    """SequenceUtils.reverseComplement (other bytes are kept as they are)"""
    return s.translate(_COMP)[::-1]


def _java_int(x):
    return int(np.int64(x).astype(np.int32))


def _java_avg(cov, n):
    """(int) ((float) cov / (float) n), JLS 5.1.3"""
    f = np.float32(np.float32(cov) / np.float32(n))
    if np.isnan(f):
        return 0
    if f >= np.float32(2147483648.0):
        return 2147483647
    if f <= np.float32(-2147483648.0):
        return -2147483648
    return int(f)


class Unitigs:
    """The unitigs of colours `colors` of a resident graph, in the order of the record number of their first k-mer, each in its
    alphanumerically lowest orientation.  The graph must stay open while this object is used."""

    def __init__(self, graph, colors=(0,)):
        cols = [int(c) for c in colors]
        self._graph, self._lib = graph, graph._lib
        self._d = self._lib.dll
        self.colors = tuple(cols)
        h = C.c_void_p()
        arr = (C.c_int * max(1, len(cols)))(*cols)
        self._lib.check(self._d.ldbg_graph_unitigs(graph._h, arr, len(cols), C.byref(h)))
        self._h = h
        n, b, L, ms = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        self._lib.check(self._d.ldbg_unitigs_info(h, C.byref(n), C.byref(b), C.byref(L), C.byref(ms)))
        self.count, self.total_bases, self.longest, self.build_ms = n.value, b.value, L.value, ms.value

    def __len__(self):
        return self.count

    def sequences(self, first=0, n=None):
        """unitigs [first, first + n) as str"""
        if n is None:
            n = self.count - first
        off = np.empty(n + 1, dtype=np.int64)
        self._lib.check(self._d.ldbg_unitigs_get(self._h, C.c_int64(first), C.c_int64(n), off.ctypes.data_as(C.c_void_p), None, C.c_int64(0)))
        buf = C.create_string_buffer(max(1, int(off[n])))
        self._lib.check(self._d.ldbg_unitigs_get(self._h, C.c_int64(first), C.c_int64(n), off.ctypes.data_as(C.c_void_p), buf, C.c_int64(int(off[n]))))
        raw = buf.raw[:int(off[n])].decode()
        return [raw[off[i]:off[i + 1]] for i in range(n)]

    def sequence(self, i):
        if not 0 <= i < self.count:
            raise IndexError(i)
        return self.sequences(i, 1)[0]

    def __iter__(self):
        step = 1 << 16
        for first in range(0, self.count, step):
            yield from self.sequences(first, min(step, self.count - first))

    def coverages(self, first=0, n=None):
        """u32 [n, C]: coverage summed over each unitig's k-mers, every colour of the graph (wraps like a Java int)"""
        if n is None:
            n = self.count - first
        cov = np.zeros((n, self._graph.getNumColors()), dtype=np.uint32)
        self._lib.check(self._d.ldbg_unitigs_coverage(self._h, C.c_int64(first), C.c_int64(n), cov.ctypes.data_as(C.c_void_p)))
        return cov

    def coverage(self, i, c):
        return int(self.coverages(i, 1)[0, c])

    def of_records(self, idx):
        """record numbers -> (unitig id, position, orientation) as int64 / int64 / int8 arrays; -1 for records that are no vertex"""
        r = np.ascontiguousarray(np.atleast_1d(np.asarray(idx, dtype=np.int64)))
        u, p, o = np.empty(r.size, np.int64), np.empty(r.size, np.int64), np.empty(r.size, np.int8)
        self._lib.check(self._d.ldbg_unitigs_of_records(self._h, r.ctypes.data_as(C.c_void_p), C.c_int64(r.size), u.ctypes.data_as(C.c_void_p),
                                                        p.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)))
        return u, p, o

    def write_fasta(self, path):
        self._lib.check(self._d.ldbg_unitigs_write_fasta(self._h, str(path).encode()))

    def write_gfa1(self, path, sample_color=0, plus_strand=False):
        """ToGfa1's output for these unitigs as its FASTA; plus_strand: '+' instead of ToGfa1's ':' for the positive strand"""
        self._lib.check(self._d.ldbg_unitigs_write_gfa1(self._h, str(path).encode(), int(sample_color), LDBG_GFA_PLUS_STRAND if plus_strand else 0))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.check(self._d.ldbg_unitigs_free(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_fasta(path):
    """FastaSequenceFile.nextSequence().getBaseString() of every record"""
    seqs, cur = [], None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if cur is not None:
                    seqs.append("".join(cur))
                cur = []
            elif cur is not None and line:
                cur.append(line)
    if cur is not None:
        seqs.append("".join(cur))
    return seqs


def _hashset_order(kmers):
    """iteration order of a HashSet<CortexByteKmer> (16 buckets, at most 4 keys) filled in the order given"""
    from .partition import java_bytes_hash
    if not kmers:
        return []
    h = java_bytes_hash(np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(len(kmers), -1))
    bucket = (h ^ (h >> np.uint32(16))) & np.uint32(15)
    return [kmers[i] for i in np.argsort(bucket, kind="stable")]


class ToGfa1:
    """J/commands/utils/ToGfa1.java:37-145 — the unitigs of a graph with coverage (S) and the links between their ends (L) as GFA1.

    FASTA=None: the unitigs of the sample colour are built on the device (Unitigs) and the library writes the file.
    FASTA given: the reference's semantics over that file's sequences (crs.get -> find_batch).
    plus_strand: '+' for the positive strand instead of ToGfa1's ':' (DESIGN.md §10)."""

    def __init__(self, GRAPH, out, FASTA=None, SAMPLE_NAME=None, plus_strand=False):
        self.GRAPH, self.FASTA, self.SAMPLE_NAME, self.out, self.plus_strand = GRAPH, FASTA, SAMPLE_NAME, str(out), plus_strand

    def _sample_color(self):
        return 0 if self.SAMPLE_NAME is None else self.GRAPH.getColorForSampleName(self.SAMPLE_NAME)

    def execute(self):
        sc = self._sample_color()
        if self.FASTA is None:
            with Unitigs(self.GRAPH, (sc,)) as u:
                u.write_gfa1(self.out, sc, self.plus_strand)
            return
        self._execute_fasta(read_fasta(str(self.FASTA)), sc)

    def _lookup(self, kmers):
        """crs.get(new CanonicalKmer(sk)) for every k-mer: (record or -1, Java-int coverage [n, C], edges [n, C])"""
        g = self.GRAPH
        if not kmers:
            return np.empty(0, np.int64), np.empty((0, g.getNumColors()), np.int32), np.empty((0, g.getNumColors()), np.uint8)
        if g._N > 2:
            return g.find_batch(kmers)
        # findRecord never answers in a table of two records or fewer; ToGfa1's HashMap of records does
        w, c, e = g.records(0, g._N)
        from .graph import CortexRecord
        recs = {}
        for i in range(g._N):
            s = CortexRecord(w[i], c[i], e[i], g._k).getKmerAsString()
            recs[s] = recs[_revcomp(s)] = i
        idx = np.array([recs.get(s, -1) for s in kmers], dtype=np.int64)
        cov = np.zeros((len(kmers), g._C), np.int32)
        ed = np.zeros((len(kmers), g._C), np.uint8)
        hit = idx >= 0
        cov[hit] = np.asarray(c, dtype=np.uint32).view(np.int32)[idx[hit]]
        ed[hit] = np.asarray(e, dtype=np.uint8)[idx[hit]]
        return idx, cov, ed

    def _execute_fasta(self, seqs, sc):
        k = self.GRAPH.getKmerSize()
        vertices, seq_names, positive, beginning, ending = {}, {}, {}, {}, {}
        for index, s in enumerate(seqs):
            for v in (s, _revcomp(s)):
                vertices.setdefault(v, None)
                beginning[v[:k]] = v
                ending[v[-k:]] = v
                seq_names[v] = index
            positive[s] = True
            positive[_revcomp(s)] = False
        order = list(vertices)
        # every k-mer of every vertex in one batch
        spans, kms = [], []
        for v in order:
            spans.append(len(kms))
            kms.extend(v[i:i + k] for i in range(len(v) - k + 1))
        spans.append(len(kms))
        idx, cov, edges = self._lookup(kms)
        csum = np.concatenate([[0], np.cumsum(np.where(idx >= 0, cov[:, sc].astype(np.int64), 0))]) if len(kms) else np.zeros(1, np.int64)
        avg, edge_list, edge_set = {}, [], set()

        def add_edge(a, b):
            if (a, b) not in edge_set:
                edge_set.add((a, b))
                edge_list.append((a, b))

        for j, v in enumerate(order):
            lo, hi = spans[j], spans[j + 1]
            avg[v] = _java_avg(_java_int(csum[hi] - csum[lo]), hi - lo)
            for side in (0, 1):
                at = lo if side == 0 else hi - 1
                sk = v[:k] if side == 0 else v[-k:]
                if idx[at] < 0:
                    raise _native.JavaNullPointerException("ToGfa1: no record for " + sk)
                canon = min(sk, _revcomp(sk))
                flipped = canon != sk
                e = int(edges[at, sc])
                # getAllPrevKmers / getAllNextKmers (TraversalUtils.java:510-557) of the k-mer as it reads in v: in the HashSet<Byte>
                # order of the edge bases, A C T G
                if side == 0:
                    bits = [b for b in "ACGT" if (e & 0xF) & (1 << "TGCA".index(b))] if flipped else \
                           [b for b in "ACGT" if (e >> 4) & (1 << (3 - "ACGT".index(b)))]
                    cands = [b + sk[:-1] for b in sorted(bits, key=lambda b: "ACTG".index(b))]
                    for x in _hashset_order(cands):
                        if x in ending:
                            add_edge(ending[x], v)
                else:
                    bits = [b for b in "ACGT" if (e >> 4) & (1 << (3 - "TGCA".index(b)))] if flipped else \
                           [b for b in "ACGT" if (e & 0xF) & (1 << "ACGT".index(b))]
                    cands = [sk[1:] + b for b in sorted(bits, key=lambda b: "ACTG".index(b))]
                    for x in _hashset_order(cands):
                        if x in beginning:
                            add_edge(v, beginning[x])
        plus = "+" if self.plus_strand else ":"
        lines = ["H\tVN:Z:1.0"]
        seen = set()
        for v in order:
            vid = seq_names[v]
            if vid not in seen:
                av = avg[v]
                lines.append("S\t%d\t%s\tRC:i:%d\tAC:i:%d" % (vid, v, _java_int(av * len(v)), av))
                seen.add(vid)
        for a, b in edge_list:
            lines.append("L\t%d\t%s\t%d\t%s\t%dM" % (seq_names[a], plus if positive[a] else "-", seq_names[b], plus if positive[b] else "-", k))
        with open(self.out, "w") as f:
            f.write("".join(x + "\n" for x in lines))
