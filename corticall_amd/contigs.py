"""Contigs threaded through a graph, and the commands that post-process Partition's FASTA — the reference's loops "for every window
of every contig: canonicalise it, ask a graph" — over ldbg_graph_thread.  No compute here beyond marshalling the
sequences and formatting the text: the windows, the lookups, the per-contig counts, the regions and the copy indices are HIP kernels;
the contigs cross the bus once, as they are.

Mirrors  J/commands/discover/call/TrimPartitions.java:35-68              J/commands/discover/call/FilterPartitions.java:41-140
         J/commands/discover/call/CountNovelKmersInPartitions.java:30-61  J/commands/discover/display/Coverage.java:29-47
The hand-over to Call (loadChildWalk, getRegions) is in traversal_utils."""
import ctypes as C
import os

import numpy as np

from . import _native
from .build import _marshal_reads

FIND_QUIRK, COPY_INDEX = 1, 2
WIN_VALID, WIN_FLIP, WIN_PAL, WIN_ROI = 1, 2, 4, 8


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Threading:
    """ldbg_threading: a batch of sequences threaded through a graph and / or a ROI graph, held on the device"""

    def __init__(self, graph, rois, seqs=None, find_quirk=False, copy_index=False, device_text=None, stream=None):
        """seqs: list of str / bytes; or device_text = (d_bases, d_offsets, n_seqs): pointers to the text and its n_seqs + 1 int64
        offsets in memory of the graphs' device"""
        any_graph = graph if graph is not None else rois
        if any_graph is None:
            raise _native.LdbgError(6, "thread: neither a graph nor a ROI graph")
        self._lib, self._d = any_graph._lib, any_graph._lib.dll
        self.GRAPH, self.ROIS = graph, rois
        self.k = any_graph.getKmerSize()
        self.has_copy_index = bool(copy_index)
        flags = (FIND_QUIRK if find_quirk else 0) | (COPY_INDEX if copy_index else 0)
        gh = graph._h if graph is not None else None
        rh = rois._h if rois is not None else None
        h = C.c_void_p()
        if device_text is None:
            text, offs = _marshal_reads(seqs)
            self._lib.check(self._d.ldbg_graph_thread(gh, rh, C.c_void_p(text.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_int64(len(offs) - 1), flags,
                                                      C.byref(h)))
        else:
            d_bases, d_offsets, n = device_text
            self._lib.check(self._d.ldbg_graph_thread_dev(gh, rh, C.c_void_p(d_bases), C.c_void_p(d_offsets), C.c_int64(n), flags, C.c_void_p(stream),
                                                          C.byref(h)))
        self._h = h
        ns, nw, nr, ms = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        self._lib.check(self._d.ldbg_threading_info(h, C.byref(ns), C.byref(nw), C.byref(nr), C.byref(ms)))
        self.n_seqs, self.n_windows, self.n_regions, self.device_ms = ns.value, nw.value, nr.value, ms.value

    def windows(self, first=0, n=None):
        """windows [first, first + n) -> (rec i64[n], info u8[n], copy_index i32[n] or None)"""
        n = self.n_windows - first if n is None else int(n)
        rec, info = np.empty(max(n, 0), dtype=np.int64), np.empty(max(n, 0), dtype=np.uint8)
        ci = np.empty(max(n, 0), dtype=np.int32) if self.has_copy_index else None
        self._lib.check(self._d.ldbg_threading_windows(self._h, C.c_int64(first), C.c_int64(n), _ptr(rec), _ptr(info), _ptr(ci) if ci is not None else None))
        return rec, info, ci

    def windows_dev(self, d_rec, d_info, d_copy_index=None, first=0, n=None, stream=None):
        """the same into memory of the graphs' device (pointers; None leaves an output out)"""
        n = self.n_windows - first if n is None else int(n)
        self._lib.check(self._d.ldbg_threading_windows_dev(self._h, C.c_int64(first), C.c_int64(n), C.c_void_p(d_rec), C.c_void_p(d_info),
                                                           C.c_void_p(d_copy_index), C.c_void_p(stream)))

    def coverage(self, colour, first=0, n=None):
        """getCoverage(colour) of every window's record -> i32[n]; JavaNullPointerException when a window has none"""
        n = self.n_windows - first if n is None else int(n)
        cov = np.empty(max(n, 0), dtype=np.int32)
        self._lib.check(self._d.ldbg_threading_coverage(self._h, int(colour), C.c_int64(first), C.c_int64(n), _ptr(cov)))
        return cov

    def summary(self, first_seq=0, n=None):
        """sequences [first_seq, first_seq + n) -> dict(win_start i64[n + 1], first_hit, last_hit, n_hits, n_distinct i32[n], ends u8[n])"""
        n = self.n_seqs - first_seq if n is None else int(n)
        m = max(n, 0)
        out = dict(win_start=np.zeros(m + 1, dtype=np.int64), first_hit=np.empty(m, dtype=np.int32), last_hit=np.empty(m, dtype=np.int32),
                   n_hits=np.empty(m, dtype=np.int32), n_distinct=np.empty(m, dtype=np.int32), ends=np.empty(m, dtype=np.uint8))
        self._lib.check(self._d.ldbg_threading_summary(self._h, C.c_int64(first_seq), C.c_int64(n), _ptr(out["win_start"]), _ptr(out["first_hit"]),
                                                       _ptr(out["last_hit"]), _ptr(out["n_hits"]), _ptr(out["n_distinct"]), _ptr(out["ends"])))
        return out

    def regions(self):
        """-> (region_offsets i64[n_seqs + 1], start i32[n_regions], stop i32[n_regions]): inclusive pairs, relative to their sequence"""
        offs = np.zeros(self.n_seqs + 1, dtype=np.int64)
        start, stop = np.empty(self.n_regions, dtype=np.int32), np.empty(self.n_regions, dtype=np.int32)
        self._lib.check(self._d.ldbg_threading_regions(self._h, _ptr(offs), _ptr(start), _ptr(stop), C.c_int64(self.n_regions)))
        return offs, start, stop

    def occurrences(self):
        """how often the windows hit every record of the graph (ldbg_threading_occurrences) -> Occurrences"""
        return Occurrences(self)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.check(self._d.ldbg_threading_free(self._h))
            self._h = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Occurrences:
    """ldbg_occurrences: per record of a threading's graph the number of windows whose canonical k-mer it is and the first of them,
    held on the device — what the reference asks of IndexedReference.find (J/utils/io/reference/IndexedReference.java:90-101), as an
    exact count"""

    def __init__(self, threading):
        self._lib, self._d = threading._lib, threading._lib.dll
        self.GRAPH = threading.GRAPH
        h = C.c_void_p()
        self._lib.check(self._d.ldbg_threading_occurrences(threading._h, C.byref(h)))
        self._h = h
        n, ms = C.c_int64(), C.c_double()
        self._lib.check(self._d.ldbg_occurrences_info(h, C.byref(n), C.byref(ms)))
        self.n_records, self.device_ms = n.value, ms.value
        self._threading = threading            # positions() reads its window starts and strands: it must still be open then

    def get(self, first=0, n=None):
        """records [first, first + n) -> (count u32[n], first window i64[n], -1 = none)"""
        n = self.n_records - first if n is None else int(n)
        count, fw = np.empty(max(n, 0), dtype=np.uint32), np.empty(max(n, 0), dtype=np.int64)
        self._lib.check(self._d.ldbg_occurrences_get(self._h, C.c_int64(first), C.c_int64(n), _ptr(count), _ptr(fw)))
        return count, fw

    def get_dev(self, d_count, d_first, first=0, n=None, stream=None):
        """the same into memory of the graph's device (pointers; None leaves an output out)"""
        n = self.n_records - first if n is None else int(n)
        self._lib.check(self._d.ldbg_occurrences_get_dev(self._h, C.c_int64(first), C.c_int64(n), C.c_void_p(d_count), C.c_void_p(d_first),
                                                         C.c_void_p(stream)))

    @property
    def count(self): return self.get()[0]

    @property
    def first(self): return self.get()[1]

    def positions(self, records):
        """the first window of each of the records -> list of (sequence index, 0-based offset in it, flipped: the window is the reverse
        complement of the record's k-mer); (-1, -1, False) for a record without an occurrence"""
        fw = self.first
        t = self._threading
        win_start = t.summary()["win_start"]
        out = []
        for r in records:
            w = int(fw[int(r)])
            if w < 0:
                out.append((-1, -1, False))
                continue
            s = int(np.searchsorted(win_start, w, side="right")) - 1
            out.append((s, w - int(win_start[s]), bool(t.windows(w, 1)[1][0] & WIN_FLIP)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.check(self._d.ldbg_occurrences_free(self._h))
            self._h = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_fasta_named(path):
    """the records of a plain-text FASTA -> list of (name, sequence): the name is the whole header line after '>' (the reference
    opens its FASTA arguments with FastaSequenceFile(file, false), J/utils/arguments/ArgumentHandler.java:284: names are not cut at
    white space), the sequence the lines up to the next header, joined"""
    recs, name, cur = [], None, []
    with open(path, "r", newline="") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(cur)))
                name, cur = line[1:], []
            elif name is not None:
                cur.append(line.strip())
    if name is not None:
        recs.append((name, "".join(cur)))
    return recs


def _records(fasta):
    if isinstance(fasta, (str, bytes, os.PathLike)):
        return read_fasta_named(fasta)
    return [(str(n), s if isinstance(s, str) else bytes(s).decode()) for n, s in fasta]


def _emit(text, out):
    if out is not None:
        with open(out, "w", newline="") as f:
            f.write(text)
    return text


class _Command:
    """a command over a FASTA (a path, or a list of (name, sequence)) and a graph.  execute(out=None) -> the text the reference
    prints, written to `out` when given; when the reference throws part-way, the text it had printed by then is written, and is
    the exception's .printed"""

    def _fail(self, exc, lines, out):
        exc.printed = _emit("".join(lines), out)
        raise exc


class TrimPartitions(_Command):
    """TrimPartitions.java:41-67: every contig cut to MARGIN windows either side of its first and last ROI window.  Kept as it is:
    subList(start, stop) is end-exclusive, so the last vertex is never written; a contig whose start ends above its stop (one without
    a ROI window and more than 2 MARGIN + 1 windows) is subList's IllegalArgumentException — CortexJDKException here, raised before
    that record is written (the reference's stream holds the record's name line by then)."""

    def __init__(self, FASTA, ROI, MARGIN=500):
        self.FASTA, self.ROI, self.MARGIN = FASTA, ROI, int(MARGIN)

    def execute(self, out=None):
        recs, k, M = _records(self.FASTA), self.ROI.getKmerSize(), self.MARGIN
        with Threading(None, self.ROI, [s for _, s in recs]) as t:
            sm = t.summary()
        lines = []
        for (name, seq), fh, lh in zip(recs, sm["first_hit"], sm["last_hit"]):
            n = len(seq) - k + 1
            start = int(fh) if fh >= 0 else len(seq) - k
            stop = int(lh) if lh >= 0 else 0
            start = start - M if start - M >= 0 else 0
            stop = stop + M if stop + M < n - 1 else n - 1
            if n > 0:
                if start > stop:
                    self._fail(_native.CortexJDKException("IllegalArgumentException: fromIndex(%d) > toIndex(%d)" % (start, stop)), lines, out)
                lines.append(">" + name + "\n")
                lines.append((seq[start:stop + k - 1] if stop > start else "") + "\n")
        return _emit("".join(lines), out)


class FilterPartitions(_Command):
    """FilterPartitions.java:56-125: the contigs with more than NOVEL_KMER_THRESHOLD distinct ROI k-mers and neither end window in
    ROI, by descending count.  Among equal counts the reference's order is the iteration order of a HashMap keyed by htsjdk's
    ReferenceSequence, which the reference tree does not pin; here ties keep input order (unpinned).  A contig shorter than k is
    substring's StringIndexOutOfBoundsException: CortexJDKException here."""

    def __init__(self, CONTIGS, ROI, NOVEL_KMER_THRESHOLD=5):
        self.CONTIGS, self.ROI, self.NOVEL_KMER_THRESHOLD = CONTIGS, ROI, int(NOVEL_KMER_THRESHOLD)

    def execute(self, out=None):
        recs, k = _records(self.CONTIGS), self.ROI.getKmerSize()
        with Threading(None, self.ROI, [s for _, s in recs]) as t:
            sm = t.summary()
        kept = []
        for i, (name, seq) in enumerate(recs):
            if len(seq) < k:
                raise _native.CortexJDKException("StringIndexOutOfBoundsException: contig '%s' is shorter than k" % name)
            if sm["n_distinct"][i] > self.NOVEL_KMER_THRESHOLD and sm["ends"][i] == 0:
                kept.append(i)
        kept.sort(key=lambda i: -int(sm["n_distinct"][i]))                # (stable)
        return _emit("".join(">%s\n%s\n" % recs[i] for i in kept), out)


class CountNovelKmersInPartitions(_Command):
    """CountNovelKmersInPartitions.java:36-46: name up to the first space, length, distinct ROI k-mers of every contig"""

    def __init__(self, CONTIGS, ROI):
        self.CONTIGS, self.ROI = CONTIGS, ROI

    def execute(self, out=None):
        recs = _records(self.CONTIGS)
        with Threading(None, self.ROI, [s for _, s in recs]) as t:
            sm = t.summary()
        lines = ["partitionName\tpartitionLength\tnovelKmers\n"]
        lines += ["%s\t%d\t%d\n" % (name.split(" ")[0], len(seq), nd) for (name, seq), nd in zip(recs, sm["n_distinct"])]
        return _emit("".join(lines), out)


class Coverage(_Command):
    """Coverage.java:32-46: one line per window: name up to the first space, the k-mer as given, its index, the sample's coverage
    of its record.  findRecord answers (SURVEY Q1 included); a window without a record is the reference's NullPointerException,
    after the lines of the windows before it."""

    def __init__(self, GRAPH, CONTIGS, SAMPLE):
        self.GRAPH, self.CONTIGS, self.SAMPLE = GRAPH, CONTIGS, SAMPLE

    def execute(self, out=None):
        g = self.GRAPH
        c = self.SAMPLE if isinstance(self.SAMPLE, (int, np.integer)) else g.getColorForSampleName(self.SAMPLE)
        recs, k = _records(self.CONTIGS), g.getKmerSize()
        missing = None
        with Threading(g, None, [s for _, s in recs], find_quirk=True) as t:
            ws = t.summary()["win_start"]
            try:
                cov = t.coverage(c)
            except _native.JavaNullPointerException as e:
                missing = e
                rec, _, _ = t.windows()
                stop = int(np.argmax(rec < 0))
                cov = t.coverage(c, 0, stop)
        lines = ["contig\tkmer\tindex\tcoverage\n"]
        for s, (name, seq) in enumerate(recs):
            short = name.split(" ")[0]
            for w in range(int(ws[s]), min(int(ws[s + 1]), len(cov))):
                i = w - int(ws[s])
                lines.append("%s\t%s\t%d\t%d\n" % (short, seq[i:i + k], i, cov[w]))
        if missing is not None:
            self._fail(missing, lines, out)
        return _emit("".join(lines), out)
