"""FindROIs, the record prefilters and Remove — the reference's loops "for every record: test it, write it" — over the device
selection of libldbg (ldbg_graph_select).  No compute here beyond building colour masks: the predicate, the
order-preserving compaction and the packing of the written records are HIP kernels; the records cross the bus once, packed.

Mirrors  J/commands/discover/roi/FindROIs.java:30-105        J/commands/prefilter/FindLowCoverage.java:32-67
         J/commands/prefilter/FindDust.java:78-135            J/commands/prefilter/FindShared.java:41-118
         J/commands/utils/Remove.java:29-86
         J/commands/discover/recover/RecoverExcludedKmers.java:29-108 (a selection with a join)
         J/commands/prefilter/FindLowComplexity.java:35-100 (host only: a gzip length per ROI record)
The prefilters write the records they EXCLUDE (the reference's cgw.addRecord sits in the else branch); that is kept."""
import ctypes as C
import os
import zlib

import numpy as np

from . import _native
from .graph import CortexCollection, CortexGraph


def _mask(colours):
    m = 0
    for c in colours:
        c = int(c)
        if c < 0:
            raise _native.LdbgError(6, "colour %d out of range" % c)
        m |= 1 << c
    if m >> 64:
        raise _native.LdbgError(6, "a colour mask holds 64 colours")
    return m


class Selection:
    """ldbg_selection: the records of a resident graph that pass a filter, in record order, held on the device"""

    def __init__(self, graph, lookup=None, all_zero=(), all_positive=(), any_positive=(), none_positive=(), cov_below=None, degree_above=None):
        self._lib, self._d = graph._lib, graph._lib.dll
        self.GRAPH = lookup if lookup is not None else graph        # the graph whose records are numbered
        f = _native.RecordFilter(_mask(all_zero), _mask(all_positive), _mask(any_positive), _mask(none_positive), -1, 0, -1, 0)
        if cov_below is not None:
            f.cov_color, f.cov_below = int(cov_below[0]), int(cov_below[1])
        if degree_above is not None:
            f.degree_color, f.degree_above = int(degree_above[0]), int(degree_above[1])
        h = C.c_void_p()
        if lookup is None:
            self._lib.check(self._d.ldbg_graph_select(graph._h, C.byref(f), C.byref(h)))
        else:
            self._lib.check(self._d.ldbg_graph_select_lookup(graph._h, C.byref(f), lookup._h, C.byref(h)))
        self._h = h
        n = C.c_int64()
        self._lib.check(self._d.ldbg_selection_count(h, C.byref(n)))
        self.count = n.value

    @classmethod
    def recover(cls, graph, child_colour, dirty):
        """ldbg_graph_recover: the records RecoverExcludedKmers writes -> (selection, numRecordsRecovered)"""
        sel = cls.__new__(cls)
        sel._lib, sel._d, sel.GRAPH = graph._lib, graph._lib.dll, graph
        h, nrec = C.c_void_p(), C.c_int64()
        sel._lib.check(sel._d.ldbg_graph_recover(graph._h, int(child_colour), dirty._h, C.byref(h), C.byref(nrec)))
        sel._h = h
        n = C.c_int64()
        sel._lib.check(sel._d.ldbg_selection_count(h, C.byref(n)))
        sel.count = n.value
        return sel, nrec.value

    @classmethod
    def variant_seeds(cls, graph, all_zero=(), covered=(), unique=()):
        """ldbg_graph_variant_seeds: the good seeds of getVariantSeeds -> selection with n_seeds, n_unique, n_good and
        device_ms.  covered: (colours, at_least, at_most) clauses; unique: (colour or -1, Occurrences or a device pointer to a byte per
        record) entries"""
        from .contigs import Occurrences
        covered, unique = list(covered), list(unique)
        if len(covered) > _native.SEED_MAX_COVERED or len(unique) > _native.SEED_MAX_UNIQUE:
            raise _native.LdbgError(6, "variant seeds: more clauses than the filter holds (%d covered, %d unique)" % (_native.SEED_MAX_COVERED, _native.SEED_MAX_UNIQUE))
        f = _native.SeedFilter()
        f.all_zero, f.n_covered, f.n_unique = _mask(all_zero), len(covered), len(unique)
        for j, (colours, lo, hi) in enumerate(covered):
            f.covered[j].mask, f.covered[j].at_least, f.covered[j].at_most = _mask(colours), int(lo), int(hi)
        keep = []
        for j, (colour, what) in enumerate(unique):
            f.unique[j].colour = int(colour)
            if isinstance(what, Occurrences):
                f.unique[j].occurrences = what._h
                keep.append(what)
            else:
                f.unique[j].d_unique = int(what)
        sel = cls.__new__(cls)
        sel._lib, sel._d, sel.GRAPH = graph._lib, graph._lib.dll, graph
        h, cn = C.c_void_p(), _native.SeedCounts()
        sel._lib.check(sel._d.ldbg_graph_variant_seeds(graph._h, C.byref(f), C.byref(h), C.byref(cn)))
        del keep
        sel._h = h
        sel.n_seeds, sel.n_unique, sel.n_good, sel.device_ms = cn.n_seeds, cn.n_unique, cn.n_good, cn.device_ms
        sel.count = cn.n_good
        return sel

    def recovered_coverage(self, first=0, n=None):
        """the child colour's coverage after the patch of selected records [first, first + n) -> i32[n] (a recover selection only)"""
        n = self.count - first if n is None else int(n)
        cov = np.empty(max(n, 0), dtype=np.int32)
        self._lib.check(self._d.ldbg_selection_recovered_coverage(self._h, C.c_int64(first), C.c_int64(n), cov.ctypes.data_as(C.c_void_p)))
        return cov

    def write_recovered(self, out):
        self._lib.check(self._d.ldbg_selection_write_recovered(self._h, str(out).encode()))

    def recovered_graph(self):
        """the graph write_recovered would write, resident without the file (ldbg_selection_open_recovered) -> CortexGraph"""
        h = C.c_void_p()
        self._lib.check(self._d.ldbg_selection_open_recovered(self._h, C.byref(h)))
        g = CortexGraph._from_handle(h, self._lib, "<recovered>")
        g._borrowed = False
        return g

    def __len__(self): return self.count

    def indices(self, first=0, n=None):
        """record numbers [first, first + n) of the selection, ascending -> i64[n]"""
        n = self.count - first if n is None else int(n)
        idx = np.empty(max(n, 0), dtype=np.int64)
        self._lib.check(self._d.ldbg_selection_indices(self._h, C.c_int64(first), C.c_int64(n), idx.ctypes.data_as(C.c_void_p)))
        return idx

    def indices_dev(self, d_ptr, first=0, n=None, stream=None):
        """the same into device memory (d_ptr: room for n int64 on the graph's device)"""
        n = self.count - first if n is None else int(n)
        self._lib.check(self._d.ldbg_selection_indices_dev(self._h, C.c_int64(first), C.c_int64(n), C.c_void_p(d_ptr), C.c_void_p(stream)))

    @staticmethod
    def _colours(colours):
        cols = [int(c) for c in colours]
        return (C.c_int * max(1, len(cols)))(*cols), len(cols)

    def write_ctx(self, out, colours, header_path=None):
        """CortexGraphWriter over the selection reduced to `colours`: under the header of header_path, or (None) the fresh header of
        FindROIs.makeCortexHeader"""
        arr, n = self._colours(colours)
        self._lib.check(self._d.ldbg_selection_write_ctx(self._h, arr, n, str(header_path).encode() if header_path is not None else None,
                                                         str(out).encode()))

    def graph(self, colours, header_path=None):
        """the graph write_ctx would write, opened as a resident table without the file (ldbg_selection_open_graph) -> CortexGraph"""
        arr, n = self._colours(colours)
        h = C.c_void_p()
        self._lib.check(self._d.ldbg_selection_open_graph(self._h, arr, n, str(header_path).encode() if header_path is not None else None,
                                                          C.byref(h)))
        g = CortexGraph._from_handle(h, self._lib, "<selection>")
        g._borrowed = False
        return g

    def close(self):
        if getattr(self, "_h", None):
            self._lib.check(self._d.ldbg_selection_free(self._h))
            self._h = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _colour(graph, c):
    return int(c) if isinstance(c, (int, np.integer)) else graph.getColorForSampleName(c)


def _header_of(roi):
    """ROI.getHeader(): the file the ROI graph was opened from; a resident ROI graph (FindROIs.graph()) has the fresh header"""
    p = roi.path
    return p if os.path.exists(p) else None


def _write_excluded(sel, roi, out):
    """the tail of the four prefilters: cgw.setHeader(ROI.getHeader()), the excluded records, close -> (numKept, numExcluded)"""
    n = roi.getNumRecords()
    with sel:
        if out is not None:
            sel.write_ctx(out, range(roi.getNumColors()), _header_of(roi))
        return n - sel.count, sel.count


class FindROIs:
    """J/commands/discover/roi/FindROIs.java:30-82 — the k-mers the child has and no parent has, as a graph of the child's colour
    under a fresh header.  parents / child: sample names (or colours)."""

    def __init__(self, graph, parents, child):
        self.GRAPH, self.PARENTS, self.CHILD = graph, list(parents), child
        self.numNovelRecords = 0

    def _select(self):
        g = self.GRAPH
        child = _colour(g, self.CHILD)
        parents = [_colour(g, p) for p in self.PARENTS]
        return g.select(all_positive=[child], all_zero=parents), child          # isNovel :72-82

    def execute(self, out=None):
        """writes the ROI graph to `out` (if given) -> the number of novel records"""
        sel, child = self._select()
        with sel:
            if out is not None:
                sel.write_ctx(out, [child])
            self.numNovelRecords = sel.count
        return self.numNovelRecords

    def graph(self):
        """the ROI graph resident on the device, without a file: what Partition, an engine's .rois(...) and the prefilters take"""
        sel, child = self._select()
        with sel:
            self.numNovelRecords = sel.count
            return sel.graph([child])


class FindLowCoverage:
    """J/commands/prefilter/FindLowCoverage.java:32-67 — ROI records with coverage below MIN_COVERAGE"""

    def __init__(self, roi, min_coverage):
        self.ROI, self.MIN_COVERAGE = roi, int(min_coverage)

    def execute(self, out=None):
        return _write_excluded(self.ROI.select(cov_below=(0, self.MIN_COVERAGE)), self.ROI, out)


class FindDust:
    """J/commands/prefilter/FindDust.java:78-135 — ROI records with more than 4 edges in colour 0 (isDust :133-135; the dfs over the
    dust chains is commented out in the reference)"""

    def __init__(self, graph, parents, roi):
        self.GRAPH, self.PARENTS, self.ROI = graph, list(parents), roi

    def execute(self, out=None):
        return _write_excluded(self.ROI.select(degree_above=(0, 4)), self.ROI, out)


class FindShared:
    """J/commands/prefilter/FindShared.java:41-118 — ROI records whose k-mer has coverage in a colour of GRAPH that is neither the
    child, a parent nor ignored.  A ROI k-mer without a record in GRAPH is the reference's NullPointerException (:63-68)."""

    def __init__(self, graph, parents, roi, ignore=()):
        self.GRAPH, self.PARENTS, self.ROI, self.IGNORE = graph, list(parents), roi, list(ignore)

    def execute(self, out=None):
        g, roi = self.GRAPH, self.ROI
        skip = {g.getColorForSampleName(roi.getSampleName(0))}
        skip.update(_colour(g, p) for p in self.PARENTS)
        skip.update(_colour(g, p) for p in self.IGNORE)
        others = [c for c in range(g.getNumColors()) if c not in skip]
        if others:
            sel = g.select(any_positive=others, lookup=roi)
        else:       # no colour to test: the reference's loop never touches the record and nothing is shared
            sel = roi.select(all_zero=[0], all_positive=[0])
        return _write_excluded(sel, roi, out)


class RecoverExcludedKmers:
    """J/commands/discover/recover/RecoverExcludedKmers.java:29-108 — the pedigree graph reduced to the records the child has, plus
    those only another sample has whose k-mer the child's uncleaned graph DIRTY holds with coverage: these get DIRTY's coverage as
    the child's.  The file has ONE colour under the child's colour block and, as CortexGraphWriter writes header.getNumColors()
    colours of the record it is given, carries colour 0's coverage and edge byte: the patch shows when the child is colour 0."""

    def __init__(self, graph, dirty):
        self.GRAPH, self.DIRTY = graph, dirty
        self.childColor, self.numWritten, self.numRecordsRecovered = -1, 0, 0

    def _select(self):
        name = self.DIRTY.getSampleName(0)
        self.childColor = self.GRAPH.getColorForSampleName(name)
        if self.childColor < 0:
            raise _native.LdbgError(1, "Sample '%s' not found in pedigree graph" % name)
        sel, self.numRecordsRecovered = Selection.recover(self.GRAPH, self.childColor, self.DIRTY)
        self.numWritten = sel.count
        return sel

    def execute(self, out=None):
        """writes the graph to `out` (if given) -> numRecordsRecovered"""
        with self._select() as sel:
            if out is not None:
                sel.write_recovered(out)
        return self.numRecordsRecovered

    def graph(self):
        """the written graph resident on the device, without a file"""
        with self._select() as sel:
            return sel.recovered_graph()


def gzip_length(b):
    """SequenceUtils.computeCompressionRatio's numerator (SequenceUtils.java:794-813): the size of a GZIPOutputStream of the bytes —
    10 header bytes, raw deflate at the default level, 8 trailer bytes"""
    c = zlib.compressobj(-1, zlib.DEFLATED, -15)
    return len(c.compress(bytes(b)) + c.flush()) + 18


class FindLowComplexity:
    """J/commands/prefilter/FindLowComplexity.java:35-100 — ROI records whose canonical k-mer compresses too well:
    (float) gzipLength / (float) k < threshold, in float32.  Host only (a ROI is 10^4..10^5 records).  graph and parents are the
    reference's arguments; as there, only their colours are logged and nothing of them is read."""

    def __init__(self, graph, parents, roi, threshold=0.70):
        self.GRAPH, self.PARENTS, self.ROI, self.COMPLEXITY_THRESHOLD = graph, list(parents), roi, np.float32(threshold)
        self.excluded = []             # ROI record numbers, ascending

    def execute(self, out=None):
        from .partition import unpack_kmers
        roi = self.ROI
        n, k = roi.getNumRecords(), roi.getKmerSize()
        self.excluded = []
        if n > 0:
            words, _, _ = roi.records(0, n)
            kmers = unpack_kmers(words, k)
            for i in range(n):
                if np.float32(gzip_length(kmers[i].tobytes())) / np.float32(k) < self.COMPLEXITY_THRESHOLD:
                    self.excluded.append(i)
        if out is not None:
            idx = np.asarray(self.excluded, dtype=np.int64)
            roi._lib.check(roi._d.ldbg_ctx_write_records(roi.getFile().encode(), idx.ctypes.data_as(C.c_void_p), C.c_int64(len(idx)), str(out).encode()))
        return n - len(self.excluded), len(self.excluded)


class Remove:
    """J/commands/utils/Remove.java:29-86 — the records of the collection [graph] + secondary (its iterator: the union of the members'
    k-mers) without coverage in a secondary colour, reduced to the primary's colours under the primary's header"""

    def __init__(self, graph, secondary, out):
        self.PGRAPH, self.SGRAPH, self.out = graph, list(secondary), out

    def execute(self):
        """-> (numKept, numRemoved)"""
        paths = [g.getFile() if isinstance(g, CortexGraph) else str(g) for g in [self.PGRAPH] + self.SGRAPH]
        lib = self.PGRAPH._lib if isinstance(self.PGRAPH, CortexGraph) else None
        cc = CortexCollection(*paths, lib=lib)
        try:
            view = cc._iter_view or cc
            P = cc._member_info[0][2]
            with CortexGraph.select(view, none_positive=range(P, view._C)) as sel:
                sel.write_ctx(self.out, range(P), paths[0])
                return sel.count, view._N - sel.count
        finally:
            cc.close()
