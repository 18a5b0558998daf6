"""FindROIs, the record prefilters and Remove — the reference's loops "for every record: test it, write it" — over the device
selection of libldbg (ldbg_graph_select).  No compute here beyond building colour masks: the predicate, the
order-preserving compaction and the packing of the written records are HIP kernels; the records cross the bus once, packed.

Mirrors  J/commands/discover/roi/FindROIs.java:30-105        J/commands/prefilter/FindLowCoverage.java:32-67
         J/commands/prefilter/FindDust.java:78-135            J/commands/prefilter/FindShared.java:41-118
         J/commands/utils/Remove.java:29-86
The four prefilters write the records they EXCLUDE (the reference's cgw.addRecord sits in the else branch); that is kept."""
import ctypes as C
import os

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
