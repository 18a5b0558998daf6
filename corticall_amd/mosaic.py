"""Tesserae (J/utils/alignment/mosaic/Tesserae.java): the child contig as a recombining mosaic of candidate haplotypes, in batches on
the device (ldbg_mosaic_align_batch), and the two host functions of Call that make its query: sectionContig
(Call.java:2383-2422) and trimQuery (:1946-1986).

The device returns, per problem, the log likelihood and maxpath_copy / maxpath_state / maxpath_pos; the three kinds of text track
(:385-492) and toString (:512-545) are text and are built here from those arrays."""
import ctypes as C

import numpy as np

from . import _native

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _canonical(sk):
    rc = sk.encode().translate(_COMP)[::-1].decode()
    return rc if rc < sk else sk


def build_tracks(panel, copy, state, pos):
    """Tesserae.java:385-492 over maxpath_*[cp .. 2 maxl] -> ([(name, track, (start, end)), ...], edit track).  panel: [(name, sequence)],
    the query first.  IndexError where the reference's charAt / get would throw."""
    n = len(copy)
    query = panel[0][1]

    def seq_of(i):
        if not 1 <= copy[i] <= len(panel):
            raise IndexError("maxpath_copy %d of a panel of %d" % (copy[i], len(panel)))
        return panel[copy[i] - 1]

    def char_of(s, p):
        if not 0 <= p < len(s):
            raise IndexError("charAt(%d) of a sequence of %d" % (p, len(s)))
        return s[p]

    path = []
    sb, start, end, pt = [], -1, -1, 1
    for i in range(n):                                     # :396-409 the query's track
        if state[i] == 3:
            sb.append("-")
        else:
            if start == -1:
                start = pt - 1
            end = pt - 1
            sb.append(char_of(query, pt - 1))
            pt += 1
    path.append((panel[0][0], "".join(sb), (start, end)))
    sb, pt = [], 1
    for i in range(n):                                     # :412-430 the edit track
        if state[i] == 1:
            sb.append("|" if char_of(query, pt - 1) == char_of(seq_of(i)[1], pos[i] - 1) else " ")
            pt += 1
        elif state[i] == 2:
            pt += 1
            sb.append("^")
        else:
            sb.append("~")
    edit = "".join(sb)
    current = seq_of(0)[0]                                 # :440-492 the copying tracks
    sb, start, end, last_known, upper = [], -1, -1, -1, True
    for i in range(n):
        before = pos[i - 1] if i > 0 else 0                # (maxpath_pos[cp - 1]: the entry the loop of :354-380 wrote last and cp++ dropped)
        if (i > 0 and copy[i] == copy[i - 1] and abs(pos[i] - pos[i - 1]) > 1) or pos[i] == last_known + 1:
            path.append((current, "".join(sb), (start, end)))
            upper = not upper
            last_known = before
            if start != end:
                start = end = pos[i] - 1
            current = seq_of(i)[0]
            sb = [" " * i]
        if i > 0 and copy[i] != copy[i - 1]:
            path.append((current, "".join(sb), (start, end)))
            upper = True
            if start != end:
                start = end = pos[i] - 1
            current = seq_of(i)[0]
            sb = [" " * i]
        if state[i] == 2:
            sb.append("-")
        else:
            c = char_of(seq_of(i)[1], pos[i] - 1)
            sb.append(c.upper() if upper else c.lower())
            if start == -1:
                start = pos[i] - 1
            end = pos[i] - 1
    path.append((current, "".join(sb), (start, end)))
    return path, edit


def format_tracks(path, edit, llk):
    """Tesserae.toString (:512-545).  The Mllk line carries Python's repr of the double: Java's Double.toString is not emulated (it
    prints fewer digits for some values)."""
    names = ["%s (%d-%d)" % (name, se[0], se[1]) for name, _, se in path]
    width = max([len(x) for x in names] + [0])
    out = []
    for i, (_, track, _) in enumerate(path):
        out.append(names[i].rjust(width) + " " + track + "\n")
        if i == 0:
            out.append(" ".rjust(width) + " " + edit + "\n")
    out.append("\nMllk: " + repr(float(llk)) + "\n")
    return "".join(out)


class MosaicAlignment:
    """one problem's result: path (the triples), edit_track, llk, and the arrays they were built from"""
    def __init__(self, path, edit_track, llk, copy, state, pos):
        self.path, self.edit_track, self.llk, self.copy, self.state, self.pos = path, edit_track, llk, copy, state, pos

    def __iter__(self):
        return iter(self.path)

    def __len__(self):
        return len(self.path)

    def __getitem__(self, i):
        return self.path[i]

    def __str__(self):
        return format_tracks(self.path, self.edit_track, self.llk)


class Tesserae:
    """Tesserae(del, eps, rho, term) (:87-92; the defaults of :14-17)"""
    def __init__(self, del_=0.025, eps=0.75, rho=0.0001, term=0.001, device=0, lib=None):
        self.params = _native.MosaicParams(del_, eps, rho, term)
        self.device = device
        self._lib = lib or _native.default_lib()
        self._last = None

    # ---- the device call
    def align_arrays(self, problems):
        """problems: [(query, targets)], targets an ordered mapping name -> sequence (or a sequence of (name, sequence)) ->
        (status u8[n], llk f64[n], path_off i64[n + 1], copy, state, pos i32[])"""
        problems = [(q, list(t.items()) if hasattr(t, "items") else list(t)) for q, t in problems]
        n = len(problems)
        qoff = np.zeros(n + 1, np.int64)
        tfirst = np.zeros(n + 1, np.int64)
        qs, ts, tlen = [], [], []
        for i, (q, t) in enumerate(problems):
            qb = q.encode("latin-1")
            qs.append(qb)
            qoff[i + 1] = qoff[i] + len(qb)
            tfirst[i + 1] = tfirst[i] + len(t)
            for _, s in t:
                sb = s.encode("latin-1")
                ts.append(sb)
                tlen.append(len(sb))
        toff = np.zeros(len(tlen) + 1, np.int64)
        if tlen:
            toff[1:] = np.cumsum(np.asarray(tlen, np.int64))
        qbytes, tbytes = b"".join(qs), b"".join(ts)
        d = self._lib.dll
        h = C.c_void_p()
        self._lib.check(d.ldbg_mosaic_align_batch(C.c_int(self.device), C.byref(self.params), C.c_int64(n), C.c_char_p(qbytes), qoff.ctypes.data_as(C.c_void_p),
                                                  tfirst.ctypes.data_as(C.c_void_p), C.c_char_p(tbytes), toff.ctypes.data_as(C.c_void_p), C.byref(h)))
        try:
            nn, ne = C.c_int64(), C.c_int64()
            self._lib.check(d.ldbg_mosaic_result_sizes(h, C.byref(nn), C.byref(ne)))
            status = np.zeros(n, np.uint8)
            llk = np.zeros(n, np.float64)
            poff = np.zeros(n + 1, np.int64)
            copy, state, pos = (np.zeros(max(1, ne.value), np.int32) for _ in range(3))
            arrs = _native.MosaicArrays(*[a.ctypes.data_as(C.c_void_p) for a in (status, llk, poff, copy, state, pos)])
            self._lib.check(d.ldbg_mosaic_result_get(h, C.byref(arrs)))
        finally:
            d.ldbg_mosaic_result_free(h)
        return status, llk, poff, copy[:ne.value], state[:ne.value], pos[:ne.value]

    @staticmethod
    def _refusal(query, targets):
        lens = [len(s) for _, s in targets]
        if not query:
            return "an empty query"
        if not targets:
            return "no targets"
        if sum(lens) == 0:
            return "targets without a base"
        if max(lens + [len(query)]) <= 2:
            return "no sequence longer than 2 (tb_divisor = 1)"
        return "the problem exceeds the traceback arena, or its traceback leaves the reference's arrays"

    def align_batch(self, problems):
        """one device call for all problems -> [MosaicAlignment or None]; None where the problem is refused (ldbg.h lists the cases)"""
        problems = [(q, list(t.items()) if hasattr(t, "items") else list(t)) for q, t in problems]
        status, llk, poff, copy, state, pos = self.align_arrays(problems)
        out = []
        for i, (q, t) in enumerate(problems):
            if status[i] != _native.LDBG_OK:
                out.append(None)
                continue
            c, s, p = (a[poff[i]:poff[i + 1]].tolist() for a in (copy, state, pos))
            path, edit = build_tracks([("query", q)] + t, c, s, p)
            out.append(MosaicAlignment(path, edit, float(llk[i]), c, s, p))
        return out

    def align(self, query, targets):
        """Tesserae.align (:95-103) -> [(name, track, (start, end)), ...] in Java's order.  targets: an ordered mapping; a caller that needs
        the order of a java.util.HashMap<String, String> applies partition.java_hashmap_order to the names' hashCodes first."""
        t = list(targets.items()) if hasattr(targets, "items") else list(targets)
        r = self.align_batch([(query, t)])[0]
        if r is None:
            raise _native.LdbgError(4, "Tesserae.align: " + self._refusal(query, t))
        self._last = r
        return r.path

    def getMaximumLogLikelihood(self):
        return self._last.llk

    @property
    def edit_track(self):
        return self._last.edit_track

    def __str__(self):
        return str(self._last)


def section_contig(rois, walk, window, split):
    """Call.sectionContig (:2383-2422).  rois: the walk's novel regions as traversal_utils.get_regions returns them (inclusive window
    pairs, in order); walk: its windows, anything with a length and slices (the record array of traversal_utils.load_child_walk, or a
    list) -> [(first, last, walk[first .. last])], or None without a region."""
    regions = list(rois)
    if not regions:
        return None
    n = len(walk)
    start = max(regions[0][0] - window, 0)
    stop = regions[-1][1] + window
    if stop >= n:
        stop = n - 1
    sections = []
    for i in range(len(regions) - 1):
        if regions[i + 1][0] - regions[i][1] > split:
            sections.append((start, regions[i][1] + window))
            start = regions[i + 1][0] - window
    sections.append((start, stop))
    out = []
    for a, b in sections:
        if a < 0 or b >= n:                                # (w.get(i) of :2412: a middle section is not clipped)
            raise IndexError("sectionContig: window %d of a walk of %d" % (a if a < 0 else b, n))
        out.append((a, b, walk[a:b + 1]))
    return out


def section_query(contig, section, rois, k):
    """What trim_query takes, from what the hand-over functions return: contig, the string traversal_utils.load_child_walk threaded
    (window i of its arrays is contig[i:i + k]); section, one (first, last, ...) triple of section_contig; rois, the whole walk's
    regions as traversal_utils.get_regions returns them -> (the section's contig, its regions in its own window numbers).

        rec, ci = traversal_utils.load_child_walk(contig, graph)
        regions = traversal_utils.get_regions(threading, s)
        for sec in section_contig(regions, rec, window, split) or []:
            sub, sub_regions = section_query(contig, sec, regions, k)
            first, end, query = trim_query(sub, targets, sub_regions, k)
    """
    first, last = int(section[0]), int(section[1])
    local = [(max(a, first) - first, min(b, last) - first) for a, b in rois if b >= first and a <= last]
    return contig[first:last + k], local


def trim_query(walk, targets, rois, k):
    """Call.trimQuery (:1946-1986).  walk: the section's contig as a string (its windows are the vertices ws; toContig of consecutive
    windows is a substring); targets: mapping name -> sequence; rois: the section's novel regions in its own window numbers, as
    get_regions returns them -> (firstIndex, lastIndex + 1, query).  IndexError where subList(-1, ...) throws: a section without a
    novel window."""
    nwin = max(0, len(walk) - k + 1)
    pos = {}
    for i in range(nwin):
        pos.setdefault(_canonical(walk[i:i + k]), []).append(i)
    novel = [i for a, b in rois for i in range(max(a, 0), min(b, nwin - 1) + 1)]
    first_novel, last_novel = (min(novel), max(novel)) if novel else (-1, -1)
    first, last = 2**31 - 1, 0
    for t in (targets.values() if hasattr(targets, "values") else [s for _, s in targets]):
        for i in range(len(t) - k + 1):
            hit = pos.get(_canonical(t[i:i + k]))
            if hit:
                first = min(first, hit[0])
                last = max(last, hit[-1])
    if first_novel < first:
        first = first_novel
    if last_novel > last:
        last = last_novel
    if first < 0 or last + 1 > nwin or first > last + 1:
        raise IndexError("trimQuery: subList(%d, %d) of %d vertices" % (first, last + 1, nwin))
    return first, last + 1, (walk[first:last + k] if last + 1 > first else "")
