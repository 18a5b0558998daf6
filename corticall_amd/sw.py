"""SmithWaterman (J/utils/alignment/sw/SmithWaterman.java with EDNAFULL): pairwise local alignment with affine gaps, in batches on the
device (ldbg_sw_align_batch), and the arithmetic of its three callers over the arrays it returns: the inversion test of
Call (Call.java:1166-1183), VerifyCalls (VerifyCalls.java:76-111) and EvaluateCalls2 (:205-219).

The device returns, per pair, the score, the ends of the alignment, its columns and two counts (the length of the aligned strings and
the columns that differ); the two strings are text and are built here from the columns and the filtered letters the library hands back."""
import ctypes as C
import re

import numpy as np

from . import _native

# align(String, String) (:46-48): one leading FASTA header; Java's \s is these six characters
_HEADER = re.compile(r"^[ \t\n\x0b\f\r]*>[^\r\n]*[\r\n]+")
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _pack(seq):
    """the header regex, then one byte per UTF-16 unit (a Java char): what is not ASCII becomes '?', which filter turns into X"""
    if isinstance(seq, bytes):
        seq = seq.decode("latin-1")
    seq = _HEADER.sub("", seq, count=1)
    if seq.isascii():
        return seq.encode("ascii")
    return "".join(c if ord(c) < 128 else ("?" if ord(c) < 0x10000 else "??") for c in seq).encode("ascii")


class SWResult:
    """SWResult.java: qseq, sseq, score; beside them the arrays of the pair"""
    def __init__(self, qseq, sseq, score, end_q=-1, end_s=-1, begin_q=-1, begin_s=-1, aligned_len=0, edits=0, columns=b""):
        self.qseq, self.sseq, self.score = qseq, sseq, score
        self.end_q, self.end_s, self.begin_q, self.begin_s = end_q, end_s, begin_q, begin_s
        self.aligned_len, self.edits, self.columns = aligned_len, edits, columns


class SWArrays:
    """the raw arrays of a batch (ldbg_sw_arrays), numpy"""
    def __init__(self, n, columns, ql, sl):
        self.status = np.zeros(n, np.uint8)
        self.score = np.zeros(n, np.float64)
        self.end_q, self.end_s, self.begin_q, self.begin_s, self.aligned_len, self.edits = (np.zeros(n, np.int32) for _ in range(6))
        self.col_off, self.q_off, self.s_off = (np.zeros(n + 1, np.int64) for _ in range(3))
        self.cols = np.zeros(max(1, columns), np.uint8)[:columns]
        self.q_letters = np.zeros(max(1, ql), np.uint8)[:ql]
        self.s_letters = np.zeros(max(1, sl), np.uint8)[:sl]

    def fields(self):
        return [getattr(self, name) for name in _native.SW_FIELDS]


def build_strings(q, s, end_q, end_s, begin_q, begin_s, cols):
    """SWResult.qseq / sseq (:237-259) from the filtered letters (bytes) and the traceback's columns"""
    if end_q < 0:
        return "", ""
    a0, a1 = [], []
    a0.append(b"-" * (begin_s - 1)); a1.append(s[:begin_s - 1])            # reversed: the subject's head was appended last
    a0.append(q[:begin_q - 1]); a1.append(b"-" * (begin_q - 1))
    x, y = begin_q - 1, begin_s - 1
    for c in cols:
        if c == 0:
            a0.append(q[x:x + 1]); a1.append(s[y:y + 1]); x += 1; y += 1
        elif c == 1:
            a0.append(b"-"); a1.append(s[y:y + 1]); y += 1
        else:
            a0.append(q[x:x + 1]); a1.append(b"-"); x += 1
    a0.append(q[end_q:]); a1.append(b"-" * (len(q) - end_q))
    a0.append(b"-" * (len(s) - end_s)); a1.append(s[end_s:])
    return b"".join(a0).decode("latin-1"), b"".join(a1).decode("latin-1")


class SmithWaterman:
    """SmithWaterman() (:34-40: EDNAFULL, open 10, extend 0.5)"""
    def __init__(self, device=0, lib=None):
        self.device = device
        self._lib = lib or _native.default_lib()

    def align_arrays(self, pairs):
        """pairs: [(query, subject)] of str (or bytes) -> SWArrays; no string is built"""
        qs = [_pack(q) for q, _ in pairs]
        ss = [_pack(s) for _, s in pairs]
        n = len(qs)
        qoff = np.zeros(n + 1, np.int64)
        soff = np.zeros(n + 1, np.int64)
        if n:
            qoff[1:] = np.cumsum(np.asarray([len(b) for b in qs], np.int64))
            soff[1:] = np.cumsum(np.asarray([len(b) for b in ss], np.int64))
        d = self._lib.dll
        h = C.c_void_p()
        self._lib.check(d.ldbg_sw_align_batch(C.c_int(self.device), C.c_int64(n), C.c_char_p(b"".join(qs)), qoff.ctypes.data_as(C.c_void_p),
                                              C.c_char_p(b"".join(ss)), soff.ctypes.data_as(C.c_void_p), C.byref(h)))
        try:
            nn, nc, nq, ns = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
            self._lib.check(d.ldbg_sw_result_sizes(h, C.byref(nn), C.byref(nc), C.byref(nq), C.byref(ns)))
            r = SWArrays(n, nc.value, nq.value, ns.value)
            arrs = _native.SwArrays(*[a.ctypes.data_as(C.c_void_p) if a.size else None for a in r.fields()])
            self._lib.check(d.ldbg_sw_result_get(h, C.byref(arrs)))
        finally:
            d.ldbg_sw_result_free(h)
        return r

    @staticmethod
    def results(r):
        """the SWResult of every pair of an SWArrays, strings built; None where the pair is refused (ldbg.h lists the cases)"""
        out = []
        for i in range(len(r.status)):
            if r.status[i] != _native.LDBG_OK:
                out.append(None)
                continue
            q = r.q_letters[r.q_off[i]:r.q_off[i + 1]].tobytes()
            s = r.s_letters[r.s_off[i]:r.s_off[i + 1]].tobytes()
            cols = r.cols[r.col_off[i]:r.col_off[i + 1]].tobytes()
            ends = int(r.end_q[i]), int(r.end_s[i]), int(r.begin_q[i]), int(r.begin_s[i])
            a0, a1 = build_strings(q, s, *ends, cols)
            out.append(SWResult(a0, a1, float(r.score[i]), *ends, int(r.aligned_len[i]), int(r.edits[i]), cols))
        return out

    def align_batch(self, pairs):
        """one device call for all pairs -> [SWResult or None]"""
        return self.results(self.align_arrays(pairs))

    def align(self, qq, ss):
        """SmithWaterman.align(String, String) (:46-71) -> SWResult"""
        r = self.align_batch([(qq, ss)])[0]
        if r is None:
            raise _native.LdbgError(4, "SmithWaterman.align: the pair exceeds what the device takes (include/ldbg.h lists the cases)")
        return r

    def getAlignment(self, qq, ss):
        """:73-87 -> [a0, a1]"""
        r = self.align(qq, ss)
        return [r.qseq, r.sseq]


def pct_identity(aligned_len, edits):
    """Call.java:1181 in float: 100.0f * (((float) (length - edits)) / ((float) length)); nan for length 0"""
    length = np.asarray(aligned_len).astype(np.float32)
    same = (np.asarray(aligned_len, np.int64) - np.asarray(edits, np.int64)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(100.0) * (same / length)


def inversion_identities(child_contig, parental_contigs, k, sw=None):
    """Call.java:1169-1183: the child's stretch against the reverse complement of parental[k:-k] of every parental contig, one batch ->
    (pctIdentity float32[n], pctIdentity >= 90 bool[n])"""
    sw = sw or SmithWaterman()
    inverted = [p[k:len(p) - k].encode("latin-1").translate(_COMP)[::-1].decode("latin-1") for p in parental_contigs]
    r = sw.align_arrays([(child_contig, inv) for inv in inverted])
    if (r.status != _native.LDBG_OK).any():
        raise _native.LdbgError(4, "inversion_identities: a pair exceeds what the device takes (include/ldbg.h lists the cases)")
    pct = pct_identity(r.aligned_len, r.edits)
    return pct, pct >= 90.0


def trimmed_accuracy(a0, a1):
    """VerifyCalls.java:80-98, 107: numMatches / numBases between the leading and the trailing '-' of a0; nan where nothing is left"""
    left = 0
    while left < len(a0) and a0[left] == "-":
        left += 1
    right = len(a0)
    while right - 1 >= 0 and a0[right - 1] == "-":
        right -= 1
    bases = max(0, right - left)
    matches = sum(1 for i in range(left, right) if a0[i] == a1[i])
    return matches / bases if bases else float("nan")
