"""Cases for Smith-Waterman in batches (ldbg_sw_align_batch), shared by tests/test_sw_hostsim.py (the TEST-ONLY host
simulation, 1 lane and 64 lanes in lock step) and tests/test_gpu_sw.py (the HIP library on an MI355X).

The yardstick is `yardstick_align`: SmithWaterman.align (J/utils/alignment/sw/SmithWaterman.java:46-294) restated statement by statement
in pure Python — the header regex, Sequence.add, EDNAFULL.filter, w x h cells of three doubles and three previous types, the scan of all
three states for the maximum, the traceback and the unaligned ends — sharing nothing with the package.  Its matrix comes from the
fixture tests/golden/nuc44.txt, so a typo in the product's table or in the fixture is caught by the other.  Every case compares, per
pair, the score by its bits, the four ends, the column bytes, aligned_len, edits and both strings.

No JVM has run the reference's class (it has no test of its own): the yardstick is a reading of the source."""
import functools
import os
import random
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_MATCH, TYPE_GAPINCOL, TYPE_GAPINROW = 0, 1, 2
PENAL_O, PENAL_E = 10.0, 0.5
JAVA_HEADER = re.compile("^[ \t\n\x0b\f\r]*>[^\r\n]*[\r\n]+")


@functools.lru_cache(maxsize=None)
def matrix():
    """EDNAFULL(): (scoreMat as a dict, acceptable)"""
    with open(os.path.join(ROOT, "tests", "golden", "nuc44.txt")) as f:
        lines = [ln.split() for ln in f if ln.strip()]
    head = lines[0]
    assert len(head) == 16 and len(lines) == 17
    score, acceptable = {}, set()
    for pt in lines[1:]:
        sc = pt[0]
        acceptable.add(sc)
        assert len(pt) == 17
        for jj in range(1, len(pt)):
            qc = head[jj - 1]
            acceptable.add(qc)
            assert (sc, qc) not in score
            score[(sc, qc)] = int(pt[jj])
    return score, acceptable


def java_chars(s):
    """a Java String's chars: UTF-16 units"""
    out = []
    for c in s:
        if ord(c) > 0xFFFF:
            out += ["\ud800", "\udc00"]
        else:
            out.append(c)
    return out


def sequence_add(s):                    # Sequence.java:48-61
    return [c for c in java_chars(s) if c not in "\r\n"]


def ednafull_filter(al):                # EDNAFULL.java:63-80
    _, acceptable = matrix()
    ret = []
    for a in al:
        if a == "\0":
            continue
        if a == "-" or a == ".":
            continue
        ret.append(a if a in acceptable else "X")
    return ret


def yardstick_align(qq, ss):
    """-> dict(q, s, qseq, sseq, score, end_q, end_s, begin_q, begin_s, cols, aligned_len, edits)"""
    score_mat, _ = matrix()
    qq2 = JAVA_HEADER.sub("", qq, count=1)
    ss2 = JAVA_HEADER.sub("", ss, count=1)
    q = ednafull_filter(sequence_add(qq2))
    s = ednafull_filter(sequence_add(ss2))
    w, h = len(q) + 1, len(s) + 1
    sc = [[[0.0, 0.0, 0.0] for _ in range(h)] for _ in range(w)]       # SWCell.score; row 0 and column 0 are set to 0 (:105-115)
    pt = [[[0, 0, 0] for _ in range(h)] for _ in range(w)]             # SWCell.prevType
    for xx in range(1, w):
        for yy in range(1, h):
            m = score_mat.get((q[xx - 1], s[yy - 1]), 10000)
            d = sc[xx - 1][yy - 1]
            fm = max(0, d[TYPE_MATCH] + m)
            fc = max(0, d[TYPE_GAPINCOL] + m)
            fr = max(0, d[TYPE_GAPINROW] + m)
            cs, cp = sc[xx][yy], pt[xx][yy]
            if fm >= fr:
                if fm >= fc:
                    cs[TYPE_MATCH], cp[TYPE_MATCH] = fm, TYPE_MATCH
                else:
                    cs[TYPE_MATCH], cp[TYPE_MATCH] = fc, TYPE_GAPINCOL
            else:
                if fr > fc:
                    cs[TYPE_MATCH], cp[TYPE_MATCH] = fr, TYPE_GAPINROW
                else:
                    cs[TYPE_MATCH], cp[TYPE_MATCH] = fc, TYPE_GAPINCOL
            left = sc[xx][yy - 1]
            fm = max(0, left[TYPE_MATCH] - PENAL_O)
            fc = max(0, left[TYPE_GAPINCOL] - PENAL_E)
            if fm >= fc:
                cs[TYPE_GAPINCOL], cp[TYPE_GAPINCOL] = fm, TYPE_MATCH
            else:
                cs[TYPE_GAPINCOL], cp[TYPE_GAPINCOL] = fc, TYPE_GAPINCOL
            up = sc[xx - 1][yy]
            fm = max(0, up[TYPE_MATCH] - PENAL_O)
            fr = max(0, up[TYPE_GAPINROW] - PENAL_E)
            if fm > fr:
                cs[TYPE_GAPINROW], cp[TYPE_GAPINROW] = fm, TYPE_MATCH
            else:
                cs[TYPE_GAPINROW], cp[TYPE_GAPINROW] = fr, TYPE_GAPINROW
    # getMaxScorePos (:274-294)
    cx = cy = -1
    maxscore = 0
    gap_state_max = False
    for xx in range(w):
        for yy in range(h):
            for i in range(3):
                if maxscore < sc[xx][yy][i]:
                    maxscore = sc[xx][yy][i]
                    cx, cy = xx, yy
                    gap_state_max = i != TYPE_MATCH
    empty = dict(q="".join(q), s="".join(s), qseq="", sseq="", score=-1.0, end_q=-1, end_s=-1, begin_q=-1, begin_s=-1, cols=b"", aligned_len=0, edits=0,
                 gap_state_max=False)
    if cx == -1:
        return empty
    sx, sy, lx, ly = cx, cy, cx, cy
    cs = sc[cx][cy][TYPE_MATCH]
    maxscore = cs
    ct = TYPE_MATCH
    cpt = pt[cx][cy][TYPE_MATCH]
    qchar, schar, cols = [q[cx - 1]], [s[cy - 1]], [0]
    while cs > 0:
        if ct == TYPE_MATCH:
            cx -= 1
            cy -= 1
        elif ct == TYPE_GAPINCOL:
            cy -= 1
        elif ct == TYPE_GAPINROW:
            cx -= 1
        ct = cpt
        cs = sc[cx][cy][ct]
        cpt = pt[cx][cy][ct]
        if cs <= 0:
            break
        if ct == TYPE_MATCH:
            qchar.append(q[cx - 1]); schar.append(s[cy - 1]); cols.append(0)
            lx, ly = cx, cy
        elif ct == TYPE_GAPINCOL:
            qchar.append("-"); schar.append(s[cy - 1]); cols.append(1)
            ly = cy
        elif ct == TYPE_GAPINROW:
            qchar.append(q[cx - 1]); schar.append("-"); cols.append(2)
            lx = cx
    for xx in range(lx - 1, 0, -1):
        qchar.append(q[xx - 1]); schar.append("-")
    for yy in range(ly - 1, 0, -1):
        schar.append(s[yy - 1]); qchar.append("-")
    qchar.reverse()
    schar.reverse()
    cols.reverse()
    for xx in range(sx + 1, w):
        qchar.append(q[xx - 1]); schar.append("-")
    for yy in range(sy + 1, h):
        schar.append(s[yy - 1]); qchar.append("-")
    a0, a1 = "".join(qchar), "".join(schar)
    edits = sum(1 for i in range(len(a0)) if a0[i] != a1[i])           # Call.java:1174-1179
    return dict(q="".join(q), s="".join(s), qseq=a0, sseq=a1, score=float(maxscore), end_q=sx, end_s=sy, begin_q=lx, begin_s=ly, cols=bytes(cols),
                aligned_len=len(a0), edits=edits, gap_state_max=gap_state_max)


@functools.lru_cache(maxsize=None)
def yard(q, s):
    return yardstick_align(q, s)


def bits(x):
    return struct.pack("<d", float(x))


def has_inner_gap(y):
    return 1 in y["cols"] or 2 in y["cols"]


def check(lib, pairs, refused=()):
    """one batch through the library against the yardstick, pair by pair -> the SWArrays"""
    from corticall_amd.sw import SmithWaterman
    sw = SmithWaterman(lib=lib)
    r = sw.align_arrays(pairs)
    res = sw.results(r)
    for i, (q, s) in enumerate(pairs):
        if i in refused:
            assert r.status[i] == 4 and res[i] is None, "pair %d should be refused" % i
            assert r.col_off[i + 1] == r.col_off[i] and r.end_q[i] == -1 and r.aligned_len[i] == 0
            continue
        assert r.status[i] == 0, "pair %d refused" % i
        y = yard(q, s)
        what = "pair %d (%d x %d)" % (i, len(y["q"]), len(y["s"]))
        assert bits(r.score[i]) == bits(y["score"]), "%s: score %r, yardstick %r" % (what, r.score[i], y["score"])
        got = (int(r.end_q[i]), int(r.end_s[i]), int(r.begin_q[i]), int(r.begin_s[i]))
        assert got == (y["end_q"], y["end_s"], y["begin_q"], y["begin_s"]), "%s: ends %r" % (what, got)
        assert r.cols[r.col_off[i]:r.col_off[i + 1]].tobytes() == y["cols"], "%s: columns" % what
        assert (int(r.aligned_len[i]), int(r.edits[i])) == (y["aligned_len"], y["edits"]), "%s: aligned_len, edits" % what
        assert r.q_letters[r.q_off[i]:r.q_off[i + 1]].tobytes().decode("latin-1") == y["q"], "%s: filtered query" % what
        assert r.s_letters[r.s_off[i]:r.s_off[i + 1]].tobytes().decode("latin-1") == y["s"], "%s: filtered subject" % what
        assert (res[i].qseq, res[i].sseq) == (y["qseq"], y["sseq"]), "%s: strings" % what
        assert bits(res[i].score) == bits(y["score"])
    return r


def same_arrays(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a.fields(), b.fields()))


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, edits, alphabet="ACGT"):
    """`edits` substitutions, deletions and insertions of 1-6 bases"""
    s = list(s)
    for _ in range(edits):
        kind = rng.randrange(3)
        at = rng.randrange(len(s) + 1)
        ln = rng.randint(1, 6)
        if kind == 0 and s:
            at = min(at, len(s) - 1)
            s[at] = rng.choice(alphabet)
        elif kind == 1:
            del s[at:at + ln]
        else:
            s[at:at] = [rng.choice(alphabet) for _ in range(ln)]
    return "".join(s)


# ---- the cases
TABLE = [("ACGTTGCATGCA", "ACGTGCATCCA", "ACGTTGCATGCA", "ACG-TGCATCCA", 36.0), ("ACGT", "ACGTACGT", "ACGT----", "ACGTACGT", 20.0), ("A", "T", "", "", -1.0),
         ("AC-G.T", "ACGT", "ACGT", "ACGT", 20.0)]
# the two strings of the class comment (:21), written for BLOSUM62: under EDNAFULL mostly X
PROTEINS = ("EEEEMDQNNSLPPYAGGTWRYII", "IIIIMDQNNSPPYAQGGTWRYEE")


def case_yardstick_table():
    for q, s, a0, a1, score in TABLE:
        y = yardstick_align(q, s)
        assert (y["qseq"], y["sseq"], y["score"]) == (a0, a1, score), (q, s, y)
    y = yardstick_align("acgt", "ACGT")
    assert (y["qseq"], y["sseq"], y["score"]) == ("XXXX", "ACGT", 40000.0)


def case_table(lib):
    check(lib, [(q, s) for q, s, _, _, _ in TABLE] + [("acgt", "ACGT"), PROTEINS])
    from corticall_amd.sw import SmithWaterman
    sw = SmithWaterman(lib=lib)
    for q, s, a0, a1, score in TABLE:
        assert sw.getAlignment(q, s) == [a0, a1]
        assert sw.align(q, s).score == score


QLENS = (0, 1, 2, 63, 64, 65, 127, 128, 129)
SLENS = (0, 1, 2, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def length_pairs():
    rng = random.Random(20)
    base = rand_seq(rng, 140)
    out = []
    for ql in QLENS:
        for sl in SLENS:
            q = mutate(rng, base, 3)[:ql]
            out.append((q.ljust(ql, "A")[:ql], mutate(rng, base[:sl], 2 if sl > 2 else 0).ljust(sl, "C")[:sl]))
    assert [len(q) for q, _ in out[::len(SLENS)]] == list(QLENS) and [len(s) for _, s in out[:len(SLENS)]] == list(SLENS)
    return out


def case_lengths(lib):
    check(lib, length_pairs())
    # alignments cross strip boundaries
    assert any(yard(q, s)["begin_q"] <= 64 < yard(q, s)["end_q"] for q, s in length_pairs())
    assert any(yard(q, s)["end_q"] == -1 for q, s in length_pairs())


def case_lds_limit(lib, monkeypatch):
    """the boundary row in the HBM scratch: LDBG_SW_LDS_CELLS below the subject lengths"""
    whole = check(lib, length_pairs())
    for cells in ("0", "60"):
        monkeypatch.setenv("LDBG_SW_LDS_CELLS", cells)
        assert same_arrays(whole, check(lib, length_pairs()))
    monkeypatch.setenv("LDBG_SW_LDS_CELLS", "0")
    check(lib, gap_pairs())


@functools.lru_cache(maxsize=None)
def random_pairs():
    rng = random.Random(300)
    out = []
    for _ in range(300):
        a = rand_seq(rng, rng.randint(0, 150), "ACGTN")
        b = mutate(rng, a, rng.randint(0, 4), "ACGTN")[:150]
        out.append((a, b))
    return out


def case_random_inputs_have_gaps():
    """a condition on the inputs, not on the product: the gap states are exercised"""
    ys = [yard(q, s) for q, s in random_pairs()]
    assert sum(1 for y in ys if has_inner_gap(y)) >= 100
    assert all(0 <= len(q) <= 150 and 0 <= len(s) <= 150 for q, s in random_pairs())


def case_random(lib):
    check(lib, random_pairs())


def tie_pairs():
    unit = "ACGT"
    rng = random.Random(7)
    block = rand_seq(rng, 30)
    spacer_q, spacer_s = "T" * 70, "G" * 9
    # two identical best cells in different strips: the block twice in the query, 100 rows apart, once in the subject
    two = (block + spacer_q + block, spacer_s + block + spacer_s)
    return [("AAAA", "AAAAAAAA"), ("AAAAAAAA", "AAAA"), (unit * 2, unit * 5), (unit * 5, unit * 2), ("A" * 70, "A" * 66), two, (two[1], two[0])]


def case_ties(lib):
    ps = tie_pairs()
    check(lib, ps)
    y = yard(*ps[5])
    assert y["end_q"] == 30 and y["score"] == 150.0, "the first of the two equal maxima wins"
    assert yard(*ps[6])["end_s"] == 30


@functools.lru_cache(maxsize=None)
def gap_pairs():
    rng = random.Random(130)
    left, mid, right = rand_seq(rng, 100), rand_seq(rng, 130), rand_seq(rng, 100)
    return [(left + mid + right, left + right), (left + right, left + mid + right)]


def case_long_gaps(lib):
    ps = gap_pairs()
    dele, ins = yard(*ps[0]), yard(*ps[1])
    assert "-" * 130 in dele["sseq"] and dele["cols"].count(2) >= 130, "the deletion of 130 bases is taken as one gap"
    assert "-" * 130 in ins["qseq"] and ins["cols"].count(1) >= 130
    check(lib, ps)


def case_letters(lib):
    codes = "ATGCSWRYKMBVHDN*"
    rng = random.Random(16)
    amb = rand_seq(rng, 90, codes)
    core = "ACGTTGCATGCAAGCTTAGC"
    ps = [(amb, mutate(rng, amb, 3, codes)), (codes, codes), (codes, codes[::-1]),
          ("AC-GT.TG\0CA\rTG\nCAAG", core), ("ACGTtGCA GCAAGCT\u00e9AGC", core), ("ACGT\U0001F9ECTGCA", "ACGTTGCA"), ("ACGT\u4e2dTGCA", "ACGTTGCA"),
          (">child contig 1\n" + core, core), (">a\r\n" + core[:10] + "\n" + core[10:] + "\n", "  >b desc\n\n" + core), (core, " \t>s\n" + core),
          (core + ">x", core), ("\n" + core, core)]
    check(lib, ps)
    assert yard(*ps[4])["q"].count("X") == 3 and yard(*ps[6])["q"].count("X") == 1 and yard(*ps[5])["q"].count("X") == 2
    assert yard(*ps[7])["q"] == core and yard(*ps[8])["q"] == core and yard(*ps[8])["s"] == core


@functools.lru_cache(maxsize=None)
def mixed_pairs():
    rng = random.Random(65)
    out = []
    for i in range(65):
        a = rand_seq(rng, (i * 37) % 140)
        out.append((a, mutate(rng, a, i % 4)) if i % 5 else (mutate(rng, a, 2), a))
    return out


def tb_bytes(lq, ls, ws=64):
    return (((lq + ws - 1) // ws) * (ls + ws - 1) * ws + 7) // 8 * 8


def case_batch(lib, n, monkeypatch=None):
    ps = mixed_pairs()[:n]
    whole = check(lib, ps)
    if monkeypatch is None:
        return
    from corticall_amd.sw import SmithWaterman
    sw = SmithWaterman(lib=lib)
    # one at a time: identical arrays
    for i, p in enumerate(ps):
        one = sw.align_arrays([p])
        for name in ("status", "score", "end_q", "end_s", "begin_q", "begin_s", "aligned_len", "edits"):
            assert getattr(one, name)[0:1].tobytes() == getattr(whole, name)[i:i + 1].tobytes(), (i, name)
        assert one.cols.tobytes() == whole.cols[whole.col_off[i]:whole.col_off[i + 1]].tobytes()
    # a small arena: 3 slices or more whether a simulated wavefront has 1 lane or 64, identical arrays
    need64 = [tb_bytes(len(q), len(s)) for q, s in ps if q and s]
    need1 = [tb_bytes(len(q), len(s), 1) for q, s in ps if q and s]
    budget = max(need64)
    assert sum(need64) >= 3 * budget and sum(need1) >= 3 * budget and max(need1) <= budget
    monkeypatch.setenv("LDBG_SW_ARENA_BYTES", str(budget))
    assert same_arrays(whole, check(lib, ps))


def case_refusals(lib, monkeypatch):
    rng = random.Random(8)
    t = rand_seq(rng, 40)
    good = (t[3:33], t)
    # min(|q|, |s|) = 107,374: refused before any budget, at once; the neighbours run
    huge = "A" * 107374
    r = check(lib, [good, (huge, huge), good, ("", t), good], refused={1})
    assert r.status.tolist() == [0, 4, 0, 0, 0]
    from corticall_amd import LdbgError
    from corticall_amd.sw import SmithWaterman
    only = SmithWaterman(lib=lib).align_arrays([(huge, huge)])
    assert only.status.tolist() == [4] and only.q_off[1] == 107374
    # over the arena budget
    big = (rand_seq(rng, 60), rand_seq(rng, 200))
    monkeypatch.setenv("LDBG_SW_ARENA_BYTES", str(tb_bytes(30, 40) + 8))
    check(lib, [good, big, good], refused={1})
    try:
        SmithWaterman(lib=lib).align(*big)
    except LdbgError as e:
        assert e.status == 4
    else:
        raise AssertionError("align did not refuse")


# ---- the callers' arithmetic against string restatements
def call_pct_identity_str(a0, a1):     # Call.java:1174-1181
    edits = sum(1 for l in range(len(a0)) if a0[l] != a1[l])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(100.0) * (np.float32(len(a0) - edits) / np.float32(len(a0)))


def verify_accuracy_str(a0, a1):       # VerifyCalls.java:80-98, 107
    num_bases = num_matches = 0.0
    left_start = 0
    i = 0
    while i < len(a0) and a0[i] == "-":
        left_start += 1
        i += 1
    right_start = len(a0)
    i = len(a0) - 1
    while i >= 0 and a0[i] == "-":
        right_start -= 1
        i -= 1
    for i in range(left_start, right_start):
        num_bases += 1
        if a0[i] == a1[i]:
            num_matches += 1
    return num_matches / num_bases if num_bases else float("nan")


def revcomp_str(s):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    return "".join(comp[c] for c in reversed(s))


def case_helpers_no_library():
    from corticall_amd.sw import pct_identity, trimmed_accuracy
    p = pct_identity(np.asarray([100, 100, 0, 7], np.int32), np.asarray([9, 11, 0, 7], np.int32))
    assert p.dtype == np.float32
    assert p[0] == np.float32(91.0) and p[0] >= 90.0 and p[1] < 90.0 and np.isnan(p[2]) and p[3] == 0
    for a0, a1 in (("--ACGT-A--", "TTACCTTAGG"), ("ACGT", "ACGT"), ("----", "ACGT"), ("", ""), ("-A", "AA"), ("A-C-", "ATCG")):
        got, want = trimmed_accuracy(a0, a1), verify_accuracy_str(a0, a1)
        assert bits(got) == bits(want) or (got != got and want != want), (a0, a1)


def case_helpers(lib):
    from corticall_amd.sw import SmithWaterman, inversion_identities, pct_identity, trimmed_accuracy
    sw = SmithWaterman(lib=lib)
    rng = random.Random(90)
    k = 5
    child = rand_seq(rng, 100)
    inv = revcomp_str(child)

    def subst(s, n):
        s = list(s)
        for at in range(5, 5 + 8 * n, 8):
            s[at] = {"A": "C", "C": "G", "G": "T", "T": "A"}[s[at]]
        return "".join(s)
    flank = lambda s: rand_seq(rng, k) + s + rand_seq(rng, k)
    parents = [flank(inv), flank(subst(inv, 9)), flank(subst(inv, 11)), flank(rand_seq(rng, 100)), flank(mutate(rng, inv, 3))]
    pct, flags = inversion_identities(child, parents, k, sw=sw)
    want = []
    for p in parents:
        y = yard(child, revcomp_str(p[k:len(p) - k]))
        want.append(call_pct_identity_str(y["qseq"], y["sseq"]))
    assert pct.dtype == np.float32 and [bits(x) for x in pct] == [bits(x) for x in want]
    assert flags.tolist() == [bool(x >= 90.0) for x in want]
    y9, y11 = yard(child, revcomp_str(parents[1][k:-k])), yard(child, revcomp_str(parents[2][k:-k]))
    assert (y9["aligned_len"], y9["edits"], y11["aligned_len"], y11["edits"]) == (100, 9, 100, 11), "a pair on either side of 90 %"
    assert flags.tolist()[:3] == [True, True, False]
    # pct_identity over the arrays of a batch equals the strings' count, the empty result's nan included
    ps = mixed_pairs()[:20] + [("A", "T")]
    r = sw.align_arrays(ps)
    got = pct_identity(r.aligned_len, r.edits)
    for i, (q, s) in enumerate(ps):
        y = yard(q, s)
        w = call_pct_identity_str(y["qseq"], y["sseq"])
        assert bits(got[i]) == bits(w) or (np.isnan(got[i]) and np.isnan(w))
    assert np.isnan(got[-1])
    # VerifyCalls over the strings the package builds
    for res, (q, s) in zip(sw.align_batch(ps), ps):
        y = yard(q, s)
        a, b = trimmed_accuracy(res.qseq, res.sseq), verify_accuracy_str(y["qseq"], y["sseq"])
        assert bits(a) == bits(b) or (a != a and b != b)
