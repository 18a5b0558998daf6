"""Cases for Tesserae in batches (ldbg_mosaic_align_batch), shared by tests/test_mosaic_hostsim.py (the TEST-ONLY host
simulation, 1 lane and 64 lanes in lock step) and tests/test_gpu_mosaic.py (the HIP library on an MI355X).

The yardstick is `yardstick_align`: Tesserae.alignAll (J/utils/alignment/mosaic/Tesserae.java:188-495) restated statement by statement
in pure Python — three-dimensional lists of doubles, the traceback kept as doubles and decoded with Java's three casts, the track
builder and toString — sharing nothing with the package.  Every case compares, per problem, llk by its bits, the three path arrays,
every track triple and the edit track."""
import json
import math
import os
import random
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = -1e32
DEFAULTS = (0.025, 0.75, 0.0001, 0.001)
EMISS = [[0.2, 0.2, 0.2, 0.2, 0.2], [0.2, 0.9, 0.05, 0.025, 0.025], [0.2, 0.05, 0.9, 0.025, 0.025], [0.2, 0.025, 0.025, 0.9, 0.05],
         [0.2, 0.025, 0.025, 0.05, 0.9]]


def convert(c):
    return {"A": 3, "C": 2, "G": 4, "T": 1}.get(c, 0)


def argmax(vec):
    m = 0
    for i in range(1, len(vec)):
        if vec[m] < vec[i]:
            m = i
    return m


def tb_divisor(maxl):
    return math.pow(10.0, float(int(math.log(maxl))))


def decode(tb_next, tb_div):
    who_next = int(tb_next) // 10
    state_next = int(tb_next - who_next * 10)
    pos_next = int((tb_next - who_next * 10 - state_next) * tb_div + 1e-6)
    return who_next, state_next, pos_next


def yardstick_align(query, targets, params=DEFAULTS):
    """-> dict(llk, copy, state, pos, path, edit, text); targets: [(name, sequence)]"""
    de, eps, rho, term = params
    ldel, leps, lrho, lterm = math.log(de), math.log(eps), math.log(rho), math.log(term)
    piM = 0.75
    piI = 1 - piM
    lpiM, lpiI = math.log(piM), math.log(piI)
    lmm, lgm, ldm = math.log(1 - 2 * de - rho - term), math.log(1 - eps - rho - term), math.log(1 - eps)
    lsm = [[math.log(x) for x in row] for row in EMISS]
    lsi = [math.log(0.2)] * 5
    panel = [("query", query)] + list(targets)
    nseq = len(targets) + 1
    maxl = max(len(s) for _, s in panel)
    l1 = len(query)

    def cube():
        return [[[0.0] * (l1 + 1) for _ in range(maxl + 1)] for _ in range(nseq + 1)]
    vt_m, vt_i, vt_d, tb_m, tb_i, tb_d = cube(), cube(), cube(), cube(), cube(), cube()
    who_copy = [1] * (nseq + 1)
    who_copy[1] = 0
    maxpath_copy, maxpath_state, maxpath_pos = [0] * (2 * maxl + 1), [0] * (2 * maxl + 1), [0] * (2 * maxl + 1)
    tb_div = tb_divisor(maxl)
    sizeL = 0.0
    for _, t in panel:
        sizeL += len(t)
    sizeL -= len(query)
    lsizeL = math.log(sizeL)
    seq = 1
    for _, t in panel:
        if who_copy[seq] == 1:
            for pos_target in range(l1 + 1):
                for pos_seq in range(len(t) + 1):
                    vt_m[seq][pos_seq][pos_target] = SMALL
                    vt_i[seq][pos_seq][pos_target] = SMALL
                    vt_d[seq][pos_seq][pos_target] = SMALL
        seq += 1
    who_max = state_max = pos_max = who_max_n = state_max_n = pos_max_n = 0
    max_r = SMALL
    seq, seq_10 = 1, 10
    for _, t in panel:
        if who_copy[seq] == 1:
            for pos_seq in range(1, len(t) + 1):
                vt_m[seq][pos_seq][1] = lpiM - lsizeL
                vt_m[seq][pos_seq][1] += lsm[convert(query[0])][convert(t[pos_seq - 1])]
                vt_i[seq][pos_seq][1] = lpiI - lsizeL
                vt_i[seq][pos_seq][1] += lsi[convert(query[0])]
                if pos_seq > 0:
                    vt_d_n = [vt_m[seq][pos_seq - 1][1] + ldel, vt_d[seq][pos_seq - 1][1] + leps]
                    i = argmax(vt_d_n)
                    vt_d[seq][pos_seq][1] = vt_d_n[i]
                    tb_d[seq][pos_seq][1] = seq_10 + 2 * i + 1 + (pos_seq - 1) / tb_div
                if vt_m[seq][pos_seq][1] > max_r:
                    max_r = vt_m[seq][pos_seq][1]
                    who_max, state_max, pos_max = seq, 1, pos_seq
                if vt_i[seq][pos_seq][1] > max_r:
                    max_r = vt_i[seq][pos_seq][1]
                    who_max, state_max, pos_max = seq, 2, pos_seq
        seq += 1
        seq_10 += 10
    for pos_target in range(2, l1 + 1):
        max_rn = SMALL + max_r
        seq, seq_10 = 1, 10
        cq = convert(query[pos_target - 1])
        for _, t in panel:
            if who_copy[seq] == 1:
                for pos_seq in range(1, len(t) + 1):
                    vt_m[seq][pos_seq][pos_target] = max_r + lrho + lpiM - lsizeL
                    tb_m[seq][pos_seq][pos_target] = who_max * 10 + state_max + pos_max / tb_div
                    vt_m_n = [vt_m[seq][pos_seq - 1][pos_target - 1] + lmm, vt_i[seq][pos_seq - 1][pos_target - 1] + lgm,
                              vt_d[seq][pos_seq - 1][pos_target - 1] + ldm]
                    i = argmax(vt_m_n)
                    if vt_m_n[i] > vt_m[seq][pos_seq][pos_target]:
                        vt_m[seq][pos_seq][pos_target] = vt_m_n[i]
                        tb_m[seq][pos_seq][pos_target] = seq_10 + i + 1 + (pos_seq - 1) / tb_div
                    vt_m[seq][pos_seq][pos_target] += lsm[cq][convert(t[pos_seq - 1])]
                    vt_i[seq][pos_seq][pos_target] = max_r + lrho + lpiI - lsizeL
                    tb_i[seq][pos_seq][pos_target] = who_max * 10 + state_max + pos_max / tb_div
                    vt_i_n = [vt_m[seq][pos_seq][pos_target - 1] + ldel, vt_i[seq][pos_seq][pos_target - 1] + leps]
                    i = argmax(vt_i_n)
                    if vt_i_n[i] > vt_i[seq][pos_seq][pos_target]:
                        vt_i[seq][pos_seq][pos_target] = vt_i_n[i]
                        tb_i[seq][pos_seq][pos_target] = seq_10 + i + 1 + pos_seq / tb_div
                    vt_i[seq][pos_seq][pos_target] += lsi[cq]
                    if pos_target < l1 and pos_seq > 1:
                        vt_d_n = [vt_m[seq][pos_seq - 1][pos_target] + ldel, vt_d[seq][pos_seq - 1][pos_target] + leps]
                        i = argmax(vt_d_n)
                        vt_d[seq][pos_seq][pos_target] = vt_d_n[i]
                        tb_d[seq][pos_seq][pos_target] = seq_10 + 2 * i + 1 + (pos_seq - 1) / tb_div
                    if vt_m[seq][pos_seq][pos_target] > max_rn:
                        max_rn = vt_m[seq][pos_seq][pos_target]
                        who_max_n, state_max_n, pos_max_n = seq, 1, pos_seq
                    if vt_i[seq][pos_seq][pos_target] > max_rn:
                        max_rn = vt_i[seq][pos_seq][pos_target]
                        who_max_n, state_max_n, pos_max_n = seq, 2, pos_seq
            seq += 1
            seq_10 += 10
        max_r = max_rn
        who_max, state_max, pos_max = who_max_n, state_max_n, pos_max_n
    llk = max_r + lterm
    cp = 2 * maxl
    maxpath_copy[cp], maxpath_state[cp], maxpath_pos[cp] = who_max, state_max, pos_max
    tb_next = 0.0
    pos_target = l1
    while pos_target >= 1:
        if state_max == 1:
            tb_next = tb_m[who_max][pos_max][pos_target]
        elif state_max == 2:
            tb_next = tb_i[who_max][pos_max][pos_target]
        elif state_max == 3:
            tb_next = tb_d[who_max][pos_max][pos_target]
        who_next, state_next, pos_next = decode(tb_next, tb_div)
        cp -= 1
        assert cp >= 0, "ArrayIndexOutOfBoundsException"
        maxpath_copy[cp], maxpath_state[cp], maxpath_pos[cp] = who_next, state_next, pos_next
        who_max, state_max, pos_max = who_next, state_next, pos_next
        if maxpath_state[cp + 1] != 3:
            pos_target -= 1
    cp += 1
    seqs = panel
    end = 2 * maxl
    path = []
    # the query's track
    sb, posStart, posEnd, pos_target = [], -1, -1, 1
    for i in range(cp, end + 1):
        if maxpath_state[i] == 3:
            sb.append("-")
        else:
            if posStart == -1:
                posStart = pos_target - 1
            posEnd = pos_target - 1
            sb.append(seqs[0][1][pos_target - 1])
            pos_target += 1
    path.append((seqs[0][0], "".join(sb), (posStart, posEnd)))
    # the edit track
    sb, pos_target = [], 1
    for i in range(cp, end + 1):
        if maxpath_state[i] == 1:
            assert maxpath_copy[i] >= 1 and maxpath_pos[i] >= 1
            sb.append("|" if seqs[0][1][pos_target - 1] == seqs[maxpath_copy[i] - 1][1][maxpath_pos[i] - 1] else " ")
            pos_target += 1
        elif maxpath_state[i] == 2:
            pos_target += 1
            sb.append("^")
        else:
            sb.append("~")
    edit = "".join(sb)
    # the copying tracks
    assert maxpath_copy[cp] >= 1
    currentTrack = seqs[maxpath_copy[cp] - 1][0]
    sb, posStart, posEnd, lastKnownPos, uppercase = [], -1, -1, -1, True
    for i in range(cp, end + 1):
        if (i > cp and maxpath_copy[i] == maxpath_copy[i - 1] and abs(maxpath_pos[i] - maxpath_pos[i - 1]) > 1) or maxpath_pos[i] == lastKnownPos + 1:
            path.append((currentTrack, "".join(sb), (posStart, posEnd)))
            uppercase = not uppercase
            lastKnownPos = maxpath_pos[i - 1]
            if posStart != posEnd:
                posStart = maxpath_pos[i] - 1
                posEnd = maxpath_pos[i] - 1
            currentTrack = seqs[maxpath_copy[i] - 1][0]
            sb = [" " * (i - cp)]
        if i > cp and maxpath_copy[i] != maxpath_copy[i - 1]:
            path.append((currentTrack, "".join(sb), (posStart, posEnd)))
            uppercase = True
            if posStart != posEnd:
                posStart = maxpath_pos[i] - 1
                posEnd = maxpath_pos[i] - 1
            currentTrack = seqs[maxpath_copy[i] - 1][0]
            sb = [" " * (i - cp)]
        if maxpath_state[i] == 2:
            sb.append("-")
        else:
            assert maxpath_copy[i] >= 1 and maxpath_pos[i] >= 1
            c = seqs[maxpath_copy[i] - 1][1][maxpath_pos[i] - 1]
            c = c.upper() if uppercase else c.lower()
            if posStart == -1:
                posStart = maxpath_pos[i] - 1
            posEnd = maxpath_pos[i] - 1
            sb.append(c)
    path.append((currentTrack, "".join(sb), (posStart, posEnd)))
    # toString
    maxNameLength = 0
    for name, _, se in path:
        maxNameLength = max(maxNameLength, len("%s (%d-%d)" % (name, se[0], se[1])))
    text = []
    for i, (name, track, se) in enumerate(path):
        text.append(("%s (%d-%d)" % (name, se[0], se[1])).rjust(maxNameLength) + " " + track + "\n")
        if i == 0:
            text.append(" ".rjust(maxNameLength) + " " + edit + "\n")
    text.append("\nMllk: " + repr(llk) + "\n")
    return dict(llk=llk, copy=maxpath_copy[cp:], state=maxpath_state[cp:], pos=maxpath_pos[cp:], path=path, edit=edit, text="".join(text))


_YARD = {}


def yard(query, targets, params=DEFAULTS):
    """the yardstick's answer, computed once per problem and shared by every test that needs it"""
    key = (query, tuple(targets), params)
    if key not in _YARD:
        _YARD[key] = yardstick_align(query, list(targets), params)
    return _YARD[key]


def bits(x):
    return struct.pack("<d", x)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, every=9):
    out = list(s)
    for i in range(rng.randrange(every), len(out), every):
        out[i] = rng.choice([c for c in "ACGT" if c != out[i]])
    return "".join(out)


def supported(query, targets):
    return bool(query) and bool(targets) and sum(len(s) for _, s in targets) > 0 and max([len(query)] + [len(s) for _, s in targets]) > 2


def check(lib, problems, params=DEFAULTS, refused=()):
    """one align_batch of `problems` [(query, [(name, seq)])] against the yardstick; refused: indices that must be marked unsupported"""
    from corticall_amd.mosaic import Tesserae
    t = Tesserae(*params, lib=lib)
    status, llk, poff, copy, state, pos = t.align_arrays(problems)
    res = t.align_batch(problems)
    assert len(res) == len(problems) == len(status)
    for i, (q, ts) in enumerate(problems):
        if i in refused:
            assert status[i] == 4 and res[i] is None and poff[i + 1] == poff[i], (i, status[i])
            continue
        assert status[i] == 0, (i, q, ts)
        y = yard(q, tuple(ts), params)
        assert bits(llk[i]) == bits(y["llk"]), (i, llk[i], y["llk"])
        assert copy[poff[i]:poff[i + 1]].tolist() == y["copy"], i
        assert state[poff[i]:poff[i + 1]].tolist() == y["state"], i
        assert pos[poff[i]:poff[i + 1]].tolist() == y["pos"], i
        assert res[i].path == y["path"], i
        assert res[i].edit_track == y["edit"], i
        assert str(res[i]) == y["text"], i
    return status, llk, poff, copy, state, pos


def golden(name):
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "tesserae_small.json")))[name]
    return d["query"], [tuple(x) for x in d["targets"]]


# ---- the cases
def case_yardstick_small_test():
    """the literal yardstick itself, on the CPU: TestTesserae.smallTest and the layout its comment documents"""
    q, ts = golden("smallTest")
    y = yard(q, tuple(ts))
    assert y["path"] == [("query", "GTAGGCGAGATGACGCCAT", (0, 18)), ("template0", "GTAGGCG", (0, 6)), ("template1", " " * 7 + "AGATGACGCCAT", (7, 18))]
    assert y["edit"] == "|" * 19
    assert y["llk"] == -26.96475012162965


def case_small_tests(lib):
    q, ts = golden("smallTest")
    check(lib, [(q, ts)])
    from corticall_amd.mosaic import Tesserae
    t = Tesserae(lib=lib)
    ps = t.align(q, dict(ts))
    assert len(ps) == 3
    assert ps == [("query", "GTAGGCGAGATGACGCCAT", (0, 18)), ("template0", "GTAGGCG", (0, 6)), ("template1", " " * 7 + "AGATGACGCCAT", (7, 18))]
    assert t.getMaximumLogLikelihood() == -26.96475012162965 and t.edit_track == "|" * 19
    assert str(t) == yard(q, tuple(ts))["text"]
    q2, ts2 = golden("anotherSmallTest")
    check(lib, [(q2, ts2)])


def unshared_kmers(s1, s2, k):
    ks1 = {s1[i:i + k] for i in range(len(s1) - k + 1)}
    ks2 = {s2[i:i + k] for i in range(len(s2) - k + 1)}
    return len(ks1 | ks2) - len(ks1 & ks2)


def case_mosaic_alignment(lib):
    """TestTesserae.testMosaicAlignment at 120 bases: the query switches template at 30 / 60 / 90"""
    rng = random.Random(1000)
    templates = [rand_seq(rng, 120), rand_seq(rng, 120)]
    ks, rb, last, phase = [], [], 0, 0
    for recomb in (30, 60, 90):
        sub = templates[phase][last:recomb]
        rb.append(sub)
        ks.append(("template%d" % phase, " " * last + sub))
        phase = 1 - phase
        last = recomb
    sub = templates[phase][last:119]
    ks.append(("template%d" % phase, " " * 90 + sub))
    rb.append(sub)
    query = "".join(rb)
    ks.insert(0, ("query", query))
    ts = [("template0", templates[0]), ("template1", templates[1])]
    check(lib, [(query, ts)])
    from corticall_amd.mosaic import Tesserae
    ps = Tesserae(lib=lib).align(query, dict(ts))
    assert len(ps) == len(ks)
    for (name, track, _), (kname, ktrack) in zip(ps, ks):
        assert name == kname
        assert unshared_kmers(track.replace(" ", ""), ktrack.replace(" ", ""), 11) <= 2


TARGET_LENGTHS = (1, 3, 63, 64, 65, 129)
QUERY_LENGTHS = (1, 2, 3, 64, 65)


def length_problems():
    rng = random.Random(19)
    out = []
    for ql in QUERY_LENGTHS:
        for tl in TARGET_LENGTHS:
            if max(ql, tl) <= 2:
                continue
            t = rand_seq(rng, tl)
            q = mutate(rng, (t * (ql // tl + 1))[:ql]) if ql > 3 else rand_seq(rng, ql)
            out.append((q, [("t%d" % tl, t)]))
    # 1, 2, 3 and 65 targets per problem, a zero-length target among others
    base = rand_seq(rng, 70)
    for nt in (1, 2, 3, 65):
        ts = [("h%d" % j, mutate(rng, base[j % 5:j % 5 + rng.randrange(3, 7)], 4)) for j in range(nt)]
        out.append((base[2:22], ts))
    out.append((base[:30], [("a", base[:20]), ("empty", ""), ("b", mutate(rng, base[10:45]))]))
    out.append((base[:30], [("empty", ""), ("b", base[5:40]), ("empty2", "")]))
    return out


def case_lengths(lib):
    ps = length_problems()
    assert {len(ts[0][1]) for _, ts in ps if len(ts) == 1} >= set(TARGET_LENGTHS)
    assert {len(ts) for _, ts in ps} >= {1, 2, 3, 65}
    check(lib, ps)


def case_hbm_columns(lib, monkeypatch):
    """the same with the rolling columns in the per-problem HBM scratch (no problem small enough for LDS)"""
    monkeypatch.setenv("LDBG_MOSAIC_LDS_CELLS", "0")
    check(lib, length_problems())
    # the carries of the D chain through global memory: the deleted runs of 70 and 130 bases, the inserted one
    dels, ins = gap_problems()
    for (q, ts), gap in zip(dels, (70, 130)):
        assert longest_run(yard(q, tuple(ts), GAP_PARAMS)["state"], 3) >= gap
    check(lib, dels + ins, GAP_PARAMS)


def mixed_problems(n):
    rng = random.Random(4242)
    out = []
    for i in range(n):
        nt = 1 + i % 4
        base = rand_seq(rng, 48)
        ts = [("p%d_%d" % (i, j), mutate(rng, base[rng.randrange(6):rng.randrange(14, 48)], 5 + j)) for j in range(nt)]
        a = rng.randrange(10)
        out.append((mutate(rng, base[a:a + 3 + (7 * i) % 30], 11), ts))
    return out


def case_batch(lib, n, monkeypatch=None):
    ps = mixed_problems(65)[:n]
    whole = check(lib, ps)
    if monkeypatch is None:
        return
    # one at a time: identical arrays
    from corticall_amd.mosaic import Tesserae
    t = Tesserae(lib=lib)
    for i, p in enumerate(ps):
        s1, l1, o1, c1, st1, p1 = t.align_arrays([p])
        assert bits(l1[0]) == bits(whole[1][i])
        for one, all_ in ((c1, whole[3]), (st1, whole[4]), (p1, whole[5])):
            assert one.tolist() == all_[whole[2][i]:whole[2][i + 1]].tolist()
    # a small arena: 3 slices or more, identical arrays
    need = [((len(q) * sum(len(s) for _, s in ts) + 7) // 8) * 8 for q, ts in ps]
    budget = max(max(need), sum(need) // 4)
    assert sum(need) >= 3 * budget and max(need) <= budget
    monkeypatch.setenv("LDBG_MOSAIC_ARENA_BYTES", str(budget))
    sliced = check(lib, ps)
    for a, b in zip(whole, sliced):
        assert a.tobytes() == b.tobytes()


def case_ties(lib):
    rng = random.Random(5)
    t = rand_seq(rng, 40)
    ps = [(t[5:35], [("first", t), ("second", t)]), (mutate(rng, t[3:33]), [("first", t), ("second", t), ("third", t)])]
    check(lib, ps)
    for q, ts in ps:
        assert {name for name, _, _ in yard(q, tuple(ts))["path"][1:]} == {"first"}


def case_non_bases(lib):
    rng = random.Random(6)
    t = rand_seq(rng, 50)
    tn = t[:10] + "NN" + t[12:20].lower() + t[20:]
    qn = t[4:15] + "n" + t[16:30] + "Nacgt" + t[35:45]
    check(lib, [(qn, [("withN", tn), ("plain", t)]), ("NNNN", [("allN", "NNNNNN")]), (t[:20].lower(), [("upper", t)])])


GAP_PARAMS = (0.025, 0.9, 1e-12, 0.001)


def longest_run(states, s):
    best = cur = 0
    for x in states:
        cur = cur + 1 if x == s else 0
        best = max(best, cur)
    return best


def gap_problems():
    rng = random.Random(77)
    dels = []
    for gap in (70, 130):
        t = rand_seq(rng, 30 + gap + 30)
        dels.append((t[:30] + t[30 + gap:], [("t", t)]))
    t = rand_seq(rng, 60)
    ins = [(t[:30] + rand_seq(rng, 70) + t[30:], [("t", t)])]
    return dels, ins


def case_long_gaps(lib):
    dels, ins = gap_problems()
    for (q, ts), gap in zip(dels, (70, 130)):
        assert longest_run(yard(q, tuple(ts), GAP_PARAMS)["state"], 3) >= gap      # a delete run across a 64-cell boundary
    assert longest_run(yard(ins[0][0], tuple(ins[0][1]), GAP_PARAMS)["state"], 2) >= 64
    check(lib, dels + ins, GAP_PARAMS)


# ---- the encode / decode quirk
def roundtrip_np(who, state, pos, div):
    """Java's encode (:270) and decode (:363-365) over arrays, in numpy's IEEE doubles (elementwise, no fused operations)"""
    tb = (who * 10 + state).astype(np.float64) + pos.astype(np.float64) / div
    w = tb.astype(np.int64) // 10
    s = (tb - (w * 10).astype(np.float64)).astype(np.int64)
    p = ((tb - (w * 10).astype(np.float64) - s.astype(np.float64)) * div + 1e-6).astype(np.int64)
    return w, s, p


def quirk_search(nseq, maxl):
    """(who, state, pos) within a panel of nseq sequences whose longest has maxl bases where the decoded position differs from the
    integer written"""
    div = tb_divisor(maxl)
    who, state, pos = np.meshgrid(np.arange(2, nseq + 1), np.arange(1, 4), np.arange(0, maxl + 1), indexing="ij")
    who, state, pos = who.ravel(), state.ravel(), pos.ravel()
    w, s, p = roundtrip_np(who, state, pos, div)
    bad = (w != who) | (s != state) | (p != pos)
    return who[bad], state[bad], pos[bad]


def quirk_problem():
    """a problem whose path runs through a cell the decode moves: 14 targets of 3..8 bases, then one of 3,000 (tb_divisor = 10^8) that
    the query copies around a position the search found for match states of the last sequence"""
    nshort, maxl, l1 = 14, 3000, 12
    who, state, pos = quirk_search(nshort + 2, maxl)
    sel = (who == nshort + 2) & (state == 1) & (pos > 100) & (pos < maxl - 100)
    assert sel.any(), "no position of the long target decodes wrongly"
    p = int(pos[sel][0])                # tb_m of (pos_seq = p + 1) writes p
    rng = random.Random(31)
    ts = [("s%d" % j, rand_seq(rng, rng.randrange(3, 9))) for j in range(nshort)]
    long_t = rand_seq(rng, maxl)
    ts.append(("long", long_t))
    start = p + 1 - 6                   # the query's 7th base sits on pos_seq = p + 1 (1-based)
    return (long_t[start - 1:start - 1 + l1], ts), p


def case_quirk(lib):
    (q, ts), p = quirk_problem()
    y = yard(q, tuple(ts))
    who = len(ts) + 1
    moved = [i for i in range(len(y["pos"]) - 1) if y["copy"][i] == y["copy"][i + 1] == who and y["state"][i + 1] == 1 and y["pos"][i + 1] == p + 1
             and y["pos"][i] != p]
    assert moved, "the yardstick's path does not pass the moved cell"
    check(lib, [(q, ts)])


def case_roundtrip(lib):
    """the kernel's encode and decode alone against numpy's doubles: who <= 200, pos <= 25,000"""
    import ctypes as C
    for div, max_pos in ((1e10, 25000), (1e8, 3000), (1e7, 1100), (100.0, 50)):
        who, state, pos = np.meshgrid(np.arange(0, 201), np.arange(1, 4), np.arange(0, max_pos + 1), indexing="ij")
        who, state, pos = (x.ravel().astype(np.int32) for x in (who, state, pos))
        out = np.zeros(3 * len(who), np.int32)
        lib.check(lib.dll.ldbg_mosaic_tb_roundtrip(0, C.c_double(div), C.c_int64(len(who)), who.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p),
                                                   pos.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        w, s, p = roundtrip_np(who.astype(np.int64), state.astype(np.int64), pos.astype(np.int64), div)
        got = out.reshape(-1, 3)
        assert (got[:, 0] == w).all() and (got[:, 1] == s).all() and (got[:, 2] == p).all()
        if div >= 1e8:
            assert (p != pos).any()     # (the precision does run out inside the range: the comparison is not hollow)


def case_refusals(lib, monkeypatch):
    rng = random.Random(8)
    t = rand_seq(rng, 40)
    good = (t[3:33], [("t", t)])
    ps = [good, ("", [("t", t)]), good, (t[:10], []), good, ("AC", [("a", "GT"), ("b", "A")]), good, ("ACG", [("e", ""), ("f", "")]), good]
    refused = {1, 3, 5, 7}
    assert [i for i, (q, ts) in enumerate(ps) if not supported(q, ts)] == sorted(refused)
    check(lib, ps, refused=refused)
    # over the arena budget: marked per problem, the neighbours unaffected
    big = (rand_seq(rng, 60), [("big", rand_seq(rng, 200))])
    monkeypatch.setenv("LDBG_MOSAIC_ARENA_BYTES", str(30 * 40 + 8))
    check(lib, [good, big, good, ("", [("t", t)]), good], refused={1, 3})
    from corticall_amd import LdbgError
    from corticall_amd.mosaic import Tesserae
    for q, ts in (ps[1], ps[3], ps[5], big):
        try:
            Tesserae(lib=lib).align(q, dict(ts))
        except LdbgError as e:
            assert e.status == 4
        else:
            raise AssertionError("align did not refuse")


# ---- sectionContig / trimQuery against string restatements
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def canonical(sk):
    rc = "".join(_COMP[c] for c in reversed(sk))
    return min(sk, rc)


def get_regions_str(rois, kmers):
    regions, start, stop = [], -1, 0
    for i, km in enumerate(kmers):
        if canonical(km) in rois:
            if start == -1:
                start = i
            stop = i
        elif start > -1:
            regions.append((start, stop))
            start, stop = -1, 0
    if start > -1:
        regions.append((start, stop))
    return regions


def section_contig_str(rois, w, window, split):
    """Call.java:2383-2422 over a list of k-mer strings"""
    regions = get_regions_str(rois, w)
    if len(regions) > 0:
        subcontigStart = regions[0][0] - window
        if subcontigStart < 0:
            subcontigStart = 0
        subcontigStop = regions[-1][1] + window
        if subcontigStop >= len(w):
            subcontigStop = len(w) - 1
        sections = []
        for i in range(len(regions) - 1):
            if regions[i + 1][0] - regions[i][1] > split:
                sections.append((subcontigStart, regions[i][1] + window))
                subcontigStart = regions[i + 1][0] - window
        sections.append((subcontigStart, subcontigStop))
        wss = []
        for a, b in sections:
            ws = []
            for i in range(a, b + 1):
                assert 0 <= i < len(w)
                ws.append(w[i])
            wss.append((a, b, ws))
        return wss
    return None


def trim_query_str(ws, targets, rois, k):
    """Call.java:1946-1986 over a list of k-mer strings"""
    firstIndex, lastIndex, firstNovel, lastNovel = 2**31 - 1, 0, -1, -1
    pos = {}
    for i in range(len(ws)):
        pos.setdefault(canonical(ws[i]), []).append(i)
        if canonical(ws[i]) in rois:
            if firstNovel == -1:
                firstNovel = i
            lastNovel = i
    for target in targets.values():
        for i in range(len(target) - k + 1):
            ck = canonical(target[i:i + k])
            if ck in pos:
                fi, li = pos[ck][0], pos[ck][-1]
                if fi < firstIndex:
                    firstIndex = fi
                if li > lastIndex:
                    lastIndex = li
    if firstNovel < firstIndex:
        firstIndex = firstNovel
    if lastNovel > lastIndex:
        lastIndex = lastNovel
    if firstIndex < 0:
        raise IndexError("subList(-1, ...)")
    sub = ws[firstIndex:lastIndex + 1]
    return firstIndex, lastIndex + 1, sub[0] + "".join(x[-1] for x in sub[1:])


def case_section_and_trim():
    from corticall_amd.mosaic import section_contig, section_query, trim_query
    k = 7
    rng = random.Random(12)
    contig = rand_seq(rng, 160)
    kmers = [contig[i:i + k] for i in range(len(contig) - k + 1)]
    spans = {0: [], 1: [(40, 48)], 3: [(5, 9), (20, 30), (120, 150)]}
    for nreg, sp in spans.items():
        rois = {canonical(kmers[i]) for a, b in sp for i in range(a, b + 1)}
        regions = get_regions_str(rois, kmers)
        assert len(regions) == nreg
        for window in (0, 3, 12, 500):           # 12 clips at the left of the first region of the three, 500 at both ends
            for split in (5, 10, 11, 89, 90, 1000):      # gaps of 10 and 89 between the three regions: either side of each
                want = None
                try:
                    want = section_contig_str(rois, kmers, window, split)
                except AssertionError:
                    try:
                        section_contig(regions, kmers, window, split)
                    except IndexError:
                        continue
                    raise AssertionError("section_contig did not raise")
                got = section_contig(regions, kmers, window, split)
                assert got == want, (nreg, window, split)
                if want is None:
                    continue
                for a, b, ws in want:
                    sub = contig[a:b + k]
                    sub_regions = get_regions_str(rois, ws)
                    targets = {"m": contig[max(0, a - 5):a + 25], "rc": "".join(_COMP[c] for c in reversed(contig[b - 10:b + k])), "far": rand_seq(rng, 40)}
                    assert trim_query(sub, targets, sub_regions, k) == trim_query_str(ws, targets, rois, k)
                    # the same from what the hand-over returns: the contig, a section of section_contig, the whole walk's regions
                    assert section_query(contig, (a, b, ws), regions, k) == (sub, sub_regions)
    # the raising case: a section without a novel window
    ws = kmers[60:80]
    for f in (lambda: trim_query(contig[60:79 + k], {"m": contig[50:90]}, [], k), lambda: trim_query_str(ws, {"m": contig[50:90]}, set(), k)):
        try:
            f()
        except IndexError:
            continue
        raise AssertionError("trimQuery did not raise")
