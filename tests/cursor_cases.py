"""Cases for cursors advanced in batches on the device (ldbg_engine_cursor_batch), shared by the host-simulation run
(tests/test_cursor_hostsim.py) and the GPU run (tests/test_gpu_cursor.py).

Nothing expected here comes from the code under test.  The yardstick restates the reference's loops over the CPU oracle's cursor
(Engine.seek / has_next / has_previous / next / previous): assemble(seed, goForward) (TraversalEngine.java:128-145), assemble(seed)
(:112-126), and the loop bodies of ComputeInheritance.callVariant (:119-165) and ComputeAssemblyQuality.callVariant (:104-149), whose
stop rules are applied here on the oracle's vertices and Graph.get_record.  Every seed of every batch is compared; a seed on which the
oracle raises must carry the matching status."""
import collections
import random

import numpy as np
import pytest

import corticall_amd as ca
from corticall_amd import BOTH, FORWARD, REVERSE, ContigStopper, CortexGraph, TraversalEngineFactory
from tests import roi_cases as rc
from tests.parity_cases import Case, FIG1, FIG1_READ, device_seeds, genome_with_repeats, mutate, rand_seq

END, LIMIT, STOP, FAILED = 0, 1, 2, 3
OK, NULLPOINTER, CAPACITY = 0, 1, 2
_B = np.frombuffer(b"ACGT", dtype=np.uint8)


def is_bases(s):
    return all(c in "ACGT" for c in s)


def decode(words, k):
    """packed k-mers u64[n, W] (2k bits right-aligned over the words, most significant word first) -> list of strings"""
    n, W = words.shape
    out = np.empty((n, k), dtype=np.uint8)
    for p in range(k):
        off = 2 * (k - 1 - p)
        out[:, p] = _B[((words[:, W - 1 - off // 64] >> np.uint64(off % 64)) & np.uint64(3)).astype(np.int64)]
    return [bytes(r).decode() for r in out]


# ---------------------------------------------------------------- the yardstick
class Yardstick:
    def __init__(self, orc, oe, og, k):
        self.orc, self.oe, self.og, self.k = orc, oe, og, k
        self._rec = {}

    def record(self, i):
        if i not in self._rec:
            w, cov, ed = self.og.get_record(i)
            self._rec[i] = (self.orc.decode_kmer(w, self.k), cov, ed)
        return self._rec[i]

    def stops(self, km, rec, fwd, colour, deg1, target):
        """-> True / False, or None for the reference's NullPointerException"""
        if colour is not None:
            if rec < 0:
                return None
            canon, cov, ed = self.record(rec)
            if cov[colour] > 0:                                        # (a Java int already)
                ind, outd = bin(ed[colour] >> 4).count("1"), bin(ed[colour] & 15).count("1")
                if not deg1:
                    return True
                same = km == canon
                if ((ind if same else outd) if fwd else (outd if same else ind)) == 1:
                    return True
        return target is not None and km == target

    def direction(self, seed, fwd, max_steps, colour=None, deg1=False, target=None):
        """-> (vertices in the order stepped, end reason, status)"""
        oe, out = self.oe, []
        has, step = (oe.has_next, oe.next) if fwd else (oe.has_previous, oe.previous)
        try:
            oe.seek(seed)
            while True:
                if not has():
                    return out, END, OK
                if len(out) >= max_steps:
                    return out, LIMIT, OK
                km, rec = step()
                out.append((km, rec))
                s = self.stops(km, rec, fwd, colour, deg1, target)
                if s is None:
                    return out, FAILED, NULLPOINTER
                if s:
                    return out, STOP, OK
        except self.orc.OracleError as ex:
            assert "NullPointerException" in str(ex), ex
            return out, FAILED, NULLPOINTER


def check(cs, oe, e, seeds, direction, engine_max, max_steps=None, colour=None, deg1=False, targets=None, device=False, tag=""):
    """one batch against the yardstick, every seed -> (per seed (reverse part, forward part) as stepped, Counter of end reasons and statuses)"""
    k = cs.k
    y = Yardstick(cs.orc, oe, cs.og, k)
    ms = max_steps if (max_steps is not None and max_steps > 0) else engine_max
    if device and len(seeds):
        r = e.assemble_batch_arrays(device_seeds(cs.lib, seeds, k), direction, max_steps, colour, deg1,
                                    device_seeds(cs.lib, targets, k) if targets is not None else None)
    else:
        r = e.assemble_batch_arrays(seeds, direction, max_steps, colour, deg1, targets)
    n = len(seeds)
    offs = r["offsets"]
    assert offs.shape == (n + 1,) and offs[0] == 0 and r["rec"].shape == (offs[n],) and r["words"].shape[0] == offs[n], tag
    strs = decode(r["words"], k) if offs[n] else []
    got = list(zip(strs, r["rec"].tolist()))
    stats, parts = collections.Counter(), []
    for i, s in enumerate(seeds):
        t = targets[i] if targets is not None and is_bases(targets[i]) else None
        rv, rr, rs = y.direction(s, False, ms, colour, deg1, t) if direction in (BOTH, REVERSE) else ([], END, OK)
        fw, fr, fs = y.direction(s, True, ms, colour, deg1, t) if direction in (BOTH, FORWARD) else ([], END, OK)
        where = (tag, i, s, direction, max_steps, colour, deg1, t)
        assert (int(r["n_reverse"][i]), int(r["n_forward"][i])) == (len(rv), len(fw)), where
        assert (int(r["end_reverse"][i]), int(r["end_forward"][i])) == (rr, fr), where
        assert int(r["status"][i]) == (rs if rs != OK else fs), where
        srec = cs.og.find(s)[0] if is_bases(s) else -1
        assert int(r["seed_rec"][i]) == srec, where
        mine = got[offs[i]:offs[i + 1]]
        exp = rv[::-1] + ([(s, srec)] if direction == BOTH else []) + fw
        if direction == BOTH and not is_bases(s):                     # no packed form to come back in: its record only
            assert len(mine) == len(exp) and mine[len(rv)][1] == -1, where
            mine = mine[:len(rv)] + [(s, -1)] + mine[len(rv) + 1:]
        assert mine == exp, where
        stats[("rev", rr)] += 1; stats[("fwd", fr)] += 1; stats[("status", rs if rs != OK else fs)] += 1
        parts.append((rv, fw, rr, fr))
    return parts, stats


# ---------------------------------------------------------------- graphs
def family(orc, lib, tmp, k, seed, with_links, n=1500, name=None):
    """kid / mom / dad genomes of about n bases with repeats and a tandem repeat (cycles); with an even k a planted palindrome"""
    rng = random.Random(seed * 7919 + k)
    base = genome_with_repeats(rng, n, n_rep=8, rep_len=(k // 2 + 1, 4 * k), copies=(2, 3))
    if k % 2 == 0:
        half = rand_seq(rng, k // 2)
        base = base[:200] + half + orc.revcomp(half) + base[200:]
    kid = mutate(rng, base, snv=0.01, indel=0.003)
    dad = mutate(rng, base, snv=0.02, indel=0.003)
    haps = [("kid", [kid]), ("mom", [base]), ("dad", [dad])]
    reads = None
    if with_links:
        rl = max(3 * k, 60)
        reads = {"kid": [kid[i:i + rl] for i in range(0, max(1, len(kid) - rl + 1), max(1, rl // 4))] + [kid[-rl:]]}
    cs = Case(orc, tmp, lib, haps, k, link_samples=(["kid"] if with_links else []), reads=reads, name=name or "c%d_%d_%d" % (k, seed, int(with_links)))
    return cs, rng


def pick_seeds(cs, rng, n, extras=True):
    kmers = cs.all_kmers()
    seeds = [rng.choice(kmers) for _ in range(n)] if n > len(kmers) else rng.sample(kmers, n)
    seeds = [s if rng.random() < 0.5 else cs.orc.revcomp(s) for s in seeds]
    if extras:
        k = cs.k
        seeds += [rand_seq(rng, k) for _ in range(4)] + ["N" * k, seeds[0].lower(), seeds[1], seeds[1], seeds[1]]
    return seeds


# ---------------------------------------------------------------- cases
def case_reference_vectors(orc, lib, tmp):
    """V9-V11 (TraversalEngineTest.java:253-386) and V7 (:210-250) as batches: every k-mer of the haplotype a seed, all three directions"""
    for name, haps, k, links in (("v9", [("mom", ["AGTTCGAATCTGGGCTATATGCT"])], 7, False),
                                 ("v10", [("kid", ["AGTTCGAATCTGGGCTATATGCT", "AGTTCGAATCTGAGCTATATGCT"])], 7, False),
                                 ("v11", [("kid", ["AGTTCGAATCTGAGCTATATGCT"])], 7, False),
                                 ("v7", [("test", [FIG1])], 5, False), ("v7l", [("test", [FIG1])], 5, True)):
        cs = Case(orc, tmp, lib, haps, k, link_samples=(["test"] if links else []), reads=({"test": [FIG1_READ]} if links else None), name=name)
        oe, e = cs.engines([0], links=(["test"] if links else []), max_len=200)
        hap = haps[0][1][0]
        seeds = [hap[i:i + k] for i in range(len(hap) - k + 1)]
        seeds += [orc.revcomp(s) for s in seeds]
        for d in (BOTH, FORWARD, REVERSE):
            check(cs, oe, e, seeds, d, 200, tag=name)
        if name == "v9":       # the contigs the reference spells from its cursor loops
            fw = e.assemble_batch(["AGTTCGA"], FORWARD)[0]
            assert "AGTTCGA" + "".join(v.getKmerAsString()[-1] for v in fw) == hap
            rv = e.assemble_batch(["ATATGCT"], REVERSE)[0]
            assert "".join(v.getKmerAsString()[0] for v in rv) + "ATATGCT" == hap
        if name == "v10":
            fw = e.assemble_batch(["AGTTCGA"], FORWARD)[0]
            assert "AGTTCGA" + "".join(v.getKmerAsString()[-1] for v in fw) == "AGTTCGAATCTG"
            rv = e.assemble_batch(["ATATGCT"], REVERSE)[0]
            assert "".join(v.getKmerAsString()[0] for v in rv) + "ATATGCT" == "GCTATATGCT"
        oe.close(); e.close()


WIDTH_K = [21, 31, 32, 33, 47, 63, 65, 97]


def case_widths(orc, lib, tmp, k, with_links):
    """W = 1..4, even k with a palindrome; 250 seeds in both orientations, absent k-mers, N x k, a lower-case seed, one seed three times"""
    cs, rng = family(orc, lib, tmp, k, 1, with_links)
    ml = 400 if with_links else 75000          # with links a cursor circles a tandem repeat until the limit (the reference does too)
    oe, e = cs.engines([0], links=(["kid"] if with_links else []), max_len=ml)
    seeds = pick_seeds(cs, rng, 250)
    _, st = check(cs, oe, e, seeds, BOTH, ml, tag="both")
    assert st[("fwd", END)] > 100 and st[("status", OK)] == len(seeds)
    check(cs, oe, e, seeds, FORWARD, ml, tag="fwd")
    check(cs, oe, e, seeds, REVERSE, ml, tag="rev", device=True)
    # the vertex objects: the same type and values assemble returns, the seed's vertex with the string it was given
    vs = e.assemble_batch(seeds[-6:])
    for s, v in zip(seeds[-6:], vs):
        exp = oe.assemble(s, ml)
        assert [(x.getKmerAsString(), x.getCortexRecord().index if x.getCortexRecord() is not None else -1) for x in v] == exp, s
        assert all(isinstance(x, ca.CortexVertex) for x in v)
    oe.close(); e.close()


BATCH_SIZES = [0, 1, 63, 64, 65, 1000]


def case_batch_size(orc, lib, tmp, n):
    cs, rng = family(orc, lib, tmp, 31, 2, False)
    oe, e = cs.engines([0], max_len=75000)
    seeds = pick_seeds(cs, rng, n, extras=False) if n else []
    for d in (BOTH, FORWARD):
        check(cs, oe, e, seeds, d, 75000, tag="n%d" % n)
    if n:
        check(cs, oe, e, seeds, REVERSE, 75000, tag="n%d dev" % n, device=True)
    oe.close(); e.close()


def case_limits(orc, lib, tmp):
    """max_steps 1, 7, <= 0 (the engine's) and one at which some cursors end with LIMIT and others with END; a stop on exactly the
    max_steps-th vertex is a STOP"""
    cs, rng = family(orc, lib, tmp, 31, 3, False)
    oe, e = cs.engines([0], max_len=40)
    seeds = pick_seeds(cs, rng, 120)
    for ms in (1, 7, 0, -5, None):
        for d in (BOTH, FORWARD, REVERSE):
            _, st = check(cs, oe, e, seeds, d, 40, max_steps=ms, tag="ms%s" % ms)
    assert st[("rev", LIMIT)] > 0 and st[("rev", END)] > 0
    _, st = check(cs, oe, e, seeds, BOTH, 40, max_steps=25, tag="ms25")
    assert st[("fwd", LIMIT)] > 0 and st[("fwd", END)] > 0
    # the target is the 5th vertex forward and max_steps is 5
    parts, _ = check(cs, oe, e, seeds, FORWARD, 40, max_steps=5)
    pick = [(s, p[1][4][0]) for s, p in zip(seeds, parts) if len(p[1]) == 5 and p[3] == LIMIT]
    assert len(pick) > 10
    parts, st = check(cs, oe, e, [s for s, _ in pick], FORWARD, 40, max_steps=5, targets=[t for _, t in pick], tag="stop at limit")
    assert st[("fwd", STOP)] == len(pick)
    oe.close(); e.close()


def case_slot_reuse(orc, lib, tmp, monkeypatch, slots, with_links, epoch0=None):
    """the pool capped at `slots` slots: 300 seeds over a graph with cycles; an item on a reused slot must see neither its predecessor's
    `seen` set nor its link store.  epoch0: the slots' epochs start there (the 14-bit epochs wrap around after three items)"""
    monkeypatch.setenv("LDBG_CURSOR_SLOTS", str(slots))
    if epoch0 is not None:
        monkeypatch.setenv("LDBG_CURSOR_EPOCH0", str(epoch0))
    cs, rng = family(orc, lib, tmp, 21, 4, with_links, n=900)
    ml = 300 if with_links else 75000
    oe, e = cs.engines([0], links=(["kid"] if with_links else []), max_len=ml)
    seeds = pick_seeds(cs, rng, 300)
    check(cs, oe, e, seeds, BOTH, ml, tag="reuse")
    check(cs, oe, e, seeds, BOTH, ml, max_steps=7, tag="reuse, small tables")       # (tables of 64 entries: swept by load again and again)
    check(cs, oe, e, seeds[:80], FORWARD, ml, tag="reuse, second batch on the pool")
    oe.close(); e.close()


def case_stop_rules(orc, lib, tmp):
    """kid-colour cursors until mom-covered / dad-covered, with and without arrival_degree_one; targets in the right and the wrong
    orientation and the "none" entry; the three batches of callVariant"""
    cs, rng = family(orc, lib, tmp, 31, 5, False)
    k = cs.k
    oe, e = cs.engines([0], max_len=75000)
    seeds = pick_seeds(cs, rng, 200)
    seen = collections.Counter()
    for colour in (1, 2):
        for deg1 in (False, True):
            for d in (FORWARD, REVERSE):
                check(cs, oe, e, seeds, d, 75000, colour=colour, deg1=deg1, tag="rule")
            parts, st = check(cs, oe, e, seeds, BOTH, 75000, colour=colour, deg1=deg1, tag="rule")
            for rv, fw, rr, fr in parts:
                seen["first step"] += (rr == STOP and len(rv) == 1) + (fr == STOP and len(fw) == 1)
                seen["never"] += rr != STOP and fr != STOP
                seen["one direction"] += (rr == STOP) != (fr == STOP)
    assert seen["first step"] > 0 and seen["never"] > 0 and seen["one direction"] > 0, seen
    # targets: the vertex d steps ahead, as stepped onto (stops there), its reverse complement (does not), "none"
    parts, _ = check(cs, oe, e, seeds, FORWARD, 75000)
    tg, kinds = [], []
    for i, (s, p) in enumerate(zip(seeds, parts)):
        fw = p[1]
        if len(fw) >= 3 and i % 3 == 0:
            tg.append(fw[len(fw) // 2][0]); kinds.append("right")
        elif len(fw) >= 3 and i % 3 == 1:
            tg.append(orc.revcomp(fw[len(fw) // 2][0])); kinds.append("wrong")
        else:
            tg.append("N" * k); kinds.append("none")
    parts, st = check(cs, oe, e, seeds, FORWARD, 75000, targets=tg, tag="targets")
    for kd, p, t in zip(kinds, parts, tg):
        if kd == "right":
            assert p[3] == STOP and p[1][-1][0] == t
        elif kd == "wrong" and t != orc.revcomp(t):
            assert p[3] != STOP or p[1][-1][0] == t
    assert st[("fwd", STOP)] >= kinds.count("right") > 10 and kinds.count("wrong") > 10
    check(cs, oe, e, seeds, BOTH, 75000, targets=tg, colour=1, tag="targets and rule", device=True)
    # callVariant: backwards to a source, forwards to a destination, then the other colour from source to destination
    for colour, deg1 in ((1, False), (2, True)):
        back, _ = check(cs, oe, e, seeds, REVERSE, 75000, colour=colour, deg1=deg1)
        fwd, _ = check(cs, oe, e, seeds, FORWARD, 75000, colour=colour, deg1=deg1)
        pairs = [(b[0][-1][0], f[1][-1][0]) for b, f in zip(back, fwd) if b[2] == STOP and f[3] == STOP]
        assert len(pairs) > 10
        oc, ec = cs.engines([colour], max_len=75000)
        _, st = check(cs, oc, ec, [a for a, _ in pairs], FORWARD, 75000, targets=[b for _, b in pairs], tag="callVariant")
        assert st[("fwd", STOP)] > 0
        oc.close(); ec.close()
    oe.close(); e.close()


class _PathCase:
    """what `check` needs of a Case, over a .ctx written by the test"""

    def __init__(self, orc, lib, path, k):
        self.orc, self.lib, self.k, self.path = orc, lib, k, path
        self.og = orc.Graph(path, tuned=True)
        self.g = CortexGraph(path, lib=lib)

    def engines(self, trav, recruit=(), max_len=75000):
        oe = self.orc.Engine(self.og, trav, recruitment_colors=recruit, max_length=max_len, stopper="ContigStopper")
        f = TraversalEngineFactory(lib=self.lib).traversalColors(*trav).graph(self.g).maxBranchLength(max_len).stoppingRule(ContigStopper)
        if recruit:
            f.recruitmentColors(*recruit)
        return oe, f.make()


def case_null_records(orc, lib, tmp):
    """a graph from which records were taken, so that edges dangle: NULLPOINTER under a colour rule, a plain vertex with rec == -1
    without one; recruitment colours with an absent seed (Q14)"""
    cs, rng = family(orc, lib, tmp, 31, 6, False, n=900)
    d = rc.read_ctx(cs.path)
    keep = np.ones(d["N"], dtype=bool)
    keep[rng.sample(range(d["N"]), d["N"] // 12)] = False
    path = rc.write_ctx(tmp / "dangling.ctx", d["k"], d["names"], d["words"][keep], d["cov"][keep], d["edges"][keep], header=d["header"])
    pc = _PathCase(orc, lib, path, 31)
    oe, e = pc.engines([0])
    kmers = [pc.og.record_string(i).split()[0] for i in range(pc.og.N)]
    seeds = rng.sample(kmers, 250) + [rand_seq(rng, 31), "N" * 31]
    seeds = [s if rng.random() < 0.5 else orc.revcomp(s) for s in seeds]
    parts, st = check(pc, oe, e, seeds, BOTH, 75000, tag="dangling")
    assert sum(1 for rv, fw, _, _ in parts if (rv and rv[-1][1] == -1) or (fw and fw[-1][1] == -1)) > 5
    for colour in (1, 2):
        _, st = check(pc, oe, e, seeds, BOTH, 75000, colour=colour, tag="dangling under a rule")
        assert st[("status", NULLPOINTER)] > 0 and st[("status", OK)] > 0
    oe.close(); e.close()
    oe, e = pc.engines([0], recruit=[1, 2])
    _, st = check(pc, oe, e, seeds, BOTH, 75000, tag="recruitment")
    assert st[("status", NULLPOINTER)] >= 2                  # the absent seeds at the least (Q14)
    check(pc, oe, e, seeds, FORWARD, 75000, colour=1, tag="recruitment under a rule")
    oe.close(); e.close()
    pc.g.close(); pc.og.close()


def _refused(fn, status, *needles):
    with pytest.raises(ca.LdbgError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    for nd in needles:
        assert nd in str(ei.value), ei.value


def case_refused(orc, lib, tmp):
    cs, rng = family(orc, lib, tmp, 31, 7, False, n=400)
    oe, e = cs.engines([0])
    seeds = pick_seeds(cs, rng, 5, extras=False)
    import ctypes as C
    from corticall_amd import _native
    res = C.c_void_p()
    a = np.frombuffer("".join(seeds).encode(), dtype=np.uint8)
    st = lib.dll.ldbg_engine_cursor_batch(e._h, a.ctypes.data_as(C.c_void_p), C.c_int64(-1), C.c_int(BOTH), C.c_int64(0), None, C.byref(res))
    assert st == 6 and b"n < 0" in lib.dll.ldbg_last_error() and not res.value
    _refused(lambda: e.assemble_batch_arrays(seeds, until_colour=3), 6, "colour 3")
    _refused(lambda: e.assemble_batch_arrays(seeds, max_steps=(1 << 20) + 1), 6, "2^20")
    _refused(lambda: e.assemble_batch_arrays(seeds, direction=3), 6, "direction")
    r = e.assemble_batch_arrays(seeds, max_steps=1 << 20)          # the bound itself is served
    assert r["status"].tolist() == [OK] * 5
    # a NULL stop is no stop
    st = lib.dll.ldbg_engine_cursor_batch(e._h, a.ctypes.data_as(C.c_void_p), C.c_int64(5), C.c_int(BOTH), C.c_int64(0), None, C.byref(res))
    assert st == 0
    nv = C.c_int64()
    assert lib.dll.ldbg_cursor_result_sizes(res, None, C.byref(nv), None) == 0 and nv.value == int(r["offsets"][5])
    assert lib.dll.ldbg_cursor_result_free(res) == 0
    # one rank's part of a hash-sharded table
    lib.check(lib.dll.ldbg_graph_set_shard(cs.g._h, 1))
    try:
        _refused(lambda: e.assemble_batch_arrays(seeds), 4, "hash-sharded")
    finally:
        lib.check(lib.dll.ldbg_graph_set_shard(cs.g._h, 0))
    check(cs, oe, e, seeds, BOTH, 75000)
    oe.close(); e.close()


def case_agrees_with_assemble(orc, lib, tmp):
    """an addition to the oracle, not a substitute: assemble_batch(seeds) == [assemble(s) for s in seeds]"""
    for with_links in (False, True):
        cs, rng = family(orc, lib, tmp, 33, 8, with_links, n=900)
        oe, e = cs.engines([0], links=(["kid"] if with_links else []), max_len=300)
        seeds = pick_seeds(cs, rng, 58, extras=False) + [rand_seq(rng, 33), "N" * 33, cs.all_kmers()[0].lower()] + [cs.all_kmers()[3]] * 3
        assert len(seeds) == 64
        flat = lambda vs: [(v.getKmerAsString(), v.getCortexRecord().index if v.getCortexRecord() is not None else -1) for v in vs]
        assert [flat(v) for v in e.assemble_batch(seeds)] == [flat(e.assemble(s)) for s in seeds]
        oe.close(); e.close()
