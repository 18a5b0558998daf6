"""Cases for callVariant in batches on the device (ldbg_engine_variant_batch) and ComputeInheritance.call_variants, shared
by the host-simulation run (tests/test_variants_hostsim.py) and the GPU run (tests/test_gpu_variants.py).

Nothing expected here comes from the package.  The yardstick writes out the three loops of ComputeInheritance.callVariant (:119-165) over
the CPU oracle's cursor (Engine.seek / has_next / has_previous / next / previous, a fresh engine per colour, through
cursor_cases.Yardstick), and trimToAlleles (:406-433), toContig (TraversalUtils.java:367-381), the float32 means (:170-174, :202-206,
numpy.float32, added in order), TableWriter's text (TableWriter.java:37-52) and the occurrence count on plain strings.  Every seed of every
batch is compared in every field; the command's table is compared as text."""
import collections
import random

import numpy as np
import pytest

import corticall_amd as ca
from corticall_amd import ContigStopper, CortexGraph, TraversalEngineFactory
from tests import cursor_cases as cc
from tests import roi_cases as rc
from tests.parity_cases import device_seeds, rand_seq

CALLED, NO_SOURCE, NO_DESTINATION, NOT_REACHED, NULLPOINTER, CAPACITY, LIMIT = range(7)
TYPES = ("SNP", "MNP", "DEL", "INS")


# ---------------------------------------------------------------- the yardstick, on strings
def to_contig(kmers):
    """TraversalUtils.toContig: the first k-mer, then the last base of each later one"""
    return kmers[0] + "".join(s[-1] for s in kmers[1:]) if kmers else ""


def trim_to_alleles(s0, s1):
    """trimToAlleles, statement by statement -> (st, s0end, s1end, why the right-hand scan stopped: 'mismatch', 'guard' or None)"""
    st, e0, e1, why = 0, len(s0), len(s1), None
    i = j = 0
    while i < len(s0) and j < len(s1):
        if s0[i] != s1[j]:
            st = i
            break
        i += 1; j += 1
    i, j = len(s0) - 1, len(s1) - 1
    while i >= 0 and j >= 0:
        if s0[i] != s1[j] or i == st - 1 or j == st - 1:
            e0, e1 = i + 1, j + 1
            why = "mismatch" if s0[i] != s1[j] else "guard"
            break
        i -= 1; j -= 1
    return st, e0, e1, why


def variant_type(a0, a1):
    return 0 if len(a0) == 1 and len(a1) == 1 else 1 if len(a0) == len(a1) else 2 if len(a0) < len(a1) else 3


def float_mean(covs):
    """float acc = 0; acc += cov ...; acc /= (float) n; (int) acc"""
    acc = np.float32(0.0)
    for v in covs:
        acc = np.float32(acc + np.float32(int(v)))
    return int(np.float32(acc / np.float32(len(covs))))


def occurrences(kmer, sequences, revcomp):
    """windows of the sequences that spell the k-mer on either strand -> list of (sequence index, 0-based offset)"""
    k, rcm, out = len(kmer), revcomp(kmer), []
    for si, s in enumerate(sequences):
        for o in range(len(s) - k + 1):
            w = s[o:o + k]
            if w == kmer or w == rcm:
                out.append((si, o))
    return out


def table_text(entries):
    """TableWriter: the header from the first entry's keys, tab-separated, NA for an absent field, a key the header lacks is dropped"""
    if not entries:
        return ""
    hdr = list(entries[0].keys())
    return "".join("\t".join(r) + "\n" for r in [hdr] + [[e.get(h, "NA") for h in hdr] for e in entries])


Want = collections.namedtuple("Want", "status source_rec dest_rec n_child n_parent st s0end s1end a0 a1 why child parent")


class Yard:
    """callVariant's loops for child colour c and other-parent colour p over the oracle's cursors"""

    def __init__(self, orc, og, k, c, p, max_len=75000):
        self.orc, self.og, self.k = orc, og, k
        self.oc = orc.Engine(og, [c], max_length=max_len, stopper="ContigStopper")
        self.op = orc.Engine(og, [p], max_length=max_len, stopper="ContigStopper")
        self.yc, self.yp, self.p, self.max_len = cc.Yardstick(orc, self.oc, og, k), cc.Yardstick(orc, self.op, og, k), p, max_len

    def close(self):
        self.oc.close(); self.op.close()

    def cov(self, rec, colour):
        return self.yc.record(rec)[1][colour]

    def call(self, seed, max_steps=None):
        ms = max_steps if max_steps and max_steps > 0 else self.max_len
        rv, rr, rs = self.yc.direction(seed, False, ms, colour=self.p)
        fw, fr, fs = self.yc.direction(seed, True, ms, colour=self.p)
        srec = self.og.find(seed)[0] if cc.is_bases(seed) else -1
        child = rv[::-1] + [(seed, srec)] + fw
        src = rv[-1][1] if rr == cc.STOP else -1
        dst = fw[-1][1] if fr == cc.STOP else -1
        cs = rs if rs != cc.OK else fs
        none = lambda status, n_parent=0, parent=(): Want(status, src, dst, len(child), n_parent, 0, 0, 0, "", "", None, child, list(parent))
        if cs != cc.OK:
            return none(NULLPOINTER if cs == cc.NULLPOINTER else CAPACITY)
        if cc.LIMIT in (rr, fr):
            return none(LIMIT)
        if rr != cc.STOP:
            return none(NO_SOURCE)
        if fr != cc.STOP:
            return none(NO_DESTINATION)
        pv, pr, ps = self.yp.direction(rv[-1][0], True, ms, target=fw[-1][0])
        parent = [rv[-1]] + pv
        if ps != cc.OK:
            return none(NULLPOINTER if ps == cc.NULLPOINTER else CAPACITY, len(parent), parent)
        if pr == cc.STOP and any(r < 0 for _, r in parent):
            return none(NULLPOINTER, len(parent), parent)
        if pr == cc.LIMIT:
            return none(LIMIT, len(parent), parent)
        if pr != cc.STOP:
            return none(NOT_REACHED, len(parent), parent)
        s0, s1 = to_contig([v for v, _ in child]), to_contig([v for v, _ in parent])
        st, e0, e1, why = trim_to_alleles(s0, s1)
        return Want(CALLED, src, dst, len(child), len(parent), st, e0, e1, s0[st:e0], s1[st:e1], why, child, parent)


def engine(lib, g, colour, max_len=75000):
    return TraversalEngineFactory(lib=lib).traversalColors(colour).graph(g).maxBranchLength(max_len).stoppingRule(ContigStopper).make()


def check(lib, orc, og, g, k, c, p, seeds, sum_colours, max_steps=None, how="strings", tag="", max_len=75000):
    """one batch against the yardstick, every seed in every field -> (list of Want, Counter of statuses and types)"""
    y = Yard(orc, og, k, c, p, max_len)
    ec, ep = engine(lib, g, c, max_len), engine(lib, g, p, max_len)
    try:
        given = seeds
        if how == "array":
            given = np.frombuffer("".join(seeds).encode(), dtype=np.uint8).reshape(len(seeds), k)
        elif how == "device" and len(seeds):
            given = device_seeds(lib, seeds, k)
        r = ec.variant_batch(ep, given, p, sum_colours, max_steps, contigs=True)
        n, cols = len(seeds), sorted(set(sum_colours))
        assert r["colours"] == cols and r["status"].shape == (n,) and r["child_sum"].shape == (n, len(cols)) and r["allele_offsets"].shape == (2 * n + 1,), tag
        assert r["allele_offsets"][0] == 0 and r["allele_offsets"][2 * n] == r["alleles"].shape[0], tag
        text = r["alleles"].tobytes().decode()
        cw = cc.decode(r["child_words"], k) if r["child_words"].shape[0] else []
        pw = cc.decode(r["parent_words"], k) if r["parent_words"].shape[0] else []
        wants, stats = [], collections.Counter()
        for i, s in enumerate(seeds):
            w = y.call(s, max_steps)
            where = (tag, i, s, w.status)
            got = tuple(int(r[f][i]) for f in ("status", "source_rec", "dest_rec", "n_child", "n_parent", "st", "s0end", "s1end"))
            assert got == (w.status, w.source_rec, w.dest_rec, w.n_child, w.n_parent, w.st, w.s0end, w.s1end), (where, got, w[:8])
            ao = r["allele_offsets"]
            assert (text[ao[2 * i]:ao[2 * i + 1]], text[ao[2 * i + 1]:ao[2 * i + 2]]) == (w.a0, w.a1), where
            assert int(r["type"][i]) == (variant_type(w.a0, w.a1) if w.status == CALLED else -1), where
            co = r["child_offsets"]
            mine = list(zip(cw[co[i]:co[i + 1]], r["child_rec"][co[i]:co[i + 1]].tolist()))
            if cc.is_bases(s):
                assert mine == w.child, where
            po = r["parent_offsets"]
            mine = list(zip(pw[po[i]:po[i + 1]], r["parent_rec"][po[i]:po[i + 1]].tolist()))
            assert mine == list(w.parent[1:]), where
            for j, col in enumerate(cols):
                covs = [y.cov(rec, col) for _, rec in w.child] if w.status == CALLED else []
                assert int(r["child_sum"][i, j]) == sum(covs), (where, col)
                assert int(r["child_flag"][i, j]) == (1 if sum(abs(v) for v in covs) >= 1 << 24 else 0), (where, col)
            covs = [y.cov(rec, p) for _, rec in w.parent] if w.status == CALLED else []
            assert int(r["parent_sum"][i]) == sum(covs) and int(r["parent_flag"][i]) == (1 if sum(abs(v) for v in covs) >= 1 << 24 else 0), where
            stats[("status", w.status)] += 1
            if w.status == CALLED:
                stats[("type", TYPES[variant_type(w.a0, w.a1)])] += 1
                stats[("why", w.why)] += 1
            wants.append(w)
        return wants, stats
    finally:
        ec.close(); ep.close(); y.close()


# ---------------------------------------------------------------- graphs
class Fam:
    """kid / mom / dad over one genome: the kid carries dad's alleles, mom the other ones; colours 0, 1, 2 (and copies of the kid beyond)"""

    def __init__(self, orc, lib, tmp, k, mom, kid, name, extra=0, mom_haps=None):
        self.orc, self.lib, self.k, self.mom, self.kid = orc, lib, k, mom, kid
        self.path = str(tmp / (name + ".ctx"))
        orc.build_graph(self.path, [("kid", [kid]), ("mom", mom_haps or [mom]), ("dad", [kid])] + [("x%d" % i, [kid]) for i in range(extra)], k)
        self.open(self.path)

    def open(self, path):
        self.og = self.orc.Graph(path, tuned=True)
        self.g = CortexGraph(path, lib=self.lib)

    def reopen(self, path):
        self.close()
        self.open(path)

    def close(self):
        self.g.close(); self.og.close()

    def kid_only(self, both=True):
        """the kid's k-mers mom does not have, in genome order, in both orientations"""
        k, mom = self.k, set()
        for i in range(len(self.mom) - k + 1):
            mom.add(self.mom[i:i + k]); mom.add(self.orc.revcomp(self.mom[i:i + k]))
        out = [self.kid[i:i + k] for i in range(len(self.kid) - k + 1) if self.kid[i:i + k] not in mom]
        return [s if (j % 2 == 0 or not both) else self.orc.revcomp(s) for j, s in enumerate(out)]

    def check(self, seeds, sum_colours=(0,), **kw):
        return check(self.lib, self.orc, self.og, self.g, self.k, 0, 1, seeds, sum_colours, **kw)


def other(rng, b):
    return rng.choice([x for x in "ACGT" if x != b])


def with_sites(rng, k, sites, flank=None):
    """mom and kid genomes: stretches of random sequence between the sites; a site is (mom allele, kid allele) or a callable of rng"""
    flank = flank or 3 * k
    mom, kid = [rand_seq(rng, flank)], []
    kid.append(mom[0])
    for site in sites:
        a, b = site(rng) if callable(site) else site
        f = rand_seq(rng, flank)
        mom += [a, f]; kid += [b, f]
    return "".join(mom), "".join(kid)


def snv(rng):
    a = rng.choice("ACGT")
    return a, other(rng, a)


# ---------------------------------------------------------------- cases
def case_family(orc, lib, tmp):
    """k = 21: SNV, 2-base MNP, 1- and 7-base insertion, 1- and 7-base deletion, a deleted copy of a 3 x 5-base tandem repeat"""
    k, rng = 21, random.Random(11)
    unit = "ACGTC"
    mnp = lambda r: ("AC", "GT")
    sites = [snv, mnp, lambda r: ("", "G"), lambda r: ("", rand_seq(r, 7)), lambda r: ("T", ""), lambda r: (rand_seq(r, 7), ""), lambda r: (unit * 3, unit * 2)]
    mom, kid = with_sites(rng, k, sites)
    f = Fam(orc, lib, tmp, k, mom, kid, "family")
    seeds = f.kid_only()
    wants, st = f.check(seeds, (0, 1, 2), tag="family")
    assert st[("status", CALLED)] >= 7 and all(st[("type", t)] >= 1 for t in TYPES), st
    assert st[("why", "guard")] >= 1 and st[("why", "mismatch")] >= 1, st       # (the repeat: the right-hand scan stops on i == st - 1 / j == st - 1)
    assert len({(w.a0, w.a1) for w in wants if w.status == CALLED}) >= 7
    f.check(seeds, (1,), how="device", tag="family, device seeds")
    f.close()


WIDTH_K = [31, 32, 33, 47, 63, 65, 97]


def case_widths(orc, lib, tmp, k):
    rng = random.Random(100 + k)
    sites = [snv] * 4
    if k % 2 == 0:                  # an even-k palindrome on the path between two sites
        half = rand_seq(rng, k // 2)
        pal = half + orc.revcomp(half)
        sites = [snv, snv, lambda r: (pal, pal), snv, snv]
    mom, kid = with_sites(rng, k, sites, flank=2 * k + 3)
    if k % 2 == 0:
        assert pal in kid and orc.revcomp(pal) == pal
    f = Fam(orc, lib, tmp, k, mom, kid, "w%d" % k)
    seeds = f.kid_only()
    if k % 2 == 0:
        seeds.append(pal)
    _, st = f.check(seeds, (0, 2), tag="k%d" % k, how="array")
    assert st[("status", CALLED)] >= 4 * k and st[("type", "SNP")] >= 4 * k, st
    f.close()


BOUNDARY_K = [31, 32, 63, 64, 65]


def case_boundaries(orc, lib, tmp, k):
    """contigs of 2k + 1 bases (an SNV) and of 2k and 2k + 1 (a 1-base indel): 63, 64, 65, 127, 128, 129 bases over these k; the first
    difference at index k and the last k from the right: 63, 64, 65"""
    rng = random.Random(200 + k)
    mom, kid = with_sites(rng, k, [snv, lambda r: ("", other(r, "A")), lambda r: (other(r, "C"), "")], flank=2 * k + 5)
    f = Fam(orc, lib, tmp, k, mom, kid, "b%d" % k)
    wants, st = f.check(f.kid_only(), (0,), tag="boundary k%d" % k)
    called = [w for w in wants if w.status == CALLED]
    assert len(called) >= 3 * (k - 2), st          # (a base beside an equal one: an indel leaves a k-mer fewer)
    lengths = {w.n_child + k - 1 for w in called} | {w.n_parent + k - 1 for w in called}
    assert {2 * k, 2 * k + 1} <= lengths, lengths
    assert any(w.st == k and w.n_child + k - 1 - w.s0end == k for w in called)
    f.close()
    return lengths


def edited(f, tmp, name, edit):
    """the family's table with edit(d, index of a k-mer) applied, reopened"""
    d = rc.read_ctx(f.path)
    idx = lambda km: f.og.find(km)[0]
    keep = edit(d, idx)
    sl = slice(None) if keep is None else keep
    path = rc.write_ctx(tmp / (name + ".ctx"), d["k"], d["names"], d["words"][sl], d["cov"][sl], d["edges"][sl], header=d["header"])
    f.reopen(str(path))


def case_tables(orc, lib, tmp):
    """hand-edited tables: identical contigs, no source, no destination, a fork on the parent's path, a record taken away, max_steps"""
    k, rng = 21, random.Random(31)
    # identical child and parent contigs: mom's coverage taken off a stretch she shares with the kid, her edges left
    g0 = rand_seq(rng, 200)
    f = Fam(orc, lib, tmp, k, g0, g0, "same")
    inner = [g0[i:i + k] for i in range(80, 95)]

    def uncover(d, idx):
        for km in inner:
            d["cov"][idx(km), 1] = 0
    edited(f, tmp, "same_e", uncover)
    wants, st = f.check(inner[::2] + [orc.revcomp(s) for s in inner[1::2]], (0, 1), tag="identical")
    assert st[("status", CALLED)] == len(inner) and st[("type", "MNP")] == len(inner) and st[("why", None)] == len(inner), st
    assert all(w.a0 == w.a1 and len(w.a0) == w.n_child + k - 1 for w in wants)
    f.close()
    # a variant within the first k bases (no source), within the last k (no destination), and a second haplotype of mom's that
    # forks off her path inside the bubble (not reached)
    body = rand_seq(rng, 6 * k)
    mom = "A" + body + "C"
    kid = "G" + body[:3 * k] + other(rng, body[3 * k]) + body[3 * k + 1:] + "T"
    fork = body[:3 * k + 5] + other(rng, body[3 * k + 5]) + body[3 * k + 6:]
    f = Fam(orc, lib, tmp, k, mom, kid, "ends", mom_haps=[mom, fork])
    seeds = f.kid_only()
    wants, st = f.check(seeds, (0,), tag="ends")
    assert st[("status", NO_SOURCE)] >= 1 and st[("status", NO_DESTINATION)] >= 1 and st[("status", NOT_REACHED)] >= 1, st
    f.close()
    # a record of the bubble taken away: the kid's cursor steps onto a vertex without a record under the colour rule
    mom, kid = with_sites(rng, k, [snv, snv])
    f = Fam(orc, lib, tmp, k, mom, kid, "gone")
    seeds = f.kid_only()
    gone = seeds[5]

    def drop(d, idx):
        keep = np.ones(d["N"], dtype=bool)
        keep[idx(gone)] = False
        return keep
    edited(f, tmp, "gone_e", drop)
    wants, st = f.check([s for s in seeds if s != gone], (0,), tag="record taken away")
    assert st[("status", NULLPOINTER)] >= 1 and st[("status", CALLED)] >= k - 2, st
    f.close()
    # max_steps: the longest direction of any batch of these seeds, one less (LIMIT) and exactly that (none)
    mom, kid = with_sites(rng, k, [snv])
    f = Fam(orc, lib, tmp, k, mom, kid, "limit")
    seeds = f.kid_only()
    wants, st = f.check(seeds, (0,), tag="no limit")
    assert st[("status", CALLED)] == len(seeds)
    need = max(w.n_parent - 1 for w in wants)           # (the parent's steps from the source: the longest of the three loops)
    assert need >= max(w.n_child - 1 for w in wants) // 2
    _, st = f.check(seeds, (0,), max_steps=need, tag="limit met")
    assert st[("status", CALLED)] == len(seeds), st
    _, st = f.check(seeds, (0,), max_steps=need - 1, tag="limit")
    assert st[("status", LIMIT)] >= 1, st
    _, st = f.check(seeds, (0,), max_steps=1, tag="one step")
    assert st[("status", LIMIT)] == len(seeds), st
    f.close()


def case_sums(orc, lib, tmp, mean_fn):
    """coverage 2^23 on three vertices (flag), a stored 0x80000000 (a negative Java int; the flag counts |cov|), a sum of 2^24 - 1 (no
    flag); masks of 1, 3 and 9 colours.  mean_fn(sum, flag, n, coverages in order) is the package's host arithmetic."""
    k, rng = 21, random.Random(51)
    mom, kid = with_sites(rng, k, [snv, snv, snv])
    f = Fam(orc, lib, tmp, k, mom, kid, "sums", extra=6)
    seeds = f.kid_only(both=False)
    b = [seeds[0:k], seeds[k:2 * k], seeds[2 * k:3 * k]]
    assert len(seeds) == 3 * k

    def edit(d, idx):
        for km in b[0][3:6]:
            d["cov"][idx(km), 0] = 1 << 23
        d["cov"][idx(b[1][4]), 3] = 0x80000000
        # the third bubble's child contig: k + 2 vertices of coverage 1 in colour 4 but one, so that they add up to 2^24 - 1
        d["cov"][idx(b[2][7]), 4] = (1 << 24) - 1 - (k + 1)
    edited(f, tmp, "sums_e", edit)
    for cols in ((0,), (0, 3, 4), tuple(range(9))):
        wants, st = f.check(seeds, cols, tag="mask of %d" % len(cols))
        assert st[("status", CALLED)] == 3 * k
    y = Yard(orc, f.og, k, 0, 1)
    seen = collections.Counter()
    for s in (b[0][0], b[1][0], b[2][0]):
        w = y.call(s)
        for col in (0, 3, 4):
            covs = [y.cov(r, col) for _, r in w.child]
            flag = sum(abs(v) for v in covs) >= 1 << 24
            naive = int(np.float32(np.float32(sum(covs)) / np.float32(len(covs))))
            seen[(col, flag, naive == float_mean(covs))] += 1
            assert mean_fn(sum(covs), flag, len(covs), covs) == float_mean(covs), (s, col)
            if not flag:
                assert naive == float_mean(covs)
    assert seen[(0, True, True)] + seen[(0, True, False)] >= 1 and seen[(3, True, True)] + seen[(3, True, False)] >= 1, seen
    w = y.call(b[2][0])
    assert sum(y.cov(r, 4) for _, r in w.child) == (1 << 24) - 1
    y.close()
    f.close()


SEED_COUNTS = [0, 1, 63, 64, 65, 1000]


def case_counts(orc, lib, tmp, n, monkeypatch=None, slots=None):
    if slots is not None:
        monkeypatch.setenv("LDBG_CURSOR_SLOTS", str(slots))
    k, rng = 21, random.Random(61)
    mom, kid = with_sites(rng, k, [snv] * 6)
    f = Fam(orc, lib, tmp, k, mom, kid, "counts")
    called_seeds = set(f.kid_only())
    pool = f.kid_only() + [mom[i:i + k] for i in range(0, 40)] + ["N" * k, rand_seq(rng, k)]
    seeds = [pool[i % len(pool)] for i in range(n)]
    if n >= 3:
        seeds[1] = seeds[2] = seeds[0]                  # one seed three times
    for how in ("strings", "array", "device"):
        _, st = f.check(seeds, (0, 1), how=how, tag="n%d %s" % (n, how))
        assert st[("status", CALLED)] >= sum(1 for s in seeds if s in called_seeds), st       # (every k-mer only the kid has lies in an SNV's bubble)
    f.close()


def _refused(fn, status, *needles):
    with pytest.raises(ca.LdbgError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    for nd in needles:
        assert nd in str(ei.value), ei.value


def case_refused(orc, lib, tmp):
    import ctypes as C
    k, rng = 21, random.Random(71)
    mom, kid = with_sites(rng, k, [snv])
    f = Fam(orc, lib, tmp, k, mom, kid, "refused")
    other_f = Fam(orc, lib, tmp, k, mom, kid, "refused_other")
    seeds = f.kid_only()[:4]
    ec, ep, eo = engine(lib, f.g, 0), engine(lib, f.g, 1), engine(lib, other_f.g, 1)
    res = C.c_void_p()
    a = np.frombuffer("".join(seeds).encode(), dtype=np.uint8)
    st = lib.dll.ldbg_engine_variant_batch(ec._h, ep._h, a.ctypes.data_as(C.c_void_p), C.c_int64(-1), C.c_int(1), C.c_int64(0), C.c_uint64(1), C.byref(res))
    assert st == 6 and b"n < 0" in lib.dll.ldbg_last_error() and not res.value
    _refused(lambda: ec.variant_batch(ep, seeds, 3, (0,)), 6, "colour 3")
    _refused(lambda: ec.variant_batch(ep, seeds, -1, (0,)), 6, "colour -1")
    _refused(lambda: ec.variant_batch(ep, seeds, 1, (0, 3)), 6, "mask")
    _refused(lambda: ec.variant_batch(eo, seeds, 1, (0,)), 6, "different graphs")
    _refused(lambda: ec.variant_batch(ep, seeds, 1, (0,), max_steps=(1 << 20) + 1), 6, "2^20")
    er = TraversalEngineFactory(lib=lib).traversalColors(1).recruitmentColors(2).graph(f.g).stoppingRule(ContigStopper).make()
    _refused(lambda: ec.variant_batch(er, seeds, 1, (0,)), 6, "recruitment")
    lp = str(tmp / "kid.ctp.gz")
    orc.build_links(f.og, lp, "kid", [kid])
    links = ca.CortexLinks(lp, f.g)
    el = TraversalEngineFactory(lib=lib).traversalColors(0).links(links).graph(f.g).stoppingRule(ContigStopper).make()
    _refused(lambda: el.variant_batch(ep, seeds, 1, (0,)), 6, "links")
    lib.check(lib.dll.ldbg_graph_set_shard(f.g._h, 1))
    try:
        _refused(lambda: ec.variant_batch(ep, seeds, 1, (0,)), 4, "hash-sharded")
    finally:
        lib.check(lib.dll.ldbg_graph_set_shard(f.g._h, 0))
    r = ec.variant_batch(ep, seeds, 1, (0,))
    assert r["status"].tolist() == [CALLED] * 4
    for e in (ec, ep, eo, er, el):
        e.close()
    links.close()
    f.close(); other_f.close()


# ---------------------------------------------------------------- the command
def package_mean(total, flagged, n, covs):
    from corticall_amd.quality import variant_mean
    return variant_mean(total, flagged, n, lambda: covs)


def command_yardstick(orc, path, samples_of, parents_map, children, ref_name, drafts_names, coordinates):
    """callVariants in the per-seed reading, written out: -> (entries in (chrom, pos) order, entries made, seeds without another parent)"""
    from tests import seed_cases as sc
    t = sc.table(path)
    og = orc.Graph(path, tuned=True)
    colour = {og.sample_name(c): c for c in range(t["C"])}
    ref, parents, drafts = colour[ref_name], sorted({colour[n] for n in parents_map.values()}), sorted({colour[n] for n in drafts_names})
    child_cols = sorted({colour[n] for n in children})
    uniq = {c: sc.count_occurrences(t, samples_of[og.sample_name(c)])[0] == 1 for c in drafts}
    S = [r for r in range(t["N"]) if sc.java_inheritance_pass(t, r, ref, parents, drafts, uniq)]
    good = sc.variant_seeds(t, S)[0]
    names = orc.java_string_hashmap_order(list(parents_map))
    seqs = [s for _, s in coordinates]
    yards, entries, made, lonely = {}, {}, 0, 0
    for r in good:
        cr = t["cov"][r]
        share = other = -1
        for pc in parents:
            if cr[pc] > 0:
                share = pc
            elif cr[pc] == 0:
                other = pc
        if other < 0:
            lonely += 1
            continue
        for c in child_cols:
            if cr[c] <= 0:
                continue
            if (c, other) not in yards:
                yards[(c, other)] = Yard(orc, og, t["k"], c, other)
            y = yards[(c, other)]
            w = y.call(t["strs"][r])
            if w.status != CALLED:
                continue
            so, do = occurrences(w.parent[0][0], seqs, orc.revcomp), occurrences(w.child[-1][0], seqs, orc.revcomp)
            if len(so) == 1 and len(do) == 1 and so[0][0] == do[0][0]:
                te = collections.OrderedDict()
                te["chrom"] = coordinates[so[0][0]][0].split()[0]
                te["pos"] = str(so[0][1] + 1)
                te["type"] = TYPES[variant_type(w.a0, w.a1)]
                te["cov_parent"] = str(float_mean([y.cov(rec, other) for _, rec in w.parent]))
                for cc in child_cols:
                    sample = og.sample_name(other if cr[cc] == 0 else share)
                    for nm in names:
                        if parents_map[nm] == sample:
                            te[og.sample_name(cc)] = "%s:%d" % (nm, float_mean([y.cov(rec, cc) for _, rec in w.child]))
                            break
                te["alleles"] = "%s/%s" % (w.a0, w.a1)
                entries[(te["chrom"], so[0][1] + 1)] = te
                made += 1
            break                                    # the first child colour that calls
    for y in yards.values():
        y.close()
    og.close()
    return [entries[key] for key in sorted(entries)], made, lonely


def case_command(orc, lib, tmp):
    from corticall_amd import ComputeInheritance
    from tests import seed_cases as sc
    k, rng = 21, random.Random(41)
    p1 = rand_seq(rng, 1600)
    p2 = list(p1)
    for s in range(120, 1500, 110):
        p2[s] = rng.choice([b for b in "ACGT" if b != p1[s]])
    p2 = "".join(p2)
    h = 800
    seen_columns = set()
    for name, k3 in (("pedigree", p1), ("pedigree_dad", p2), ("pedigree_big", p1)):
        kids = [p1[:h] + p2[h:], p2[:h] + p1[h:], k3]
        samples = [("ref", [p1]), ("mom", [p1]), ("dad", [p2]), ("mom_asm", [p1]), ("dad_asm", [p2]), ("k1", [kids[0]]), ("k2", [kids[1]]), ("k3", [kids[2]])]
        samples_of = dict(samples)
        path = str(tmp / (name + ".ctx"))
        orc.build_graph(path, samples, k)
        if name == "pedigree_big":
            # coverage 2^23 on three vertices of the first site's child contig (k1) and of its parent contig (dad): flagged sums, which the
            # command redoes in float32, in order, over the downloaded contigs
            d, t = rc.read_ctx(path), sc.table(path)
            for j in (3, 4, 5):
                d["cov"][t["index"][sc.canonical(p1[120 - k + 1 + j:120 + 1 + j])], 5] = 1 << 23
                d["cov"][t["index"][sc.canonical(p2[120 - k + 1 + j:120 + 1 + j])], 2] = 1 << 23
            path = str(rc.write_ctx(tmp / "pedigree_big_e.ctx", d["k"], d["names"], d["words"], d["cov"], d["edges"], header=d["header"]))
        g = CortexGraph(path, lib=lib)
        drafts = {"mom_asm": [("m", p1)], "dad_asm": sc.write_fasta(tmp / (name + "_dad.fa"), [("d", p2)], width=70)}
        parents_map = {"mother": "mom", "father": "dad", "mama": "mom"}          # two keys for one sample: the first in HashMap order names it
        children = ["k1", "k2", "k3"]
        runs = [("given", [("chr1 the first parent", p1)]), ("twice", [("a", p1), ("b", p1[300:700])])]
        if k3 is p2:
            runs = [("default", None)]
        if name == "pedigree_big":
            runs = runs[:1]
        for what, coordinates in runs:
            refs = dict(drafts)
            if coordinates is None:
                # REFERENCES["ref"] (:167-168); its sample becomes a draft colour, as in the reference
                refs["ref"] = sc.write_fasta(tmp / (name + "_ref.fa"), [("chrR", p1)], width=60)
            cmd = ComputeInheritance(g, refs, parents_map, set(children), "ref")
            want, made, lonely = command_yardstick(orc, path, samples_of, parents_map, children, "ref", list(refs),
                                                   coordinates if coordinates is not None else [("chrR", p1)])
            assert len(want) >= 5 and made > len(want), (name, what, len(want), made)       # several seeds land on one (chrom, pos)
            out = tmp / (name + "_" + what + ".tsv")
            got = cmd.call_variants(coordinates, out=str(out))
            assert [list(e.items()) for e in got] == [list(e.items()) for e in want], (name, what)
            assert open(out, newline="").read() == table_text(want), (name, what)
            assert (cmd.n_variants, cmd.n_no_other_parent) == (made, lonely) and cmd.status_counts.get(CALLED, 0) >= made, (name, what)
            for e in want:
                seen_columns.add(tuple((c, e[c].split(":")[0]) for c in children if c in e))
            if what == "twice":
                assert len(want) < len(first_want)       # a source that occurs twice in the reference makes no entry
            first_want = want
            try:
                cmd.execute()
                raise AssertionError("execute() ran")
            except NotImplementedError as e:
                assert "callVariants" in str(e) and "call_variants()" in str(e)
        if name == "pedigree":
            # no coordinates and no "ref" entry
            with pytest.raises(KeyError):
                ComputeInheritance(g, drafts, parents_map, set(children), "ref").call_variants()
            # a single parent colour: no seed has another parent; nothing is called and the file is empty
            one = {"mother": "mom"}
            cmd = ComputeInheritance(g, drafts, one, set(children), "ref")
            want, made, lonely = command_yardstick(orc, path, samples_of, one, children, "ref", list(drafts), [("chr1", p1)])
            out = tmp / "single.tsv"
            assert cmd.call_variants([("chr1", p1)], out=str(out)) == [] == want and open(out).read() == ""
            assert (cmd.n_variants, cmd.n_no_other_parent) == (0, lonely) and lonely >= 10
        g.close()
    # the children inherit different halves: the parent named in a child's column differs between rows, and k2 / k1 lack coverage at
    # seeds of the first / second half (the cr.cov(cc) == 0 branch)
    assert len(seen_columns) >= 3, seen_columns
