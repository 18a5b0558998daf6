"""FindOrphans cases (corticall_amd.partition.FindOrphans) shared by the host-simulation run (tests/test_orphans_hostsim.py) and the GPU
run (tests/test_gpu_orphans.py).

The yardstick is J/commands/prefilter/FindOrphans.java:45-134 restated over the oracle engine, one seed at a time: child colour, BOTH,
AND, joining colours = parents, OrphanStopper, rois; getNextVertices / getPrevVertices of every ROI k-mer not yet an orphan, a dfs from
those that lack one of the two, the canonical k-mers of the vertices of every non-empty dfs into `orphans`.

What the reference's rule makes of it.  A seed is searched only when getNextVertices or getPrevVertices is empty, that is when its
record has out-degree or in-degree 0 in the child's colour — and that is OrphanStopper.hasTraversalSucceeded on the very first vertex,
in both directions.  Both half-searches therefore return their empty graph at once: every dfs is non-null and has no vertex, no chain
is counted, `orphans` stays empty and every ROI record is kept.  The yardstick says so for every graph here (facts: seeds == empty_dfs,
null_dfs == skipped_ends == 0), so three outcomes the cases were meant to show — a chain whose second endpoint is skipped, an
endpoint whose dfs is null, an excluded record — cannot occur under the reference's rule on any input; case_find_orphans asserts what
the yardstick does say.  The loop itself (skip, null, chain, the set that is larger than the ROI) is checked by case_orphan_loop: the
same class and the same yardstick under other stopping rules, on the same graphs, where all of it does occur."""
import random

import numpy as np

import corticall_amd as ca
from corticall_amd import CortexGraph, FindOrphans
from tests import roi_cases as rc
from tests.parity_cases import mutate, rand_seq

ORPHAN_K = [9, 21, 31, 47]
# haplotype seeds under which the conditions on the yardstick's own outcome hold (asserted in the case)
ORPHAN_SEEDS = {9: 0, 21: 0, 31: 0, 47: 0}


def findorphans_reference(orc, og, oroi, parents, stopper="OrphanStopper"):
    """-> (numOrphanChains, orphans: set of canonical k-mers, facts about the run)"""
    child = og.color_for_sample_name(oroi.sample_name(0))
    pcols = [og.color_for_sample_name(p) for p in parents]
    oe = orc.Engine(og, [child], rois=oroi, joining_colors=pcols, op_and=True, stopper=stopper)
    orphans, chains = set(), 0
    facts = dict(skipped_ends=0, null_dfs=0, empty_dfs=0, seeds=0)
    for i in range(oroi.N):                                                 # for (CortexRecord rr : ROI) :74
        rr = oroi.record_string(i).split()[0]
        if og.find(rr)[0] < 0:
            raise ca.JavaNullPointerException(rr)                           # cr.getKmerAsByteKmer() :89
        is_end = len(oe.next_vertices(rr)) == 0 or len(oe.prev_vertices(rr)) == 0
        if rr in orphans:
            facts["skipped_ends"] += int(is_end)
            continue
        if is_end:
            facts["seeds"] += 1
            r = oe.dfs(rr)
            if r.is_null:
                facts["null_dfs"] += 1
            elif r.nv == 0:
                facts["empty_dfs"] += 1
            else:
                chains += 1
                for kmer, rec, _, _ in r.vertices():
                    orphans.add(orc.canonical(kmer) if rec >= 0 else None)  # CortexVertex.getCanonicalKmer(): null without a record
            r.free()
    oe.close()
    return chains, orphans, facts


def family(orc, k, seed):
    """two parents and a child that is a mosaic of them, plus: child-only contigs unconnected to the parents (k + 5 .. k + 40 bases), one
    child-only sequence of exactly k bases, a novel bubble joined to parental sequence on both sides, a novel tip hanging off parental
    sequence, and two child-only haplotypes that share a prefix (the dfs forks)"""
    rng = random.Random(4200 + 101 * seed + k)
    mom = rand_seq(rng, 700)
    dad = mutate(rng, mom, snv=0.02, indel=0.0)
    kid = list(mom[:350] + dad[350:])
    p = 200
    kid[p] = next(b for b in "ACGT" if b not in (mom[p], dad[p]))           # the bubble: k child-only k-mers between parental ones
    kid = "".join(kid)
    extra = [rand_seq(rng, k + n) for n in (5, 17, 40)]                     # orphan contigs
    extra.append(rand_seq(rng, k))                                          # a lone k-mer
    extra.append(kid[450:450 + k + 6] + rand_seq(rng, k // 2 + 3))          # a tip
    prefix = rand_seq(rng, k + 10)
    extra += [prefix + rand_seq(rng, k + 4), prefix + rand_seq(rng, k + 9)]  # a fork
    return [("kid", [kid] + extra), ("mom", [mom]), ("dad", [dad])]


def novel_kmers(orc, haps, k):
    parents = set()
    for name, hs in haps[1:]:
        for h in hs:
            parents |= {orc.canonical(h[i:i + k]) for i in range(len(h) - k + 1)}
    return [h[i:i + k] for h in haps[0][1] for i in range(len(h) - k + 1) if orc.canonical(h[i:i + k]) not in parents]


def check_orphans(orc, lib, tmp, k, stopper):
    haps = family(orc, k, ORPHAN_SEEDS[k])
    gp, rp = str(tmp / "family.ctx"), str(tmp / "roi.ctx")
    orc.build_graph(gp, haps, k)
    orc.build_graph(rp, [("kid", novel_kmers(orc, haps, k))], k)
    og, oroi = orc.Graph(gp, tuned=True), orc.Graph(rp, tuned=True)
    chains, orphans, facts = findorphans_reference(orc, og, oroi, ["mom", "dad"], stopper)
    roi_kmers = [oroi.record_string(i).split()[0] for i in range(oroi.N)]
    exp_excluded = [i for i, km in enumerate(roi_kmers) if km in orphans]
    g, roi = CortexGraph(gp, lib=lib), CortexGraph(rp, lib=lib)
    fo = FindOrphans(g, roi, ["mom", "dad"])
    if stopper != "OrphanStopper":
        fo._stopping_rule = getattr(ca, stopper)                            # the class's test seam; the reference's rule is the default
    out = tmp / ("orphans_%s.ctx" % stopper)
    kept, excluded = fo.execute(out)
    assert fo.excluded == exp_excluded, (k, stopper, sorted(set(fo.excluded) ^ set(exp_excluded)))
    assert (kept, excluded) == (oroi.N - len(exp_excluded), len(exp_excluded))
    assert (fo.numOrphanChains, fo.numOrphanKmers) == (chains, len(orphans)), (fo.numOrphanChains, chains, fo.numOrphanKmers, len(orphans))
    assert out.read_bytes() == rc.expected_excluded(rp, exp_excluded, lib, tmp, "orphans_" + stopper)
    back, whole = rc.read_ctx(out), rc.read_ctx(rp)
    assert back["N"] == excluded and (back["words"] == whole["words"][exp_excluded]).all() and back["header"] == whole["header"]
    assert fo.execute() == (kept, excluded)                                 # without a file
    lone = orc.canonical(haps[0][1][4])                                     # the child-only sequence of exactly k bases
    assert lone in roi_kmers and (roi_kmers.index(lone) in fo.excluded) == (lone in orphans)
    roi.close(); g.close(); oroi.close(); og.close()
    return chains, orphans, facts, exp_excluded, oroi.N, lone


def case_find_orphans(orc, lib, tmp, k):
    """the reference's rule: see the module docstring for why nothing is found"""
    chains, orphans, facts, excluded, n, lone = check_orphans(orc, lib, tmp, k, "OrphanStopper")
    assert facts["seeds"] >= 8 and facts["empty_dfs"] == facts["seeds"] and facts["null_dfs"] == 0 and facts["skipped_ends"] == 0, facts
    assert (chains, len(orphans), excluded) == (0, 0, []) and lone not in orphans


# rule -> what the yardstick's own outcome must show under it
LOOP_RULES = ["ContigStopper", "ContaminantStopper", "DestinationStopper"]


def case_orphan_loop(orc, lib, tmp, k, stopper):
    """the loop where it has something to do: chains whose second endpoint is skipped because the first put it into `orphans`, more
    orphans than ROI records (ContigStopper walks on into parental sequence), kept and excluded records side by side
    (ContaminantStopper), every endpoint's dfs null (DestinationStopper without a sink)"""
    chains, orphans, facts, excluded, n, lone = check_orphans(orc, lib, tmp, k, stopper)
    if stopper == "ContigStopper":
        assert facts["skipped_ends"] >= 1 and chains >= 3 and len(orphans) > n and len(excluded) > 0, (facts, chains, len(orphans), n)
    elif stopper == "ContaminantStopper":
        assert facts["skipped_ends"] >= 1 and chains >= 3 and 0 < len(excluded) < n, (facts, chains, len(excluded), n)
    else:
        assert facts["null_dfs"] == facts["seeds"] >= 8 and chains == 0 and excluded == [], facts


def case_orphans_null_record(orc, lib, tmp):
    """a ROI k-mer without a record in GRAPH: the reference dereferences the null (FindOrphans.java:88-89)"""
    k = 21
    haps = family(orc, k, 0)
    gp, sp = str(tmp / "family.ctx"), str(tmp / "stranger.ctx")
    orc.build_graph(gp, haps, k)
    orc.build_graph(sp, [("kid", [rand_seq(random.Random(3), 80)])], k)
    g, stranger = CortexGraph(gp, lib=lib), CortexGraph(sp, lib=lib)
    try:
        FindOrphans(g, stranger, ["mom", "dad"]).execute(tmp / "never.ctx")
        raise AssertionError("a ROI k-mer without a record did not raise")
    except ca.JavaNullPointerException:
        pass
    try:
        findorphans_reference(orc, orc.Graph(gp, tuned=True), orc.Graph(sp, tuned=True), ["mom", "dad"])
        raise AssertionError("the yardstick accepted it")
    except ca.JavaNullPointerException:
        pass
    stranger.close(); g.close()
