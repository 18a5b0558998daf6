"""The fixed-layout walk kernels (csrc/walk.cpp: k_walk_rows<W, C>, the probe-row layout of graph.h: row_layout compiled in) against the
generic k_walk<W, 64, false>: cases built on the helpers of tests/parity_cases.py, shared by the host simulation
(tests/test_hostsim_walk_rows.py) and the device (tests/test_gpu_walk_rows.py).

The fixed kernels are switched on with LDBG_WALK_ROWS (walk.cpp: walk_rows_fit says why they are not the default yet).  Every case runs
twice: as the library dispatches it by default, every launch on the generic kernel, and with the knob set.  The helpers compare every
batch with the oracle; a spy on TraversalEngine.walk_batch_arrays keeps what every batch returned (contig bytes, offsets, walk lengths,
k-mers traversed, or the error), and the two runs must agree byte for byte.  The profile family walk_fixed_rows counts the launches that
took a fixed kernel: under the knob above zero for a FIXED case and zero for a GENERIC one, and zero for every case without the knob."""
import random

import corticall_amd as ca
from tests import parity_cases as pc

KNOB = "LDBG_WALK_ROWS"


def fixed_rows(lib):
    return int(ca.profile_get("walk_fixed_rows", lib=lib)[0])


def recorded(monkeypatch, lib, case, *args):
    """run case(*args) -> (what every walk batch returned, launches that took a fixed kernel)"""
    seen = []
    real = ca.TraversalEngine.walk_batch_arrays

    def spy(self, seeds, *a, **kw):
        try:
            arena, offs, wl = real(self, seeds, *a, **kw)
        except Exception as ex:
            seen.append(type(ex).__name__)
            raise
        seen.append((None if arena is None else arena.tobytes(), None if offs is None else offs.tobytes(), None if wl is None else wl.tobytes(),
                     self.kmers_traversed))
        return arena, offs, wl
    with monkeypatch.context() as m:
        m.setattr(ca.TraversalEngine, "walk_batch_arrays", spy)
        ca.profile_reset(lib=lib)
        case(*args)
        return seen, fixed_rows(lib)


def both_kernels(monkeypatch, lib, fixed, case, *args):
    """the case on the generic kernel and under the knob: the same bytes; walk_fixed_rows says which kernel ran.  -> batches of the case"""
    plain, n_plain = recorded(monkeypatch, lib, case, *args)
    assert len(plain) > 0
    assert n_plain == 0, "%s%r without %s: walk_fixed_rows = %d" % (case.__name__, args[3:], KNOB, n_plain)
    with monkeypatch.context() as m:
        m.setenv(KNOB, "1")
        rows, n_fixed = recorded(monkeypatch, lib, case, *args)
    assert (n_fixed > 0) == fixed, "%s%r under %s: walk_fixed_rows = %d" % (case.__name__, args[3:], KNOB, n_fixed)
    assert len(rows) == len(plain)
    for i, (x, y) in enumerate(zip(plain, rows)):
        assert x == y, "%s%r: batch %d differs between the fixed and the generic kernel" % (case.__name__, args[3:], i)
    return len(plain)


def second_launch(monkeypatch, lib, case, *args):
    """The second launch of a batch — the strands handed back (ST_RETRY_PLAIN), walked again from their seeds WITHOUT the run index —
    through the fixed kernel.  No case of the suites makes the run steps hand a strand back (runstep.h: a cursor that runs out inside a
    piece), so LDBG_WALK_FORCE_RETRY sends every strand round: walk_retried_strands above zero, two fixed launches per run, and the
    bytes of the plain run on the generic kernel, of the forced run on the generic kernel and of the forced run on the fixed kernel equal
    (each batch also against the oracle, in the helper)."""
    def retried():
        return int(ca.profile_get("walk_retried_strands", lib=lib)[0])
    plain, n_plain = recorded(monkeypatch, lib, case, *args)
    assert n_plain == 0 and retried() == 0 and len(plain) > 0
    with monkeypatch.context() as m:
        m.setenv("LDBG_WALK_FORCE_RETRY", "1")
        forced, n_forced = recorded(monkeypatch, lib, case, *args)
        again_generic = retried()
        m.setenv(KNOB, "1")
        rows, n_fixed = recorded(monkeypatch, lib, case, *args)
        again_fixed = retried()
        runs = int(ca.profile_get("walk_fixed_rows", lib=lib)[1])      # walk runs (a batch is one, or more where a pool ran dry and it was split)
    assert n_forced == 0 and again_generic > 0
    assert again_fixed == again_generic, (again_fixed, again_generic)
    assert runs >= len(rows) and n_fixed == 2 * runs, "walk_fixed_rows = %d over %d runs: a second launch did not take the fixed kernel" % (n_fixed, runs)
    assert plain == forced == rows


def case_q6_walks(orc, lib, tmp):
    """the walks of parity_cases.case_hash_collision (quirk Q6: k-mers whose two orientations hash alike, tests/golden/hash_collisions.txt)
    for the odd k of one and two words (W = 1 and 2, two colours), the seed-by-seed walks with a recruitment colour and their Q14 errors
    included: strict_flip through the folded row decode.  Left out are its searches and cursors, which run k_dfs and the cursor kernels
    and take the whole helper to five minutes."""
    import os
    rng = random.Random(5)
    for x in open(os.path.join(pc.GOLDEN, "hash_collisions.txt")).read().split():
        k = len(x)
        if not (k & 1) or k > 63:
            continue
        flank = lambda n: pc.rand_seq(rng, n)
        xo = x if rng.random() < 0.5 else orc.revcomp(x)
        h1 = flank(3 * k) + xo + flank(3 * k)
        h2 = flank(2 * k) + h1[2 * k: 5 * k + 5] + flank(2 * k)        # shares the colliding k-mer, forks around it
        h3 = flank(k) + orc.revcomp(xo) + flank(k)
        cs = pc.Case(orc, tmp, lib, [("a", [h1, h2, h3]), ("b", [h1])], k, link_samples=["a"], reads={"a": [h1, h2, h3]}, name="q6_%d_%s" % (k, x[:6]))
        assert not orc.is_flipped(orc.revcomp(orc.canonical(x)))
        seeds = [x, orc.revcomp(x)] + [h1[i:i + k] for i in range(2 * k, 4 * k + 1, 3)]
        seeds += [orc.revcomp(s) for s in seeds]
        for links in ([], ["a"]):
            pc.compare_walks(cs, seeds, trav=[0], links=links, max_len=300)
            oe, e = cs.engines(trav=[1], links=links, recruit=[0], max_len=300)
            for sd in seeds:
                try:
                    exp = oe.walk(sd)[0]
                except orc.OracleError as ex:
                    assert "NullPointerException" in str(ex)
                    exp = None
                try:
                    got = e.walk_batch([sd])[0][0]
                except ca.JavaNullPointerException:
                    got = None
                assert got == exp, (sd, got, exp)


def case_one_colour(orc, lib, tmp, k, seed):
    """a one-colour graph with repeats, walked with and without its links, both directions and each alone (C = 1: the edge byte and the
    flag byte share the word the row decode reads with nothing between them)"""
    rng = random.Random(9100 + 13 * k + seed)
    g1 = pc.genome_with_repeats(rng, max(600, 12 * k), n_rep=5, rep_len=(k // 2 + 1, 3 * k), copies=(2, 3))
    rl = max(3 * k, 40)
    reads = {"a": [g1[i:i + rl] for i in range(0, max(1, len(g1) - rl + 1), max(1, rl // 4))] + [g1[-rl:]]}
    cs = pc.Case(orc, tmp, lib, [("a", [g1])], k, link_samples=["a"], reads=reads, name="one%d_%d" % (k, seed))
    kmers = cs.all_kmers()
    seeds = rng.sample(kmers, min(60, len(kmers)))
    seeds = [s if rng.random() < 0.5 else orc.revcomp(s) for s in seeds] + [pc.rand_seq(rng, k), "N" * k, g1[:k], g1[-k:]]
    exp = pc.compare_walks(cs, seeds, trav=[0], max_len=75000)
    assert max(len(c) for c in exp) > 3 * k
    pc.compare_walks(cs, seeds, trav=[0], links=["a"], max_len=400)
    pc.compare_walks(cs, seeds[:30], trav=[0], links=["a"], direction=pc.FORWARD, op=pc.AND, max_len=400)
    pc.compare_walks(cs, seeds[:30], trav=[0], direction=pc.REVERSE, max_len=75000)
    pc.compare_walks(cs, seeds[:30], trav=[0], links=["a"], max_len=7)


# (case, its arguments after (orc, lib, tmp)): every instantiation k_walk_rows<W, C>, W in {1, 2} x C in {1, 2, 3}; k = 5, 31, 47, 63; with
# and without links
FIXED = [
    (pc.case_random_walks, (31, 4, True)),      # W 1, C 3
    (pc.case_random_walks, (5, 6, False)),      # W 1, C 3, the smallest odd k
    (pc.case_random_walks, (47, 5, True)),      # W 2, C 3: the reference pipeline's shape
    (pc.case_random_walks, (63, 7, False)),     # W 2, C 3, the largest odd k of two words
    (pc.case_run_steps, (0,)),                  # W 1, C 2: run steps, REPEAT descriptors
    (pc.case_run_steps, (1, 47)),               # W 2, C 2
    (case_one_colour, (31, 0)),                 # W 1, C 1
    (case_one_colour, (63, 1)),                 # W 2, C 1
    (pc.case_big_link_stores, ()),              # W 1, C 1, k = 5: link stores beyond LDS
    (case_q6_walks, ()),                        # W 1 and 2, C 2: Q6 vertices (strict_flip) through the folded row decode
]
# on the device: without the second run-step case (its oracle share takes it past a few seconds; <2, 2> runs there in case_q6_walks,
# whose k = 47 and 63 graphs have two colours)
FIXED_DEVICE = [c for c in FIXED if c != (pc.case_run_steps, (1, 47))]
# what stays on k_walk<W, 64, false>: even k, three words, four colours
GENERIC = [
    (pc.case_random_walks, (46, 8, True)),
    (pc.case_random_walks, (65, 10, False)),
    (pc.case_many_walks, (4, 31, True)),
    (pc.case_many_walks, (4, 31, False)),
]


def case_id(c):
    return c[0].__name__[5:] + "".join("-%s" % x for x in c[1])
