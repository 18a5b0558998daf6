"""Lanes that take a second strand or search ("Frontier refill"): the parity cases of tests/parity_cases.py with fewer
lanes than running strands, so that every lane of k_walk / k_dfs goes back to the queue with the registers, the link store (LDS part
and HBM tail), the repeat snapshots, the frame stack and the visited table its previous strand left behind — and two batches beyond
the residency cap of the device, where the same happens with no knob set.  Shared by the host simulation
(tests/test_hostsim_refill.py, `-m "not gpu"`) and the real-hardware run (tests/test_gpu_refill.py, `-m gpu`).

A refill test proves something only if it reached the path: the library counts, per launch, the running strands beyond the lanes
(profile families walk_refills / dfs_refills: a lower bound on the strands begun by a lane that had one before), and every test here
ends with that count above zero for the kernel it is about."""
import random

import numpy as np

import corticall_amd as ca
from corticall_amd import BOTH, ContigStopper, TraversalEngineFactory
from tests import parity_cases as pc


def few_slots(monkeypatch, slots=64, **more_env):
    """at most `slots` lanes for every launch of k_walk and k_dfs from here on (LDBG_MAX_SLOTS; the library reads its knobs in every
    walk_prepare / dfs_prepare), and any further knob, e.g. LDBG_VT_INITIAL=64"""
    monkeypatch.setenv("LDBG_MAX_SLOTS", str(slots))
    for name, value in more_env.items():
        monkeypatch.setenv(name, str(value))


def refills(lib, family):
    """strands (family "walk_refills") or searches ("dfs_refills") that ran beyond the lanes of their launch since the last profile_reset"""
    assert family in ("walk_refills", "dfs_refills")
    return int(ca.profile_get(family, lib=lib)[0])


def refilled(lib, family, case, *args, **kw):
    """run `case` and require that lanes of the family's kernel took a further strand while it ran"""
    ca.profile_reset(lib=lib)
    case(*args, **kw)
    n = refills(lib, family)
    assert n > 0, "%s ran without a lane taking a second strand (%s = %d)" % (case.__name__, family, n)
    return n


# ------------------------------------------------------------------ the cases under few_slots(64): (case, its arguments after (orc, lib, tmp))
WALK_CASES = [(pc.case_random_walks, a) for a in ((31, 4, True), (47, 5, True), (32, 8, False), (65, 10, False))] \
    + [(pc.case_dense_cycles, (s,)) for s in (0, 2)] \
    + [(pc.case_run_steps, a) for a in ((0,), (3,), (1, 21, 8))] \
    + [(pc.case_big_link_stores, ()), (pc.case_partition, (31, 2, True)), (pc.case_findtips, (31, 2, True))]
# (knob, value) on top of the 64 lanes; each runs case_random_walks(31, 4, True) and case_dense_cycles(2)
WALK_KNOBS = [("LDBG_VT_INITIAL", 64), ("LDBG_WALK_BLOCK", 16), ("LDBG_WALK_BLOCK", 32), ("LDBG_FETCH_STRIDE", 1)]
DFS_CASES = [(pc.case_dfs_rules, a) for a in ((31, 4, True), (21, 3, False))] \
    + [(pc.case_dfs_dense, (s,)) for s in (0, 1)] \
    + [(pc.case_dfs_run_steps, (s,)) for s in (0, 231)] \
    + [(pc.case_many_dfs, min(pc.MANY_DFS))]
STEPS_ALONE = [(1, {}), (3, {}), (3, {"LDBG_FETCH_STRIDE": 1}), (0, {})]      # case_steps_alone_and_in_a_batch: (seed, further knobs)
SHARDED_WALKS = [(47, True, 2), (31, True, 5)]           # case_sharded_walks_one_rank_rccl: (k, with_links, colours)
SHARDED_DFS = [(21, 3), (32, 5)]                         # case_sharded_dfs_one_rank_rccl: (k, colours)


def case_id(c):
    return c[0].__name__[5:] + "".join("-%s" % x for x in c[1])


def case_walk_knobs(orc, lib, tmp, monkeypatch, knob, value, random_walks=True):
    few_slots(monkeypatch, 64, **{knob: value})
    if random_walks:
        refilled(lib, "walk_refills", pc.case_random_walks, orc, lib, tmp, 31, 4, True)
    refilled(lib, "walk_refills", pc.case_dense_cycles, orc, lib, tmp, 2)


def case_dfs_second_launch(orc, lib, tmp, monkeypatch):
    """the second launch, without the run index and with the retry[] queue, refilling: every search is sent round again"""
    few_slots(monkeypatch, 64, LDBG_DFS_FORCE_RETRY=1)
    refilled(lib, "dfs_refills", pc.case_dfs_run_steps, orc, lib, tmp, 0)
    refilled(lib, "dfs_refills", pc.case_dfs_dense, orc, lib, tmp, 1)


def case_step_counts_unchanged(orc, lib, tmp, monkeypatch, case, *args):
    """strands are independent: fewer lanes change the order they run in, never the steps they take.  (In the host simulation the
    wavefronts of a launch run one after the other and the first drains the queue with or without the knob, so there this compares two
    refilling runs; case_steps_alone_and_in_a_batch compares with strands that began in a fresh lane.)"""
    kinds = ("walk_steps_general", "walk_steps_lean", "walk_steps_run")
    ca.profile_reset(lib=lib)
    case(orc, lib, tmp, *args)
    plain = [ca.profile_get(f, lib=lib)[0] for f in kinds]
    assert refills(lib, "walk_refills") == 0 and sum(plain) > 0
    few_slots(monkeypatch, 64)
    refilled(lib, "walk_refills", case, orc, lib, tmp, *args)
    assert [ca.profile_get(f, lib=lib)[0] for f in kinds] == plain


# ------------------------------------------------------------------ beyond the residency cap with no knob (GPU only)
BEYOND_N = 70000          # 2 x 70,000 strands > 8 wavefronts x 256 CUs x 64 lanes = 131,072, the most lanes any device gives a launch


def _beyond_cap_graph(orc, lib, tmp, name):
    """a case_random_walks-style graph (1,500 bases, three colours, the child's links) and 70,000 seeds drawn with repetition from all its
    k-mers in both orientations -> (case, distinct seeds, index of every batch seed among them)"""
    k = 31
    rng = random.Random(70000 + k)
    base = pc.genome_with_repeats(rng, 1500, n_rep=8, rep_len=(k // 2 + 1, 4 * k), copies=(2, 3))
    kid = pc.mutate(rng, base, snv=0.01, indel=0.003)
    dad = pc.mutate(rng, base, snv=0.02, indel=0.003)
    rl = 3 * k
    reads = {"kid": [kid[i:i + rl] for i in range(0, max(1, len(kid) - rl + 1), rl // 4)] + [kid[-rl:]]}
    cs = pc.Case(orc, tmp, lib, [("kid", [kid]), ("mom", [base]), ("dad", [dad, pc.mutate(rng, dad)])], k, link_samples=["kid"], reads=reads, name=name)
    kmers = cs.all_kmers()
    distinct = kmers + [orc.revcomp(s) for s in kmers if orc.revcomp(s) != s]
    draw = np.random.default_rng(70000)          # every k-mer in both orientations once, the rest drawn with repetition, in random order
    which = draw.permutation(np.concatenate([np.arange(len(distinct)), draw.integers(0, len(distinct), BEYOND_N - len(distinct))]))
    assert len(which) == BEYOND_N and len(distinct) < BEYOND_N // 4
    return cs, distinct, which


def case_beyond_cap_walks(orc, lib, tmp):
    """70,000 walk seeds in one batch, the project's default direction (BOTH): more strands than the device has lanes for, so lanes refill
    with no knob set — and the per-strand arrays (block table, link-store tails, snapshots) are sized for a batch larger than its lanes.
    Every contig and walk length against the oracle's for its seed, kmers_traversed against the sum"""
    cs, distinct, which = _beyond_cap_graph(orc, lib, tmp, "cap_w")
    k = cs.k
    oe = orc.Engine(cs.og, [0], links=[cs.olinks["kid"]], max_length=100, stopper="ContigStopper")
    exp_c, exp_n, exp_t = [], [], []
    for s in distinct:       # one by one: the k-mers each walk traverses
        t0 = oe.kmers_traversed()
        c, nv = oe.walk(s)
        exp_c.append(c); exp_n.append(nv); exp_t.append(oe.kmers_traversed() - t0)
    exp_n, exp_t = np.array(exp_n, dtype=np.int64), np.array(exp_t, dtype=np.int64)
    e = (TraversalEngineFactory(lib=lib).traversalColors(0).graph(cs.g).maxBranchLength(100).stoppingRule(ContigStopper)
         .links(cs.links["kid"]).make())
    d_km = np.frombuffer("".join(distinct).encode(), dtype=np.uint8).reshape(len(distinct), k)
    ca.profile_reset(lib=lib)
    arena, offs, wl = e.walk_batch_arrays(np.ascontiguousarray(d_km[which]))
    assert refills(lib, "walk_refills") > 0
    assert len(wl) == BEYOND_N and (wl == exp_n[which]).all()
    exp_len = np.array([len(c) for c in exp_c], dtype=np.int64)
    assert (np.diff(offs) == exp_len[which]).all()
    raw = arena.tobytes()
    exp_b = [c.encode() for c in exp_c]
    for i, d in enumerate(which.tolist()):
        assert raw[offs[i]:offs[i + 1]] == exp_b[d], (i, distinct[d])
    assert e.kmers_traversed == int(exp_t[which].sum()), (e.kmers_traversed, int(exp_t[which].sum()))
    assert max(exp_len) > 3 * k and len(set(exp_c)) > 20      # walks of many kinds, long ones among them


def case_beyond_cap_dfs(orc, lib, tmp):
    """70,000 dfs sources in one batch, both directions, ExplorationStopper (a rule the run steps support): (null, vertices, edges) of
    every search against the oracle's for its source; the vertex and edge tuples of the first occurrence of every distinct source and of
    1,000 further searches.  maxLength 40, not the walks' 100: what the test is about is the size of the batch, and reading some
    9,000 graphs vertex by vertex on the host is what its time goes into"""
    cs, distinct, which = _beyond_cap_graph(orc, lib, tmp, "cap_d")
    k = cs.k
    oe, e = pc.dfs_engines(cs, trav=[0], stopper="ExplorationStopper", links=["kid"], direction=BOTH, max_len=40)
    exp = []
    t_each = []
    for s in distinct:
        t0 = oe.kmers_traversed()
        r = oe.dfs(s)
        exp.append(None if r.is_null else (r.vertices(), r.edges()))
        t_each.append(oe.kmers_traversed() - t0)
        r.free()
    sizes = np.array([(1, 0, 0) if x is None else (0, len(x[0]), len(x[1])) for x in exp], dtype=np.int64)
    src = np.ascontiguousarray(np.frombuffer("".join(distinct).encode(), dtype=np.uint8).reshape(len(distinct), k)[which]).reshape(-1)
    ca.profile_reset(lib=lib)
    batch = e.dfs_batch_arrays(src, BEYOND_N)
    assert refills(lib, "dfs_refills") > 0
    assert e.dfs_kmers_traversed == int(np.array(t_each, dtype=np.int64)[which].sum())
    graphs = [batch.graph(i) for i in range(BEYOND_N)]
    got = np.array([(1, 0, 0) if g is None else (0, g.nv, g.ne) for g in graphs], dtype=np.int64)
    assert (got == sizes[which]).all(), np.nonzero((got != sizes[which]).any(axis=1))[0][:8]
    _, first = np.unique(which, return_index=True)
    look = sorted(set(first.tolist()) | set(np.random.default_rng(7).integers(0, BEYOND_N, 1000).tolist()))
    for i in look:
        x = exp[which[i]]
        if x is not None:
            assert graphs[i].vertex_tuples() == x[0] and graphs[i].edge_tuples() == x[1], (i, distinct[which[i]])
    assert sizes[:, 0].sum() < len(distinct) and sizes[:, 1].max() > 2 * 40      # searches that return graphs; some larger than two branches of maxLength: they fork


# ------------------------------------------------------------------ a batch takes the steps of its strands, each walked alone
STEP_KINDS = ("walk_steps_general", "walk_steps_lean", "walk_steps_run")


def _step_counts(lib):
    return [int(ca.profile_get(f, lib=lib)[0]) for f in STEP_KINDS]


def case_steps_alone_and_in_a_batch(orc, lib, tmp, monkeypatch, seed, max_len=150, **more_env):
    """Strands are independent: what a lane did before it began a strand must not change the steps that strand takes.  The graph of
    parity_cases.case_dense_cycles (link-guided walks through cycles: anchors and snapshots of the repeat detection in nearly every strand);
    every k-mer in both orientations is walked ALONE first, each direction in a batch of its own (one strand begun, in a lane that
    had none before; the other ticket is skipped), then all of them in one batch over 64 lanes.  The step counts of the batch are the
    sums of the strands' own — a lane that kept the anchor, the period, the marks or the choices of its previous strand finds the
    repetitions of the next one at other steps (runstep.h: periodic_check) —, and the contigs are the oracle's."""
    rng = random.Random(seed)
    k = rng.choice([4, 5, 6])
    g1 = "".join(rng.choice("ACGT") for _ in range(rng.randint(40, 160)))
    g2 = pc.mutate(rng, g1, snv=0.05)
    reads = {"a": [g1[i:i + 5 * k] for i in range(0, len(g1), k)], "b": [g2]}
    cs = pc.Case(orc, tmp, lib, [("a", [g1]), ("b", [g2])], k, link_samples=["a", "b"], reads=reads, name="alone%d" % seed)
    seeds = cs.all_kmers()
    seeds = seeds + [orc.revcomp(s) for s in seeds]
    assert len(seeds) > 64
    alone = [0, 0, 0]
    for direction in (pc.FORWARD, pc.REVERSE):
        e = cs.engines(trav=[0], links=["a"], max_len=max_len, direction=direction)[1]
        ca.profile_reset(lib=lib)
        for s in seeds:
            e.walk_batch([s])
        assert refills(lib, "walk_refills") == 0
        alone = [x + y for x, y in zip(alone, _step_counts(lib))]
        e.close()
    few_slots(monkeypatch, 64, **more_env)
    oe, e = cs.engines(trav=[0], links=["a"], max_len=max_len)
    ca.profile_reset(lib=lib)
    got, wl = e.walk_batch(seeds)
    assert refills(lib, "walk_refills") > 0
    assert _step_counts(lib) == alone, (_step_counts(lib), alone)
    assert got == [oe.walk(s)[0] for s in seeds]
