"""Contigs spelled from the stored paths by k_contigs_rle and, for REPEAT descriptors, k_contigs_repeat (csrc/walk.cpp): cases shared by the
host-simulation run (tests/test_hostsim_contigs_repeat.py) and the real-hardware run (tests/test_gpu_contigs_repeat.py).  Every contig is
compared byte for byte with the oracle's and with the dense path of the same build (LDBG_EAGER_PATHS=1: k_expand_paths + k_contigs).

The graphs are the smallest that hold the cases: a tandem array whose reads lie inside it (the links send a walk round it until
maxLength: one REPEAT per strand), flanks long enough that the stored entries before the REPEAT cross a group of 64 and a path block,
and one long unbranched stretch cut by maxLength at every run length that takes another path of the copy (1-7 single bytes, 8 one access,
8 * 16 * 4 one full round of four accesses per lane of a 16-lane group, one more a second round)."""
import os
import random

from tests import parity_cases as pc


def three_ways(case, seeds, **cfg):
    """stored paths (k_contigs_rle + k_contigs_repeat) == oracle == dense path of the same build"""
    seeds = list(seeds)
    exp = pc.compare_walks(case, seeds, **cfg)
    os.environ["LDBG_EAGER_PATHS"] = "1"            # (read by the library at every batch)
    try:
        _, e = case.engines(**cfg)
        dense, _ = e.walk_batch(seeds)
    finally:
        del os.environ["LDBG_EAGER_PATHS"]
    assert dense == exp, [(s, d, x) for s, d, x in zip(seeds, dense, exp) if d != x][:2]
    return exp


def tandem_case(orc, lib, tmp, k, unit_len, copies, flank, seed, name):
    """flank + unit * copies + flank, reads = every window of 6k bases INSIDE the array: at the array's exit the links say "round again" """
    rng = random.Random(seed)
    unit = pc.rand_seq(rng, unit_len)
    arr = unit * copies
    g = pc.rand_seq(rng, flank) + arr + pc.rand_seq(rng, flank)
    reads = {"a": [arr[i:i + 6 * k] for i in range(0, max(1, len(arr) - 6 * k + 1))]}
    return pc.Case(orc, tmp, lib, [("a", [g])], k, link_samples=["a"], reads=reads, name=name), g, flank, len(arr)


def array_seeds(orc, g, k, flank, arr_len, n):
    """n k-mers from inside the array, every other one reverse-complemented"""
    at = range(flank + k, flank + arr_len - 2 * k)
    step = max(1, len(at) // n)
    return [orc.revcomp(g[i:i + k]) if j % 2 else g[i:i + k] for j, i in enumerate(list(at)[::step][:n])]


def case_no_repeat(orc, lib, tmp):
    """the tandem graph walked without links, and the flanks alone with them: no strand ends in a REPEAT"""
    cs, g, flank, arr_len = tandem_case(orc, lib, tmp, 9, 12, 8, 80, 11, "norep")
    seeds = array_seeds(orc, g, 9, flank, arr_len, 8) + [g[:9], g[-9:]]
    three_ways(cs, seeds, trav=[0], max_len=400)
    three_ways(cs, [g[:9], g[20:29]], trav=[0], links=["a"], max_len=60)


def case_every_walk_repeats(orc, lib, tmp, n=7):
    """seeds inside the array in the orientation of its reads, with links: both strands of every seed circle until maxLength (period 12); then
    a batch of both orientations on a period of 20, where some walks circle and others end at once"""
    cs, g, flank, arr_len = tandem_case(orc, lib, tmp, 9, 12, 8, 80, 20, "all")
    seeds = [g[i:i + 9] for i in range(flank + 12 + 4, flank + 12 + 4 + min(n, 7))]      # (the unit's other five k-mers end their walk at once)
    exp = three_ways(cs, seeds, trav=[0], links=["a"], max_len=1200)
    assert all(len(c) > 2 * 1200 for c in exp)
    cs, g, flank, arr_len = tandem_case(orc, lib, tmp, 15, 20, 10, 80, 5, "mix")
    exp = three_ways(cs, array_seeds(orc, g, 15, flank, arr_len, 10), trav=[0], links=["a"], max_len=1500)
    assert min(len(c) for c in exp) < 100 and max(len(c) for c in exp) > 2 * 1500
    return len(seeds)


def case_short_period_and_len(orc, lib, tmp, n=6, max_lens=range(46, 66)):
    """period 5 (< 8: a chunk of eight bases wraps round the revolution), maxLength swept one by one: the REPEAT's `len` takes every
    residue mod 8 and every value below 8 just past the point where the repetition is proven (48 vertices)"""
    cs, g, flank, arr_len = tandem_case(orc, lib, tmp, 9, 5, 14, 80, 7, "short")
    seeds = array_seeds(orc, g, 9, flank, arr_len, n)
    for ml in max_lens:
        three_ways(cs, seeds, trav=[0], links=["a"], max_len=ml)


def case_repeat_after_long_flank(orc, lib, tmp, n=66, k=15, flank=1100):
    """the run index switched off (LDBG_NO_RUNS: one stored entry per vertex) and seeds at n consecutive places of a flank longer than a
    path block: the forward strands reach the array after > 1024 stored entries, and the REPEAT head falls on every place of a group of
    64 — the last one among them, where the payload word is the first entry of the next group"""
    cs, g, flank, arr_len = tandem_case(orc, lib, tmp, k, 7, 30, flank, 5, "flank")
    seeds = [g[i:i + k] for i in range(n)]
    os.environ["LDBG_NO_RUNS"] = "1"            # (read by an engine before its first batch)
    try:
        exp = three_ways(cs, seeds, trav=[0], links=["a"], max_len=flank + 150)
    finally:
        del os.environ["LDBG_NO_RUNS"]
    assert all(len(c) > flank + 150 for c in exp)


def case_run_lengths(orc, lib, tmp, max_lens=tuple(range(2, 16)) + tuple(range(508, 522))):
    """one unbranched stretch of 700 vertices, maxLength cutting it at every length: runs of 1-7, 8, 8 * 16 * 4 and 8 * 16 * 4 + 1 vertices;
    the seed and its reverse complement, both strands: ascending and descending runs, plain and mirrored"""
    rng = random.Random(3)
    k = 11
    g = pc.rand_seq(rng, 700 + k - 1)
    cs = pc.Case(orc, tmp, lib, [("a", [g])], k, link_samples=["a"], reads={"a": [g]}, name="runs")
    seeds = [g[:k], orc.revcomp(g[:k]), g[-k:], orc.revcomp(g[-k:]), g[300:300 + k], orc.revcomp(g[300:300 + k])]
    for ml in max_lens:
        three_ways(cs, seeds, trav=[0], max_len=ml)
        three_ways(cs, seeds, trav=[0], links=["a"], max_len=ml)
