"""Graph construction cases (ldbg_graph_build / ldbg_graph_build_ctx) shared by the host-simulation run
(tests/test_build_hostsim.py) and the GPU run (tests/test_gpu_build.py).

The yardstick is the oracle's build_graph, a restatement of TempGraphAssembler.buildGraph that keeps a std::map of strings: the
file the library writes must equal the oracle's file byte for byte, header included.  (The oracle orients a k-mer by
CanonicalKmer's hash test, the library by value — SURVEY Q6: an input holding a k-mer whose Arrays.hashCode equals its reverse
complement's, p ~ 2^-32 per k-mer, would show up here as a byte difference.)"""
import ctypes as C

import numpy as np

import corticall_amd as ca
from corticall_amd import BOTH, OR, ContigStopper, CortexGraph, TraversalEngineFactory
from corticall_amd import _native
from corticall_amd.build import SPLIT_NON_ACGT, Build, build_ctx
from corticall_amd.partition import unpack_kmers

K = 31
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


def revcomp(s):
    return s.encode().translate(_COMP)[::-1].decode()


def mutate(rng, s, rate):
    a = np.frombuffer(s.encode(), dtype=np.uint8).copy()
    hit = np.nonzero(rng.random(len(a)) < rate)[0]
    a[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=len(hit))]
    return a.tobytes().decode()


def windows(samples, k):
    return sum(max(0, len(s) - k + 1) for _, seqs in samples for s in seqs)


def check_file(orc, lib, tmp, samples, k, tag, oracle_samples=None, split=False):
    """the library's file against the oracle's -> (records written, the library's file, the oracle's file)"""
    want, got = tmp / (tag + "_want.ctx"), tmp / (tag + ".ctx")
    orc.build_graph(str(want), oracle_samples if oracle_samples is not None else samples, k)
    n = build_ctx(samples, k, got, split_non_acgt=split, lib=lib)
    a, b = got.read_bytes(), want.read_bytes()
    assert len(a) == len(b), (tag, len(a), len(b))
    assert a == b, tag
    W, C_ = (k + 31) // 32, len(samples)
    assert n == (len(a) - header_len(C_, samples)) // (8 * W + 5 * C_)
    return n, got, want


def header_len(C_, samples):
    return 6 + 16 + 12 * C_ + sum(4 + len(n.encode()) for n, _ in samples) + 16 * C_ + 16 * C_ + 6


# ---------------------------------------------------------------- cases
SHAPE_WINDOWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 20001, 70000]


def shape_samples(M):
    rng = np.random.default_rng(M)
    if M == 0:
        return [("s", [rand_seq(rng, K - 1)])]
    a = M // 3                                           # two sequences when there is room: a + (M - a) windows
    lens = [M + K - 1] if a == 0 else [a + K - 1, M - a + K - 1]
    return [("s", [rand_seq(rng, n) for n in lens])]


def case_shapes(orc, lib, tmp, M):
    """total windows around a ballot word, a chunk of the run scan, and sizes at which the sort's 16,384 chunk owners hold uneven
    chunks longer than one key (20001, 70000)"""
    samples = shape_samples(M)
    assert windows(samples, K) == M
    n, got, want = check_file(orc, lib, tmp, samples, K, "shape%d" % M)
    assert n <= M and (n > 0) == (M > 0)
    g, ref = CortexGraph.build(samples, K, lib=lib), CortexGraph(want, lib=lib)       # M = 0: a header-only file opens as a graph of 0 records
    assert g.getNumRecords() == ref.getNumRecords() == n
    g.close()
    ref.close()


KMER_SIZES = [3, 4, 5, 31, 32, 33, 47, 63, 64, 65, 96, 127, 128]


def case_kmer_sizes(orc, lib, tmp, k):
    """2 colours, about 3,000 windows; every even k has a planted palindromic k-mer with neighbours on both sides"""
    rng = np.random.default_rng(100 + k)
    a = rand_seq(rng, 1500 + k - 1)
    if k % 2 == 0:
        half = rand_seq(rng, k // 2)
        pal = half + revcomp(half)
        assert pal == revcomp(pal)
        a = a[:100] + pal + a[100 + k:]
        assert a[100:100 + k] == pal and len(a) == 1500 + k - 1
    b = mutate(rng, a, 0.01)
    samples = [("one", [a]), ("two", [b])]
    n, _, _ = check_file(orc, lib, tmp, samples, k, "k%d" % k)
    assert n > 0


EDGE_VARIANTS = ["len0", "lenk-1", "lenk", "lenk+1", "reads", "empty_sample", "subset_sample", "mixed_case"]


def case_sequence_edges(orc, lib, tmp, variant):
    rng = np.random.default_rng(EDGE_VARIANTS.index(variant))
    k = K
    x, y = rand_seq(rng, 900), rand_seq(rng, 700)
    if variant.startswith("len"):
        n = {"len0": 0, "lenk-1": k - 1, "lenk": k, "lenk+1": k + 1}[variant]
        s = rand_seq(rng, n)
        samples = [("a", [s]), ("b", [s, x, s])]
        assert windows(samples[:1], k) == max(0, n - k + 1)
    elif variant == "reads":                             # window tiles straddle many sequence boundaries
        starts = rng.integers(0, len(x) + len(y) - 2 * (k + 5), size=5000)
        g = x + y
        reads = [g[s:s + k + int(l)] for s, l in zip(starts, rng.integers(0, 6, size=5000))]
        samples = [("a", reads[:2500]), ("b", reads[2500:])]
    elif variant == "empty_sample":
        samples = [("a", [x]), ("none", []), ("c", [y, x[:200]])]
    elif variant == "subset_sample":                     # every k-mer of b occurs in a
        samples = [("a", [x]), ("b", [x[100:400], revcomp(x[500:600])])]
    else:
        mixed = "".join(c.lower() if i % 3 else c for i, c in enumerate(y))
        samples = [("a", [x.lower()]), ("b", [mixed, x])]
    n, _, want = check_file(orc, lib, tmp, samples, k, "edge_" + variant.replace("+", "p").replace("-", "m"))
    assert n > 0
    if variant == "mixed_case":                          # the oracle upper-cases: the same file as the upper-case input's
        up = tmp / "upper.ctx"
        orc.build_graph(str(up), [(nm, [s.upper() for s in seqs]) for nm, seqs in samples], k)
        assert up.read_bytes() == want.read_bytes()


COLOURS = [1, 2, 3, 8, 32]


def case_colours(orc, lib, tmp, C_):
    """overlapping haplotypes derived from one ancestor"""
    rng = np.random.default_rng(200 + C_)
    anc = rand_seq(rng, 600)
    samples = [("s%d" % c, [mutate(rng, anc, 0.01)] + ([mutate(rng, anc[50:400], 0.02)] if c % 2 else [])) for c in range(C_)]
    n, _, _ = check_file(orc, lib, tmp, samples, 21, "colours%d" % C_)
    assert n >= 580


HEAVY = ["poly_a", "tandem7", "random5k_k31", "random5k_k6"]


def case_heavy_kmers(orc, lib, tmp, variant):
    """k-mers seen very often: one record takes 100,000 windows (poly-A), seven records 50,000 windows between them, and at k = 6
    almost every k-mer is repeated"""
    rng = np.random.default_rng(300 + HEAVY.index(variant))
    k = 6 if variant.endswith("k6") else K
    if variant == "poly_a":
        samples = [("a", ["A" * (100000 + k)]), ("b", ["A" * 40 + "C" + rand_seq(rng, 100) + "G" + "T" * 50])]
    elif variant == "tandem7":
        samples = [("a", [("ACGGTCA" * 7200)[:50000]]), ("b", [rand_seq(rng, 100)])]
    else:
        x = rand_seq(rng, 5000)
        samples = [("a", [x]), ("b", [mutate(rng, x, 0.02)])]
    n, got, _ = check_file(orc, lib, tmp, samples, k, "heavy_" + variant)
    if variant == "poly_a":
        g = CortexGraph(got, lib=lib)
        cr = g.findRecord("A" * k)
        assert cr.getCoverage(0) == 100001 and cr.getCoverage(1) == 40 - k + 1 + 50 - k + 1   # (T...T is the same canonical k-mer)
        g.close()
    if variant == "tandem7":
        assert n <= 7 + 100 - k + 1


def case_reference_shapes(orc, lib, tmp):
    """the graphs of the reference's own builder tests (TraversalEngineTest.java:49-122, tests/test_oracle_golden.py V3-V5)"""
    n, _, _ = check_file(orc, lib, tmp, [("mom", ["AATA"]), ("dad", ["AATG"])], 3, "v3")
    assert n == 3
    h = "AGTTCTGATCTGGGCTATATGCT"
    n, got, _ = check_file(orc, lib, tmp, [("mom", [h]), ("dad", [h]), ("kid", [h])], 5, "v4")
    assert n == 19
    g = CortexGraph(got, lib=lib)
    assert g.getRecord(0).toString() == "AGAAC 1 1 1 .c.....T .c.....T .c.....T"
    g.close()
    n, _, _ = check_file(orc, lib, tmp, [("mom", ["AGTTCTGATCTGGGCTATATGCT"]), ("dad", ["AGTTCGAATCTGGGCTATATGCT"]),
                                         ("kid", ["AGTTCTGATCTGGGCTATGGCTA"])], 5, "v5")
    assert n > 19
    # a dict gives the samples in insertion order; CortexGraph.build(path=...) writes the same file and opens it
    out = tmp / "v3_dict.ctx"
    g = CortexGraph.build({"mom": ["AATA"], "dad": ["AATG"]}, 3, path=out, lib=lib)
    assert out.read_bytes() == (tmp / "v3_want.ctx").read_bytes() and g.getNumRecords() == 3 and g.getSampleName(1) == "dad"
    g.close()


def case_resident(orc, lib, tmp):
    """the graph ldbg_graph_build leaves on the device against a graph opened from the oracle's file: the built table is a
    first-class graph"""
    rng = np.random.default_rng(400)
    k = 21
    anc = rand_seq(rng, 1200)
    anc = anc[:500] + anc[200:260] + anc[500:]                                         # a repeat
    samples = [("kid", [mutate(rng, anc, 0.02)]), ("mom", [anc]), ("dad", [mutate(rng, anc, 0.01), anc[300:700]])]
    want = tmp / "resident_want.ctx"
    orc.build_graph(str(want), samples, k)
    res, fil = CortexGraph.build(samples, k, lib=lib), CortexGraph(want, lib=lib)
    info = lambda g: (g.getKmerSize(), g.getKmerBits(), g.getNumColors(), g.getNumRecords(), g.getVersion(),
                      [g.getSampleName(c) for c in range(g.getNumColors())], g.getColors())
    assert info(res) == info(fil)
    n = res.getNumRecords()
    assert n > 1000
    a, b = res.records(0, n), fil.records(0, n)
    assert all((x == y).all() for x, y in zip(a, b))
    fw = unpack_kmers(a[0], k)
    rc = np.frombuffer(b"".join(revcomp(s.tobytes().decode()).encode() for s in fw), dtype=np.uint8).reshape(n, k)
    absent = []
    present = {s.tobytes() for s in fw} | {s.tobytes() for s in rc}
    while len(absent) < 100:
        q = rand_seq(rng, k).encode()
        if q not in present:
            absent.append(np.frombuffer(q, dtype=np.uint8))
    for q in (fw, rc, np.array(absent)):
        ia, ib = res.find_batch(q), fil.find_batch(q)
        assert all((x == y).all() for x, y in zip(ia, ib))
    assert (res.find_batch(fw)[0] == np.arange(n)).all() and (res.find_batch(rc)[0] == np.arange(n)).all()
    assert (res.find_batch(np.array(absent))[0] == -1).all()
    # ContigStopper walks from 50 seeds: an engine on the built graph against the oracle's engine on the oracle's file
    seeds = [fw[i].tobytes().decode() for i in rng.choice(n, size=50, replace=False)]
    og = orc.Graph(str(want))
    oe = orc.Engine(og, [0], stopper="ContigStopper")
    e = (TraversalEngineFactory(lib=lib).traversalColors(0).traversalDirection(BOTH).combinationOperator(OR).graph(res)
         .stoppingRule(ContigStopper).make())
    got, wl = e.walk_batch(seeds)
    arena, offs, nv = oe.walk_batch(np.frombuffer("".join(seeds).encode(), dtype=np.uint8).reshape(50, k))
    raw = arena.tobytes()
    assert [raw[offs[i]:offs[i + 1]].decode() for i in range(50)] == list(got) and (np.asarray(wl) == nv).all()
    assert max(len(c) for c in got) > k
    e.close()
    oe.close()
    og.close()
    res.close()
    fil.close()


NON_ACGT_BYTES = [b"N", b".", b"\n", b"\xc1"]


def case_non_acgt(orc, lib, tmp, bad):
    rng = np.random.default_rng(500 + NON_ACGT_BYTES.index(bad))
    k = K
    x, y = rand_seq(rng, 400).encode(), rand_seq(rng, 300).encode()
    inputs = {"first": bad + x[1:], "last": x[:-1] + bad, "inside": x[:150] + bad + x[151:], "run": x[:90] + bad * 5 + x[95:200] + bad + x[201:]}
    for where, s in inputs.items():
        samples = [("a", [y, s]), ("b", [y[50:200]])]
        out = tmp / ("bad_%s.ctx" % where)
        try:                                             # default: as the reference, which throws when it encodes such a k-mer
            build_ctx(samples, k, out, lib=lib)
            raise AssertionError("a %r %s did not raise" % (bad, where))
        except ca.CortexJDKException:
            pass
        assert not out.exists(), "a file was left behind"
        try:
            CortexGraph.build(samples, k, lib=lib)
            raise AssertionError("a %r %s did not raise" % (bad, where))
        except ca.CortexJDKException:
            pass
        # LDBG_BUILD_SPLIT_NON_ACGT: the oracle's build of the pieces, cut here
        pieces = [(nm, [p.decode() for q in seqs for p in (q if isinstance(q, bytes) else q.encode()).split(bad)]) for nm, seqs in samples]
        n, _, _ = check_file(orc, lib, tmp, samples, k, "split_%s" % where, oracle_samples=pieces, split=True)
        assert n > 0
    # a sequence shorter than k is never encoded: its bytes do not matter
    check_file(orc, lib, tmp, [("a", [y, bad * (k - 1)])], k, "short_bad", oracle_samples=[("a", [y.decode()])])
    # Build: one FASTA per sample, split on
    fa, fb = tmp / "a.fa", tmp / "b.fa"
    fa.write_bytes(b">one\n" + x[:100] + b"\n" + x[100:200] + b"\nNNNN" + x[200:] + b"\n>two\n" + y + b"\n")
    fb.write_bytes(b">only\r\n" + y[:120].lower() + b"\r\n")
    out = tmp / "fasta.ctx"
    n = Build({"a": fa, "b": fb}, k, out, lib=lib).execute()
    want = tmp / "fasta_want.ctx"
    orc.build_graph(str(want), [("a", [x[:200].decode(), x[200:].decode(), y.decode()]), ("b", [y[:120].decode()])], k)
    assert out.read_bytes() == want.read_bytes() and n > 0


def case_deterministic(orc, lib, tmp):
    samples = shape_samples(70000)
    a, b = tmp / "det_a.ctx", tmp / "det_b.ctx"
    build_ctx(samples, K, a, lib=lib)
    build_ctx(samples, K, b, lib=lib)
    assert a.read_bytes() == b.read_bytes()


def _raw(lib, samples, k, flags=0, out=True):
    """ldbg_graph_build on hand-made ldbg_build_sample entries: (name, bases, offsets, n_sequences) -> status"""
    arr = (_native.BuildSample * max(1, len(samples)))()
    keep = []
    for i, (name, bases, offs, n) in enumerate(samples):
        o = np.asarray(offs, dtype=np.int64) if offs is not None else None
        keep += [o, bases, name]
        arr[i].sample_name = name
        arr[i].bases = C.cast(C.c_char_p(bases), C.c_void_p) if bases is not None else None
        arr[i].offsets = o.ctypes.data if o is not None else None
        arr[i].n_sequences = n
    h = C.c_void_p()
    st = lib.dll.ldbg_graph_build(arr if samples is not None else None, len(samples), k, flags, 0, C.byref(h) if out else None)
    assert not h.value or st == 0
    if h.value:
        lib.dll.ldbg_graph_close(h)
    return st


def case_bad_arguments(orc, lib, tmp):
    ARG, UNSUPPORTED = 6, 4
    seq = b"ACGTACGTACGTTTGACA"
    good = (b"s", seq, [0, len(seq)], 1)
    assert _raw(lib, [good], 5) == 0
    for k in (2, 0, -1, 129, 160):                                              # k below 3 or above what the loader accepts (W <= 4)
        assert _raw(lib, [good], k) == ARG, k
    assert _raw(lib, [good], 3) == 0 and _raw(lib, [good], 128) == 0            # (128 > len: no window, still a graph of one colour)
    assert _raw(lib, [], 5) == ARG                                              # no samples
    assert lib.dll.ldbg_graph_build(None, 1, 5, 0, 0, C.byref(C.c_void_p())) == ARG
    many = [(b"s%d" % i, seq, [0, len(seq)], 1) for i in range(_native.MAX_COLORS + 1)]
    assert _raw(lib, many, 5) == ARG and _raw(lib, many[:-1], 5) == 0          # more colours than the loader accepts
    assert _raw(lib, [good, (b"t", seq, [0, 4], 1), good], 5) == ARG            # duplicate sample names
    assert _raw(lib, [(None, seq, [0, 4], 1)], 5) == ARG                        # null pointers
    assert _raw(lib, [(b"s", None, [0, 4], 1)], 5) == ARG
    assert _raw(lib, [(b"s", seq, None, 1)], 5) == ARG
    assert _raw(lib, [good], 5, out=False) == ARG
    assert _raw(lib, [(b"s", None, None, 0)], 5) == 0                           # (a sample without sequences needs neither)
    assert _raw(lib, [(b"s", seq, [0, 10, 8, 18], 3)], 5) == ARG                # decreasing offsets
    assert _raw(lib, [(b"s", seq, [-1, 10], 1)], 5) == ARG
    assert _raw(lib, [(b"s", seq, [0, 10, 10, 18], 3)], 5) == 0                 # (an empty sequence is fine)
    assert _raw(lib, [good], 5, flags=2) == ARG                                 # an unknown flag
    assert lib.dll.ldbg_graph_build_ctx((_native.BuildSample * 1)(), 1, 5, 0, 0, None, None) == ARG
    # 2^32 windows: refused from the offsets alone, before anything is read or allocated
    assert _raw(lib, [(b"s", seq, [0, (1 << 32) + 5 - 1], 1)], 5) == UNSUPPORTED
    assert _raw(lib, [(b"s", seq, [0, 1 << 31], 1), (b"t", seq, [0, (1 << 31) + 8], 1)], 5) == UNSUPPORTED
    assert SPLIT_NON_ACGT == 1
