// Unitigs of a colour set on the device (unitigs.h): unique mutual links -> list ranking by pointer jumping ->
// pure cycles cut at their smallest member (a second pointer-jumping pass carrying a minimum) -> mirror choice and head flag ->
// ids and base offsets by a chunked scan -> sequence, labels and coverage.  As in runs.cpp every kernel is a grid-stride loop
// over oriented vertices a = 2 * record + flip (or over records, or unitigs), reads and writes only what no other thread of the
// same launch writes or reads (apart from the 8-byte (pointer, value) words of the jumping passes), and never waits for another:
// the TEST-ONLY host simulation runs them as they are.
#include "unitigs.h"
#include "listrank.h"

#include <stdio.h>

#include <algorithm>
#include <unordered_set>

namespace ldbg {

namespace {

static_assert(LDBG_UNITIG_NONE == LDBG_LIST_NONE, "listrank.h ranks the lists of k_ug_links as they are");

struct UgCtx {
    GraphView g;        // java_tiny off: unitigs answer from the table itself, as ToGfa1's HashMap of records does
    uint64_t smask;     // colours of S
    int use_nbr;        // the load-time neighbour index can resolve edges (else: binary search of the neighbour k-mer)
};

LDBG_HOSTDEV bool ug_vertex(const UgCtx& x, int64_t rec) {
    for (int c = 0; c < x.g.C; c++)
        if (((x.smask >> c) & 1ull) && graph_cov(x.g, rec, c) != 0u) return true;
    return false;
}
LDBG_HOSTDEV uint32_t ug_edges(const UgCtx& x, int64_t rec) {
    uint32_t e = 0;
    for (int c = 0; c < x.g.C; c++)
        if ((x.smask >> c) & 1ull) e |= graph_edges(x.g, rec, c);
    return e;
}
LDBG_HOSTDEV bool ug_palindrome(const GraphView& g, int64_t rec) { return (graph_row(g, rec)[g.flags_off] & LDBG_ROW_PALINDROME) != 0; }
LDBG_HOSTDEV uint32_t rev4(uint32_t m) { return ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3); }
// bit b = base b appended (out) / prepended (in) to the oriented k-mer, from the record's edge byte (CortexRecord.java:214-275;
// the flipped k-mer's out-edges are the complemented in-edges, TraversalUtils.getOutEdges / getInEdges :560-590)
LDBG_HOSTDEV uint32_t ug_out(uint32_t e, bool flip) { return flip ? (e >> 4) : (e & 0xFu); }
LDBG_HOSTDEV uint32_t ug_in(uint32_t e, bool flip) { return rev4(flip ? (e & 0xFu) : (e >> 4)); }
LDBG_HOSTDEV unsigned ug_low(uint32_t m) { return m & 1u ? 0u : (m & 2u ? 1u : (m & 4u ? 2u : 3u)); }
LDBG_HOSTDEV int ug_popc(uint32_t m) { return (int)(m & 1u) + (int)((m >> 1) & 1u) + (int)((m >> 2) & 1u) + (int)((m >> 3) & 1u); }
LDBG_HOSTDEV char ug_ascii(unsigned b) { return b == 0 ? 'A' : (b == 1 ? 'C' : (b == 2 ? 'G' : 'T')); }

template <int W>
LDBG_HOSTDEV Kmer<W> ug_str(const GraphView& g, uint32_t a) {
    const Kmer<W> c = graph_key<W>(g, a >> 1);
    return (a & 1u) ? kmer_revcomp<W>(c, g.k) : c;
}
// oriented vertex of a k-mer string: record | (string != canonical k-mer), or NONE
template <int W>
LDBG_HOSTDEV uint32_t ug_find(const GraphView& g, const Kmer<W>& s) {
    bool f;
    const Kmer<W> c = kmer_canonical<W>(s, g.k, &f);
    const int64_t r = graph_find_canonical<W>(g, c);
    return r < 0 ? LDBG_UNITIG_NONE : ((uint32_t)r << 1) | (f ? 1u : 0u);
}
// the neighbour of oriented vertex a through base b (appended if fwd, else prepended), or NONE if that k-mer has no record
template <int W>
LDBG_HOSTDEV uint32_t ug_step(const UgCtx& x, uint32_t a, bool fwd, unsigned b) {
    if (x.use_nbr) {
        const bool f = (a & 1u) != 0;
        // the flipped k-mer's successor through b is the reverse complement of the record's predecessor through 3 - b (and back)
        const int j = !f ? (fwd ? (int)b : 4 + (int)b) : (fwd ? 4 + (int)(3u - b) : (int)(3u - b));
        const uint32_t ent = graph_nbr(x.g, a >> 1, j);
        if (!ent) return LDBG_UNITIG_NONE;
        const uint32_t r = (ent & 0x7FFFFFFFu) - 1u;
        const bool nf = ((ent >> 31) != 0) != f;
        return (r << 1) | (nf ? 1u : 0u);
    }
    const Kmer<W> s = ug_str<W>(x.g, a);
    return ug_find<W>(x.g, fwd ? kmer_next<W>(s, x.g.k, b) : kmer_prev<W>(s, x.g.k, b));
}

// succ[a] = b iff a -> b is a unitig edge (out(a) = {b}, in(b) = {a}, both vertices, distinct records, no palindrome); pred likewise
template <int W>
LDBG_KERNEL void k_ug_links(UgCtx x, int64_t n2, uint32_t* succ, uint32_t* pred) {
    const int k = x.g.k;
    for (int64_t i = global_tid(); i < n2; i += global_nthreads()) {
        const uint32_t a = (uint32_t)i, rec = a >> 1;
        const bool f = (a & 1u) != 0;
        uint32_t s = LDBG_UNITIG_NONE, p = LDBG_UNITIG_NONE;
        if (ug_vertex(x, rec) && !ug_palindrome(x.g, rec)) {
            const uint32_t e = ug_edges(x, rec);
            const Kmer<W> key = graph_key<W>(x.g, rec);
            const unsigned first = f ? 3u - kmer_base<W>(key, k, k - 1) : kmer_base<W>(key, k, 0);
            const unsigned last = f ? 3u - kmer_base<W>(key, k, 0) : kmer_base<W>(key, k, k - 1);
            const uint32_t om = ug_out(e, f), im = ug_in(e, f);
            if (ug_popc(om) == 1) {
                const uint32_t y = ug_step<W>(x, a, true, ug_low(om));
                if (y != LDBG_UNITIG_NONE && (y >> 1) != rec && ug_vertex(x, y >> 1) && !ug_palindrome(x.g, y >> 1)) {
                    const uint32_t yin = ug_in(ug_edges(x, y >> 1), (y & 1u) != 0);
                    if (ug_popc(yin) == 1 && ug_low(yin) == first) s = y;        // y's only predecessor is a
                }
            }
            if (ug_popc(im) == 1) {
                const uint32_t y = ug_step<W>(x, a, false, ug_low(im));
                if (y != LDBG_UNITIG_NONE && (y >> 1) != rec && ug_vertex(x, y >> 1) && !ug_palindrome(x.g, y >> 1)) {
                    const uint32_t yout = ug_out(ug_edges(x, y >> 1), (y & 1u) != 0);
                    if (ug_popc(yout) == 1 && ug_low(yout) == last) p = y;       // y's only successor is a
                }
            }
        }
        succ[i] = s; pred[i] = p;
    }
}
// members of pure cycles (their ancestor still has a predecessor): pd[a] = pointer | minimum oriented id seen << 32
LDBG_KERNEL void k_ug_cycle_init(int64_t n2, const uint32_t* pred, unsigned long long* pd, unsigned long long* n_cyc) {
    unsigned long long n = 0;
    for (int64_t i = global_tid(); i < n2; i += global_nthreads()) {
        if (pred[(uint32_t)pd[i]] == LDBG_UNITIG_NONE) continue;
        pd[i] = (unsigned long long)pred[i] | ((unsigned long long)i << 32);
        n++;
    }
    if (n) atomic_add_u64(n_cyc, n);
}
// one round of pointer jumping that carries the minimum over the window behind each cycle member
LDBG_KERNEL void k_ug_cycle_jump(int64_t n2, const uint32_t* pred, unsigned long long* pd) {
    for (int64_t i = global_tid(); i < n2; i += global_nthreads()) {
        const unsigned long long me = LDBG_GLOBAL(unsigned long long, pd)[i];
        const uint32_t p = (uint32_t)me;
        if (pred[p] == LDBG_UNITIG_NONE) continue;         // not a cycle member (p is its settled head)
        const unsigned long long up = LDBG_GLOBAL(unsigned long long, pd)[p];
        const unsigned long long m = std::min(me >> 32, up >> 32);
        LDBG_GLOBAL(unsigned long long, pd)[i] = (unsigned long long)(uint32_t)up | (m << 32);
    }
}
// pd[a] = minimum of its cycle | bit 63 for cycle members
LDBG_KERNEL void k_ug_cycle_mark(int64_t n2, const uint32_t* pred, unsigned long long* pd) {
    for (int64_t i = global_tid(); i < n2; i += global_nthreads())
        if (pred[(uint32_t)pd[i]] != LDBG_UNITIG_NONE) pd[i] = (pd[i] >> 32) | (1ull << 63);
}
// Cut every cycle at its minimum m.  The copy whose minimum is even holds the smallest canonical k-mer in forward orientation: it
// starts there (the edge into m goes).  Its mirror has minimum m ^ 1 and loses the mirror image of that edge, m ^ 1 -> its
// successor, so the two copies stay mirror images of one another.  Ranking restarts from the new predecessors.
LDBG_KERNEL void k_ug_cycle_break(int64_t n2, uint32_t* succ, uint32_t* pred, unsigned long long* pd) {
    for (int64_t i = global_tid(); i < n2; i += global_nthreads()) {
        const unsigned long long me = pd[i];
        if (!(me >> 63)) continue;
        const uint32_t m = (uint32_t)me, a = (uint32_t)i;
        uint32_t s = succ[i], p = pred[i];
        if (!(m & 1u)) { if (a == m) p = LDBG_UNITIG_NONE; if (s == m) s = LDBG_UNITIG_NONE; }
        else { if (a == m) s = LDBG_UNITIG_NONE; if (p == m) p = LDBG_UNITIG_NONE; }
        succ[i] = s; pred[i] = p;
        pd[i] = p == LDBG_UNITIG_NONE ? (unsigned long long)i : ((unsigned long long)p | (1ull << 32));
    }
}
// tails report to their head: tail[h] = t (tail overwrites pred, which no later kernel needs)
LDBG_KERNEL void k_ug_tails(int64_t n2, const uint32_t* succ, const unsigned long long* pd, uint32_t* tail) {
    for (int64_t i = global_tid(); i < n2; i += global_nthreads())
        if (succ[i] == LDBG_UNITIG_NONE) tail[(uint32_t)pd[i]] = (uint32_t)i;
}
// Of a path h .. t and its mirror t^1 .. h^1 the one whose first k-mer is smaller is reported (alphanumericallyLowestOrientation,
// SequenceUtils.java:206-234: the sequences differ within the first k bases, since no path is its own mirror).  A palindrome alone
// ties with itself: its forward orientation.  hv[record] = bases of the unitig it heads | flip << 31 (0: heads none); the head's
// pd entry gets bit 63.
template <int W>
LDBG_KERNEL void k_ug_heads(UgCtx x, int64_t N, unsigned long long* pd, const uint32_t* tail, uint32_t* hv) {
    for (int64_t r = global_tid(); r < N; r += global_nthreads()) {
        uint32_t v = 0;
        if (ug_vertex(x, r)) {
            for (uint32_t f = 0; f < 2; f++) {
                const uint32_t a = ((uint32_t)r << 1) | f;
                if ((uint32_t)pd[a] != a) continue;
                const uint32_t t = tail[a];
                if ((int64_t)t >= 2 * N) continue;                 // (every head has its tail after the ranking)
                const int c = kmer_cmp<W>(ug_str<W>(x.g, a), ug_str<W>(x.g, t ^ 1u));
                if (!(c < 0 || (c == 0 && f == 0))) continue;
                const uint32_t L = (uint32_t)(pd[t] >> 32) + 1u;
                v = ((uint32_t)x.g.k + L - 1u) | (f << 31);
                pd[a] |= 1ull << 63;
            }
        }
        hv[r] = v;
    }
}
#define UG_SCAN_OWNERS 16384
// per chunk of records: unitigs headed there, their bases, the longest (stats[2] holds ~longest)
LDBG_KERNEL void k_ug_scan_sums(int64_t N, int64_t chunk, const uint32_t* hv, unsigned long long* sums, unsigned long long* stats) {
    for (int64_t t = global_tid(); t < UG_SCAN_OWNERS; t += global_nthreads()) {
        const int64_t lo = std::min<int64_t>(t * chunk, N), hi = std::min<int64_t>(lo + chunk, N);
        unsigned long long c = 0, b = 0, mx = 0;
        for (int64_t i = lo; i < hi; i++) {
            const uint32_t v = hv[i];
            if (!v) continue;
            const unsigned long long bases = v & 0x7FFFFFFFu;
            c++; b += bases; mx = std::max(mx, bases);
        }
        sums[t] = c; sums[UG_SCAN_OWNERS + t] = b;
        if (mx) atomic_min_u64(stats + 2, ~mx);
    }
}
LDBG_KERNEL void k_ug_scan_top(unsigned long long* sums, unsigned long long* stats) {
    if (global_tid() != 0) return;
    unsigned long long rc = 0, rb = 0;
    for (int t = 0; t < UG_SCAN_OWNERS; t++) {
        const unsigned long long c = sums[t], b = sums[UG_SCAN_OWNERS + t];
        sums[t] = rc; sums[UG_SCAN_OWNERS + t] = rb;
        rc += c; rb += b;
    }
    stats[0] = rc; stats[1] = rb;
}
// unitig ids in record order of the heads: off / hd / tl per unitig, hv[head record] = its id
LDBG_KERNEL void k_ug_scan_apply(int64_t N, int64_t chunk, uint32_t* hv, const uint32_t* tail, const unsigned long long* sums,
                                 unsigned long long* off, uint32_t* hd, uint32_t* tl) {
    for (int64_t t = global_tid(); t < UG_SCAN_OWNERS; t += global_nthreads()) {
        const int64_t lo = std::min<int64_t>(t * chunk, N), hi = std::min<int64_t>(lo + chunk, N);
        unsigned long long rc = sums[t], rb = sums[UG_SCAN_OWNERS + t];
        for (int64_t i = lo; i < hi; i++) {
            const uint32_t v = hv[i];
            if (!v) continue;
            const uint32_t a = ((uint32_t)i << 1) | (v >> 31);
            off[rc] = rb; hd[rc] = a; tl[rc] = tail[a];
            hv[i] = (uint32_t)rc;
            rc++; rb += v & 0x7FFFFFFFu;
        }
    }
}
// every member of a reported path: its label, its bases (the head all k, every other member its last base), its coverage
template <int W>
LDBG_KERNEL void k_ug_assign(UgCtx x, int64_t n2, const unsigned long long* pd, const uint32_t* hv, const unsigned long long* off,
                             unsigned long long* lab, uint32_t* cov, uint8_t* seq) {
    const int k = x.g.k, C = x.g.C;
    for (int64_t i = global_tid(); i < n2; i += global_nthreads()) {
        const unsigned long long me = pd[i];
        const uint32_t h = (uint32_t)me;
        if (!(pd[h] >> 63)) continue;                      // the mirror path, or no path of a vertex
        const uint32_t a = (uint32_t)i, rec = a >> 1, d = (uint32_t)(me >> 32) & 0x7FFFFFFFu;
        const uint32_t uid = hv[h >> 1];
        lab[rec] = (unsigned long long)uid | ((unsigned long long)d << 32) | ((unsigned long long)(a & 1u) << 63);
        const Kmer<W> s = ug_str<W>(x.g, a);
        const unsigned long long o = off[uid];
        if (d == 0) {
            for (int j = 0; j < k; j++) seq[o + j] = (uint8_t)ug_ascii(kmer_base<W>(s, k, j));
        } else {
            seq[o + (unsigned long long)(k - 1) + d] = (uint8_t)ug_ascii(kmer_base<W>(s, k, k - 1));
        }
        for (int c = 0; c < C; c++) {
            const uint32_t v = graph_cov(x.g, rec, c);
            if (v) atomic_add_u32(cov + (size_t)uid * C + c, v);
        }
    }
}
// GFA link candidates of unitigs [u0, u0 + n): for each of the two vertices (0: as reported, 1: reverse complement), the
// predecessors of its first k-mer (slots 0..3, by base) and the successors of its last k-mer (slots 4..7) in the sample colour
// (ToGfa1.java:95-125), resolved through findRecord to the vertex whose last (resp. first) k-mer they are: 2 * unitig + strand,
// or NONE.  hsh: Arrays.hashCode of the candidate k-mer (its HashSet<CortexByteKmer> bucket).
template <int W>
LDBG_KERNEL void k_ug_gfa(GraphView g, int sc, int64_t u0, int64_t n, const unsigned long long* lab, const unsigned long long* off,
                          const uint32_t* hd, const uint32_t* tl, uint32_t* tgt, uint32_t* hsh) {
    const int k = g.k;
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) {
        const int64_t u = u0 + i;
        const uint32_t H = hd[u], T = tl[u];
        for (int v = 0; v < 2; v++) {
            for (int side = 0; side < 2; side++) {         // 0: ins of the first k-mer, 1: outs of the last
                const uint32_t a = side == 0 ? (v ? T ^ 1u : H) : (v ? H ^ 1u : T);
                const uint32_t e = graph_edges(g, a >> 1, sc);
                const uint32_t m = side == 0 ? ug_in(e, (a & 1u) != 0) : ug_out(e, (a & 1u) != 0);
                const Kmer<W> s = ug_str<W>(g, a);
                for (unsigned b = 0; b < 4; b++) {
                    uint32_t t = LDBG_UNITIG_NONE, hh = 0;
                    if ((m >> b) & 1u) {
                        const Kmer<W> cand = side == 0 ? kmer_prev<W>(s, k, b) : kmer_next<W>(s, k, b);
                        hh = kmer_java_hash<W>(cand, k);
                        const uint32_t y = ug_find<W>(g, cand);
                        if (y != LDBG_UNITIG_NONE) {
                            const unsigned long long l = lab[y >> 1];
                            const uint32_t w = (uint32_t)l;
                            if (w != LDBG_UNITIG_NONE) {
                                const uint32_t pos = (uint32_t)(l >> 32) & 0x7FFFFFFFu;
                                const bool fy = (y & 1u) != 0, o = (l >> 63) != 0;
                                const uint32_t len = (uint32_t)(off[w + 1] - off[w]) - (uint32_t)k + 1u;
                                // ins look for a last k-mer: the reported strand's last, or the reverse strand's (= rc of the first)
                                // outs look for a first k-mer: the reported strand's first, or the reverse strand's (= rc of the last)
                                const uint32_t want_fwd = side == 0 ? len - 1u : 0u, want_rev = side == 0 ? 0u : len - 1u;
                                if (fy == o && pos == want_fwd) t = w << 1;
                                else if (fy != o && pos == want_rev) t = (w << 1) | 1u;
                            }
                        }
                    }
                    const int64_t slot = i * 16 + v * 8 + side * 4 + (int)b;
                    tgt[slot] = t; hsh[slot] = hh;
                }
            }
        }
    }
}
LDBG_KERNEL void k_ug_gather(int64_t n, const int64_t* recs, const unsigned long long* lab, unsigned long long* out) {
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) out[i] = lab[recs[i]];
}

// Java's (int) of a float (JLS 5.1.3)
int32_t java_f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)f;
}

struct FileOut {
    FILE* f;
    explicit FileOut(const std::string& p) : f(fopen(p.c_str(), "wb")) {
        if (!f) throw StatusError(LDBG_ERR_CORTEXJDK, "cannot write " + p);
    }
    ~FileOut() { if (f) fclose(f); }
    void put(const std::string& s) { if (!s.empty() && fwrite(s.data(), 1, s.size(), f) != s.size()) throw StatusError(LDBG_ERR_CORTEXJDK, "write failed"); }
    void close() { const int rc = fclose(f); f = nullptr; if (rc != 0) throw StatusError(LDBG_ERR_CORTEXJDK, "write failed"); }
};

const int64_t kHostChunk = 1 << 22;     // unitigs per host round trip of the writers

}  // namespace

Unitigs::Unitigs(const Graph& g, const int* colors, int n_colors) : graph(g) {
    check_whole_table(g, "unitigs");
    if (n_colors < 1) throw StatusError(LDBG_ERR_ARG, "unitigs: no colour given");
    for (int i = 0; i < n_colors; i++) {
        if (colors[i] < 0 || colors[i] >= g.hdr.C || colors[i] >= 64) throw StatusError(LDBG_ERR_ARG, "unitigs: colour out of range");
        color_mask |= 1ull << colors[i];
    }
    const int64_t N = g.view.N, n2 = 2 * N;
    // 32-bit oriented ids, 31-bit positions and unitig lengths (k + L - 1 bases with L <= N)
    if (N > (int64_t)0x7FFFFF00) throw StatusError(LDBG_ERR_UNSUPPORTED, "unitigs: more than 2^31 - 256 records on one device");
    const int W = g.view.W;
    UgCtx x{g.view, color_mask, 0};
    x.g.java_tiny = 0;
    x.use_nbr = g.view.nbr_on && N > 2 ? 1 : 0;     // (a table of two records or fewer was indexed with findRecord's quirk Q1)
    rt::set_device(g.device);
    rt::stream_t s = g.stream;
    rt::Event e0, e1;
    e0.record(s);
    DevBlocks tmp;
    d_lab_ = own_.get<uint64_t>((size_t)std::max<int64_t>(N, 1));
    rt::dmemset(d_lab_, 0xFF, (size_t)N * 8, s);
    unsigned long long* stats = tmp.get<unsigned long long>(8);
    rt::dmemset(stats, 0, 64, s);
    rt::dmemset(stats + 2, 0xFF, 8, s);
    if (N > 0) {
        // temporaries: 32 bytes per record
        uint32_t* succ = tmp.get<uint32_t>((size_t)n2);
        uint32_t* pred = tmp.get<uint32_t>((size_t)n2);
        unsigned long long* pd = tmp.get<unsigned long long>((size_t)n2);
        unsigned long long* sums = tmp.get<unsigned long long>((size_t)UG_SCAN_OWNERS * 2);
        const int grid = grid_for(n2);
        LDBG_LAUNCH_W(W, k_ug_links, grid, 256, s, x, n2, succ, pred);
        unsigned* d_changed = (unsigned*)(stats + 4);
        rank_lists(pd, pred, n2, d_changed, rank_rounds(n2) + 1, s);
        LDBG_LAUNCH(k_ug_cycle_init, grid, 256, s, n2, (const uint32_t*)pred, pd, stats + 3);
        unsigned long long n_cyc = 0;
        rt::d2h(&n_cyc, stats + 3, 8, s);
        rt::stream_sync(s);
        if (n_cyc) {
            int rounds = 1;
            while ((1ull << rounds) < n_cyc) rounds++;
            for (int r = 0; r < rounds; r++) LDBG_LAUNCH(k_ug_cycle_jump, grid, 256, s, n2, (const uint32_t*)pred, pd);
            LDBG_LAUNCH(k_ug_cycle_mark, grid, 256, s, n2, (const uint32_t*)pred, pd);
            LDBG_LAUNCH(k_ug_cycle_break, grid, 256, s, n2, succ, pred, pd);
            rank_lists(pd, nullptr, n2, d_changed, rank_rounds(n2) + 1, s);       // (k_ug_cycle_break has set pd of the cut cycles)
        }
        uint32_t* tail = pred;
        uint32_t* hv = succ;
        LDBG_LAUNCH(k_ug_tails, grid, 256, s, n2, (const uint32_t*)succ, (const unsigned long long*)pd, tail);
        LDBG_LAUNCH_W(W, k_ug_heads, grid_for(N), 256, s, x, N, pd, (const uint32_t*)tail, hv);
        const int64_t chunk = (N + UG_SCAN_OWNERS - 1) / UG_SCAN_OWNERS;
        LDBG_LAUNCH(k_ug_scan_sums, UG_SCAN_OWNERS / 256, 256, s, N, chunk, (const uint32_t*)hv, sums, stats);
        LDBG_LAUNCH(k_ug_scan_top, 1, 64, s, sums, stats);
        unsigned long long st[3] = {0, 0, 0};
        rt::d2h(st, stats, 24, s);
        rt::stream_sync(s);
        count = (int64_t)st[0]; total_bases = (int64_t)st[1]; longest = st[2] == ~0ull ? 0 : (int64_t)~st[2];
        d_off_ = own_.get<uint64_t>((size_t)(count + 1));
        d_hd_ = own_.get<uint32_t>((size_t)std::max<int64_t>(count, 1));
        d_tl_ = own_.get<uint32_t>((size_t)std::max<int64_t>(count, 1));
        d_cov_ = own_.get<uint32_t>((size_t)std::max<int64_t>(count, 1) * g.view.C);
        d_seq_ = own_.get<uint8_t>((size_t)std::max<int64_t>(total_bases, 1));
        rt::dmemset(d_cov_, 0, (size_t)count * g.view.C * 4, s);
        const uint64_t end = (uint64_t)total_bases;
        rt::h2d(d_off_ + count, &end, 8, s);
        LDBG_LAUNCH(k_ug_scan_apply, UG_SCAN_OWNERS / 256, 256, s, N, chunk, hv, (const uint32_t*)tail, (const unsigned long long*)sums,
                    (unsigned long long*)d_off_, d_hd_, d_tl_);
        LDBG_LAUNCH_W(W, k_ug_assign, grid, 256, s, x, n2, (const unsigned long long*)pd, (const uint32_t*)hv, (const unsigned long long*)d_off_,
                      (unsigned long long*)d_lab_, d_cov_, d_seq_);
        rt::stream_sync(s);
        members = total_bases - count * (int64_t)(g.view.k - 1);
    } else {
        d_off_ = own_.get<uint64_t>(1);
        rt::dmemset(d_off_, 0, 8, s);
    }
    e1.record(s);
    rt::stream_sync(s);
    build_ms = rt::Event::elapsed_ms(e0, e1);
    profile_add("unitigs", build_ms);
}

void Unitigs::get(int64_t first, int64_t n, int64_t* offsets, char* bases, int64_t capacity, bool device_out, rt::stream_t s) const {
    if (first < 0 || n < 0 || first + n > count) throw StatusError(LDBG_ERR_ARG, "unitig range outside 0.." + std::to_string(count));
    rt::set_device(graph.device);
    std::vector<uint64_t> off((size_t)n + 1);
    rt::d2h(off.data(), d_off_ + first, (size_t)(n + 1) * 8, s);
    rt::stream_sync(s);
    const int64_t need = (int64_t)(off[n] - off[0]);
    std::vector<int64_t> rel((size_t)n + 1);
    for (int64_t i = 0; i <= n; i++) rel[i] = (int64_t)(off[i] - off[0]);
    if (device_out) rt::h2d(offsets, rel.data(), (size_t)(n + 1) * 8, s);
    else memcpy(offsets, rel.data(), (size_t)(n + 1) * 8);
    if (!bases) { rt::stream_sync(s); return; }                  // sizes only
    if (need > capacity) {
        if (device_out) rt::stream_sync(s);
        throw StatusError(LDBG_ERR_CAPACITY, "unitig buffer too small: need " + std::to_string(need));
    }
    if (need) {
        if (device_out) rt::d2d(bases, d_seq_ + off[0], (size_t)need, s);
        else rt::d2h(bases, d_seq_ + off[0], (size_t)need, s);
    }
    rt::stream_sync(s);
}

void Unitigs::coverage(int64_t first, int64_t n, uint32_t* cov) const {
    if (first < 0 || n < 0 || first + n > count) throw StatusError(LDBG_ERR_ARG, "unitig range outside 0.." + std::to_string(count));
    rt::set_device(graph.device);
    const int C = graph.view.C;
    rt::d2h(cov, d_cov_ + (size_t)first * C, (size_t)n * C * 4, graph.stream);
    rt::stream_sync(graph.stream);
}

void Unitigs::of_records(const int64_t* recs, int64_t n, int64_t* uid, int64_t* pos, int8_t* orient) const {
    if (n <= 0) return;
    for (int64_t i = 0; i < n; i++)
        if (recs[i] < 0 || recs[i] >= graph.view.N) throw StatusError(LDBG_ERR_ARG, "record index out of range");
    rt::set_device(graph.device);
    rt::stream_t s = graph.stream;
    DevBlocks tmp;
    int64_t* dr = tmp.get<int64_t>((size_t)n);
    unsigned long long* dl = tmp.get<unsigned long long>((size_t)n);
    std::vector<uint64_t> l((size_t)n);
    rt::h2d(dr, recs, (size_t)n * 8, s);
    LDBG_LAUNCH(k_ug_gather, grid_for(n), 256, s, n, (const int64_t*)dr, (const unsigned long long*)d_lab_, dl);
    rt::d2h(l.data(), dl, (size_t)n * 8, s);
    rt::stream_sync(s);
    for (int64_t i = 0; i < n; i++) {
        const bool none = (uint32_t)l[i] == LDBG_UNITIG_NONE;
        if (uid) uid[i] = none ? -1 : (int64_t)(uint32_t)l[i];
        if (pos) pos[i] = none ? -1 : (int64_t)((l[i] >> 32) & 0x7FFFFFFFu);
        if (orient) orient[i] = none ? (int8_t)-1 : (int8_t)(l[i] >> 63);
    }
}

void Unitigs::write_fasta(const std::string& path) const {
    FileOut out(path);
    std::string buf;
    std::vector<int64_t> rel;
    std::vector<char> bases;
    for (int64_t u0 = 0; u0 < count; u0 += kHostChunk) {
        const int64_t n = std::min<int64_t>(kHostChunk, count - u0);
        rel.resize((size_t)n + 1);
        get(u0, n, rel.data(), nullptr, 0, false, graph.stream);
        bases.resize((size_t)std::max<int64_t>(rel[n], 1));
        get(u0, n, rel.data(), bases.data(), rel[n], false, graph.stream);
        buf.clear();
        for (int64_t i = 0; i < n; i++) {
            buf += '>'; buf += std::to_string(u0 + i); buf += '\n';
            buf.append(bases.data() + rel[i], (size_t)(rel[i + 1] - rel[i]));
            buf += '\n';
        }
        out.put(buf);
    }
    out.close();
}

// ToGfa1.execute (J/commands/utils/ToGfa1.java:37-145) over these unitigs as its FASTA (ids = FASTA order).
//   S lines: one per unitig, AC = (int)((float)cov / (float)nkmers) over the sample colour's Java-int coverage sum, RC = AC * length.
//   L lines: in the insertion order of the JGraphT edge set: vertices v, rc(v) per unitig; per vertex the predecessors of its first
//   k-mer, then the successors of its last, each in HashSet<CortexByteKmer> order (bucket (h ^ h >>> 16) & 15 of a 16-bucket table,
//   ties in insertion order, which is the order of the HashSet<Byte> of edge bases: A, C, T, G); an edge already present is dropped.
//   The positive strand is written ':' (ToGfa1's own string; '+' with LDBG_GFA_PLUS_STRAND).  A unitig that is one palindromic
//   k-mer is one vertex whose positiveStrand entry was overwritten by its reverse complement: '-'.
void Unitigs::write_gfa1(const std::string& path, int sc, int flags) const {
    if (sc < 0 || sc >= graph.view.C) throw StatusError(LDBG_ERR_ARG, "sample colour out of range");
    rt::set_device(graph.device);
    rt::stream_t s = graph.stream;
    const int k = graph.view.k, C = graph.view.C, W = graph.view.W;
    const char plus = (flags & LDBG_GFA_PLUS_STRAND) ? '+' : ':';
    FileOut out(path);
    out.put("H\tVN:Z:1.0\n");
    std::vector<uint8_t> pal((size_t)count, 0);       // one palindromic k-mer
    std::string buf;
    std::vector<int64_t> rel;
    std::vector<char> bases;
    std::vector<uint32_t> cov;
    for (int64_t u0 = 0; u0 < count; u0 += kHostChunk) {
        const int64_t n = std::min<int64_t>(kHostChunk, count - u0);
        rel.resize((size_t)n + 1);
        get(u0, n, rel.data(), nullptr, 0, false, s);
        bases.resize((size_t)std::max<int64_t>(rel[n], 1));
        get(u0, n, rel.data(), bases.data(), rel[n], false, s);
        cov.resize((size_t)n * C);
        coverage(u0, n, cov.data());
        buf.clear();
        for (int64_t i = 0; i < n; i++) {
            const char* sq = bases.data() + rel[i];
            const int64_t len = rel[i + 1] - rel[i], nk = len - k + 1;
            if (len == k) {
                bool p = true;
                for (int j = 0; j < k && p; j++) {
                    const char c = sq[k - 1 - j];
                    p = sq[j] == (c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A');
                }
                pal[(size_t)(u0 + i)] = p ? 1 : 0;
            }
            const int32_t cv = (int32_t)cov[(size_t)i * C + sc];
            const int32_t ac = java_f2i((float)cv / (float)nk);
            const int32_t rc = (int32_t)((uint32_t)ac * (uint32_t)len);
            buf += "S\t"; buf += std::to_string(u0 + i); buf += '\t';
            buf.append(sq, (size_t)len);
            buf += "\tRC:i:"; buf += std::to_string(rc); buf += "\tAC:i:"; buf += std::to_string(ac); buf += '\n';
        }
        out.put(buf);
    }
    const std::string tail_s = "\t" + std::to_string(k) + "M\n";
    auto vname = [&](uint32_t v, std::string& b) {
        b += std::to_string(v >> 1); b += '\t';
        b += (v & 1u) || pal[v >> 1] ? '-' : plus;
    };
    std::unordered_set<uint64_t> seen;
    const int64_t gchunk = std::min<int64_t>(kHostChunk, std::max<int64_t>(count, 1));
    DevBlocks tmp;
    uint32_t* d_tgt = tmp.get<uint32_t>((size_t)gchunk * 16);
    uint32_t* d_hsh = tmp.get<uint32_t>((size_t)gchunk * 16);
    std::vector<uint32_t> tgt((size_t)gchunk * 16), hsh((size_t)gchunk * 16);
    GraphView gv = graph.view;
    gv.java_tiny = 0;
    static const int byte_order[4] = {0, 1, 3, 2};     // HashSet<Byte> of 'A' 'C' 'G' 'T': buckets 1, 3, 7, 4
    for (int64_t u0 = 0; u0 < count; u0 += gchunk) {
        const int64_t n = std::min<int64_t>(gchunk, count - u0);
        LDBG_LAUNCH_W(W, k_ug_gfa, grid_for(n), 256, s, gv, sc, u0, n, (const unsigned long long*)d_lab_, (const unsigned long long*)d_off_,
                      (const uint32_t*)d_hd_, (const uint32_t*)d_tl_, d_tgt, d_hsh);
        rt::d2h(tgt.data(), d_tgt, (size_t)n * 64, s);
        rt::d2h(hsh.data(), d_hsh, (size_t)n * 64, s);
        rt::stream_sync(s);
        buf.clear();
        for (int64_t i = 0; i < n; i++) {
            const int64_t u = u0 + i;
            for (int v = 0; v < (pal[(size_t)u] ? 1 : 2); v++) {
                const uint32_t me = ((uint32_t)u << 1) | (uint32_t)v;
                for (int side = 0; side < 2; side++) {
                    const size_t base = (size_t)i * 16 + (size_t)v * 8 + (size_t)side * 4;
                    int ord[4], no = 0;
                    for (int j = 0; j < 4; j++) {
                        const int b = byte_order[j];
                        if (tgt[base + b] != LDBG_UNITIG_NONE) ord[no++] = b;      // (candidates without a vertex add no edge)
                    }
                    auto bucket = [&](int b) { const uint32_t h = hsh[base + b]; return (h ^ (h >> 16)) & 15u; };
                    std::stable_sort(ord, ord + no, [&](int p, int q) { return bucket(p) < bucket(q); });
                    for (int j = 0; j < no; j++) {
                        const uint32_t t = tgt[base + ord[j]];
                        if (t == LDBG_UNITIG_NONE) continue;
                        const uint32_t src = side == 0 ? t : me, dst = side == 0 ? me : t;
                        if (!seen.insert(((uint64_t)src << 32) | dst).second) continue;
                        buf += "L\t"; vname(src, buf); buf += '\t'; vname(dst, buf); buf += tail_s;
                    }
                }
            }
        }
        out.put(buf);
    }
    out.close();
}

}  // namespace ldbg
