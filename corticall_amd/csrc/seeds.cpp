// Variant seeds on the device (seeds.h).
//   occurrences: one lane per window of a threading -> one atomic add and one atomic minimum on its record.  A count and a minimum
//     do not depend on the order in which the lanes arrive.
//   pass A: one record per lane over the coverage and edge planes -> the filter's answer as a ballot word per 64 records (the layout
//     Selection::compact scans and compacts) and one byte per record: bits 0-3 the in-edge bases of its covered colours, bits 4-7
//     their out-edge bases, bit b = base b in A C G T order.
//   pass B: one lane per (record of S, orientation, declared predecessor base) -> the predecessor p is a start when nothing leads to
//     it and one edge leaves it; the lane then follows the chain for at most three steps and stores 1 into the record's good byte
//     (every writer stores the same value).  An edge X -> Y exists when X is a vertex of S that declares Y's last base as a successor or
//     Y is one that declares X's first base as a predecessor, so a vertex's in- and out-set cost at most four lookups each through the
//     table's radix index (by value: findRecord's quirk Q1 has no part in it).  Starts are counted with one atomic per wavefront.
//   The good bytes become ballot words and are compacted like S.
// Every kernel is launched one wavefront per workgroup and uses no wavefront primitive beyond ballot and popcount.  The TEST-ONLY host
// simulation runs the kernels as they are.
#include "seeds.h"

#include "wavescan.h"

namespace ldbg {

namespace {

// ---- occurrences
LDBG_KERNEL void k_occ_count(const int64_t* rec, int64_t M, uint32_t* count, unsigned long long* first) {
    for (int64_t m = global_tid(); m < M; m += global_nthreads()) {
        const int64_t r = rec[m];
        if (r < 0) continue;
        atomic_add_u32(count + r, 1u);
        atomic_min_u64(first + r, (unsigned long long)m);
    }
}

const Graph& threaded_graph(const Threading& t) {
    if (!t.graph) throw StatusError(LDBG_ERR_ARG, "occurrences: the threading was made without a graph");
    return *t.graph;
}

// ---- pass A
LDBG_HOSTDEV unsigned rev4(unsigned x) { return ((x & 1u) << 3) | ((x & 2u) << 1) | ((x & 4u) >> 1) | ((x & 8u) >> 3); }

struct SeedMaskCtx {
    const uint32_t* cov;       // [C][N]
    const uint8_t* edges;      // [C][N]
    int64_t N;
    int C;
    uint64_t all_zero;
    uint64_t cmask[LDBG_SEED_MAX_COVERED];
    int32_t lo[LDBG_SEED_MAX_COVERED], hi[LDBG_SEED_MAX_COVERED];
    int n_unique;
    int32_t ucol[LDBG_SEED_MAX_UNIQUE];
    const uint32_t* ucount[LDBG_SEED_MAX_UNIQUE];      // occurrences: unique = count == 1
    const uint8_t* ubytes[LDBG_SEED_MAX_UNIQUE];       // a caller's bytes: unique = non-zero
};

// ballots[g] bit b: record 64 g + b is in S; chunk_cnt[ch]: records of chunk ch in S; eb[r]: the declared bases of record r
LDBG_WAVE_KERNEL void k_seed_mask(SeedMaskCtx x, uint8_t* eb, unsigned long long* ballots, uint32_t* chunk_cnt) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t n = x.N, wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SELECT_CHUNK;
        const int lim = chunk_lim(n, c0, LDBG_SELECT_CHUNK);
        unsigned long long cur[1] = {0};
        uint32_t cnt = 0;
        for (int t = 0; t < lim; t += ws) {
            const int64_t i = c0 + t + lane;
            const bool in = i < n;
            bool ok = in;
            unsigned in_u = 0, out_u = 0;
            uint64_t covered = 0;
            for (int c = 0; c < x.C; c++) {
                const size_t at = (size_t)c * (size_t)n + (size_t)i;
                const int32_t v = in ? (int32_t)LDBG_GLOBAL(const uint32_t, x.cov)[at] : 0;      // CortexRecord.getCoverage: the Java int
                const unsigned e = in ? (unsigned)LDBG_GLOBAL(const uint8_t, x.edges)[at] : 0u;
                if (v > 0) {
                    covered |= 1ull << c;
                    if (__builtin_popcount(e >> 4) != 1 || __builtin_popcount(e & 15u) != 1) ok = false;      // isSinglyConnected
                    in_u |= rev4(e >> 4);      // getInEdgesAsBytes: bit 3 - b of the high nibble is base b
                    out_u |= e & 15u;          // getOutEdgesAsBytes: bit b of the low nibble is base b
                }
                if (((x.all_zero >> c) & 1ull) && v != 0) ok = false;
            }
#pragma unroll 1
            for (int j = 0; j < LDBG_SEED_MAX_COVERED; j++)
                if (x.cmask[j]) {
                    const int m = __builtin_popcountll(covered & x.cmask[j]);
                    if (m < x.lo[j] || m > x.hi[j]) ok = false;
                }
#pragma unroll 1
            for (int j = 0; j < x.n_unique; j++)
                if (ok && (x.ucol[j] < 0 || ((covered >> x.ucol[j]) & 1ull))) {
                    const bool one = x.ucount[j] ? LDBG_GLOBAL(const uint32_t, x.ucount[j])[i] == 1u : LDBG_GLOBAL(const uint8_t, x.ubytes[j])[i] != 0;
                    if (!one) ok = false;
                }
            if (in) eb[i] = (uint8_t)(in_u | (out_u << 4));
            cnt += ballot_step(c0, t, {ok}, cur, {ballots});
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();      // (host simulation: a lane that has left the kernel counts as inactive in a ballot the others have yet to read)
}

// the good bytes as ballot words and chunk counts
LDBG_WAVE_KERNEL void k_seed_good(const uint8_t* good, int64_t n, unsigned long long* ballots, uint32_t* chunk_cnt) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SELECT_CHUNK;
        const int lim = chunk_lim(n, c0, LDBG_SELECT_CHUNK);
        unsigned long long cur[1] = {0};
        uint32_t cnt = 0;
        for (int t = 0; t < lim; t += ws) {
            const int64_t i = c0 + t + lane;
            const bool ok = i < n && good[i] != 0;
            cnt += ballot_step(c0, t, {ok}, cur, {ballots});
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();
}

// ---- pass B
struct SeedWalkCtx {
    GraphView g;
    const unsigned long long* in_s;       // the ballot words of pass A
    const uint8_t* eb;
};

// A vertex of the string graph: rec >= 0 when its canonical k-mer is a record of S; din / dout: the first bases of the predecessors and
// the last bases of the successors that record declares for this orientation (an even-k palindrome is one vertex with both sets)
struct SeedVertex { int64_t rec; unsigned din, dout; };

LDBG_DEV SeedVertex seed_declared(unsigned e, int flip, bool pal) {
    const unsigned in_u = e & 15u, out_u = e >> 4;
    SeedVertex o;
    o.rec = 0;
    o.din = pal ? (in_u | rev4(out_u)) : flip ? rev4(out_u) : in_u;
    o.dout = pal ? (out_u | rev4(in_u)) : flip ? rev4(in_u) : out_u;
    return o;
}

// kmer_cmp as a chain of selects: the lanes of a wavefront compare different k-mers, and a branch per word is a saved mask per word
template <int W>
LDBG_DEV int seed_cmp(const Kmer<W>& a, const Kmer<W>& b) {
    int r = 0;
#pragma unroll
    for (int i = W - 1; i >= 0; i--) r = a.w[i] < b.w[i] ? -1 : a.w[i] > b.w[i] ? 1 : r;
    return r;
}

// graph_find_canonical (graph.h) with that comparison, and by value: no look at java_tiny (SURVEY Q1 does not apply)
template <int W>
LDBG_DEV int64_t seed_find(const GraphView& g, const Kmer<W>& q) {
    const uint32_t px = kmer_prefix<W>(q, g.k, g.p);
    uint32_t lo = g.pstart[px], hi = g.pstart[px + 1];
    int64_t at = -1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const int c = seed_cmp<W>(graph_key<W>(g, (int64_t)mid), q);
        if (c == 0) at = (int64_t)mid;
        lo = c < 0 ? mid + 1 : lo;
        hi = c < 0 ? hi : mid;          // (a hit ends the search: hi = mid, and the records are distinct)
        if (c == 0) lo = hi;
    }
    return at;
}

template <int W>
LDBG_DEV SeedVertex seed_vertex(const SeedWalkCtx& x, const Kmer<W>& v) {
    const Kmer<W> rc = kmer_revcomp<W>(v, x.g.k);
    const int cmp = seed_cmp<W>(rc, v);
    const int64_t r = seed_find<W>(x.g, cmp < 0 ? rc : v);
    SeedVertex o{-1, 0u, 0u};
    if (r >= 0 && ((x.in_s[r >> 6] >> (r & 63)) & 1ull)) {
        o = seed_declared(x.eb[r], cmp < 0, cmp == 0);
        o.rec = r;
    }
    return o;
}

// The first base of a k-mer sits in word 0 (W = ceil(k / 32)): no choice of a word at run time, as kmer_base and kmer_prev make it
template <int W>
LDBG_DEV unsigned seed_first_base(const Kmer<W>& v, int k) { return (unsigned)((v.w[0] >> ((2 * (k - 1)) & 63)) & 3ull); }
template <int W>
LDBG_DEV Kmer<W> seed_prev(const Kmer<W>& a, int k, unsigned b) {
    Kmer<W> r;
#pragma unroll
    for (int i = W - 1; i > 0; i--) r.w[i] = (a.w[i] >> 2) | (a.w[i - 1] << 62);
    r.w[0] = (a.w[0] >> 2) | ((uint64_t)b << ((2 * (k - 1)) & 63));
    return r;
}

// does any edge lead to v, given the predecessors v declares itself
template <int W>
LDBG_DEV bool seed_has_in(const SeedWalkCtx& x, const Kmer<W>& v, unsigned own) {
    bool any = own != 0;
    const unsigned last = (unsigned)(v.w[W - 1] & 3ull);
#pragma unroll 1
    for (unsigned c = 0; c < 4 && !any; c++) {
        const SeedVertex p = seed_vertex<W>(x, seed_prev<W>(v, x.g.k, c));
        any = p.rec >= 0 && ((p.dout >> last) & 1u);
    }
    return any;
}

// the last bases of v's successors, given those v declares itself
template <int W>
LDBG_DEV unsigned seed_out(const SeedWalkCtx& x, const Kmer<W>& v, unsigned own) {
    unsigned m = own;
    const unsigned first = seed_first_base<W>(v, x.g.k);
#pragma unroll 1
    for (unsigned c = 0; c < 4; c++) {
        if ((m >> c) & 1u) continue;
        const SeedVertex s = seed_vertex<W>(x, kmer_next<W>(v, x.g.k, c));
        if (s.rec >= 0 && ((s.din >> first) & 1u)) m |= 1u << c;
    }
    return m;
}

// Record r of S in orientation o (0: as stored) and its declared predecessor base c.  Returns whether that predecessor is a start; a
// start has one successor, this vertex, so no other lane answers for it.
template <int W>
LDBG_DEV bool seed_lane(const SeedWalkCtx& x, int64_t r, int o, unsigned c, uint8_t* good) {
    const int k = x.g.k;
    const Kmer<W> f = graph_key<W>(x.g, r), rc = kmer_revcomp<W>(f, k);
    const bool pal = kmer_eq<W>(f, rc);
    if (pal && o) return false;
    const SeedVertex me = seed_declared(x.eb[r], o, pal);
    if (!((me.din >> c) & 1u)) return false;
    const Kmer<W> p = seed_prev<W>(o ? rc : f, k, c);
    const SeedVertex pv = seed_vertex<W>(x, p);
    if (seed_has_in<W>(x, p, pv.din)) return false;
    // the chain from p: follow the single successor while the out-degree is 1, stop at a vertex already on the chain; with more
    // than 3 vertices its second vertex, this record, is a good seed.  c1 and c2 hold p until the chain has a second and a third vertex.
    Kmer<W> cur = p, c1 = p, c2 = p;
    unsigned own = pv.dout;
    bool start = false;
#pragma unroll 1
    for (int step = 0; step < 3; step++) {
        const unsigned m = seed_out<W>(x, cur, own);
        if (__builtin_popcount(m) != 1) break;
        start = true;
        const Kmer<W> nx = kmer_next<W>(cur, k, (unsigned)__builtin_ctz(m));
        if (kmer_eq<W>(nx, p) || kmer_eq<W>(nx, c1) || kmer_eq<W>(nx, c2)) break;
        if (step == 2) { good[r] = 1; break; }
        if (step == 0) c1 = nx; else c2 = nx;
        cur = nx;
        own = seed_vertex<W>(x, nx).dout;
    }
    return start;
}

template <int W>
LDBG_WAVE_KERNEL void k_seed_walk(SeedWalkCtx x, const uint32_t* s_idx, int64_t n_s, uint8_t* good, unsigned long long* n_starts) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, items = n_s * 8, nb = (items + ws - 1) / ws;
    unsigned long long cnt = 0;
    for (int64_t b = wave; b < nb; b += nwaves) {
        const int64_t it = b * ws + lane;
        bool start = false;
        if (it < items) start = seed_lane<W>(x, (int64_t)s_idx[it >> 3], (int)((it >> 2) & 1), (unsigned)(it & 3), good);
        cnt += (unsigned)__builtin_popcountll(wave_ballot(start));
    }
    wave_fence();
    if (lane == 0 && cnt) atomic_add_u64(n_starts, cnt);
}

}  // namespace

// ---------------------------------------------------------------- occurrences
Occurrences::Occurrences(const Threading& t) : graph(threaded_graph(t)) {
    const int64_t n = graph.view.N, M = t.n_windows;
    n_records = n;
    rt::set_device(graph.device);
    const OwnStream own;
    d_count_ = own_.get<uint32_t>((size_t)std::max<int64_t>(n, 1));
    d_first_ = own_.get<unsigned long long>((size_t)std::max<int64_t>(n, 1));
    rt::dmemset(d_count_, 0, (size_t)n * 4, own.s);
    rt::dmemset(d_first_, 0xFF, (size_t)n * 8, own.s);
    if (n > 0 && M > 0) {
        DevTimer tm;
        tm.begin(own.s);
        LDBG_LAUNCH(k_occ_count, grid_for(M), 256, own.s, t.rec_dev(), M, d_count_, d_first_);
        tm.end(own.s);
        device_ms = tm.ms;
    }
    rt::stream_sync(own.s);
    profile_add("occurrences", device_ms);
}

void Occurrences::get(int64_t first, int64_t n, uint32_t* count, int64_t* first_window, bool device_out, rt::stream_t stream) const {
    if (first < 0 || n < 0 || first > n_records || n > n_records - first) throw StatusError(LDBG_ERR_ARG, "occurrences: records out of range");
    if (n == 0) return;
    rt::set_device(graph.device);
    const OwnStream own;
    rt::stream_t s = stream ? stream : own.s;
    if (count) { if (device_out) rt::d2d(count, d_count_ + first, (size_t)n * 4, s); else rt::d2h(count, d_count_ + first, (size_t)n * 4, s); }
    if (first_window) {      // (all ones is -1 already: the same bytes)
        if (device_out) rt::d2d(first_window, d_first_ + first, (size_t)n * 8, s); else rt::d2h(first_window, d_first_ + first, (size_t)n * 8, s);
    }
    rt::stream_sync(s);
}

// ---------------------------------------------------------------- the seed pass
void variant_seeds(Selection& sel, const SeedFilter& f, ldbg_seed_counts* counts) {
    const Graph& g = sel.graph;
    if (!is_whole_table(g) || g.path == "<collection>")
        throw StatusError(LDBG_ERR_UNSUPPORTED, "variant seeds: the graph must be one resident graph file, not a collection, one rank's part of a hash-sharded table or its image");
    const int C = g.hdr.C;
    if (C > 64) throw StatusError(LDBG_ERR_UNSUPPORTED, "variant seeds: a graph of more than 64 colours");
    const uint64_t colours = C == 64 ? ~0ull : ((1ull << C) - 1ull);
    if (f.n_covered < 0 || f.n_covered > LDBG_SEED_MAX_COVERED) throw StatusError(LDBG_ERR_ARG, "variant seeds: more covered clauses than the filter holds");
    if (f.n_unique < 0 || f.n_unique > LDBG_SEED_MAX_UNIQUE) throw StatusError(LDBG_ERR_ARG, "variant seeds: more unique entries than the filter holds");
    if (f.all_zero & ~colours) throw StatusError(LDBG_ERR_ARG, "variant seeds: a colour mask names a colour the graph does not have");
    SeedMaskCtx x{};
    x.cov = g.view.cov; x.edges = g.view.edges; x.N = g.view.N; x.C = C;
    x.all_zero = f.all_zero;
    for (int j = 0; j < f.n_covered; j++) {
        if (f.covered[j].mask & ~colours) throw StatusError(LDBG_ERR_ARG, "variant seeds: a colour mask names a colour the graph does not have");
        x.cmask[j] = f.covered[j].mask; x.lo[j] = f.covered[j].at_least; x.hi[j] = f.covered[j].at_most;
    }
    x.n_unique = f.n_unique;
    for (int j = 0; j < f.n_unique; j++) {
        const SeedUnique& u = f.unique[j];
        if (u.colour < -1 || u.colour >= C) throw StatusError(LDBG_ERR_ARG, "variant seeds: unique colour " + std::to_string(u.colour) + " out of range");
        if ((u.occurrences != nullptr) == (u.d_unique != nullptr))
            throw StatusError(LDBG_ERR_ARG, "variant seeds: a unique entry takes either occurrences or a byte per record, not neither or both");
        if (u.occurrences && &u.occurrences->graph != &g) throw StatusError(LDBG_ERR_ARG, "variant seeds: occurrences made over another graph");
        x.ucol[j] = u.colour;
        x.ucount[j] = u.occurrences ? u.occurrences->count_dev() : nullptr;
        x.ubytes[j] = u.d_unique;
    }
    ldbg_seed_counts cn{0, 0, 0, 0.0};
    const int64_t n = g.view.N;
    if (n > 0) {
        rt::set_device(g.device);
        rt::stream_t s = g.stream;
        const int64_t nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
        DevBlocks tmp;
        uint8_t* eb = tmp.get<uint8_t>((size_t)n);
        uint8_t* good = tmp.get<uint8_t>((size_t)n);
        unsigned long long* ballots = tmp.get<unsigned long long>((size_t)nchunks * (LDBG_SELECT_CHUNK / 64));
        uint32_t* chunk_cnt = tmp.get<uint32_t>((size_t)nchunks);
        unsigned long long* n_starts = tmp.get<unsigned long long>(1);
        DevTimer tm;
        tm.begin(s);
        LDBG_LAUNCH(k_seed_mask, waves_for(nchunks), 64, s, x, eb, ballots, chunk_cnt);
        tm.end(s);
        Selection in_s(g);
        in_s.compact(ballots, chunk_cnt, s);
        cn.n_seeds = in_s.count;
        if (in_s.count > 0) {
            const SeedWalkCtx w{g.view, ballots, eb};
            unsigned long long starts = 0;
            rt::dmemset(good, 0, (size_t)n, s);
            rt::dmemset(n_starts, 0, 8, s);
            tm.begin(s);
            LDBG_LAUNCH_W(g.view.W, k_seed_walk, waves_for((in_s.count * 8 + 63) / 64), 64, s, w, in_s.records_dev(), in_s.count, good, n_starts);
            LDBG_LAUNCH(k_seed_good, waves_for(nchunks), 64, s, (const uint8_t*)good, n, ballots, chunk_cnt);      // (the walk is done with S's ballots)
            tm.end(s);
            rt::d2h(&starts, n_starts, 8, s);
            rt::stream_sync(s);
            cn.n_unique = (int64_t)starts;
            sel.compact(ballots, chunk_cnt, s);
        }
        cn.n_good = sel.count;
        cn.device_ms = tm.ms + in_s.select_ms + sel.select_ms;
        sel.select_ms = cn.device_ms;
    }
    profile_add("seeds", cn.device_ms);
    if (counts) *counts = cn;
}

}  // namespace ldbg
