// Link construction on the device (linkbuild.h): the read text packed to 2-bit words (bldpack.h) -> one window per
// lane: its canonical k-mer looked up in the resident table, "is a vertex of the colour's string graph", in- and out-degree, from
// the record's own edges and, where those do not state an edge, from the neighbour's (a colour need not be edge-consistent) -> one
// position per lane and strand: fork and convergence flags (the reverse strand reads the same windows backwards with the degrees
// swapped) -> prefix sums over all positions: the rank of every position among the forks, the fork bases compacted into one string
// in which every strand owns a stretch, the terms c * 31^(distance from the strand's last fork) whose sums give String.hashCode of
// every suffix -> one descriptor per link: canonical key, orientation, (offset, length) into the fork string, suffix hash, the place
// of the link in the reference's insertion order -> the stable radix sort of sort.cpp over (key, orientation | length | hash) ->
// duplicates of the suffix another strand gave already are dropped after comparing the bytes -> the survivors go to the host, which
// applies the three HashMap orders and writes the text.  No kernel waits for another workgroup.  The TEST-ONLY host simulation runs
// the kernels as they are.
#include "linkbuild.h"

#include <stdio.h>
#include <zlib.h>

#include <algorithm>
#include <numeric>
#include <set>
#include <tuple>

#include "bldpack.h"
#include "devmem.h"
#include "wavescan.h"

namespace ldbg {

namespace {

// a window's info word
#define LNK_VERTEX 1u          // the window's string is a vertex of the colour's string graph
#define LNK_FLIP 2u            // its reverse complement is the smaller: the key is the reverse complement
#define LNK_PAL 4u             // it is its own reverse complement
#define LNK_INDEG(x) (((x) >> 4) & 7u)
#define LNK_OUTDEG(x) (((x) >> 8) & 7u)

typedef WinCtx ReadsCtx;        // the reads that have two windows or more (bldpack.h)

struct LnkDesc { uint32_t q, q0, bucket, off, len; };     // position, first position of its strand, bucket of order 3, junctions = fork string [off, off + len)

// does the edge byte e of a record state the out-edge (in-edge) with base b of its k-mer read in the orientation f (true: the
// reverse complement of the record's k-mer)?  A palindrome is read both ways (loadGraph adds its edges twice).
LDBG_DEV bool lnk_states_out(unsigned e, bool f, bool pal, unsigned b) { return ((!f) && ((e >> b) & 1u)) || ((f || pal) && ((e >> (4 + b)) & 1u)); }
LDBG_DEV bool lnk_states_in(unsigned e, bool f, bool pal, unsigned b) { return ((!f) && ((e >> (7 - b)) & 1u)) || ((f || pal) && ((e >> (3 - b)) & 1u)); }

// the neighbour s of a window: does its record (coverage above 0 in the colour) state the edge back, with base b?
template <int W>
LDBG_DEV bool lnk_nbr_states(const GraphView& g, int col, const Kmer<W>& s, bool want_in, unsigned b) {
    const Kmer<W> rc = kmer_revcomp<W>(s, g.k);
    const int cmp = kmer_cmp<W>(rc, s);
    const int64_t idx = graph_find_canonical<W>(g, cmp < 0 ? rc : s);
    if (idx < 0 || (int32_t)graph_cov(g, idx, col) <= 0) return false;
    const unsigned e = graph_edges(g, idx, col);
    return want_in ? lnk_states_in(e, cmp < 0, cmp == 0, b) : lnk_states_out(e, cmp < 0, cmp == 0, b);
}

// one window per lane: keys[w][m] = word w of the canonical k-mer of window m (k_bld_extract's shifts), info[m] = vertex | flip |
// palindrome | indeg << 4 | outdeg << 8 of the window's string in the string graph of colour col.  An edge u -> v exists when u's
// record states the out-edge or v's record states the in-edge; only records with coverage in the colour speak.  A window with a
// byte that is no upper-case base is no vertex.
template <int W>
LDBG_KERNEL void k_lnk_windows(ReadsCtx x, GraphView g, int col, uint64_t* keys, uint16_t* info) {
    for (int64_t m = global_tid(); m < x.M; m += global_nthreads()) {
        const int64_t lo = win_seq(x, m), gp = x.seq_beg[lo] + (m - x.win_start[lo]);
        const Kmer<W> a = win_kmer<W>(x, gp);
        const bool ok = win_valid(x, gp);
        unsigned out = 0;
        Kmer<W> c = a;
        if (ok) {
            const Kmer<W> rc = kmer_revcomp<W>(a, x.k);
            const int cmp = kmer_cmp<W>(rc, a);
            const bool f = cmp < 0, pal = cmp == 0;
            if (f) c = rc;
            const int64_t own = graph_find_canonical<W>(g, c);
            const bool has = own >= 0 && (int32_t)graph_cov(g, own, col) > 0;
            const unsigned e = has ? graph_edges(g, own, col) : 0u;
            const unsigned first = kmer_base<W>(a, x.k, 0), last = (unsigned)(a.w[W - 1] & 3ull);
            unsigned indeg = 0, outdeg = 0;
            for (unsigned b = 0; b < 4; b++) {
                bool so = has && lnk_states_out(e, f, pal, b);
                if (!so) so = lnk_nbr_states<W>(g, col, kmer_next<W>(a, x.k, b), true, first);
                bool si = has && lnk_states_in(e, f, pal, b);
                if (!si) si = lnk_nbr_states<W>(g, col, kmer_prev<W>(a, x.k, b), false, last);
                outdeg += so ? 1u : 0u;
                indeg += si ? 1u : 0u;
            }
            out = ((has || indeg + outdeg > 0) ? LNK_VERTEX : 0u) | (f ? LNK_FLIP : 0u) | (pal ? LNK_PAL : 0u) | (indeg << 4) | (outdeg << 8);
        }
#pragma unroll
        for (int w = 0; w < W; w++) keys[(size_t)w * (size_t)x.M + (size_t)m] = ok ? c.w[w] : 0ull;
        info[m] = (uint16_t)out;
    }
}

// position q of the 2 M strand positions: read r owns [2 win_start[r], 2 win_start[r + 1]), the given strand first
struct StrandPos {
    int64_t beg, w0, nw, p, q0, qe;
    bool rev;
};
LDBG_DEV StrandPos lnk_resolve(const ReadsCtx& x, int64_t q) {
    int64_t lo = 0, hi = x.nr;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (2 * x.win_start[mid] <= q) lo = mid; else hi = mid;
    }
    StrandPos s;
    s.beg = x.seq_beg[lo];
    s.w0 = x.win_start[lo];
    s.nw = x.win_start[lo + 1] - s.w0;
    const int64_t local = q - 2 * s.w0;
    s.rev = local >= s.nw;
    s.p = s.rev ? local - s.nw : local;
    s.q0 = 2 * s.w0 + (s.rev ? s.nw : 0);
    s.qe = s.q0 + s.nw;
    return s;
}
// window p of the strand among the read's windows: the reverse strand's window p is the reverse complement of the read's nw - 1 - p
LDBG_DEV int64_t lnk_window(const StrandPos& s, int64_t p) { return s.w0 + (s.rev ? s.nw - 1 - p : p); }

// fork[q] (with the base the strand takes there) and conv[q] of every position; *bad when a window other than a strand's last is
// no vertex
LDBG_KERNEL void k_lnk_flags(ReadsCtx x, const uint16_t* info, int64_t P, uint32_t* fork, uint8_t* cb, unsigned* bad) {
    bool miss = false;
    for (int64_t q = global_tid(); q < P; q += global_nthreads()) {
        const StrandPos s = lnk_resolve(x, q);
        const unsigned in = info[lnk_window(s, s.p)];
        const bool v = (in & LNK_VERTEX) != 0;
        if (s.p <= s.nw - 2 && !v) miss = true;
        bool fk = false, cv = false;
        unsigned base = 0;
        if (s.p >= 1) {
            const unsigned pi = info[lnk_window(s, s.p - 1)];
            fk = v && (s.rev ? LNK_INDEG(pi) : LNK_OUTDEG(pi)) > 1u;
            cv = (s.rev ? LNK_OUTDEG(in) : LNK_INDEG(in)) > 1u;
        }
        if (fk) base = s.rev ? 3u - bld_base(x.packed, s.beg + s.nw - 1 - s.p) : bld_base(x.packed, s.beg + s.p + x.k - 1);
        fork[q] = fk ? 1u : 0u;
        cb[q] = (uint8_t)((cv ? 1u : 0u) | (base << 1));
    }
    if (miss) atomic_or_u32(bad, 1u);
}

LDBG_DEV uint32_t lnk_pow31(uint32_t e) {
    uint32_t r = 1, b = 31;
    while (e) { if (e & 1u) r *= b; b *= b; e >>= 1; }
    return r;
}

// fork t of all forks (F = forks before a position): G[t] = its base, term[t] = base * 31^(forks of the strand after it), so that
// String.hashCode of a suffix of the strand's fork string is a difference of prefix sums of the terms
LDBG_KERNEL void k_lnk_terms(ReadsCtx x, int64_t P, const uint32_t* fork, const uint8_t* cb, const uint32_t* F, uint32_t* term, uint8_t* G) {
    for (int64_t q = global_tid(); q < P; q += global_nthreads()) {
        if (!fork[q]) continue;
        const StrandPos s = lnk_resolve(x, q);
        const uint32_t t = F[q], b = (cb[q] >> 1) & 3u;
        const uint32_t ch = b == 0 ? 65u : (b == 1 ? 67u : (b == 2 ? 71u : 84u));
        G[t] = (uint8_t)ch;
        term[t] = ch * lnk_pow31(F[s.qe] - 1u - t);
    }
}

// link[q]: a convergence with a fork at or after it; *bytes += the junction bytes of the links
LDBG_KERNEL void k_lnk_linkflags(ReadsCtx x, int64_t P, const uint8_t* cb, const uint32_t* F, uint32_t* link, unsigned long long* bytes) {
    unsigned long long sum = 0;
    for (int64_t q = global_tid(); q < P; q += global_nthreads()) {
        uint32_t len = 0;
        if (cb[q] & 1u) { const StrandPos s = lnk_resolve(x, q); len = F[s.qe] - F[q]; }
        link[q] = len > 0 ? 1u : 0u;
        sum += len;
    }
    if (sum) atomic_add_u64(bytes, sum);
}

// the descriptor of every link (D = links before a position): planes dk[0..W) = the canonical key of the k-mer before the
// convergence, dk[W] = forward << 63 | length << 32 | hashCode of the junctions; desc = where the junctions are and where the link
// stands in the reference's order of insertion: strand after strand, inside a strand by the bucket of commons-math3's Pair.hashCode
// of (k-mer string, position) in a HashMap sized for the strand's links, then by position
template <int W>
LDBG_KERNEL void k_lnk_desc(ReadsCtx x, int64_t P, const uint64_t* keys, const uint16_t* info, const uint32_t* link, const uint32_t* F, const uint32_t* PS,
                            const uint32_t* D, int64_t ND, uint64_t* dk, LnkDesc* desc) {
    for (int64_t q = global_tid(); q < P; q += global_nthreads()) {
        if (!link[q]) continue;
        const StrandPos s = lnk_resolve(x, q);
        const size_t d = D[q], m = (size_t)lnk_window(s, s.p - 1);
        const unsigned in = info[m];
        Kmer<W> c;
#pragma unroll
        for (int w = 0; w < W; w++) c.w[w] = keys[(size_t)w * (size_t)x.M + m];
        const bool canon = s.rev ? (in & (LNK_FLIP | LNK_PAL)) != 0 : (in & LNK_FLIP) == 0;     // the strand's string is the canonical one
        const Kmer<W> sk = canon ? c : kmer_revcomp<W>(c, x.k);
        uint32_t sh = 0;                                    // String.hashCode of the strand's string
        for (int i = 0; i < x.k; i++) {
            const unsigned b = kmer_base<W>(sk, x.k, i);
            sh = 31u * sh + (b == 0 ? 65u : (b == 1 ? 67u : (b == 2 ? 71u : 84u)));
        }
        const uint32_t nl = D[s.qe] - D[s.q0], i = (uint32_t)s.p;
        uint64_t cap = 16;
        while ((uint64_t)nl > cap * 3 / 4) cap *= 2;
        uint32_t ph = (37u * sh + i) ^ (i >> 16);
        ph ^= ph >> 16;
        const uint32_t off = F[q], end = F[s.qe];
        LnkDesc o;
        o.q = (uint32_t)q; o.q0 = (uint32_t)s.q0; o.bucket = ph & (uint32_t)(cap - 1); o.off = off; o.len = end - off;
        desc[d] = o;
#pragma unroll
        for (int w = 0; w < W; w++) dk[(size_t)w * (size_t)ND + d] = c.w[w];
        dk[(size_t)W * (size_t)ND + d] = ((uint64_t)(canon ? 1u : 0u) << 63) | ((uint64_t)o.len << 32) | (uint64_t)(PS[end] - PS[off]);
    }
}

// sorted descriptor x: keep[x] = 0 when the one before it has the same key, orientation, length and hash, comes from another strand
// and its junction bytes are the same (a duplicate inside one strand stays: which of the two the reference inserts first is for the
// host to say); *nkmers += keys that start at x
template <int W>
LDBG_KERNEL void k_lnk_mark(const uint64_t* dk, const LnkDesc* desc, const uint32_t* perm, int64_t ND, const uint8_t* G, uint32_t* keep, unsigned long long* nkmers) {
    unsigned long long heads = 0;
    for (int64_t x = global_tid(); x < ND; x += global_nthreads()) {
        const size_t a = perm[x];
        bool head = x == 0, dup = false;
        if (x > 0) {
            const size_t b = perm[x - 1];
#pragma unroll
            for (int w = 0; w < W; w++) head |= dk[(size_t)w * (size_t)ND + a] != dk[(size_t)w * (size_t)ND + b];
            const LnkDesc da = desc[a], db = desc[b];
            if (!head && dk[(size_t)W * (size_t)ND + a] == dk[(size_t)W * (size_t)ND + b] && da.q0 != db.q0) {
                dup = true;
                for (uint32_t t = 0; t < da.len; t++)
                    if (G[(size_t)da.off + t] != G[(size_t)db.off + t]) { dup = false; break; }
            }
        }
        keep[x] = dup ? 0u : 1u;
        heads += head ? 1u : 0u;
    }
    if (heads) atomic_add_u64(nkmers, heads);
}

// the kept descriptors in sorted order (KO = kept before x): out_keys[o] = W key words and the orientation word, out_desc[o]
template <int W>
LDBG_KERNEL void k_lnk_compact(const uint64_t* dk, const LnkDesc* desc, const uint32_t* perm, int64_t ND, const uint32_t* keep, const uint32_t* KO,
                               uint64_t* out_keys, LnkDesc* out_desc) {
    for (int64_t x = global_tid(); x < ND; x += global_nthreads()) {
        if (!keep[x]) continue;
        const size_t a = perm[x], o = KO[x];
#pragma unroll
        for (int w = 0; w <= W; w++) out_keys[o * (size_t)(W + 1) + (size_t)w] = dk[(size_t)w * (size_t)ND + a];
        out_desc[o] = desc[a];
    }
}

int32_t jbytes_hash(const std::string& s) { uint32_t h = 1; for (char c : s) h = 31u * h + (uint32_t)(int32_t)(signed char)c; return (int32_t)h; }

}  // namespace

BuiltLinks build_links(const Graph& g, const char* sample_name, const char* bases, const int64_t* offsets, int64_t n_reads, int flags) {
    if (!sample_name) throw StatusError(LDBG_ERR_ARG, "links build: no sample name");
    if (flags != 0) throw StatusError(LDBG_ERR_ARG, "links build: unknown flag");
    if (n_reads < 0 || (n_reads > 0 && (!bases || !offsets))) throw StatusError(LDBG_ERR_ARG, "links build: reads but no text or offsets");
    for (int64_t i = 0; i < n_reads; i++)
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) throw StatusError(LDBG_ERR_ARG, "links build: the offsets decrease");
    check_whole_table(g, "links build");
    if (g.path == "<collection>") throw StatusError(LDBG_ERR_UNSUPPORTED, "links build: not over a collection of graphs (Join them first)");
    const int col = g.color_for_sample_name(sample_name);
    if (col < 0 || col >= g.hdr.C) throw StatusError(LDBG_ERR_CORTEXJDK, std::string("Sample '") + sample_name + "' not found in graph");
    const int k = g.hdr.k, W = g.hdr.W;
    // the windows of the reads that have two or more (a shorter read has no junction to record), counted from the offsets alone
    std::vector<int64_t> win_start{0}, seq_beg;
    for (int64_t i = 0; i < n_reads; i++) {
        const int64_t L = offsets[i + 1] - offsets[i];
        if (L < (int64_t)k + 1) continue;
        seq_beg.push_back(offsets[i] - offsets[0]);
        win_start.push_back(win_start.back() + (L - k + 1));
        if (win_start.back() >= (1ll << 31)) throw StatusError(LDBG_ERR_UNSUPPORTED, "links build: 2^31 or more k-mer windows in one call");
    }
    if (rt::device_count() <= g.device) throw StatusError(LDBG_ERR_HIP, "no HIP device " + std::to_string(g.device) + " available (libldbg has no CPU fallback)");

    BuiltLinks out;
    out.k = k;
    out.num_kmers_in_graph = g.hdr.num_records;
    out.sample = sample_name;
    const int64_t nr = (int64_t)seq_beg.size(), M = win_start.back(), P = 2 * M;
    if (M == 0) return out;
    const int64_t L = offsets[n_reads] - offsets[0], nwords = (L + 31) / 32;

    std::vector<uint64_t> h_keys;
    std::vector<LnkDesc> h_desc;
    std::vector<uint8_t> h_G;
    int64_t NK = 0;
    rt::set_device(g.device);
    {
        DevBlocks tmp;
        const OwnStream own;
        rt::stream_t s = own.s;
        DevTimer tm;
        uint8_t* d_ascii = tmp.get<uint8_t>((size_t)nwords * 32);
        uint64_t* d_packed = tmp.get<uint64_t>((size_t)nwords);
        uint32_t* d_valid = tmp.get<uint32_t>((size_t)nwords);
        int64_t* d_reads = tmp.get<int64_t>((size_t)(2 * nr + 1));
        uint64_t* d_keys = tmp.get<uint64_t>((size_t)M * W);
        uint16_t* d_info = tmp.get<uint16_t>((size_t)M);
        uint32_t* d_fork = tmp.get<uint32_t>((size_t)P);
        uint8_t* d_cb = tmp.get<uint8_t>((size_t)P);
        uint32_t* d_F = tmp.get<uint32_t>((size_t)P + 1);
        const size_t maxchunks = (size_t)((P + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK) + 1;
        uint32_t* d_sums = tmp.get<uint32_t>(maxchunks);
        uint32_t* d_offs = tmp.get<uint32_t>(maxchunks + 1);
        unsigned long long* d_stat = tmp.get<unsigned long long>(3);      // [0] a window that is no vertex, [1] junction bytes, [2] k-mers with links
        rt::dmemset(d_ascii + L, 0, (size_t)(nwords * 32 - L), s);
        rt::h2d(d_ascii, bases + offsets[0], (size_t)L, s);
        rt::h2d(d_reads, win_start.data(), (size_t)(nr + 1) * 8, s);
        rt::h2d(d_reads + nr + 1, seq_beg.data(), (size_t)nr * 8, s);
        rt::dmemset(d_stat, 0, 24, s);
        GraphView view = g.view;
        view.java_tiny = 0;                                   // (loadGraph reads the records one by one: findRecord's quirk Q1 has no part in it)
        const ReadsCtx x{d_packed, d_valid, d_reads, d_reads + nr + 1, nr, M, k};
        tm.begin(s);
        LDBG_LAUNCH(k_bld_pack, grid_for(nwords), 256, s, (const uint8_t*)d_ascii, nwords, d_packed, d_valid);
        LDBG_LAUNCH(k_lnk_upper_only, grid_for(nwords), 256, s, (const uint8_t*)d_ascii, nwords, d_valid);
        LDBG_LAUNCH_W(W, k_lnk_windows, grid_for(M), 256, s, x, view, col, d_keys, d_info);
        LDBG_LAUNCH(k_lnk_flags, grid_for(P), 256, s, x, (const uint16_t*)d_info, P, d_fork, d_cb, (unsigned*)d_stat);
        scan_u32(d_fork, P, d_F, d_sums, d_offs, s);
        unsigned long long st[3] = {0, 0, 0};
        uint32_t NF = 0;
        rt::d2h(st, d_stat, 8, s);
        rt::d2h(&NF, d_F + P, 4, s);
        tm.end(s);
        rt::stream_sync(s);
        // loadGraph's DirectedGraph throws from outDegreeOf / inDegreeOf on a string it does not hold (TempLinksAssembler.java:64-78)
        if (st[0] & 0xFFFFFFFFull) throw StatusError(LDBG_ERR_CORTEXJDK, "no such vertex in graph (a read holds a k-mer that the sample's colour does not)");
        tmp.drop(d_ascii); tmp.drop(d_valid);

        uint32_t* d_term = tmp.get<uint32_t>((size_t)NF + 1);
        uint32_t* d_PS = tmp.get<uint32_t>((size_t)NF + 1);
        uint8_t* d_G = tmp.get<uint8_t>((size_t)NF + 1);
        uint32_t* d_link = tmp.get<uint32_t>((size_t)P);
        uint32_t* d_D = tmp.get<uint32_t>((size_t)P + 1);
        tm.begin(s);
        LDBG_LAUNCH(k_lnk_terms, grid_for(P), 256, s, x, P, (const uint32_t*)d_fork, (const uint8_t*)d_cb, (const uint32_t*)d_F, d_term, d_G);
        scan_u32(d_term, NF, d_PS, d_sums, d_offs, s);
        LDBG_LAUNCH(k_lnk_linkflags, grid_for(P, 256, 256), 256, s, x, P, (const uint8_t*)d_cb, (const uint32_t*)d_F, d_link, d_stat + 1);
        scan_u32(d_link, P, d_D, d_sums, d_offs, s);
        uint32_t ND32 = 0;
        rt::d2h(st, d_stat, 16, s);
        rt::d2h(&ND32, d_D + P, 4, s);
        tm.end(s);
        rt::stream_sync(s);
        const int64_t ND = ND32;
        // (sizes from the scans, before a descriptor exists: the junction bytes grow with the square of a strand's forks)
        if (ND >= (1ll << 31) || st[1] >= (1ull << 31))
            throw StatusError(LDBG_ERR_UNSUPPORTED, "links build: 2^31 or more links or junction bytes in one call (" + std::to_string(ND) + " links, " +
                                                        std::to_string(st[1]) + " bytes): build in batches of reads");
        tmp.drop(d_fork); tmp.drop(d_term);
        if (ND > 0) {
            uint64_t* d_dk = tmp.get<uint64_t>((size_t)ND * (W + 1));
            LnkDesc* d_desc = tmp.get<LnkDesc>((size_t)ND);
            uint32_t* d_perm = tmp.get<uint32_t>((size_t)ND);
            uint32_t* d_keep = tmp.get<uint32_t>((size_t)ND);
            uint32_t* d_KO = tmp.get<uint32_t>((size_t)ND + 1);
            tm.begin(s);
            LDBG_LAUNCH_W(W, k_lnk_desc, grid_for(P), 256, s, x, P, (const uint64_t*)d_keys, (const uint16_t*)d_info, (const uint32_t*)d_link, (const uint32_t*)d_F,
                          (const uint32_t*)d_PS, (const uint32_t*)d_D, ND, d_dk, d_desc);
            tm.end(s);
            tmp.drop(d_keys); tmp.drop(d_info); tmp.drop(d_link); tmp.drop(d_D); tmp.drop(d_F); tmp.drop(d_PS); tmp.drop(d_cb); tmp.drop(d_packed); tmp.drop(d_reads);
            tm.begin(s);
            radix_sort_permutation_dev(ND, W + 1, 2 * k - 64 * (W - 1), d_dk, d_perm, s);
            LDBG_LAUNCH_W(W, k_lnk_mark, grid_for(ND, 256, 256), 256, s, (const uint64_t*)d_dk, (const LnkDesc*)d_desc, (const uint32_t*)d_perm, ND, (const uint8_t*)d_G,
                          d_keep, d_stat + 2);
            scan_u32(d_keep, ND, d_KO, d_sums, d_offs, s);
            uint32_t NK32 = 0;
            rt::d2h(&NK32, d_KO + ND, 4, s);
            tm.end(s);
            rt::stream_sync(s);
            NK = NK32;
            uint64_t* d_ok = tmp.get<uint64_t>((size_t)NK * (W + 1));
            LnkDesc* d_od = tmp.get<LnkDesc>((size_t)NK);
            tm.begin(s);
            LDBG_LAUNCH_W(W, k_lnk_compact, grid_for(ND), 256, s, (const uint64_t*)d_dk, (const LnkDesc*)d_desc, (const uint32_t*)d_perm, ND, (const uint32_t*)d_keep,
                          (const uint32_t*)d_KO, d_ok, d_od);
            tm.end(s);
            h_keys.resize((size_t)NK * (W + 1));
            h_desc.resize((size_t)NK);
            h_G.resize((size_t)NF);
            rt::d2h(h_keys.data(), d_ok, h_keys.size() * 8, s);
            rt::d2h(h_desc.data(), d_od, h_desc.size() * sizeof(LnkDesc), s);
            rt::d2h(h_G.data(), d_G, h_G.size(), s);
            rt::stream_sync(s);
        }
        profile_add("links_build", tm.ms);
    }

    // the reduced set, sorted by key: per k-mer the junction records in the reference's order of insertion (equal records collapse onto
    // the first), then the three orders.  Orders 1 and 2 are those of links.cpp's HashSet emulation, applied here on the host: they are
    // sorts by bucket at a capacity that depends on counts known only after the duplicates are gone, over far fewer elements than the
    // device saw, and the text is written here anyway.
    struct Cand { std::tuple<uint32_t, uint32_t, uint32_t> seq; HostJunction j; };
    struct Group { std::tuple<uint32_t, uint32_t, uint32_t> seq; HostLinksRecord rec; };
    std::vector<Group> groups;
    const size_t R = (size_t)W + 1;
    for (size_t o = 0; o < (size_t)NK;) {
        size_t e = o + 1;
        while (e < (size_t)NK && std::equal(&h_keys[o * R], &h_keys[o * R] + W, &h_keys[e * R])) e++;
        std::vector<Cand> cs;
        for (size_t i = o; i < e; i++) {
            const LnkDesc& d = h_desc[i];
            Cand c;
            c.seq = std::make_tuple(d.q0, d.bucket, d.q);
            c.j.is_fw = (h_keys[i * R + W] >> 63) != 0;
            c.j.num_kmers = c.j.num_junctions = (int)d.len;
            c.j.cov = {1};
            c.j.junctions.assign((const char*)&h_G[d.off], d.len);
            cs.push_back(std::move(c));
        }
        std::sort(cs.begin(), cs.end(), [](const Cand& a, const Cand& b) { return a.seq < b.seq; });
        Group gr;
        gr.seq = cs[0].seq;
        gr.rec.kmer.assign((size_t)k, 'A');
        words_to_ascii(&h_keys[o * R], k, W, &gr.rec.kmer[0]);
        std::set<std::pair<bool, std::string>> seen;        // (a heavy k-mer collects many distinct suffixes: no scan of the kept ones)
        for (Cand& c : cs)
            if (seen.insert(std::make_pair(c.j.is_fw, c.j.junctions)).second) gr.rec.juncs.push_back(std::move(c.j));
        // the HashSet of linkMap, then the ArrayList -> HashSet copy of new CortexLinksRecord (TempLinksAssembler.java:161-165)
        links_hashset_order(gr.rec.juncs);
        links_hashset_order(gr.rec.juncs);
        groups.push_back(std::move(gr));
        o = e;
    }
    std::sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) { return a.seq < b.seq; });
    int cap = 16;
    while (groups.size() > (size_t)cap * 3 / 4) cap *= 2;
    std::vector<uint32_t> bucket(groups.size());
    std::vector<size_t> order(groups.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    for (size_t i = 0; i < groups.size(); i++) { uint32_t h = (uint32_t)jbytes_hash(groups[i].rec.kmer); h ^= h >> 16; bucket[i] = h & (uint32_t)(cap - 1); }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return bucket[a] < bucket[b]; });
    for (size_t i : order) {
        out.num_links += (int64_t)groups[i].rec.juncs.size();
        for (HostJunction& j : groups[i].rec.juncs) j.num_kmers = -1;      // (as the parser of a version 4 file leaves it)
        out.records.push_back(std::move(groups[i].rec));
    }
    return out;
}

std::string built_links_text(const BuiltLinks& b) {
    const std::string n = std::to_string(b.num_links);
    std::string t = "{\n        \"file_format\": \"ctp\",\n        \"format_version\": 4,\n        \"file_key\": 0,\n        \"graph\": {\n"
                    "                \"num_colours\": 1,\n                \"kmer_size\": " + std::to_string(b.k) + ",\n"
                    "                \"num_kmers_in_graph\": " + std::to_string(b.num_kmers_in_graph) + ",\n                \"colours\": [{\n"
                    "                        \"colour\": 0,\n                        \"sample\": \"" + b.sample + "\",\n"
                    "                        \"total_sequence\": 0,\n                        \"cleaned_tips\": false,\n"
                    "                        \"cleaned_unitigs\": false\n                }]\n        },\n        \"paths\": {\n"
                    "                \"num_kmers_with_paths\": " + std::to_string(b.records.size()) + ",\n                \"num_paths\": " + n + ",\n"
                    "                \"path_bytes\": " + n + "\n        }\n}\n\n";
    for (const HostLinksRecord& r : b.records) {            // CortexLinksRecord.toString (:58-74) and a newline
        t += r.kmer + " " + std::to_string(r.juncs.size()) + "\n";
        for (const HostJunction& j : r.juncs) {
            t += j.is_fw ? "F " : "R ";
            t += std::to_string(j.num_junctions) + " ";
            for (size_t c = 0; c < j.cov.size(); c++) { if (c) t += ","; t += std::to_string(j.cov[c]); }
            t += " " + j.junctions + "\n";
        }
    }
    t += "\n";
    return t;
}

void built_links_write(const BuiltLinks& b, const std::string& out_path) {
    const std::string text = built_links_text(b);
    gzFile f = gzopen(out_path.c_str(), "wb");
    if (!f) throw StatusError(LDBG_ERR_CORTEXJDK, "Could not get a file for links creation: '" + out_path + "'");
    bool ok = true;
    for (size_t o = 0; o < text.size() && ok; o += (size_t)1 << 30) {
        const unsigned nb = (unsigned)std::min<size_t>((size_t)1 << 30, text.size() - o);
        ok = gzwrite(f, text.data() + o, nb) == (int)nb;
    }
    ok = gzclose(f) == Z_OK && ok;
    if (!ok) { remove(out_path.c_str()); throw StatusError(LDBG_ERR_CORTEXJDK, "Unable to write links to file '" + out_path + "'"); }
}

}  // namespace ldbg
