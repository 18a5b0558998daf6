// Sequences threaded through a graph on the device (thread.h): the text packed to 2-bit words with validity bits
// (bldpack.h) -> one window per lane: the k-mer as given, its canonical form, its record in the graph and in the ROI graph, the first
// and last hit of its sequence by one atomic each -> prefix sums over the hit flags: hits per sequence at the sequence boundaries ->
// region heads (a hit whose predecessor in the sequence is none) scanned: every region's start and stop placed from the scan, regions
// per sequence at the boundaries -> the keys (sequence, ROI record) of the hits compacted and sorted (sort.cpp), a key that differs
// from its predecessor flagged, the flags scanned: distinct ROI k-mers per sequence at the boundaries -> with copy indices: the stable
// sort of the windows by (sequence, validity, k-mer as given), run heads flagged and their sorted positions compacted: a window's
// copy index is its distance from the head of its run.  No kernel waits for another workgroup.  The TEST-ONLY host simulation runs
// the kernels as they are.
#include "thread.h"

#include "bldpack.h"
#include "wavescan.h"

namespace ldbg {

namespace {

struct ThrOut {
    int64_t* rec;          // [M]
    uint8_t* info;         // [M]
    uint32_t* hit;         // [M] 1 where the ROI graph holds the window's k-mer
    uint32_t* rrec;        // [M] its record there
    uint32_t* seq;         // [M] the window's sequence
    unsigned* first;       // [nr] smallest hitting window of the sequence (0xFFFFFFFF: none)
    unsigned* last;        // [nr] largest, plus one (0: none)
    uint64_t* planes;      // [W + 1][M] with copy indices: sequence << 1 | invalid, then the k-mer as given; else null
};

// one window per lane
template <int W>
LDBG_KERNEL void k_thr_windows(WinCtx x, GraphView g, int has_g, GraphView r, int has_r, ThrOut o) {
    for (int64_t m = global_tid(); m < x.M; m += global_nthreads()) {
        const int64_t sq = win_seq(x, m), rel = m - x.win_start[sq], gp = x.seq_beg[sq] + rel;
        const Kmer<W> a = win_kmer<W>(x, gp);
        const bool ok = win_valid(x, gp);
        unsigned in = 0;
        int64_t rec = -1, rr = -1;
        if (ok) {
            const Kmer<W> rc = kmer_revcomp<W>(a, x.k);
            const int cmp = kmer_cmp<W>(rc, a);
            const Kmer<W> c = cmp < 0 ? rc : a;
            in = LDBG_WIN_VALID | (cmp < 0 ? LDBG_WIN_FLIP : 0u) | (cmp == 0 ? LDBG_WIN_PAL : 0u);
            if (has_g) rec = graph_find_canonical<W>(g, c);
            if (has_r) rr = graph_find_canonical<W>(r, c);
            if (rr >= 0) {
                in |= LDBG_WIN_ROI;
                atomic_min_u32(o.first + sq, (unsigned)rel);
                atomic_max_u32(o.last + sq, (unsigned)rel + 1u);
            }
        }
        o.rec[m] = rec;
        o.info[m] = (uint8_t)in;
        o.hit[m] = rr >= 0 ? 1u : 0u;
        o.rrec[m] = rr >= 0 ? (uint32_t)rr : 0u;
        o.seq[m] = (uint32_t)sq;
        if (o.planes) {
            o.planes[m] = ((uint64_t)sq << 1) | (ok ? 0ull : 1ull);
#pragma unroll
            for (int w = 0; w < W; w++) o.planes[(size_t)(w + 1) * (size_t)x.M + (size_t)m] = ok ? a.w[w] : 0ull;
        }
    }
}

// head[m]: window m is a hit and the first window of its sequence, or the one before it is no hit
LDBG_KERNEL void k_thr_heads(const int64_t* win_start, const uint32_t* seq, const uint32_t* hit, int64_t M, uint32_t* head) {
    for (int64_t m = global_tid(); m < M; m += global_nthreads())
        head[m] = hit[m] && (m == win_start[seq[m]] || !hit[m - 1]) ? 1u : 0u;
}

// RH = heads before a window: region RH[m] starts at a head m, and the region a tail m closes is the last one opened up to m
LDBG_KERNEL void k_thr_regions(const int64_t* win_start, const uint32_t* seq, const uint32_t* hit, const uint32_t* head, const uint32_t* RH, int64_t M,
                               int32_t* start, int32_t* stop) {
    for (int64_t m = global_tid(); m < M; m += global_nthreads()) {
        if (!hit[m]) continue;
        const uint32_t sq = seq[m];
        const int32_t rel = (int32_t)(m - win_start[sq]);
        if (head[m]) start[RH[m]] = rel;
        if (m + 1 == win_start[sq + 1] || !hit[m + 1]) stop[RH[m + 1] - 1u] = rel;
    }
}

// H = hits before a window: the key (sequence, ROI record) of hit m goes to place H[m]
LDBG_KERNEL void k_thr_hit_keys(const uint32_t* seq, const uint32_t* hit, const uint32_t* rrec, const uint32_t* H, int64_t M, uint64_t* keys) {
    for (int64_t m = global_tid(); m < M; m += global_nthreads())
        if (hit[m]) keys[H[m]] = ((uint64_t)seq[m] << 32) | (uint64_t)rrec[m];
}

// sorted key x of n keys of `planes` words: flag[x] = it differs from the one before it
LDBG_KERNEL void k_thr_run_heads(const uint64_t* keys, int planes, const uint32_t* perm, int64_t n, uint32_t* flag) {
    for (int64_t x = global_tid(); x < n; x += global_nthreads()) {
        bool head = x == 0;
        if (x > 0) {
            const size_t a = perm[x], b = perm[x - 1];
            for (int w = 0; w < planes; w++) head |= keys[(size_t)w * (size_t)n + a] != keys[(size_t)w * (size_t)n + b];
        }
        flag[x] = head ? 1u : 0u;
    }
}

// R = run heads before a sorted position: heads[R[x]] = x for every head
LDBG_KERNEL void k_thr_head_pos(const uint32_t* flag, const uint32_t* R, int64_t n, uint32_t* heads) {
    for (int64_t x = global_tid(); x < n; x += global_nthreads())
        if (flag[x]) heads[R[x]] = (uint32_t)x;
}

// the window at sorted position x stands x - (head of its run) places after the first window of its sequence with the same string
LDBG_KERNEL void k_thr_copy_index(const uint64_t* plane0, const uint32_t* perm, const uint32_t* R, const uint32_t* heads, int64_t n, int32_t* copy) {
    for (int64_t x = global_tid(); x < n; x += global_nthreads()) {
        const size_t m = perm[x];
        copy[m] = (plane0[m] & 1ull) ? 0 : (int32_t)((uint32_t)x - heads[R[x + 1] - 1u]);
    }
}

struct SeqOut { int32_t *first, *last, *n_hits, *n_distinct; uint8_t* ends; int64_t* reg_off; };

// one sequence per lane: the scans read at its boundaries
LDBG_KERNEL void k_thr_seq(const int64_t* win_start, int64_t nr, const uint32_t* hit, const uint32_t* H, const uint32_t* RH, const uint32_t* DF,
                           const unsigned* first, const unsigned* last, SeqOut o) {
    for (int64_t s = global_tid(); s <= nr; s += global_nthreads()) {
        const int64_t a = win_start[s];
        o.reg_off[s] = RH[a];
        if (s == nr) continue;
        const int64_t b = win_start[s + 1];
        o.first[s] = (int32_t)first[s];
        o.last[s] = (int32_t)last[s] - 1;
        o.n_hits[s] = (int32_t)(H[b] - H[a]);
        o.n_distinct[s] = DF ? (int32_t)(DF[H[b]] - DF[H[a]]) : 0;
        o.ends[s] = (uint8_t)(b > a ? (hit[a] ? 1u : 0u) | (hit[b - 1] ? 2u : 0u) : 0u);
    }
}

LDBG_KERNEL void k_thr_coverage(GraphView g, int colour, const int64_t* rec, int64_t n, int32_t* cov, unsigned* missing) {
    bool miss = false;
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) {
        const int64_t r = rec[i];
        if (r < 0) miss = true;
        cov[i] = r < 0 ? 0 : (int32_t)graph_cov(g, r, colour);
    }
    if (miss) atomic_or_u32(missing, 1u);
}

int bits_for(uint64_t v) { int b = 1; while (b < 64 && (v >> b)) b++; return b; }       // bits that hold every value up to v

}  // namespace

Threading::Threading(const Graph* g, const Graph* rois, const char* bases, const int64_t* offsets, int64_t n, int fl, bool on_device, rt::stream_t stream)
    : graph(g), flags(fl), n_seqs(n) {
    if (!g && !rois) throw StatusError(LDBG_ERR_ARG, "thread: neither a graph nor a ROI graph");
    if (fl & ~(LDBG_THREAD_FIND_QUIRK | LDBG_THREAD_COPY_INDEX)) throw StatusError(LDBG_ERR_ARG, "thread: unknown flag");
    const Graph& any = g ? *g : *rois;
    if (g && rois && (g->hdr.k != rois->hdr.k)) throw StatusError(LDBG_ERR_ARG, "thread: the graph and the ROI graph differ in k");
    if (g && rois && g->device != rois->device) throw StatusError(LDBG_ERR_ARG, "thread: the graph and the ROI graph are on different devices");
    if (n < 0 || (n > 0 && (!bases || !offsets))) throw StatusError(LDBG_ERR_ARG, "thread: sequences but no text or offsets");
    if (n >= (1ll << 31)) throw StatusError(LDBG_ERR_UNSUPPORTED, "thread: 2^31 or more sequences in one call");
    if (g) check_whole_table(*g, "thread");
    if (rois) check_whole_table(*rois, "thread");
    device = any.device;
    const int k = any.hdr.k, W = any.hdr.W;
    if (rt::device_count() <= device) throw StatusError(LDBG_ERR_HIP, "no HIP device " + std::to_string(device) + " available (libldbg has no CPU fallback)");
    rt::set_device(device);
    const OwnStream own;
    rt::stream_t s = stream ? stream : own.s;

    std::vector<int64_t> off_host;
    if (on_device && n > 0) {                              // (the offsets are what sizes everything: they come to the host first)
        off_host.resize((size_t)n + 1);
        rt::d2h(off_host.data(), offsets, (size_t)(n + 1) * 8, s);
        rt::stream_sync(s);
        offsets = off_host.data();
    }
    // the windows, counted from the offsets alone
    win_start_.assign((size_t)n + 1, 0);
    std::vector<int64_t> seq_beg((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) throw StatusError(LDBG_ERR_ARG, "thread: the offsets decrease");
        const int64_t L = offsets[i + 1] - offsets[i];
        seq_beg[(size_t)i] = offsets[i] - offsets[0];
        win_start_[(size_t)i + 1] = win_start_[(size_t)i] + std::max<int64_t>(0, L - k + 1);
        if (win_start_[(size_t)i + 1] >= (1ll << 31)) throw StatusError(LDBG_ERR_UNSUPPORTED, "thread: 2^31 or more k-mer windows in one call");
    }
    const int64_t M = win_start_[(size_t)n];
    n_windows = M;
    first_.assign((size_t)n, -1); last_.assign((size_t)n, -1); n_hits_.assign((size_t)n, 0); n_distinct_.assign((size_t)n, 0);
    ends_.assign((size_t)n, 0); reg_off_.assign((size_t)n + 1, 0);
    if (M == 0) return;

    const int64_t L = offsets[n] - offsets[0], nwords = (L + 31) / 32;
    const bool want_copy = (fl & LDBG_THREAD_COPY_INDEX) != 0;
    d_rec_ = own_.get<int64_t>((size_t)M);
    d_info_ = own_.get<uint8_t>((size_t)M);
    if (want_copy) d_copy_ = own_.get<int32_t>((size_t)M);

    DevBlocks tmp;
    DevTimer tm;
    uint8_t* d_ascii = tmp.get<uint8_t>((size_t)nwords * 32);
    uint64_t* d_packed = tmp.get<uint64_t>((size_t)nwords);
    uint32_t* d_valid = tmp.get<uint32_t>((size_t)nwords);
    int64_t* d_seqs = tmp.get<int64_t>((size_t)(2 * n + 1));
    uint32_t* d_hit = tmp.get<uint32_t>((size_t)M);
    uint32_t* d_rrec = tmp.get<uint32_t>((size_t)M);
    uint32_t* d_seq = tmp.get<uint32_t>((size_t)M);
    unsigned* d_fl = tmp.get<unsigned>((size_t)(2 * n));
    uint32_t* d_H = tmp.get<uint32_t>((size_t)M + 1);
    uint32_t* d_head = tmp.get<uint32_t>((size_t)M);
    uint32_t* d_RH = tmp.get<uint32_t>((size_t)M + 1);
    const size_t maxchunks = (size_t)((M + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK) + 1;
    uint32_t* d_sums = tmp.get<uint32_t>(maxchunks);
    uint32_t* d_offs = tmp.get<uint32_t>(maxchunks + 1);
    const int P = W + 1;                                              // planes of a copy-index key
    uint64_t* d_planes = want_copy ? tmp.get<uint64_t>((size_t)M * (size_t)P) : nullptr;
    int32_t* d_so32 = tmp.get<int32_t>((size_t)(4 * n));             // first, last, hits, distinct
    uint8_t* d_ends = tmp.get<uint8_t>((size_t)n);
    int64_t* d_regoff = tmp.get<int64_t>((size_t)n + 1);

    rt::dmemset(d_ascii + L, 0, (size_t)(nwords * 32 - L), s);
    if (on_device) rt::d2d(d_ascii, bases + offsets[0], (size_t)L, s);
    else rt::h2d(d_ascii, bases + offsets[0], (size_t)L, s);
    rt::h2d(d_seqs, win_start_.data(), (size_t)(n + 1) * 8, s);
    rt::h2d(d_seqs + n + 1, seq_beg.data(), (size_t)n * 8, s);
    rt::dmemset(d_fl, 0xFF, (size_t)n * 4, s);
    rt::dmemset(d_fl + n, 0, (size_t)n * 4, s);
    GraphView gv = any.view, rv = any.view;
    if (g) gv = g->view;
    if (rois) rv = rois->view;
    if (!(fl & LDBG_THREAD_FIND_QUIRK)) gv.java_tiny = 0;
    rv.java_tiny = 0;                                                 // (membership in a HashSet filled by iteration: findRecord's quirk Q1 has no part in it)
    const int64_t* d_ws = d_seqs;
    const WinCtx x{d_packed, d_valid, d_ws, d_seqs + n + 1, n, M, k};
    const ThrOut o{d_rec_, d_info_, d_hit, d_rrec, d_seq, d_fl, d_fl + n, d_planes};
    tm.begin(s);
    LDBG_LAUNCH(k_bld_pack, grid_for(nwords), 256, s, (const uint8_t*)d_ascii, nwords, d_packed, d_valid);
    LDBG_LAUNCH(k_lnk_upper_only, grid_for(nwords), 256, s, (const uint8_t*)d_ascii, nwords, d_valid);
    LDBG_LAUNCH_W(W, k_thr_windows, grid_for(M), 256, s, x, gv, g ? 1 : 0, rv, rois ? 1 : 0, o);
    scan_u32(d_hit, M, d_H, d_sums, d_offs, s);
    LDBG_LAUNCH(k_thr_heads, grid_for(M), 256, s, d_ws, (const uint32_t*)d_seq, (const uint32_t*)d_hit, M, d_head);
    scan_u32(d_head, M, d_RH, d_sums, d_offs, s);
    uint32_t NH = 0, NR = 0;
    rt::d2h(&NH, d_H + M, 4, s);
    rt::d2h(&NR, d_RH + M, 4, s);
    tm.end(s);
    rt::stream_sync(s);
    tmp.drop(d_ascii); tmp.drop(d_packed); tmp.drop(d_valid);
    n_regions = NR;

    int32_t *d_rs = nullptr, *d_re = nullptr;
    uint32_t* d_DF = nullptr;
    if (NR > 0) {
        d_rs = tmp.get<int32_t>((size_t)NR);
        d_re = tmp.get<int32_t>((size_t)NR);
        tm.begin(s);
        LDBG_LAUNCH(k_thr_regions, grid_for(M), 256, s, d_ws, (const uint32_t*)d_seq, (const uint32_t*)d_hit, (const uint32_t*)d_head, (const uint32_t*)d_RH, M, d_rs, d_re);
        tm.end(s);
    }
    if (NH > 0) {                                                     // distinct ROI k-mers per sequence
        uint64_t* d_keys = tmp.get<uint64_t>((size_t)NH);
        uint32_t* d_perm = tmp.get<uint32_t>((size_t)NH);
        uint32_t* d_flag = tmp.get<uint32_t>((size_t)NH);
        d_DF = tmp.get<uint32_t>((size_t)NH + 1);
        tm.begin(s);
        LDBG_LAUNCH(k_thr_hit_keys, grid_for(M), 256, s, (const uint32_t*)d_seq, (const uint32_t*)d_hit, (const uint32_t*)d_rrec, (const uint32_t*)d_H, M, d_keys);
        radix_sort_permutation_dev(NH, 1, 32 + bits_for((uint64_t)(n - 1)), d_keys, d_perm, s);
        LDBG_LAUNCH(k_thr_run_heads, grid_for(NH), 256, s, (const uint64_t*)d_keys, 1, (const uint32_t*)d_perm, (int64_t)NH, d_flag);
        scan_u32(d_flag, NH, d_DF, d_sums, d_offs, s);
        tm.end(s);
        rt::stream_sync(s);
        tmp.drop(d_keys); tmp.drop(d_perm); tmp.drop(d_flag);
    }
    const SeqOut so{d_so32, d_so32 + n, d_so32 + 2 * n, d_so32 + 3 * n, d_ends, d_regoff};
    tm.begin(s);
    LDBG_LAUNCH(k_thr_seq, grid_for(n + 1), 256, s, d_ws, n, (const uint32_t*)d_hit, (const uint32_t*)d_H, (const uint32_t*)d_RH, (const uint32_t*)d_DF,
                (const unsigned*)d_fl, (const unsigned*)(d_fl + n), so);
    tm.end(s);
    rt::d2h(first_.data(), d_so32, (size_t)n * 4, s);
    rt::d2h(last_.data(), d_so32 + n, (size_t)n * 4, s);
    rt::d2h(n_hits_.data(), d_so32 + 2 * n, (size_t)n * 4, s);
    rt::d2h(n_distinct_.data(), d_so32 + 3 * n, (size_t)n * 4, s);
    rt::d2h(ends_.data(), d_ends, (size_t)n, s);
    rt::d2h(reg_off_.data(), d_regoff, (size_t)(n + 1) * 8, s);
    reg_start_.resize(NR); reg_stop_.resize(NR);
    if (NR > 0) {
        rt::d2h(reg_start_.data(), d_rs, (size_t)NR * 4, s);
        rt::d2h(reg_stop_.data(), d_re, (size_t)NR * 4, s);
    }
    rt::stream_sync(s);
    tmp.drop(d_hit); tmp.drop(d_rrec); tmp.drop(d_seq); tmp.drop(d_H); tmp.drop(d_head); tmp.drop(d_RH); tmp.drop(d_DF); tmp.drop(d_rs); tmp.drop(d_re);

    if (want_copy) {
        uint32_t* d_perm = tmp.get<uint32_t>((size_t)M);
        uint32_t* d_flag = tmp.get<uint32_t>((size_t)M);
        uint32_t* d_R = tmp.get<uint32_t>((size_t)M + 1);
        uint32_t* d_heads = tmp.get<uint32_t>((size_t)M);
        tm.begin(s);
        radix_sort_permutation_dev(M, P, 1 + bits_for((uint64_t)(n - 1)), d_planes, d_perm, s);
        LDBG_LAUNCH(k_thr_run_heads, grid_for(M), 256, s, (const uint64_t*)d_planes, P, (const uint32_t*)d_perm, M, d_flag);
        scan_u32(d_flag, M, d_R, d_sums, d_offs, s);
        LDBG_LAUNCH(k_thr_head_pos, grid_for(M), 256, s, (const uint32_t*)d_flag, (const uint32_t*)d_R, M, d_heads);
        LDBG_LAUNCH(k_thr_copy_index, grid_for(M), 256, s, (const uint64_t*)d_planes, (const uint32_t*)d_perm, (const uint32_t*)d_R, (const uint32_t*)d_heads, M, d_copy_);
        tm.end(s);
        rt::stream_sync(s);
    }
    device_ms = tm.ms;
    profile_add("thread", tm.ms);
}

void Threading::check_range(int64_t first, int64_t n, int64_t total, const char* what) const {
    if (first < 0 || n < 0 || first > total || n > total - first) throw StatusError(LDBG_ERR_ARG, std::string("thread: ") + what + " out of range");
}

void Threading::windows(int64_t first, int64_t n, int64_t* rec, uint8_t* info, int32_t* copy_index, bool device_out, rt::stream_t stream) const {
    check_range(first, n, n_windows, "windows");
    if (copy_index && !(flags & LDBG_THREAD_COPY_INDEX)) throw StatusError(LDBG_ERR_ARG, "thread: made without LDBG_THREAD_COPY_INDEX");
    if (n == 0) return;
    rt::set_device(device);
    const OwnStream own;
    rt::stream_t s = stream ? stream : own.s;
    auto out = [&](void* dst, const void* src, size_t nb) { if (device_out) rt::d2d(dst, src, nb, s); else rt::d2h(dst, src, nb, s); };
    if (rec) out(rec, d_rec_ + first, (size_t)n * 8);
    if (info) out(info, d_info_ + first, (size_t)n);
    if (copy_index) out(copy_index, d_copy_ + first, (size_t)n * 4);
    rt::stream_sync(s);
}

void Threading::coverage(int colour, int64_t first, int64_t n, int32_t* cov) const {
    check_range(first, n, n_windows, "windows");
    if (!graph) throw StatusError(LDBG_ERR_ARG, "thread: coverage without a graph");
    if (colour < 0 || colour >= graph->hdr.C) throw StatusError(LDBG_ERR_ARG, "thread: colour " + std::to_string(colour) + " out of range");
    if (n == 0) return;
    if (!cov) throw StatusError(LDBG_ERR_ARG, "thread: null output");
    rt::set_device(device);
    const OwnStream own;
    DevBlocks tmp;
    int32_t* d_cov = tmp.get<int32_t>((size_t)n);
    unsigned* d_miss = tmp.get<unsigned>(1);
    unsigned miss = 0;
    rt::dmemset(d_miss, 0, 4, own.s);
    LDBG_LAUNCH(k_thr_coverage, grid_for(n), 256, own.s, graph->view, colour, (const int64_t*)(d_rec_ + first), n, d_cov, d_miss);
    rt::d2h(&miss, d_miss, 4, own.s);
    rt::d2h(cov, d_cov, (size_t)n * 4, own.s);
    rt::stream_sync(own.s);
    // (cr.getCoverage(c) on the null findRecord returned: Coverage.java:41-42.  The coverages of the windows before it are in cov.)
    if (miss) throw StatusError(LDBG_ERR_NULLPOINTER, "thread: a window's k-mer has no record in the graph");
}

void Threading::summary(int64_t first_seq, int64_t n, int64_t* win_start, int32_t* first_hit, int32_t* last_hit, int32_t* n_hits, int32_t* n_distinct,
                        uint8_t* ends) const {
    check_range(first_seq, n, n_seqs, "sequences");
    const size_t f = (size_t)first_seq, c = (size_t)n;
    if (win_start) std::copy(win_start_.begin() + f, win_start_.begin() + f + c + 1, win_start);
    if (first_hit) std::copy(first_.begin() + f, first_.begin() + f + c, first_hit);
    if (last_hit) std::copy(last_.begin() + f, last_.begin() + f + c, last_hit);
    if (n_hits) std::copy(n_hits_.begin() + f, n_hits_.begin() + f + c, n_hits);
    if (n_distinct) std::copy(n_distinct_.begin() + f, n_distinct_.begin() + f + c, n_distinct);
    if (ends) std::copy(ends_.begin() + f, ends_.begin() + f + c, ends);
}

void Threading::regions(int64_t* region_offsets, int32_t* start, int32_t* stop, int64_t capacity) const {
    if (region_offsets) std::copy(reg_off_.begin(), reg_off_.end(), region_offsets);
    if (capacity < n_regions) throw StatusError(LDBG_ERR_CAPACITY, "thread: " + std::to_string(n_regions) + " regions");
    if (n_regions > 0 && (!start || !stop)) throw StatusError(LDBG_ERR_ARG, "thread: null output");
    std::copy(reg_start_.begin(), reg_start_.end(), start);
    std::copy(reg_stop_.begin(), reg_stop_.end(), stop);
}

}  // namespace ldbg
