// Graph construction on the device (build.h): the uploaded ASCII packed to 2-bit words with a validity bit per base ->
// one window per lane: the k-mer by shifts out of the packed words, its canonical form as key planes, colour and edge byte as a
// 16-bit tag -> the stable radix sort of sort.cpp over the key planes -> run heads (one 64-bit ballot per 64 sorted windows, one
// count per chunk, the chunk counts scanned by one wavefront: wavescan.h) -> every run reduced to coverages and edge
// bytes -> the records staged in LDS and written in the file's layout.  No kernel waits for another workgroup.  The sort is stable
// and the windows are numbered sample by sample, so the windows of a run arrive colour by colour: a wavefront sums each stretch of
// one (record, colour) among its 64 windows with ballots and issues one atomic add and one atomic OR per stretch — a k-mer seen
// 100,000 times costs 1,600 atomics, spread over as many wavefronts.  Sums and ORs of integers do not depend on the order of arrival.
// The TEST-ONLY host simulation runs the kernels as they are.
#include "build.h"
#include "bldpack.h"
#include "wavescan.h"

#include <stdio.h>

#include <algorithm>
#include <set>

namespace ldbg {

namespace {

#define BLD_GROUPS (LDBG_BUILD_CHUNK / 64)
#define BLD_STAGE_WORDS LDBG_STAGE_WORDS(LDBG_MAX_COLORS)

struct ExtractCtx {
    const uint64_t* packed;
    const uint32_t* valid;
    const int64_t* win_start;      // [nseq + 1] first window of every sequence (each has at least one), win_start[nseq] = M
    const int64_t* seq_beg;        // [nseq] first and one past the last byte of the sequence in the uploaded text
    const int64_t* seq_end;
    const uint8_t* colour;         // [nseq]
    int64_t nseq, M;
    int k;
};

// one window per lane: keys[w][m] = word w of the canonical k-mer of window m, tags[m] = colour << 8 | edge byte of the window as
// CortexRecord stores it (in-edge base X: bit 7 - X, out-edge base X: bit X, both complemented and swapped when the k-mer is
// flipped).  Neighbouring lanes read the same or the next packed words and write neighbouring elements of every plane.  *bad is set
// when a window holds a byte that is no base.
template <int W>
LDBG_KERNEL void k_bld_extract(ExtractCtx x, uint64_t* keys, uint16_t* tags, unsigned* bad) {
    bool miss = false;
    for (int64_t m = global_tid(); m < x.M; m += global_nthreads()) {
        int64_t lo = 0, hi = x.nseq;                       // win_start[lo] <= m < win_start[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (x.win_start[mid] <= m) lo = mid; else hi = mid;
        }
        const int64_t i = m - x.win_start[lo], beg = x.seq_beg[lo], g = beg + i, end = x.seq_end[lo];
        const int64_t E = 2 * (g + x.k), wi = (E - 1) >> 6;
        const int r = (int)(E - 64 * wi);                  // 2..64: bits of packed word wi that end the k-mer
        uint64_t pw[W + 1];
#pragma unroll
        for (int j = 0; j <= W; j++) pw[j] = wi - j >= 0 ? x.packed[wi - j] : 0ull;
        Kmer<W> a;
#pragma unroll
        for (int j = 0; j < W; j++) a.w[W - 1 - j] = r == 64 ? pw[j] : (pw[j] >> (64 - r)) | (pw[j + 1] << r);
        const int top = 2 * x.k - 64 * (W - 1);
        if (top < 64) a.w[0] &= (1ull << top) - 1ull;
        for (int64_t j = g >> 5; j <= (g + x.k - 1) >> 5; j++) {
            const int b0 = (int)(std::max<int64_t>(g, 32 * j) - 32 * j), b1 = (int)(std::min<int64_t>(g + x.k, 32 * j + 32) - 32 * j);
            const uint32_t mask = (b1 == 32 ? ~0u : (1u << b1) - 1u) & ~((1u << b0) - 1u);
            if (~x.valid[j] & mask) miss = true;
        }
        bool f;
        const Kmer<W> c = kmer_canonical<W>(a, x.k, &f);
        const int pb = i > 0 ? (int)bld_base(x.packed, g - 1) : -1, nb = g + x.k < end ? (int)bld_base(x.packed, g + x.k) : -1;
        unsigned e = 0;
        if (!f) { if (pb >= 0) e |= 1u << (7 - pb); if (nb >= 0) e |= 1u << nb; }
        else { if (nb >= 0) e |= 1u << (4 + nb); if (pb >= 0) e |= 1u << (3 - pb); }
#pragma unroll
        for (int w = 0; w < W; w++) keys[(size_t)w * (size_t)x.M + (size_t)m] = c.w[w];
        tags[m] = (uint16_t)(((unsigned)x.colour[lo] << 8) | e);
    }
    if (miss) atomic_or_u32(bad, 1u);
}

// ballots[g] bit b: sorted window 64 g + b starts a run of equal k-mers; chunk_cnt[ch]: runs that start in chunk ch
template <int W>
LDBG_WAVE_KERNEL void k_bld_heads(const uint64_t* keys, const uint32_t* perm, int64_t M, unsigned long long* ballots, uint32_t* chunk_cnt) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (M + LDBG_BUILD_CHUNK - 1) / LDBG_BUILD_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_BUILD_CHUNK;
        const int lim = chunk_lim(M, c0, LDBG_BUILD_CHUNK);
        unsigned long long cur[1] = {0};
        uint32_t cnt = 0;
        for (int t = 0; t < lim; t += ws) {
            const int64_t p = c0 + t + lane;
            bool head = false;
            if (p < M) {
                head = p == 0;
                if (p > 0) {
                    const size_t a = perm[p], b = perm[p - 1];
#pragma unroll
                    for (int w = 0; w < W; w++) head |= keys[(size_t)w * (size_t)M + a] != keys[(size_t)w * (size_t)M + b];
                }
            }
            cnt += ballot_step(c0, t, {head}, cur, {ballots});
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();
}

// cov[r][c] += windows, edges[r][c] |= edge bytes of colour c in run r; first_win[r] = the run's first window (its k-mer).
// A run's record number is the number of heads up to its windows; among a wavefront's windows each stretch of one (record, colour)
// is summed with ballots and its first lane issues the atomics (cov and edges are zeroed; edges: one byte per entry, ORed as dwords).
LDBG_WAVE_KERNEL void k_bld_reduce(const uint16_t* tags, const uint32_t* perm, int64_t M, int C, const unsigned long long* ballots,
                                   const unsigned long long* chunk_off, uint32_t* first_win, uint32_t* cov, uint32_t* edges) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (M + LDBG_BUILD_CHUNK - 1) / LDBG_BUILD_CHUNK;
    const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane), wsmask = ws == 64 ? ~0ull : (1ull << ws) - 1ull;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_BUILD_CHUNK;
        const int lim = chunk_lim(M, c0, LDBG_BUILD_CHUNK);
        unsigned long long run = chunk_off[ch];            // runs that start before this step's windows
        for (int t = 0; t < lim; t += ws) {
            const int64_t p = c0 + t + lane;
            const bool live = p < M;
            const unsigned long long hm = (ballots[(c0 + t) >> 6] >> (t & 63)) & wsmask;
            const bool head = (hm >> lane) & 1ull;
            const uint32_t win = live ? perm[p] : 0u, tag = live ? (uint32_t)tags[win] : 0u, col = tag >> 8;
            const uint32_t prev = wave_shfl_u32(col, lane - 1);
            const unsigned long long bnd = wave_ballot(live && (head || lane == 0 || col != prev)), lv = wave_ballot(live);
            const unsigned long long above = bnd & ~upto;
            const int end = above ? __builtin_ctzll(above) : __builtin_popcountll(lv);      // the stretch is lanes [lane, end)
            const unsigned long long seg = (end >= 64 ? ~0ull : (1ull << end) - 1ull) & ~below;
            uint32_t e = 0;
#pragma unroll
            for (int b = 0; b < 8; b++) e |= (wave_ballot((tag >> b) & 1u) & seg) ? 1u << b : 0u;
            if (live && ((bnd >> lane) & 1ull)) {
                const unsigned long long rec = run + (unsigned)__builtin_popcountll(hm & upto) - 1ull;
                const size_t idx = (size_t)rec * (size_t)C + col;
                atomic_add_u32(&cov[idx], (uint32_t)(end - lane));
                if (e) atomic_or_u32(&edges[idx >> 2], e << (8 * (idx & 3)));
                if (head) first_win[rec] = win;
            }
            run += (unsigned)__builtin_popcountll(hm);
        }
    }
    wave_fence();
}

// CortexGraphWriter.addRecord (CortexGraphWriter.java:115-138) of every run: 8W k-mer bytes | 4C coverage bytes | C edge bytes.  Records
// leave through the LDS stage of wavescan.h
template <int W>
LDBG_WAVE_KERNEL void k_bld_records(const uint64_t* keys, int64_t M, const uint32_t* first_win, const uint32_t* cov, const uint8_t* edges, int C,
                                    int64_t N, uint8_t* out) {
#ifndef LDBG_HOSTSIM
    __shared__ uint32_t stage[BLD_STAGE_WORDS];
#else
    static uint32_t stage[BLD_STAGE_WORDS];          // (one simulated wavefront at a time: rt.h)
#endif
    const int ws = LDBG_WS, lane = wave_lane(), R = 8 * W + 5 * C;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nb = (N + ws - 1) / ws;
    for (int64_t b = wave; b < nb; b += nwaves) {
        const int64_t first = b * ws;
        const int nrec = (int)std::min<int64_t>(ws, N - first);
        uint8_t* dst = out + (size_t)first * (size_t)R;
        uint8_t* lb = stage_bytes(stage, dst);
        if (lane < nrec) {
            const size_t r = (size_t)(first + lane), win = first_win[r];
            uint8_t* p = lb + lane * R;
#pragma unroll
            for (int w = 0; w < W; w++) { const uint64_t v = keys[(size_t)w * (size_t)M + win]; __builtin_memcpy(p + 8 * w, &v, 8); }
            for (int c = 0; c < C; c++) {
                const uint32_t v = cov[r * (size_t)C + c];
                __builtin_memcpy(p + 8 * W + 4 * c, &v, 4);
                p[8 * W + 4 * C + c] = edges[r * (size_t)C + c];
            }
        }
        stage_write_out(stage, dst, nrec, R);
    }
}

bool is_base(uint8_t c) { c &= 0xDFu; return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

}  // namespace

BuiltRecords build_records(const ldbg_build_sample* samples, int n_samples, int k, int flags, int device) {
    if (!samples || n_samples < 1) throw StatusError(LDBG_ERR_ARG, "build: no samples");
    if (n_samples > LDBG_MAX_COLORS) throw StatusError(LDBG_ERR_ARG, "build: more than " + std::to_string(LDBG_MAX_COLORS) + " samples (colours)");
    if (k < 3 || k > 128) throw StatusError(LDBG_ERR_ARG, "build: k-mer size " + std::to_string(k) + " outside 3..128");
    if (flags & ~LDBG_BUILD_SPLIT_NON_ACGT) throw StatusError(LDBG_ERR_ARG, "build: unknown flag");
    const bool split = (flags & LDBG_BUILD_SPLIT_NON_ACGT) != 0;
    std::set<std::string> names;
    for (int c = 0; c < n_samples; c++) {
        const ldbg_build_sample& sm = samples[c];
        if (!sm.sample_name) throw StatusError(LDBG_ERR_ARG, "build: sample " + std::to_string(c) + " has no name");
        if (!names.insert(sm.sample_name).second) throw StatusError(LDBG_ERR_ARG, std::string("build: two samples are called '") + sm.sample_name + "'");
        if (sm.n_sequences < 0 || (sm.n_sequences > 0 && (!sm.offsets || !sm.bases))) throw StatusError(LDBG_ERR_ARG, "build: sample " + std::to_string(c) + " has sequences but no text or offsets");
        for (int64_t i = 0; i < sm.n_sequences; i++)
            if (sm.offsets[i] < 0 || sm.offsets[i + 1] < sm.offsets[i]) throw StatusError(LDBG_ERR_ARG, "build: the offsets of sample " + std::to_string(c) + " decrease");
    }
    // the windows, numbered sample by sample, sequence by sequence: (first byte in the uploaded text, one past the last, colour) of
    // every stretch that holds a window.  Upload position of sample c's text: text0[c].
    std::vector<int64_t> text0((size_t)n_samples + 1, 0), win_start{0}, seq_beg, seq_end;
    std::vector<uint8_t> colour;
    auto stretch = [&](int c, int64_t beg, int64_t end) {      // bytes [beg, end) of sample c's text
        if (end - beg < k) return;
        seq_beg.push_back(text0[(size_t)c] + beg - samples[c].offsets[0]);
        seq_end.push_back(text0[(size_t)c] + end - samples[c].offsets[0]);
        colour.push_back((uint8_t)c);
        win_start.push_back(win_start.back() + (end - beg - k + 1));
    };
    for (int c = 0; c < n_samples; c++) {
        const ldbg_build_sample& sm = samples[c];
        const int64_t ns = sm.n_sequences;
        text0[(size_t)c + 1] = text0[(size_t)c] + (ns > 0 ? sm.offsets[ns] - sm.offsets[0] : 0);
        for (int64_t i = 0; i < ns; i++) {
            if (!split) { stretch(c, sm.offsets[i], sm.offsets[i + 1]); continue; }
            int64_t from = sm.offsets[i];                       // LDBG_BUILD_SPLIT_NON_ACGT: every other byte ends a stretch
            for (int64_t j = from; j <= sm.offsets[i + 1]; j++)
                if (j == sm.offsets[i + 1] || !is_base((uint8_t)sm.bases[j])) { stretch(c, from, j); from = j + 1; }
        }
        // (checked as the count grows and before anything is allocated: the sort numbers windows in 32 bits)
        if (win_start.back() >= (1ll << 32))
            throw StatusError(LDBG_ERR_UNSUPPORTED, "build: 2^32 or more k-mer windows in one call (build in batches and Join them)");
    }
    const int64_t M = win_start.back(), L = text0[(size_t)n_samples], nseq = (int64_t)seq_beg.size();
    const int W = (k + 31) / 32, C = n_samples;
    if (rt::device_count() <= device) throw StatusError(LDBG_ERR_HIP, "no HIP device " + std::to_string(device) + " available (libldbg has no CPU fallback)");

    BuiltRecords out;
    out.device = device;
    out.hdr.version = 6; out.hdr.k = k; out.hdr.W = W; out.hdr.C = C;
    out.hdr.colors.resize((size_t)C);
    for (int c = 0; c < C; c++) out.hdr.colors[(size_t)c].sample_name = samples[c].sample_name;
    out.hdr.record_size = 8LL * W + 5LL * C;
    out.header = serialize_ctx_header(out.hdr);
    out.hdr.data_offset = (int64_t)out.header.size();
    if (M == 0) return out;

    rt::set_device(device);
    DevBlocks tmp;
    const OwnStream own;
    rt::stream_t s = own.s;
    double ms_extract = 0, ms_sort = 0, ms_reduce = 0, ms_pack = 0;
    rt::Event e0, e1, e2, e3, e4, e5, e6, e7;
    const int64_t nwords = (L + 31) / 32;
    uint8_t* d_ascii = tmp.get<uint8_t>((size_t)nwords * 32);
    uint64_t* d_packed = tmp.get<uint64_t>((size_t)nwords);
    uint32_t* d_valid = tmp.get<uint32_t>((size_t)nwords);
    int64_t* d_seqs = tmp.get<int64_t>((size_t)(3 * nseq + 1));
    uint8_t* d_colour = tmp.get<uint8_t>((size_t)nseq);
    uint64_t* d_keys = tmp.get<uint64_t>((size_t)M * W);
    uint16_t* d_tags = tmp.get<uint16_t>((size_t)M);
    uint32_t* d_perm = tmp.get<uint32_t>((size_t)M);
    unsigned long long* d_stat = tmp.get<unsigned long long>(2);          // [0] records, [1] a window with a byte that is no base
    rt::dmemset(d_ascii + L, 0, (size_t)(nwords * 32 - L), s);
    for (int c = 0; c < C; c++)
        if (samples[c].n_sequences > 0)
            rt::h2d(d_ascii + text0[(size_t)c], samples[c].bases + samples[c].offsets[0], (size_t)(text0[(size_t)c + 1] - text0[(size_t)c]), s);
    rt::h2d(d_seqs, win_start.data(), (size_t)(nseq + 1) * 8, s);
    rt::h2d(d_seqs + nseq + 1, seq_beg.data(), (size_t)nseq * 8, s);
    rt::h2d(d_seqs + 2 * nseq + 1, seq_end.data(), (size_t)nseq * 8, s);
    rt::h2d(d_colour, colour.data(), (size_t)nseq, s);
    rt::dmemset(d_stat, 0, 16, s);
    e0.record(s);
    LDBG_LAUNCH(k_bld_pack, grid_for(nwords), 256, s, (const uint8_t*)d_ascii, nwords, d_packed, d_valid);
    const ExtractCtx x{d_packed, d_valid, d_seqs, d_seqs + nseq + 1, d_seqs + 2 * nseq + 1, d_colour, nseq, M, k};
    LDBG_LAUNCH_W(W, k_bld_extract, grid_for(M), 256, s, x, d_keys, d_tags, (unsigned*)(d_stat + 1));
    e1.record(s);
    unsigned long long st[2] = {0, 0};
    rt::d2h(st, d_stat, 16, s);
    rt::stream_sync(s);
    ms_extract = rt::Event::elapsed_ms(e0, e1);
    // CortexRecord.encodeBinaryKmer -> charToBinaryNucleotide (CortexRecord.java:347-360) throws on the first such k-mer
    if (st[1] & 0xFFFFFFFFull) throw StatusError(LDBG_ERR_CORTEXJDK, "Nucleotide is not a valid character nucleotide (a sequence holds a byte other than ACGTacgt)");
    tmp.drop(d_ascii); tmp.drop(d_valid); tmp.drop(d_seqs); tmp.drop(d_colour); tmp.drop(d_packed);

    e2.record(s);
    radix_sort_permutation_dev(M, W, 2 * k - 64 * (W - 1), d_keys, d_perm, s);
    e3.record(s);

    const int64_t nchunks = (M + LDBG_BUILD_CHUNK - 1) / LDBG_BUILD_CHUNK;
    unsigned long long* d_ballots = tmp.get<unsigned long long>((size_t)nchunks * BLD_GROUPS);
    uint32_t* d_cnt = tmp.get<uint32_t>((size_t)nchunks);
    unsigned long long* d_off = tmp.get<unsigned long long>((size_t)nchunks);
    e4.record(s);
    LDBG_LAUNCH_W(W, k_bld_heads, waves_for(nchunks), 64, s, (const uint64_t*)d_keys, (const uint32_t*)d_perm, M, d_ballots, d_cnt);
    LDBG_LAUNCH(k_chunk_top<unsigned long long>, 1, 64, s, nchunks, (const uint32_t*)d_cnt, d_off, d_stat);
    rt::d2h(st, d_stat, 8, s);
    rt::stream_sync(s);
    const int64_t N = (int64_t)st[0];
    check_record_count(N, "<build>");
    const size_t cells = (size_t)N * (size_t)C;
    uint32_t* d_first = tmp.get<uint32_t>((size_t)N);
    uint32_t* d_cov = tmp.get<uint32_t>(cells);
    uint32_t* d_edges = tmp.get<uint32_t>((cells + 3) / 4);
    rt::dmemset(d_cov, 0, cells * 4, s);
    rt::dmemset(d_edges, 0, (cells + 3) / 4 * 4, s);
    LDBG_LAUNCH(k_bld_reduce, waves_for(nchunks), 64, s, (const uint16_t*)d_tags, (const uint32_t*)d_perm, M, C, (const unsigned long long*)d_ballots,
                (const unsigned long long*)d_off, d_first, d_cov, d_edges);
    e5.record(s);
    rt::stream_sync(s);
    tmp.drop(d_tags); tmp.drop(d_perm); tmp.drop(d_ballots);
    out.d_records.reset((uint8_t*)rt::dmalloc((size_t)N * (size_t)out.hdr.record_size));
    e6.record(s);
    LDBG_LAUNCH_W(W, k_bld_records, waves_for((N + 63) / 64), 64, s, (const uint64_t*)d_keys, M, (const uint32_t*)d_first, (const uint32_t*)d_cov,
                  (const uint8_t*)d_edges, C, N, out.d_records.get());
    e7.record(s);
    rt::stream_sync(s);
    ms_sort = rt::Event::elapsed_ms(e2, e3);
    ms_reduce = rt::Event::elapsed_ms(e4, e5);
    ms_pack = rt::Event::elapsed_ms(e6, e7);
    profile_add("build_extract", ms_extract);
    profile_add("build_sort", ms_sort);
    profile_add("build_reduce", ms_reduce);
    profile_add("build_pack", ms_pack);
    profile_add("build", ms_extract + ms_sort + ms_reduce + ms_pack);
    out.N = N;
    out.hdr.num_records = N;
    return out;
}

void build_write_ctx(const BuiltRecords& b, const std::string& out_path) {
    rt::set_device(b.device);
    const OwnStream own;
    write_records_file(b.header, b.d_records.get(), (size_t)b.N * (size_t)b.hdr.record_size, b.device, own.s, out_path);
}

}  // namespace ldbg
