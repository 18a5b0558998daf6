// Record selection on the device (select.h): a streaming pass over the coverage and edge planes the filter names ->
// one 64-bit ballot per 64 records and one count per chunk -> exclusive scan of the chunk counts by one wavefront -> the record
// numbers scattered in record order from the ballots -> the selected records gathered into the file's record layout.  Every
// kernel is launched one wavefront per workgroup and uses wavefront primitives only; no workgroup waits for another, nothing is
// placed with an atomic, so the result is the same from run to run.  The TEST-ONLY host simulation runs the kernels as they are
// (a simulated wavefront may be narrower than 64 lanes: the kernels assemble a ballot word from 64 / lanes ballots then).
#include "select.h"

#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>

namespace ldbg {

namespace {

#ifdef LDBG_HOSTSIM
#define SEL_WS wave_size()
#else
#define SEL_WS 64              // (every kernel here is launched with 64-thread workgroups)
#endif
#define SEL_UNROLL 8           // ballots per step of a wavefront: independent loads in flight per plane
#define SEL_GROUPS (LDBG_SELECT_CHUNK / 64)
static_assert(SEL_GROUPS == 64, "k_sel_scatter gives a wavefront one ballot word per lane");

struct SelCtx {
    const uint32_t* cov;       // [C][N] of the graph the filter reads
    const uint8_t* edges;
    int64_t N;
    uint64_t all_zero, all_positive, any_positive, none_positive;
    uint64_t cov_planes;       // colours whose coverage plane is read
    int cov_color, cov_below, degree_color, degree_above;
};

// ballots[g] bit b: record 64 g + b passes; chunk_cnt[ch]: records of chunk ch that pass.  via (FindShared): the record of the
// filter's graph for each of the n records, -1 = none (*null_seen is set, the record does not pass)
LDBG_WAVE_KERNEL void k_sel_mask(SelCtx x, int64_t n, const int64_t* via, unsigned* null_seen, unsigned long long* ballots, uint32_t* chunk_cnt) {
    const int ws = SEL_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    bool miss = false;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SELECT_CHUNK;
        const int lim = (int)std::min<int64_t>(LDBG_SELECT_CHUNK, (n - c0 + 63) & ~(int64_t)63);
        unsigned long long cur = 0;
        uint32_t cnt = 0;
        for (int t = 0; t < lim; t += SEL_UNROLL * ws) {
            int64_t rec[SEL_UNROLL];
            bool ok[SEL_UNROLL], anyp[SEL_UNROLL];
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; j++) {
                const int64_t i = c0 + t + j * ws + lane;
                ok[j] = i < n; anyp[j] = false; rec[j] = i;
                if (via && ok[j]) {
                    rec[j] = LDBG_GLOBAL(const int64_t, via)[i];
                    if (rec[j] < 0) { ok[j] = false; miss = true; }
                }
            }
            for (uint64_t m = x.cov_planes; m; m &= m - 1) {
                const int c = __builtin_ctzll(m);
                const uint32_t* plane = x.cov + (size_t)c * (size_t)x.N;
                const bool z = (x.all_zero >> c) & 1ull, p = (x.all_positive >> c) & 1ull, a = (x.any_positive >> c) & 1ull,
                           np = (x.none_positive >> c) & 1ull, lt = c == x.cov_color;
                int32_t v[SEL_UNROLL];
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) v[j] = ok[j] ? (int32_t)LDBG_GLOBAL(const uint32_t, plane)[rec[j]] : 0;
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) {      // CortexRecord.getCoverage: the Java int
                    if ((z && v[j] != 0) || (p && v[j] <= 0) || (np && v[j] > 0) || (lt && v[j] >= x.cov_below)) ok[j] = false;
                    if (a && v[j] > 0) anyp[j] = true;
                }
            }
            if (x.any_positive) {
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) ok[j] = ok[j] && anyp[j];
            }
            if (x.degree_color >= 0) {
                const uint8_t* plane = x.edges + (size_t)x.degree_color * (size_t)x.N;
                uint32_t e[SEL_UNROLL];
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) e[j] = ok[j] ? (uint32_t)LDBG_GLOBAL(const uint8_t, plane)[rec[j]] : 0u;
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) ok[j] = ok[j] && __builtin_popcount(e[j]) > x.degree_above;
            }
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; j++) {
                const int s = t + j * ws;
                if (s >= lim) break;
                cur |= wave_ballot(ok[j]) << (s & 63);
                if (((s + ws) & 63) == 0) {
                    if (lane == 0) ballots[(c0 + s) >> 6] = cur;
                    cnt += (uint32_t)__builtin_popcountll(cur);
                    cur = 0;
                }
            }
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();      // (host simulation: a lane that has left the kernel counts as inactive in a ballot the others have yet to read)
    if (miss) atomic_or_u32(null_seen, 1u);
}

// exclusive prefix sums of the chunk counts, by one wavefront
LDBG_WAVE_KERNEL void k_sel_top(int64_t nchunks, const uint32_t* chunk_cnt, unsigned long long* chunk_off, unsigned long long* total) {
    const int ws = SEL_WS, lane = wave_lane();
    if (global_tid() / ws != 0) return;
    unsigned long long run = 0;
    for (int64_t b = 0; b < nchunks; b += ws) {
        const int64_t i = b + lane;
        const uint32_t v = i < nchunks ? chunk_cnt[i] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v);
        if (i < nchunks) chunk_off[i] = run + incl - v;
        run += wave_bcast_u32(incl, ws - 1);
    }
    wave_fence();
    if (lane == 0) *total = run;
}

// out[chunk_off[ch] + rank of the record among the chunk's passing records] = record, read back from the ballots
LDBG_WAVE_KERNEL void k_sel_scatter(int64_t n, const unsigned long long* ballots, const unsigned long long* chunk_off, uint32_t* out) {
    const int ws = SEL_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    const int64_t ngroups = (n + 63) >> 6, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        unsigned long long run = chunk_off[ch];
        for (int g0 = 0; g0 < SEL_GROUPS && ch * SEL_GROUPS + g0 < ngroups; g0 += ws) {
            const int64_t g = ch * SEL_GROUPS + g0 + lane;
            const unsigned long long m = g < ngroups ? ballots[g] : 0ull;
            const uint32_t c = (uint32_t)__builtin_popcountll(m), incl = wave_incl_scan_u32(c);
            const unsigned long long base = run + incl - c;
            for (int jj = 0; jj < ws; jj++) {
                const unsigned long long mj = wave_bcast_u64(m, jj);
                if (!mj) continue;
                const unsigned long long bj = wave_bcast_u64(base, jj);
                for (int bit = lane; bit < 64; bit += ws)
                    if ((mj >> bit) & 1ull)
                        out[bj + (unsigned)__builtin_popcountll(mj & ((1ull << bit) - 1ull))] = (uint32_t)(((ch * SEL_GROUPS + g0 + jj) << 6) + bit);
            }
            run += wave_bcast_u32(incl, ws - 1);
        }
    }
    wave_fence();
}

LDBG_KERNEL void k_sel_widen(const uint32_t* in, int64_t n, int64_t* out) {
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) out[i] = (int64_t)in[i];
}

struct PackCtx {
    GraphView g;
    int nproj;
    uint8_t proj[LDBG_SELECT_MAX_PROJ];
};
#define SEL_STAGE_WORDS (64 * (32 + 5 * LDBG_SELECT_MAX_PROJ) / 4 + 2)

// CortexGraphWriter.addRecord (CortexGraphWriter.java:115-138) of the selected records: 8W k-mer bytes | 4C' coverage bytes | C' edge
// bytes each, from the record's probe row (one or two lines hold all of it).  Records are 13, 21, 29 ... bytes: a wavefront stages
// its records in LDS, shifted so that LDS and output agree modulo 4, and writes the stretch out as whole dwords.
template <int W>
LDBG_WAVE_KERNEL void k_sel_pack(PackCtx x, const uint32_t* idx, int64_t count, uint8_t* out) {
#ifndef LDBG_HOSTSIM
    __shared__ uint32_t stage[SEL_STAGE_WORDS];
#else
    static uint32_t stage[SEL_STAGE_WORDS];          // (one simulated wavefront at a time: rt.h)
#endif
    const int ws = SEL_WS, lane = wave_lane(), R = 8 * W + 5 * x.nproj;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nb = (count + ws - 1) / ws;
    for (int64_t b = wave; b < nb; b += nwaves) {
        const int64_t first = b * ws;
        const int nrec = (int)std::min<int64_t>(ws, count - first);
        uint8_t* dst = out + (size_t)first * (size_t)R;
        const int mis = (int)((uintptr_t)dst & 3u);
        uint8_t* lb = (uint8_t*)stage + mis;
        if (lane < nrec) {
            const uint8_t* row = graph_row(x.g, (int64_t)idx[first + lane]);
            uint8_t* p = lb + lane * R;
#pragma unroll
            for (int w = 0; w < W; w++) { const uint64_t v = ((const uint64_t*)row)[w]; __builtin_memcpy(p + 8 * w, &v, 8); }
            for (int c = 0; c < x.nproj; c++) {
                const uint32_t v = ((const uint32_t*)(row + x.g.cov_off))[x.proj[c]];
                __builtin_memcpy(p + 8 * W + 4 * c, &v, 4);
                p[8 * W + 4 * x.nproj + c] = row[x.g.edges_off + x.proj[c]];
            }
        }
        wave_fence();
        const int nbytes = nrec * R, head = mis ? std::min(nbytes, 4 - mis) : 0, nd = (nbytes - head) >> 2;
        for (int i = lane; i < head; i += ws) dst[i] = lb[i];
        const uint32_t* ls = stage + ((mis + head) >> 2);
        uint32_t* gd = (uint32_t*)(dst + head);
        for (int i = lane; i < nd; i += ws) gd[i] = ls[i];
        for (int i = head + 4 * nd + lane; i < nbytes; i += ws) dst[i] = lb[i];
        wave_fence();                                  // (the next stretch overwrites the stage)
    }
}

// ---- RecoverExcludedKmers: the selection above with a join.  The pass over the coverage planes makes TWO ballots per 64
// records — kept (the child colour has coverage) and candidate (it has none, another colour has) —, the candidates are compacted by the
// scan and scatter above, their k-mers are looked up in DIRTY by the findRecord kernel, and the candidates DIRTY covers join the kept
// ballots before the second scan.  The second scatter writes the record numbers and, beside them, the child's coverage after the patch.
struct RecCtx {
    const uint32_t* cov;       // [C][N] of GRAPH
    int64_t N;
    int C, child;
};

// kept[g] bit b: record 64 g + b has coverage in the child colour; cand[g] bit b: it has none and some other colour has; cand_cnt[ch]:
// candidates of chunk ch.  Coverage is CortexRecord.getCoverage: the Java int.
LDBG_WAVE_KERNEL void k_rec_classify(RecCtx x, unsigned long long* kept, unsigned long long* cand, uint32_t* cand_cnt) {
    const int ws = SEL_WS, lane = wave_lane();
    const int64_t n = x.N, wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SELECT_CHUNK;
        const int lim = (int)std::min<int64_t>(LDBG_SELECT_CHUNK, (n - c0 + 63) & ~(int64_t)63);
        unsigned long long cur_k = 0, cur_c = 0;
        uint32_t cnt = 0;
        for (int t = 0; t < lim; t += SEL_UNROLL * ws) {
            bool in[SEL_UNROLL], kp[SEL_UNROLL], other[SEL_UNROLL];
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; j++) { in[j] = c0 + t + j * ws + lane < n; kp[j] = false; other[j] = false; }
            for (int c = 0; c < x.C; c++) {
                const uint32_t* plane = x.cov + (size_t)c * (size_t)x.N + (size_t)(c0 + t + lane);
                const bool child = c == x.child;
                int32_t v[SEL_UNROLL];
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) v[j] = in[j] ? (int32_t)LDBG_GLOBAL(const uint32_t, plane)[j * ws] : 0;
#pragma unroll
                for (int j = 0; j < SEL_UNROLL; j++) {
                    if (v[j] > 0 && child) kp[j] = true;
                    if (v[j] > 0 && !child) other[j] = true;
                }
            }
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; j++) {
                const int s = t + j * ws;
                if (s >= lim) break;
                cur_k |= wave_ballot(kp[j]) << (s & 63);
                cur_c |= wave_ballot(!kp[j] && other[j]) << (s & 63);
                if (((s + ws) & 63) == 0) {
                    if (lane == 0) { kept[(c0 + s) >> 6] = cur_k; cand[(c0 + s) >> 6] = cur_c; }
                    cnt += (uint32_t)__builtin_popcountll(cur_c);
                    cur_k = 0; cur_c = 0;
                }
            }
        }
        if (lane == 0) cand_cnt[ch] = cnt;
    }
    wave_fence();
}

// cr.getCanonicalKmer() of the candidates, as the findRecord kernel takes its queries: words[i * W + w]
LDBG_KERNEL void k_rec_keys(const uint64_t* keys, int64_t N, int W, const uint32_t* idx, int64_t n, uint64_t* words) {
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) {
        const size_t r = idx[i];
        for (int w = 0; w < W; w++) words[i * W + w] = keys[(size_t)w * (size_t)N + r];
    }
}

// dr != null && dr.getCoverage(0) > 0 of every candidate (dcov[j * dC]: DIRTY's colour-0 coverage of the j-th candidate's k-mer as the
// findRecord kernel reports it, 0 without a record): the bit joins the kept ballots IN PLACE.  chunk_cnt[ch]: written records of chunk ch;
// *n_rec: candidates recovered (a sum: the order of the additions does not show)
LDBG_WAVE_KERNEL void k_rec_merge(int64_t n, unsigned long long* kept, const unsigned long long* cand, const unsigned long long* cand_off,
                                  const uint32_t* dcov, int dC, uint32_t* chunk_cnt, unsigned long long* n_rec) {
    const int ws = SEL_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    const int64_t ngroups = (n + 63) >> 6, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    unsigned long long rec = 0;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        unsigned long long run = cand_off[ch];
        uint32_t cnt = 0;
        for (int g0 = 0; g0 < SEL_GROUPS && ch * SEL_GROUPS + g0 < ngroups; g0 += ws) {
            const int64_t g = ch * SEL_GROUPS + g0 + lane;
            const unsigned long long m = g < ngroups ? cand[g] : 0ull;
            unsigned long long kp = g < ngroups ? kept[g] : 0ull;
            const uint32_t c = (uint32_t)__builtin_popcountll(m), incl = wave_incl_scan_u32(c);
            unsigned long long j = run + incl - c, add = 0;
            for (unsigned long long mm = m; mm; mm &= mm - 1, j++)
                if ((int32_t)dcov[j * (unsigned)dC] > 0) add |= mm & (0ull - mm);
            kp |= add;
            if (g < ngroups) kept[g] = kp;
            const uint32_t tot = wave_incl_scan_u32((uint32_t)__builtin_popcountll(kp) | ((uint32_t)__builtin_popcountll(add) << 16));
            const uint32_t both = wave_bcast_u32(tot, ws - 1);          // (at most 64 * 64 = 4096 in either half)
            cnt += both & 0xFFFFu;
            rec += both >> 16;
            run += wave_bcast_u32(incl, ws - 1);
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();
    if (lane == 0 && rec) atomic_add_u64(n_rec, rec);
}

// k_sel_scatter of the merged ballots, and beside each record number the child's coverage cgw.addRecord is given: the record's own, or
// DIRTY's for a recovered candidate (its rank among the chunk's candidates finds it in dcov)
LDBG_WAVE_KERNEL void k_rec_scatter(RecCtx x, const unsigned long long* merged, const unsigned long long* cand, const unsigned long long* sel_off,
                                    const unsigned long long* cand_off, const uint32_t* dcov, int dC, uint32_t* out, int32_t* col) {
    const int ws = SEL_WS, lane = wave_lane();
    const int64_t n = x.N, wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    const int64_t ngroups = (n + 63) >> 6, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    const uint32_t* plane = x.cov + (size_t)x.child * (size_t)x.N;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        unsigned long long run = sel_off[ch], crun = cand_off[ch];
        for (int g0 = 0; g0 < SEL_GROUPS && ch * SEL_GROUPS + g0 < ngroups; g0 += ws) {
            const int64_t g = ch * SEL_GROUPS + g0 + lane;
            const unsigned long long m = g < ngroups ? merged[g] : 0ull, cm = g < ngroups ? cand[g] : 0ull;
            const uint32_t c = (uint32_t)__builtin_popcountll(m), incl = wave_incl_scan_u32(c);
            const uint32_t cc = (uint32_t)__builtin_popcountll(cm), cincl = wave_incl_scan_u32(cc);
            const unsigned long long base = run + incl - c, cbase = crun + cincl - cc;
            for (int jj = 0; jj < ws; jj++) {
                const unsigned long long mj = wave_bcast_u64(m, jj);
                if (!mj) continue;
                const unsigned long long bj = wave_bcast_u64(base, jj), cmj = wave_bcast_u64(cm, jj), cbj = wave_bcast_u64(cbase, jj);
                for (int bit = lane; bit < 64; bit += ws)
                    if ((mj >> bit) & 1ull) {
                        const unsigned long long below = (1ull << bit) - 1ull;
                        const size_t r = (size_t)(((ch * SEL_GROUPS + g0 + jj) << 6) + bit);
                        const unsigned long long pos = bj + (unsigned)__builtin_popcountll(mj & below);
                        out[pos] = (uint32_t)r;
                        col[pos] = (cmj >> bit) & 1ull ? (int32_t)dcov[(cbj + (unsigned)__builtin_popcountll(cmj & below)) * (unsigned)dC]
                                                       : (int32_t)LDBG_GLOBAL(const uint32_t, plane)[r];
                    }
            }
            run += wave_bcast_u32(incl, ws - 1);
            crun += wave_bcast_u32(cincl, ws - 1);
        }
    }
    wave_fence();
}

// coverages[childColor] = dr.getCoverage(0) as the file shows it (child colour 0): the column over the coverage field of the packed
// records.  A record is 8W + 5 bytes, so the field is not aligned: four byte stores
LDBG_KERNEL void k_rec_patch(const int32_t* col, int64_t count, int R, int off, uint8_t* out) {
    for (int64_t i = global_tid(); i < count; i += global_nthreads()) {
        const uint32_t v = (uint32_t)col[i];
        uint8_t* p = out + (size_t)i * (size_t)R + (size_t)off;
        p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
    }
}

int waves_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(items, 8192)); }

void check_resident(const Graph& g, const char* what) {
    if (g.is_image || g.is_shard || g.d_nbrg)
        throw StatusError(LDBG_ERR_UNSUPPORTED, std::string(what) + ": not over one rank's part of a hash-sharded table");
}

void check_projection(const Graph& g, const int* colours, int n) {
    if (n < 1 || !colours) throw StatusError(LDBG_ERR_ARG, "selection: no colour to write");
    if (n > LDBG_SELECT_MAX_PROJ) throw StatusError(LDBG_ERR_ARG, "selection: more than " + std::to_string(LDBG_SELECT_MAX_PROJ) + " colours to write");
    for (int i = 0; i < n; i++)
        if (colours[i] < 0 || colours[i] >= g.hdr.C) throw StatusError(LDBG_ERR_ARG, "selection: colour " + std::to_string(colours[i]) + " out of range");
}

}  // namespace

Selection::Selection(const Graph& g, const ldbg_record_filter& f, const Graph* lookup) : graph(lookup ? *lookup : g) {
    check_resident(g, "select");
    if (lookup) check_resident(*lookup, "select");
    const int C = g.hdr.C;
    if (C > 64) throw StatusError(LDBG_ERR_UNSUPPORTED, "select: a graph of more than 64 colours");
    const uint64_t colours = C == 64 ? ~0ull : ((1ull << C) - 1ull);
    if ((f.all_zero | f.all_positive | f.any_positive | f.none_positive) & ~colours) throw StatusError(LDBG_ERR_ARG, "select: a colour mask names a colour the graph does not have");
    if (f.cov_color < -1 || f.cov_color >= C) throw StatusError(LDBG_ERR_ARG, "select: coverage colour out of range");
    if (f.degree_color < -1 || f.degree_color >= C) throw StatusError(LDBG_ERR_ARG, "select: degree colour out of range");
    if (lookup && (lookup->hdr.k != g.hdr.k || lookup->device != g.device))
        throw StatusError(LDBG_ERR_ARG, "select: the two graphs differ in k-mer size or device");
    SelCtx x{g.view.cov, g.view.edges, g.view.N, f.all_zero, f.all_positive, f.any_positive, f.none_positive,
             f.all_zero | f.all_positive | f.any_positive | f.none_positive | (f.cov_color >= 0 ? 1ull << f.cov_color : 0ull),
             f.cov_color, f.cov_below, f.degree_color, f.degree_above};
    const int64_t n = graph.view.N;
    if (n == 0) return;
    rt::set_device(graph.device);
    rt::stream_t s = graph.stream;
    const int64_t nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    uint64_t* d_words = nullptr;
    int64_t* d_via = nullptr;
    unsigned long long *ballots = nullptr, *chunk_off = nullptr, *stat = nullptr;
    uint32_t* chunk_cnt = nullptr;
    auto free_tmp = [&] { rt::dfree(d_words); rt::dfree(d_via); rt::dfree(ballots); rt::dfree(chunk_off); rt::dfree(stat); rt::dfree(chunk_cnt); };
    try {
        if (lookup) {     // rr.getCanonicalKmer() -> GRAPH.findRecord: the k-mers of the query's records through the findRecord kernel
            d_words = (uint64_t*)rt::dmalloc((size_t)n * graph.view.W * 8);
            d_via = (int64_t*)rt::dmalloc((size_t)n * 8);
            lookup->records_dev(0, n, d_words, nullptr, nullptr, s);
            g.find_dev(d_words, n, d_via, nullptr, nullptr, s);
        }
        ballots = (unsigned long long*)rt::dmalloc((size_t)nchunks * SEL_GROUPS * 8);
        chunk_cnt = (uint32_t*)rt::dmalloc((size_t)nchunks * 4);
        chunk_off = (unsigned long long*)rt::dmalloc((size_t)nchunks * 8);
        stat = (unsigned long long*)rt::dmalloc(16);        // [0] records selected, [1] a query without a record
        rt::dmemset(stat, 0, 16, s);
        rt::Event e0, e1, e2, e3;
        e0.record(s);
        LDBG_LAUNCH(k_sel_mask, waves_for(nchunks), 64, s, x, n, (const int64_t*)d_via, (unsigned*)(stat + 1), ballots, chunk_cnt);
        LDBG_LAUNCH(k_sel_top, 1, 64, s, nchunks, (const uint32_t*)chunk_cnt, chunk_off, stat);
        e1.record(s);
        unsigned long long st[2] = {0, 0};
        rt::d2h(st, stat, 16, s);
        rt::stream_sync(s);
        if (st[1] & 0xFFFFFFFFull)
            throw StatusError(LDBG_ERR_NULLPOINTER, "a k-mer of the query graph has no record in the graph: findRecord returned null (FindShared.java:63-68)");
        count = (int64_t)st[0];
        select_ms = rt::Event::elapsed_ms(e0, e1);
        if (count > 0) {
            d_idx_ = (uint32_t*)rt::dmalloc((size_t)count * 4);
            e2.record(s);
            LDBG_LAUNCH(k_sel_scatter, waves_for(nchunks), 64, s, n, (const unsigned long long*)ballots, (const unsigned long long*)chunk_off, d_idx_);
            e3.record(s);
            rt::stream_sync(s);
            select_ms += rt::Event::elapsed_ms(e2, e3);
        }
    } catch (...) {
        free_tmp();
        rt::dfree(d_idx_);
        d_idx_ = nullptr;
        throw;
    }
    free_tmp();
    profile_add("select", select_ms);
}

Selection::Selection(const Graph& g, int child, const Graph& dirty) : graph(g) {
    check_resident(g, "recover");
    if (dirty.is_image || dirty.is_shard || dirty.d_nbrg || dirty.path == "<collection>")
        throw StatusError(LDBG_ERR_UNSUPPORTED, "recover: DIRTY must be one resident graph file, not a collection, one rank's part of a hash-sharded table or its image");
    const int C = g.hdr.C, dC = dirty.hdr.C;
    if (C > 64) throw StatusError(LDBG_ERR_UNSUPPORTED, "recover: a graph of more than 64 colours");
    if (child < 0 || child >= C) throw StatusError(LDBG_ERR_ARG, "recover: child colour " + std::to_string(child) + " out of range");
    if (dirty.hdr.k != g.hdr.k || dirty.device != g.device) throw StatusError(LDBG_ERR_ARG, "recover: the two graphs differ in k-mer size or device");
    child_colour = child;
    const int64_t n = g.view.N;
    if (n == 0) return;
    rt::set_device(g.device);
    rt::stream_t s = g.stream;
    const int64_t nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    const RecCtx x{g.view.cov, n, C, child};
    unsigned long long *kept = nullptr, *cand = nullptr, *cand_off = nullptr, *sel_off = nullptr, *stat = nullptr;
    uint32_t *cand_cnt = nullptr, *chunk_cnt = nullptr, *cand_idx = nullptr, *d_dcov = nullptr;
    uint64_t* d_words = nullptr;
    int64_t* d_didx = nullptr;
    auto free_tmp = [&] {
        rt::dfree(kept); rt::dfree(cand); rt::dfree(cand_off); rt::dfree(sel_off); rt::dfree(stat); rt::dfree(cand_cnt); rt::dfree(chunk_cnt);
        rt::dfree(cand_idx); rt::dfree(d_dcov); rt::dfree(d_words); rt::dfree(d_didx);
    };
    try {
        kept = (unsigned long long*)rt::dmalloc((size_t)nchunks * SEL_GROUPS * 8);
        cand = (unsigned long long*)rt::dmalloc((size_t)nchunks * SEL_GROUPS * 8);
        cand_cnt = (uint32_t*)rt::dmalloc((size_t)nchunks * 4);
        chunk_cnt = (uint32_t*)rt::dmalloc((size_t)nchunks * 4);
        cand_off = (unsigned long long*)rt::dmalloc((size_t)nchunks * 8);
        sel_off = (unsigned long long*)rt::dmalloc((size_t)nchunks * 8);
        stat = (unsigned long long*)rt::dmalloc(24);        // [0] candidates, [1] records written, [2] records recovered
        rt::dmemset(stat, 0, 24, s);
        rt::Event e0, e1, e2, e3, e4, e5, e6, e7;
        e0.record(s);
        LDBG_LAUNCH(k_rec_classify, waves_for(nchunks), 64, s, x, kept, cand, cand_cnt);
        LDBG_LAUNCH(k_sel_top, 1, 64, s, nchunks, (const uint32_t*)cand_cnt, cand_off, stat);
        e1.record(s);
        unsigned long long st[3] = {0, 0, 0};
        rt::d2h(st, stat, 24, s);
        rt::stream_sync(s);
        const int64_t ncand = (int64_t)st[0];
        select_ms = rt::Event::elapsed_ms(e0, e1);
        if (ncand > 0) {       // DIRTY.findRecord(cr.getCanonicalKmer()): the candidates' k-mers through the findRecord kernel (Q1 included)
            cand_idx = (uint32_t*)rt::dmalloc((size_t)ncand * 4);
            d_words = (uint64_t*)rt::dmalloc((size_t)ncand * (size_t)g.view.W * 8);
            d_didx = (int64_t*)rt::dmalloc((size_t)ncand * 8);
            d_dcov = (uint32_t*)rt::dmalloc((size_t)ncand * (size_t)dC * 4);
            e2.record(s);
            LDBG_LAUNCH(k_sel_scatter, waves_for(nchunks), 64, s, n, (const unsigned long long*)cand, (const unsigned long long*)cand_off, cand_idx);
            LDBG_LAUNCH(k_rec_keys, grid_for(ncand), 256, s, g.view.keys, n, g.view.W, (const uint32_t*)cand_idx, ncand, d_words);
            e3.record(s);
            dirty.find_dev(d_words, ncand, d_didx, d_dcov, nullptr, s);
        }
        e4.record(s);
        LDBG_LAUNCH(k_rec_merge, waves_for(nchunks), 64, s, n, kept, (const unsigned long long*)cand, (const unsigned long long*)cand_off,
                    (const uint32_t*)d_dcov, dC, chunk_cnt, stat + 2);
        LDBG_LAUNCH(k_sel_top, 1, 64, s, nchunks, (const uint32_t*)chunk_cnt, sel_off, stat + 1);
        e5.record(s);
        rt::d2h(st, stat, 24, s);
        rt::stream_sync(s);
        count = (int64_t)st[1];
        n_recovered = (int64_t)st[2];
        if (ncand > 0) select_ms += rt::Event::elapsed_ms(e2, e3);
        select_ms += rt::Event::elapsed_ms(e4, e5);
        if (count > 0) {
            d_idx_ = (uint32_t*)rt::dmalloc((size_t)count * 4);
            d_cov_ = (int32_t*)rt::dmalloc((size_t)count * 4);
            e6.record(s);
            LDBG_LAUNCH(k_rec_scatter, waves_for(nchunks), 64, s, x, (const unsigned long long*)kept, (const unsigned long long*)cand,
                        (const unsigned long long*)sel_off, (const unsigned long long*)cand_off, (const uint32_t*)d_dcov, dC, d_idx_, d_cov_);
            e7.record(s);
            rt::stream_sync(s);
            select_ms += rt::Event::elapsed_ms(e6, e7);
        }
    } catch (...) {
        free_tmp();
        rt::dfree(d_idx_); rt::dfree(d_cov_);
        d_idx_ = nullptr; d_cov_ = nullptr;
        throw;
    }
    free_tmp();
    profile_add("recover", select_ms);
}

Selection::~Selection() { rt::dfree(d_idx_); rt::dfree(d_cov_); }

void Selection::check_recovered() const {
    if (child_colour < 0) throw StatusError(LDBG_ERR_ARG, "selection: not made by ldbg_graph_recover");
}

void Selection::recovered_coverage(int64_t first, int64_t n, int32_t* cov) const {
    check_recovered();
    if (first < 0 || n < 0 || first + n > count) throw StatusError(LDBG_ERR_ARG, "selection range outside 0.." + std::to_string(count));
    if (n == 0) return;
    if (!cov) throw StatusError(LDBG_ERR_ARG, "selection: null output");
    rt::set_device(graph.device);
    rt::d2h(cov, d_cov_ + first, (size_t)n * 4, graph.stream);
    rt::stream_sync(graph.stream);
}

std::vector<uint8_t> Selection::recovered_header() const {
    check_recovered();
    CtxHeader h;
    h.version = graph.hdr.version; h.k = graph.hdr.k; h.W = graph.hdr.W; h.C = 1;
    h.colors.push_back(graph.hdr.colors[(size_t)child_colour]);
    return serialize_ctx_header(h);
}

uint8_t* Selection::pack_recovered() const {
    check_recovered();
    const int zero = 0;
    uint8_t* d = pack(&zero, 1);
    if (!d || child_colour != 0) return d;
    rt::stream_t s = graph.stream;
    try {
        rt::Event e0, e1;
        e0.record(s);
        LDBG_LAUNCH(k_rec_patch, grid_for(count), 256, s, (const int32_t*)d_cov_, count, 8 * graph.view.W + 5, 8 * graph.view.W, d);
        e1.record(s);
        rt::stream_sync(s);
        profile_add("select_pack", rt::Event::elapsed_ms(e0, e1));
    } catch (...) { rt::dfree(d); throw; }
    return d;
}

void Selection::write_recovered(const std::string& out_path) const {
    const std::vector<uint8_t> hdr = recovered_header();
    write_file(hdr, pack_recovered(), (size_t)count * (8 * (size_t)graph.view.W + 5), out_path);
}

void Selection::indices(int64_t first, int64_t n, int64_t* idx, bool device_out, rt::stream_t s) const {
    if (first < 0 || n < 0 || first + n > count) throw StatusError(LDBG_ERR_ARG, "selection range outside 0.." + std::to_string(count));
    if (n == 0) return;
    if (!idx) throw StatusError(LDBG_ERR_ARG, "selection: null output");
    rt::set_device(graph.device);
    int64_t* d = device_out ? idx : (int64_t*)rt::dmalloc((size_t)n * 8);
    try {
        LDBG_LAUNCH(k_sel_widen, grid_for(n), 256, s, (const uint32_t*)(d_idx_ + first), n, d);
        if (!device_out) rt::d2h(idx, d, (size_t)n * 8, s);
        rt::stream_sync(s);
    } catch (...) { if (!device_out) rt::dfree(d); throw; }
    if (!device_out) rt::dfree(d);
}

std::vector<uint8_t> Selection::header(const int* colours, int n_colours, const char* header_path) const {
    check_projection(graph, colours, n_colours);
    CtxHeader h;
    if (header_path) {
        FILE* f = fopen(header_path, "rb");
        if (!f) throw StatusError(LDBG_ERR_CORTEXJDK, std::string("Cortex graph file '") + header_path + "' not found");
        struct stat st{};
        std::vector<uint8_t> raw;
        if (fstat(fileno(f), &st) == 0) {
            raw.resize((size_t)std::min<int64_t>((int64_t)st.st_size, (int64_t)1 << 22));
            if (!raw.empty() && fread(raw.data(), 1, raw.size(), f) != raw.size()) raw.clear();
        }
        fclose(f);
        h = parse_ctx_header(raw.data(), raw.size(), (int64_t)st.st_size, header_path);
        if (h.k != graph.hdr.k) throw StatusError(LDBG_ERR_ARG, std::string("selection: the header of '") + header_path + "' has another k-mer size");
        if (h.C != n_colours)
            throw StatusError(LDBG_ERR_ARG, std::string("selection: the header of '") + header_path + "' has " + std::to_string(h.C) + " colours, the records " + std::to_string(n_colours));
    } else {
        h.version = 6; h.k = graph.hdr.k; h.W = graph.hdr.W; h.C = n_colours;
        h.colors.resize((size_t)n_colours);
        for (int i = 0; i < n_colours; i++) h.colors[(size_t)i].sample_name = graph.hdr.colors[(size_t)colours[i]].sample_name;
    }
    return serialize_ctx_header(h);
}

uint8_t* Selection::pack(const int* colours, int n_colours) const {
    check_projection(graph, colours, n_colours);
    if (count == 0) return nullptr;
    rt::set_device(graph.device);
    rt::stream_t s = graph.stream;
    PackCtx x;
    x.g = graph.view;
    x.nproj = n_colours;
    memset(x.proj, 0, sizeof x.proj);
    for (int i = 0; i < n_colours; i++) x.proj[i] = (uint8_t)colours[i];
    const size_t R = 8 * (size_t)graph.view.W + 5 * (size_t)n_colours;
    uint8_t* d = (uint8_t*)rt::dmalloc((size_t)count * R);
    try {
        rt::Event e0, e1;
        e0.record(s);
        LDBG_LAUNCH_W(graph.view.W, k_sel_pack, waves_for((count + 63) / 64), 64, s, x, (const uint32_t*)d_idx_, count, d);
        e1.record(s);
        rt::stream_sync(s);
        profile_add("select_pack", rt::Event::elapsed_ms(e0, e1));
    } catch (...) { rt::dfree(d); throw; }
    return d;
}

void Selection::write_ctx(const int* colours, int n_colours, const char* header_path, const std::string& out_path) const {
    const std::vector<uint8_t> hdr = header(colours, n_colours, header_path);
    write_file(hdr, pack(colours, n_colours), (size_t)count * (8 * (size_t)graph.view.W + 5 * (size_t)n_colours), out_path);
}

// the header and the `total` packed bytes at d (device memory, freed here) as a file
void Selection::write_file(const std::vector<uint8_t>& hdr, const uint8_t* d_packed, size_t total, const std::string& out_path) const {
    uint8_t* d = (uint8_t*)d_packed;
    const size_t step = (size_t)64 << 20;
    void* pin = nullptr;
    FILE* f = nullptr;
    bool ok = true;
    try {
        f = fopen(out_path.c_str(), "wb");
        if (!f) throw StatusError(LDBG_ERR_CORTEXJDK, "Unable to open file '" + out_path + "'");
        ok = fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size();
        if (total) pin = rt::hmalloc_pinned(std::min(total, step));
        for (size_t o = 0; o < total && ok; o += step) {
            const size_t nb = std::min(step, total - o);
            rt::d2h(pin, d + o, nb, graph.stream);
            rt::stream_sync(graph.stream);
            ok = fwrite(pin, 1, nb, f) == nb;
        }
    } catch (...) {
        if (f) fclose(f);
        rt::hfree_pinned(pin); rt::dfree(d);
        throw;
    }
    ok = fclose(f) == 0 && ok;
    rt::hfree_pinned(pin); rt::dfree(d);
    if (!ok) throw StatusError(LDBG_ERR_CORTEXJDK, "Unable to write record to file '" + out_path + "'");
}

}  // namespace ldbg
