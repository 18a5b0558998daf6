// Record selection on the device (select.h): a streaming pass over the coverage and edge planes the filter names ->
// one 64-bit ballot per 64 records and one count per chunk -> exclusive scan of the chunk counts by one wavefront -> the record
// numbers scattered in record order from the ballots -> the selected records gathered into the file's record layout.  Every
// kernel is launched one wavefront per workgroup and uses wavefront primitives only; no workgroup waits for another, nothing is
// placed with an atomic, so the result is the same from run to run.  The ballot words, the scan of the chunk counts and the LDS stage of
// the packed records are those of wavescan.h.  The TEST-ONLY host simulation runs the kernels as they are.
#include "select.h"
#include "wavescan.h"

#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>

namespace ldbg {

namespace {

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
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    bool miss = false;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SELECT_CHUNK;
        const int lim = chunk_lim(n, c0, LDBG_SELECT_CHUNK);
        unsigned long long cur[1] = {0};
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
                cnt += ballot_step(c0, s, {ok[j]}, cur, {ballots});
            }
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();      // (host simulation: a lane that has left the kernel counts as inactive in a ballot the others have yet to read)
    if (miss) atomic_or_u32(null_seen, 1u);
}

// RecoverExcludedKmers writes a column beside the record numbers: the child's coverage cgw.addRecord is given, the record's own (plane) or
// DIRTY's for a recovered candidate (its rank among the chunk's candidates finds it in dcov)
struct ScatterColumn {
    const uint32_t* plane;
    const unsigned long long *cand, *cand_off;
    const uint32_t* dcov;
    int dC;
    int32_t* col;
};

// out[chunk_off[ch] + rank of the record among the chunk's passing records] = record, read back from the ballots
template <bool WithColumn>
LDBG_WAVE_KERNEL void k_sel_scatter(int64_t n, const unsigned long long* ballots, const unsigned long long* chunk_off, uint32_t* out, ScatterColumn x) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    const int64_t ngroups = (n + 63) >> 6, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        unsigned long long run = chunk_off[ch], crun = WithColumn ? x.cand_off[ch] : 0ull;
        for (int g0 = 0; g0 < SEL_GROUPS && ch * SEL_GROUPS + g0 < ngroups; g0 += ws) {
            const int64_t g = ch * SEL_GROUPS + g0 + lane;
            const GroupWord w = group_word(ballots, g, ngroups, run);
            GroupWord cw{0ull, 0ull};
            if (WithColumn) cw = group_word(x.cand, g, ngroups, crun);
            for (int jj = 0; jj < ws; jj++) {
                const unsigned long long mj = wave_bcast_u64(w.m, jj);
                if (!mj) continue;
                const unsigned long long bj = wave_bcast_u64(w.base, jj);
                const unsigned long long cmj = WithColumn ? wave_bcast_u64(cw.m, jj) : 0ull, cbj = WithColumn ? wave_bcast_u64(cw.base, jj) : 0ull;
                for (int bit = lane; bit < 64; bit += ws)
                    if ((mj >> bit) & 1ull) {
                        const unsigned long long below = (1ull << bit) - 1ull;
                        const size_t r = (size_t)(((ch * SEL_GROUPS + g0 + jj) << 6) + bit);
                        const unsigned long long pos = bj + (unsigned)__builtin_popcountll(mj & below);
                        out[pos] = (uint32_t)r;
                        if (WithColumn)
                            x.col[pos] = (cmj >> bit) & 1ull ? (int32_t)x.dcov[(cbj + (unsigned)__builtin_popcountll(cmj & below)) * (unsigned)x.dC]
                                                             : (int32_t)LDBG_GLOBAL(const uint32_t, x.plane)[r];
                    }
            }
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
#define SEL_STAGE_WORDS LDBG_STAGE_WORDS(LDBG_SELECT_MAX_PROJ)

// CortexGraphWriter.addRecord (CortexGraphWriter.java:115-138) of the selected records: 8W k-mer bytes | 4C' coverage bytes | C' edge
// bytes each, from the record's probe row (one or two lines hold all of it), through the LDS stage of wavescan.h
template <int W>
LDBG_WAVE_KERNEL void k_sel_pack(PackCtx x, const uint32_t* idx, int64_t count, uint8_t* out) {
#ifndef LDBG_HOSTSIM
    __shared__ uint32_t stage[SEL_STAGE_WORDS];
#else
    static uint32_t stage[SEL_STAGE_WORDS];          // (one simulated wavefront at a time: rt.h)
#endif
    const int ws = LDBG_WS, lane = wave_lane(), R = 8 * W + 5 * x.nproj;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nb = (count + ws - 1) / ws;
    for (int64_t b = wave; b < nb; b += nwaves) {
        const int64_t first = b * ws;
        const int nrec = (int)std::min<int64_t>(ws, count - first);
        uint8_t* dst = out + (size_t)first * (size_t)R;
        uint8_t* lb = stage_bytes(stage, dst);
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
        stage_write_out(stage, dst, nrec, R);
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
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t n = x.N, wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SELECT_CHUNK;
        const int lim = chunk_lim(n, c0, LDBG_SELECT_CHUNK);
        unsigned long long cur[2] = {0, 0};
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
                cnt += ballot_step(c0, s, {kp[j], !kp[j] && other[j]}, cur, {kept, cand});
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
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    const int64_t ngroups = (n + 63) >> 6, nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    unsigned long long rec = 0;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        unsigned long long run = cand_off[ch];
        uint32_t cnt = 0;
        for (int g0 = 0; g0 < SEL_GROUPS && ch * SEL_GROUPS + g0 < ngroups; g0 += ws) {
            const int64_t g = ch * SEL_GROUPS + g0 + lane;
            const GroupWord w = group_word(cand, g, ngroups, run);
            unsigned long long kp = g < ngroups ? kept[g] : 0ull;
            unsigned long long j = w.base, add = 0;
            for (unsigned long long mm = w.m; mm; mm &= mm - 1, j++)
                if ((int32_t)dcov[j * (unsigned)dC] > 0) add |= mm & (0ull - mm);
            kp |= add;
            if (g < ngroups) kept[g] = kp;
            const uint32_t tot = wave_incl_scan_u32((uint32_t)__builtin_popcountll(kp) | ((uint32_t)__builtin_popcountll(add) << 16));
            const uint32_t both = wave_bcast_u32(tot, ws - 1);          // (at most 64 * 64 = 4096 in either half)
            cnt += both & 0xFFFFu;
            rec += both >> 16;
        }
        if (lane == 0) chunk_cnt[ch] = cnt;
    }
    wave_fence();
    if (lane == 0 && rec) atomic_add_u64(n_rec, rec);
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

void check_projection(const Graph& g, const int* colours, int n) {
    if (n < 1 || !colours) throw StatusError(LDBG_ERR_ARG, "selection: no colour to write");
    if (n > LDBG_SELECT_MAX_PROJ) throw StatusError(LDBG_ERR_ARG, "selection: more than " + std::to_string(LDBG_SELECT_MAX_PROJ) + " colours to write");
    for (int i = 0; i < n; i++)
        if (colours[i] < 0 || colours[i] >= g.hdr.C) throw StatusError(LDBG_ERR_ARG, "selection: colour " + std::to_string(colours[i]) + " out of range");
}

}  // namespace

Selection::Selection(const Graph& g, const ldbg_record_filter& f, const Graph* lookup) : graph(lookup ? *lookup : g) {
    check_whole_table(g, "select");
    if (lookup) check_whole_table(*lookup, "select");
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
    DevBlocks tmp;
    int64_t* d_via = nullptr;
    if (lookup) {     // rr.getCanonicalKmer() -> GRAPH.findRecord: the k-mers of the query's records through the findRecord kernel
        uint64_t* d_words = tmp.get<uint64_t>((size_t)n * graph.view.W);
        d_via = tmp.get<int64_t>((size_t)n);
        lookup->records_dev(0, n, d_words, nullptr, nullptr, s);
        g.find_dev(d_words, n, d_via, nullptr, nullptr, s);
    }
    unsigned long long* ballots = tmp.get<unsigned long long>((size_t)nchunks * SEL_GROUPS);
    uint32_t* chunk_cnt = tmp.get<uint32_t>((size_t)nchunks);
    unsigned long long* chunk_off = tmp.get<unsigned long long>((size_t)nchunks);
    unsigned long long* stat = tmp.get<unsigned long long>(2);        // [0] records selected, [1] a query without a record
    rt::dmemset(stat, 0, 16, s);
    rt::Event e0, e1, e2, e3;
    e0.record(s);
    LDBG_LAUNCH(k_sel_mask, waves_for(nchunks), 64, s, x, n, (const int64_t*)d_via, (unsigned*)(stat + 1), ballots, chunk_cnt);
    LDBG_LAUNCH(k_chunk_top<unsigned long long>, 1, 64, s, nchunks, (const uint32_t*)chunk_cnt, chunk_off, stat);
    e1.record(s);
    unsigned long long st[2] = {0, 0};
    rt::d2h(st, stat, 16, s);
    rt::stream_sync(s);
    if (st[1] & 0xFFFFFFFFull)
        throw StatusError(LDBG_ERR_NULLPOINTER, "a k-mer of the query graph has no record in the graph: findRecord returned null (FindShared.java:63-68)");
    count = (int64_t)st[0];
    select_ms = rt::Event::elapsed_ms(e0, e1);
    if (count > 0) {
        d_idx_ = own_.get<uint32_t>((size_t)count);
        e2.record(s);
        LDBG_LAUNCH(k_sel_scatter<false>, waves_for(nchunks), 64, s, n, (const unsigned long long*)ballots, (const unsigned long long*)chunk_off, d_idx_, ScatterColumn{});
        e3.record(s);
        rt::stream_sync(s);
        select_ms += rt::Event::elapsed_ms(e2, e3);
    }
    profile_add("select", select_ms);
}

Selection::Selection(const Graph& g, int child, const Graph& dirty) : graph(g) {
    check_whole_table(g, "recover");
    if (!is_whole_table(dirty) || dirty.path == "<collection>")
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
    DevBlocks tmp;
    unsigned long long* kept = tmp.get<unsigned long long>((size_t)nchunks * SEL_GROUPS);
    unsigned long long* cand = tmp.get<unsigned long long>((size_t)nchunks * SEL_GROUPS);
    uint32_t* cand_cnt = tmp.get<uint32_t>((size_t)nchunks);
    uint32_t* chunk_cnt = tmp.get<uint32_t>((size_t)nchunks);
    unsigned long long* cand_off = tmp.get<unsigned long long>((size_t)nchunks);
    unsigned long long* sel_off = tmp.get<unsigned long long>((size_t)nchunks);
    unsigned long long* stat = tmp.get<unsigned long long>(3);        // [0] candidates, [1] records written, [2] records recovered
    uint32_t* d_dcov = nullptr;
    rt::dmemset(stat, 0, 24, s);
    rt::Event e0, e1, e2, e3, e4, e5, e6, e7;
    e0.record(s);
    LDBG_LAUNCH(k_rec_classify, waves_for(nchunks), 64, s, x, kept, cand, cand_cnt);
    LDBG_LAUNCH(k_chunk_top<unsigned long long>, 1, 64, s, nchunks, (const uint32_t*)cand_cnt, cand_off, stat);
    e1.record(s);
    unsigned long long st[3] = {0, 0, 0};
    rt::d2h(st, stat, 24, s);
    rt::stream_sync(s);
    const int64_t ncand = (int64_t)st[0];
    select_ms = rt::Event::elapsed_ms(e0, e1);
    if (ncand > 0) {       // DIRTY.findRecord(cr.getCanonicalKmer()): the candidates' k-mers through the findRecord kernel (Q1 included)
        uint32_t* cand_idx = tmp.get<uint32_t>((size_t)ncand);
        uint64_t* d_words = tmp.get<uint64_t>((size_t)ncand * (size_t)g.view.W);
        int64_t* d_didx = tmp.get<int64_t>((size_t)ncand);
        d_dcov = tmp.get<uint32_t>((size_t)ncand * (size_t)dC);
        e2.record(s);
        LDBG_LAUNCH(k_sel_scatter<false>, waves_for(nchunks), 64, s, n, (const unsigned long long*)cand, (const unsigned long long*)cand_off, cand_idx, ScatterColumn{});
        LDBG_LAUNCH(k_rec_keys, grid_for(ncand), 256, s, g.view.keys, n, g.view.W, (const uint32_t*)cand_idx, ncand, d_words);
        e3.record(s);
        dirty.find_dev(d_words, ncand, d_didx, d_dcov, nullptr, s);
    }
    e4.record(s);
    LDBG_LAUNCH(k_rec_merge, waves_for(nchunks), 64, s, n, kept, (const unsigned long long*)cand, (const unsigned long long*)cand_off,
                (const uint32_t*)d_dcov, dC, chunk_cnt, stat + 2);
    LDBG_LAUNCH(k_chunk_top<unsigned long long>, 1, 64, s, nchunks, (const uint32_t*)chunk_cnt, sel_off, stat + 1);
    e5.record(s);
    rt::d2h(st, stat, 24, s);
    rt::stream_sync(s);
    count = (int64_t)st[1];
    n_recovered = (int64_t)st[2];
    if (ncand > 0) select_ms += rt::Event::elapsed_ms(e2, e3);
    select_ms += rt::Event::elapsed_ms(e4, e5);
    if (count > 0) {
        d_idx_ = own_.get<uint32_t>((size_t)count);
        d_cov_ = own_.get<int32_t>((size_t)count);
        const ScatterColumn col{g.view.cov + (size_t)child * (size_t)n, cand, cand_off, d_dcov, dC, d_cov_};
        e6.record(s);
        LDBG_LAUNCH(k_sel_scatter<true>, waves_for(nchunks), 64, s, n, (const unsigned long long*)kept, (const unsigned long long*)sel_off, d_idx_, col);
        e7.record(s);
        rt::stream_sync(s);
        select_ms += rt::Event::elapsed_ms(e6, e7);
    }
    profile_add("recover", select_ms);
}

void Selection::compact(const unsigned long long* ballots, const uint32_t* chunk_cnt, rt::stream_t s) {
    const int64_t n = graph.view.N;
    own_.clear();
    d_idx_ = nullptr; d_cov_ = nullptr; count = 0;
    if (n == 0) return;
    const int64_t nchunks = (n + LDBG_SELECT_CHUNK - 1) / LDBG_SELECT_CHUNK;
    DevBlocks tmp;
    unsigned long long* chunk_off = tmp.get<unsigned long long>((size_t)nchunks);
    unsigned long long* total = tmp.get<unsigned long long>(1);
    rt::Event e0, e1, e2, e3;
    e0.record(s);
    LDBG_LAUNCH(k_chunk_top<unsigned long long>, 1, 64, s, nchunks, chunk_cnt, chunk_off, total);
    e1.record(s);
    unsigned long long tot = 0;
    rt::d2h(&tot, total, 8, s);
    rt::stream_sync(s);
    count = (int64_t)tot;
    select_ms += rt::Event::elapsed_ms(e0, e1);
    if (count > 0) {
        d_idx_ = own_.get<uint32_t>((size_t)count);
        e2.record(s);
        LDBG_LAUNCH(k_sel_scatter<false>, waves_for(nchunks), 64, s, n, ballots, (const unsigned long long*)chunk_off, d_idx_, ScatterColumn{});
        e3.record(s);
        rt::stream_sync(s);
        select_ms += rt::Event::elapsed_ms(e2, e3);
    }
}

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

DevRecords Selection::pack_recovered() const {
    check_recovered();
    const int zero = 0;
    DevRecords d = pack(&zero, 1);
    if (!d || child_colour != 0) return d;
    rt::stream_t s = graph.stream;
    rt::Event e0, e1;
    e0.record(s);
    LDBG_LAUNCH(k_rec_patch, grid_for(count), 256, s, (const int32_t*)d_cov_, count, 8 * graph.view.W + 5, 8 * graph.view.W, d.get());
    e1.record(s);
    rt::stream_sync(s);
    profile_add("select_pack", rt::Event::elapsed_ms(e0, e1));
    return d;
}

void Selection::write_recovered(const std::string& out_path) const {
    const std::vector<uint8_t> hdr = recovered_header();
    write_records_file(hdr, pack_recovered().get(), (size_t)count * (8 * (size_t)graph.view.W + 5), graph.device, graph.stream, out_path);
}

void Selection::indices(int64_t first, int64_t n, int64_t* idx, bool device_out, rt::stream_t s) const {
    if (first < 0 || n < 0 || first + n > count) throw StatusError(LDBG_ERR_ARG, "selection range outside 0.." + std::to_string(count));
    if (n == 0) return;
    if (!idx) throw StatusError(LDBG_ERR_ARG, "selection: null output");
    rt::set_device(graph.device);
    DevBlocks tmp;
    int64_t* d = device_out ? idx : tmp.get<int64_t>((size_t)n);
    LDBG_LAUNCH(k_sel_widen, grid_for(n), 256, s, (const uint32_t*)(d_idx_ + first), n, d);
    if (!device_out) rt::d2h(idx, d, (size_t)n * 8, s);
    rt::stream_sync(s);
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

DevRecords Selection::pack(const int* colours, int n_colours) const {
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
    DevRecords d((uint8_t*)rt::dmalloc((size_t)count * R));
    rt::Event e0, e1;
    e0.record(s);
    LDBG_LAUNCH_W(graph.view.W, k_sel_pack, waves_for((count + 63) / 64), 64, s, x, (const uint32_t*)d_idx_, count, d.get());
    e1.record(s);
    rt::stream_sync(s);
    profile_add("select_pack", rt::Event::elapsed_ms(e0, e1));
    return d;
}

void Selection::write_ctx(const int* colours, int n_colours, const char* header_path, const std::string& out_path) const {
    const std::vector<uint8_t> hdr = header(colours, n_colours, header_path);
    write_records_file(hdr, pack(colours, n_colours).get(), (size_t)count * (8 * (size_t)graph.view.W + 5 * (size_t)n_colours), graph.device, graph.stream, out_path);
}

}  // namespace ldbg
