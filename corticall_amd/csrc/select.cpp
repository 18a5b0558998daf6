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

Selection::~Selection() { rt::dfree(d_idx_); }

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
    uint8_t* d = pack(colours, n_colours);
    const size_t total = (size_t)count * (8 * (size_t)graph.view.W + 5 * (size_t)n_colours), step = (size_t)64 << 20;
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
