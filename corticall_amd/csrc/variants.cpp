// callVariant of n seeds on the device (variants.h): ComputeInheritance.java:102-236 in its per-seed reading.
//   batch 1 (cursor.cpp): assemble(seed) on the child's engine until a vertex covered in the other parent's colour, both directions.
//   k_variant_chain: one lane per seed -> the seed's preliminary status, its source and destination records, and the third batch's
//     seeds (the source as stepped) and targets (the destination) as ASCII; a seed without both gets N x k, which is no k-mer.
//   batch 3 (cursor.cpp): next() on the parent's engine from the source until the destination.
//   k_variant_call: one wavefront per seed -> the coverage sums (lanes stride over the vertices, one butterfly per colour), then
//     trimToAlleles on the two contigs' bases, 64 per round from the left and from the right, the position found by ballot.
//   scan_u32 over the allele lengths (wavescan.h), k_variant_alleles: one wavefront per seed writes the allele bytes.
// No contig string exists anywhere: base i of a contig is base i of its first vertex for i < k and the last base of vertex i - k + 1
// after that (toContig, TraversalUtils.java:367-381), read from the packed words.  Integer arithmetic only.  Every kernel but the chain
// is launched one wavefront per workgroup; the TEST-ONLY host simulation runs them as they are.
#include "variants.h"

#include "devmem.h"
#include "wavescan.h"

namespace ldbg {

namespace {

#define LDBG_VARIANT_PENDING 255u      // between the chain and the call: a seed with both ends (no value of the public enum)

struct VcArgs {
    GraphView g;
    int64_t n;
    int k, stop_colour, ncol;
    uint64_t mask;
    // the first batch
    const int64_t* c_off; const uint64_t* c_words; const int64_t* c_rec; const uint8_t* c_end; const uint8_t* c_status;
    // the third batch
    const int64_t* p_off; const uint64_t* p_words; const int64_t* p_rec; const uint8_t* p_end; const uint8_t* p_status;
    unsigned char* seeds3; unsigned char* targets3;
    // per seed
    uint8_t* status; int64_t* source_rec; int64_t* dest_rec; int32_t* n_child; int32_t* n_parent; int32_t* st; int32_t* s0end; int32_t* s1end;
    int64_t* child_sum; uint8_t* child_flag; int64_t* parent_sum; uint8_t* parent_flag;
    uint32_t* allele_len;                // [2n]
    unsigned long long* total;           // allele bytes of the batch as 64 bits (the scan counts modulo 2^32)
    const int64_t* allele_off; uint8_t* alleles;
};

// base p of a packed k-mer in memory, 0..3
template <int W>
LDBG_DEV unsigned vc_kmer_base(const uint64_t* w, int k, int p) {
    const int bit = 2 * (k - 1 - p);
    return (unsigned)((w[W - 1 - (bit >> 6)] >> (bit & 63)) & 3ull);
}
LDBG_DEV unsigned char vc_char(unsigned b) { return (unsigned char)(b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : 'T'); }
template <int W>
LDBG_DEV void vc_ascii(const uint64_t* w, int k, unsigned char* out) {
    for (int p = 0; p < k; p++) out[p] = vc_char(vc_kmer_base<W>(w, k, p));
}

template <int W>
LDBG_KERNEL void k_variant_chain(VcArgs a) {
    const int k = a.k;
    for (int64_t i = global_tid(); i < a.n; i += global_nthreads()) {
        const unsigned cs = a.c_status[i], er = a.c_end[i], ef = a.c_end[a.n + i];
        const int64_t co = a.c_off[i], nc = a.c_off[i + 1] - co;
        const unsigned s = cs == LDBG_CURSOR_NULLPOINTER ? LDBG_VARIANT_NULLPOINTER
                         : cs == LDBG_CURSOR_CAPACITY   ? LDBG_VARIANT_CAPACITY
                         : (er == LDBG_CURSOR_LIMIT || ef == LDBG_CURSOR_LIMIT) ? LDBG_VARIANT_LIMIT
                         : er != LDBG_CURSOR_STOP ? LDBG_VARIANT_NO_SOURCE
                         : ef != LDBG_CURSOR_STOP ? LDBG_VARIANT_NO_DESTINATION : LDBG_VARIANT_PENDING;
        a.status[i] = (uint8_t)s;
        a.n_child[i] = (int32_t)nc;
        a.source_rec[i] = er == LDBG_CURSOR_STOP ? a.c_rec[co] : -1;
        a.dest_rec[i] = ef == LDBG_CURSOR_STOP ? a.c_rec[co + nc - 1] : -1;
        unsigned char* s3 = a.seeds3 + (size_t)i * (size_t)k;
        unsigned char* t3 = a.targets3 + (size_t)i * (size_t)k;
        if (s == LDBG_VARIANT_PENDING) {
            vc_ascii<W>(a.c_words + (size_t)co * W, k, s3);
            vc_ascii<W>(a.c_words + (size_t)(co + nc - 1) * W, k, t3);
        } else {
            for (int p = 0; p < k; p++) { s3[p] = 'N'; t3[p] = 'N'; }
        }
    }
}

// a contig as its vertices' packed words: vertex 0 at `first`, vertex v >= 1 at rest + (v - 1) W
struct VcContig { const uint64_t* first; const uint64_t* rest; };
template <int W>
LDBG_DEV unsigned vc_base(const VcContig& c, int k, int i) {
    if (i < k) return vc_kmer_base<W>(c.first, k, i);
    return (unsigned)(LDBG_GLOBAL(const uint64_t, c.rest)[(size_t)(i - k) * W + (W - 1)] & 3ull);
}

LDBG_DEV uint64_t vc_wave_sum(uint64_t v) {
    for (int m = wave_size() >> 1; m > 0; m >>= 1) v += wave_shfl_xor_u64(v, m);
    return v;
}

// the sum of getCoverage(colour) (the Java int) over the records rec[0 .. n) and one more record `extra` (-1: none); *mag = the sum of the
// magnitudes.  Every lane receives both.
LDBG_DEV int64_t vc_cov_sum(const GraphView& g, const int64_t* rec, int64_t n, int64_t extra, int colour, uint64_t* mag) {
    const int ws = LDBG_WS, lane = wave_lane();
    int64_t s = 0;
    uint64_t m = 0;
    for (int64_t j = lane; j < n; j += ws) {
        const int64_t v = (int64_t)(int32_t)graph_cov(g, LDBG_GLOBAL(const int64_t, rec)[j], colour);
        s += v; m += (uint64_t)(v < 0 ? -v : v);
    }
    if (lane == 0 && extra >= 0) {
        const int64_t v = (int64_t)(int32_t)graph_cov(g, extra, colour);
        s += v; m += (uint64_t)(v < 0 ? -v : v);
    }
    *mag = vc_wave_sum(m);
    return (int64_t)vc_wave_sum((uint64_t)s);
}
LDBG_DEV bool vc_any_null(const int64_t* rec, int64_t n) {
    const int ws = LDBG_WS, lane = wave_lane();
    bool bad = false;
    for (int64_t j = lane; j < n; j += ws) bad |= LDBG_GLOBAL(const int64_t, rec)[j] < 0;
    return wave_ballot(bad) != 0ull;
}

template <int W>
LDBG_WAVE_KERNEL void k_variant_call(VcArgs a) {
    const int ws = LDBG_WS, lane = wave_lane(), k = a.k;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    unsigned long long bytes = 0;
    for (int64_t i = wave_uniform_i64(wave); i < a.n; i += nwaves) {
        unsigned s = a.status[i];
        const int64_t co = wave_uniform_i64(a.c_off[i]), nc = wave_uniform_i64(a.c_off[i + 1]) - co;
        const int64_t po = wave_uniform_i64(a.p_off[i]), np = wave_uniform_i64(a.p_off[i + 1]) - po;
        int32_t n_parent = 0, st = 0, e0 = 0, e1 = 0;
        if (s == LDBG_VARIANT_PENDING) {
            n_parent = (int32_t)np + 1;
            const unsigned ps = a.p_status[i], pe = a.p_end[i];
            const bool null_rec = vc_any_null(a.c_rec + co, nc) || vc_any_null(a.p_rec + po, np);
            s = (ps == LDBG_CURSOR_NULLPOINTER || (ps == LDBG_CURSOR_OK && pe == LDBG_CURSOR_STOP && null_rec)) ? LDBG_VARIANT_NULLPOINTER
              : ps == LDBG_CURSOR_CAPACITY ? LDBG_VARIANT_CAPACITY
              : pe == LDBG_CURSOR_LIMIT ? LDBG_VARIANT_LIMIT
              : pe != LDBG_CURSOR_STOP ? LDBG_VARIANT_NOT_REACHED : LDBG_VARIANT_CALLED;
        }
        const bool called = s == LDBG_VARIANT_CALLED;
        // ---- coverages (:170-174, :202-206)
        int col = 0;
        for (int c = 0; c < a.g.C && c < 64; c++) {
            if (!((a.mask >> c) & 1ull)) continue;
            uint64_t mag = 0;
            const int64_t sum = called ? vc_cov_sum(a.g, a.c_rec + co, nc, -1, c, &mag) : 0;
            if (lane == 0) {
                a.child_sum[(size_t)i * a.ncol + col] = sum;
                a.child_flag[(size_t)i * a.ncol + col] = mag >= (1ull << 24) ? 1 : 0;
            }
            col++;
        }
        {
            uint64_t mag = 0;
            const int64_t sum = called ? vc_cov_sum(a.g, a.p_rec + po, np, LDBG_GLOBAL(const int64_t, a.c_rec)[co], a.stop_colour, &mag) : 0;
            if (lane == 0) { a.parent_sum[i] = sum; a.parent_flag[i] = mag >= (1ull << 24) ? 1 : 0; }
        }
        // ---- trimToAlleles (:406-433) on toContig of the two vertex lists
        if (called) {
            const VcContig c0{a.c_words + (size_t)co * W, a.c_words + (size_t)(co + 1) * W};
            const VcContig c1{a.c_words + (size_t)co * W, a.p_words + (size_t)po * W};
            const int L0 = (int)nc + k - 1, L1 = (int)np + 1 + k - 1, m = L0 < L1 ? L0 : L1;
            for (int t = 0; t < m; t += ws) {                  // the first index at which they differ within the shorter one, or 0
                const int x = t + lane;
                const bool differ = x < m && vc_base<W>(c0, k, x) != vc_base<W>(c1, k, x);
                const unsigned long long b = wave_ballot(differ);
                if (b) { st = t + __builtin_ctzll(b); break; }
            }
            e0 = L0; e1 = L1;
            for (int t = 0; t < m; t += ws) {                  // from the right, in step: i = L0 - 1 - q, j = L1 - 1 - q, both >= 0 for q < m
                const int q = t + lane, x = L0 - 1 - q, y = L1 - 1 - q;
                const bool stop = q < m && (vc_base<W>(c0, k, x) != vc_base<W>(c1, k, y) || x == st - 1 || y == st - 1);
                const unsigned long long b = wave_ballot(stop);
                if (b) { const int q0 = t + __builtin_ctzll(b); e0 = L0 - q0; e1 = L1 - q0; break; }
            }
        }
        if (lane == 0) {
            a.status[i] = (uint8_t)s;
            a.n_parent[i] = n_parent;
            a.st[i] = st; a.s0end[i] = e0; a.s1end[i] = e1;
            a.allele_len[2 * i] = (uint32_t)(e0 - st);
            a.allele_len[2 * i + 1] = (uint32_t)(e1 - st);
            bytes += (unsigned long long)(e0 - st) + (unsigned long long)(e1 - st);
        }
    }
    wave_fence();      // (host simulation: a lane that has left the kernel counts as inactive in a ballot the others have yet to read)
    if (lane == 0 && bytes) atomic_add_u64(a.total, bytes);
}

template <int W>
LDBG_WAVE_KERNEL void k_variant_alleles(VcArgs a) {
    const int ws = LDBG_WS, lane = wave_lane(), k = a.k;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    for (int64_t i = wave_uniform_i64(wave); i < a.n; i += nwaves) {
        if (a.status[i] != LDBG_VARIANT_CALLED) continue;
        const int64_t co = wave_uniform_i64(a.c_off[i]), po = wave_uniform_i64(a.p_off[i]);
        const VcContig c0{a.c_words + (size_t)co * W, a.c_words + (size_t)(co + 1) * W};
        const VcContig c1{a.c_words + (size_t)co * W, a.p_words + (size_t)po * W};
        const int st = a.st[i], n0 = a.s0end[i] - st, n1 = a.s1end[i] - st;
        uint8_t* d0 = a.alleles + a.allele_off[2 * i];
        uint8_t* d1 = a.alleles + a.allele_off[2 * i + 1];
        for (int b = lane; b < n0; b += ws) LDBG_GLOBAL(uint8_t, d0)[b] = vc_char(vc_base<W>(c0, k, st + b));
        for (int b = lane; b < n1; b += ws) LDBG_GLOBAL(uint8_t, d1)[b] = vc_char(vc_base<W>(c1, k, st + b));
    }
}

LDBG_KERNEL void k_variant_offsets(int64_t n, const uint32_t* off32, int64_t* offsets) {
    for (int64_t i = global_tid(); i <= n; i += global_nthreads()) offsets[i] = (int64_t)off32[i];
}

void check_engine(const Engine& e, const char* which) {
    check_whole_table(*e.graph, "variant batch");
    if (e.cfg.nlinks > 0 || !e.my_links.empty()) throw StatusError(LDBG_ERR_ARG, std::string("variant batch: the ") + which + " engine has links bound");
    if (e.cfg.n_recruitment > 0) throw StatusError(LDBG_ERR_ARG, std::string("variant batch: the ") + which + " engine has recruitment colours");
}

}  // namespace

VariantResult::~VariantResult() {
    for (void* p : {d_status, d_source_rec, d_dest_rec, d_n_child, d_n_parent, d_st, d_s0end, d_s1end, d_child_sum, d_child_flag, d_parent_sum, d_parent_flag,
                    d_allele_offsets, d_alleles})
        rt::dfree(p);
}

void VariantResult::get(const ldbg_variant_arrays& a, bool on_device, rt::stream_t s) const {
    rt::set_device(device);
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        if (!dst || !bytes) return;
        if (on_device) rt::d2d(dst, src, bytes, s); else rt::d2h(dst, src, bytes, s);
    };
    const size_t m = (size_t)n_colours;
    copy(a.status, d_status, (size_t)n);
    copy(a.source_rec, d_source_rec, (size_t)n * 8);
    copy(a.dest_rec, d_dest_rec, (size_t)n * 8);
    copy(a.n_child, d_n_child, (size_t)n * 4);
    copy(a.n_parent, d_n_parent, (size_t)n * 4);
    copy(a.st, d_st, (size_t)n * 4);
    copy(a.s0end, d_s0end, (size_t)n * 4);
    copy(a.s1end, d_s1end, (size_t)n * 4);
    copy(a.child_sum, d_child_sum, (size_t)n * m * 8);
    copy(a.child_flag, d_child_flag, (size_t)n * m);
    copy(a.parent_sum, d_parent_sum, (size_t)n * 8);
    copy(a.parent_flag, d_parent_flag, (size_t)n);
    copy(a.allele_offsets, d_allele_offsets, (size_t)(2 * n + 1) * 8);
    copy(a.alleles, d_alleles, (size_t)allele_bytes);
    if (!on_device) rt::stream_sync(s);
    if (child) child->get(a.child_offsets, a.child_words, a.child_rec, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, on_device, s);
    if (parent) parent->get(a.parent_offsets, a.parent_words, a.parent_rec, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, on_device, s);
}

VariantResult* variant_batch(Engine& child, CursorBatchHost& child_pool, Engine& parent, CursorBatchHost& parent_pool, const char* seeds, int64_t n, bool on_device,
                             int stop_colour, int64_t max_steps, uint64_t sum_mask) {
    check_engine(child, "child");
    check_engine(parent, "parent");
    if (child.graph != parent.graph) throw StatusError(LDBG_ERR_ARG, "variant batch: the two engines are over different graphs");
    const Graph& g = *child.graph;
    const int W = g.hdr.W, k = g.hdr.k, C = g.hdr.C;
    if (n < 0) throw StatusError(LDBG_ERR_ARG, "variant batch: n < 0");
    if (n > 0 && !seeds) throw StatusError(LDBG_ERR_ARG, "variant batch: null seeds");
    if (stop_colour < 0 || stop_colour >= C) throw StatusError(LDBG_ERR_ARG, "variant batch: colour " + std::to_string(stop_colour) + " of a graph of " + std::to_string(C));
    if (C < 64 && (sum_mask >> C) != 0ull) throw StatusError(LDBG_ERR_ARG, "variant batch: the mask names a colour the graph of " + std::to_string(C) + " does not have");
    std::unique_ptr<VariantResult> res(new VariantResult);
    res->device = g.device; res->W = W; res->k = k; res->n = n;
    res->n_colours = __builtin_popcountll(sum_mask);
    // ---- the first batch
    const ldbg_cursor_stop rule{stop_colour, 0, nullptr};
    res->child.reset(child_pool.run(seeds, n, on_device, LDBG_DIR_BOTH, max_steps, &rule));
    child.enter();
    rt::stream_t s = child.estream();
    res->d_allele_offsets = rt::dmalloc((size_t)(2 * n + 1) * 8);
    if (n == 0) {
        res->parent.reset(parent_pool.run(nullptr, 0, true, LDBG_DIR_FORWARD, max_steps, nullptr));
        rt::dmemset(res->d_allele_offsets, 0, 8, s);
        rt::stream_sync(s);
        profile_add("variants", 0.0);
        return res.release();
    }
    const size_t m = (size_t)std::max(1, res->n_colours);
    res->d_status = rt::dmalloc((size_t)n);
    res->d_source_rec = rt::dmalloc((size_t)n * 8); res->d_dest_rec = rt::dmalloc((size_t)n * 8);
    res->d_n_child = rt::dmalloc((size_t)n * 4); res->d_n_parent = rt::dmalloc((size_t)n * 4);
    res->d_st = rt::dmalloc((size_t)n * 4); res->d_s0end = rt::dmalloc((size_t)n * 4); res->d_s1end = rt::dmalloc((size_t)n * 4);
    res->d_child_sum = rt::dmalloc((size_t)n * m * 8); res->d_child_flag = rt::dmalloc((size_t)n * m);
    res->d_parent_sum = rt::dmalloc((size_t)n * 8); res->d_parent_flag = rt::dmalloc((size_t)n);
    struct Tmp { std::vector<void*> v; ~Tmp() { for (void* x : v) rt::tfree(x); } void* get(size_t b) { void* x = rt::tmalloc(b); v.push_back(x); return x; } } tmp;
    const int64_t n2 = 2 * n, nchunks = (n2 + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK;
    uint32_t* d_len = (uint32_t*)tmp.get((size_t)n2 * 4);
    uint32_t* d_off32 = (uint32_t*)tmp.get((size_t)(n2 + 1) * 4);
    uint32_t* d_sums = (uint32_t*)tmp.get((size_t)(nchunks + 1) * 4);
    uint32_t* d_offs = (uint32_t*)tmp.get((size_t)(nchunks + 1) * 4);
    unsigned long long* d_total = (unsigned long long*)tmp.get(8);
    VcArgs a{};
    a.g = child.view.g;
    a.n = n; a.k = k; a.stop_colour = stop_colour; a.ncol = res->n_colours; a.mask = sum_mask;
    const CursorBatchResult& cr = *res->child;
    a.c_off = (const int64_t*)cr.d_offsets; a.c_words = (const uint64_t*)cr.d_words; a.c_rec = (const int64_t*)cr.d_rec;
    a.c_end = (const uint8_t*)cr.d_end; a.c_status = (const uint8_t*)cr.d_status;
    a.seeds3 = (unsigned char*)tmp.get((size_t)n * k); a.targets3 = (unsigned char*)tmp.get((size_t)n * k);
    a.status = (uint8_t*)res->d_status; a.source_rec = (int64_t*)res->d_source_rec; a.dest_rec = (int64_t*)res->d_dest_rec;
    a.n_child = (int32_t*)res->d_n_child; a.n_parent = (int32_t*)res->d_n_parent;
    a.st = (int32_t*)res->d_st; a.s0end = (int32_t*)res->d_s0end; a.s1end = (int32_t*)res->d_s1end;
    a.child_sum = (int64_t*)res->d_child_sum; a.child_flag = (uint8_t*)res->d_child_flag;
    a.parent_sum = (int64_t*)res->d_parent_sum; a.parent_flag = (uint8_t*)res->d_parent_flag;
    a.allele_len = d_len; a.total = d_total;
    DevTimer tm;
    tm.begin(s);
    LDBG_LAUNCH_W(W, k_variant_chain, grid_for(n), 256, s, a);
    tm.end(s);                                   // (waits: the third batch runs on the parent engine's stream)
    // ---- the third batch: from the source until the destination, on the parent's engine
    const ldbg_cursor_stop until{-1, 0, (const char*)a.targets3};
    res->parent.reset(parent_pool.run((const char*)a.seeds3, n, true, LDBG_DIR_FORWARD, max_steps, &until));
    const CursorBatchResult& pr = *res->parent;
    a.p_off = (const int64_t*)pr.d_offsets; a.p_words = (const uint64_t*)pr.d_words; a.p_rec = (const int64_t*)pr.d_rec;
    a.p_end = (const uint8_t*)pr.d_end + n; a.p_status = (const uint8_t*)pr.d_status;
    child.enter();
    rt::dmemset(d_total, 0, 8, s);
    tm.begin(s);
    LDBG_LAUNCH_W(W, k_variant_call, waves_for(n), 64, s, a);
    scan_u32(d_len, n2, d_off32, d_sums, d_offs, s);
    LDBG_LAUNCH(k_variant_offsets, grid_for(n2 + 1), 256, s, n2, (const uint32_t*)d_off32, (int64_t*)res->d_allele_offsets);
    tm.end(s);
    unsigned long long total = 0;
    rt::d2h(&total, d_total, 8, s);
    rt::stream_sync(s);
    if (total >= (1ull << 32)) throw StatusError(LDBG_ERR_UNSUPPORTED, "variant batch: 2^32 allele bytes or more in one result (" + std::to_string(total) + "); split the batch");
    res->allele_bytes = (int64_t)total;
    res->d_alleles = rt::dmalloc((size_t)std::max<int64_t>(1, res->allele_bytes));
    a.allele_off = (const int64_t*)res->d_allele_offsets; a.alleles = (uint8_t*)res->d_alleles;
    tm.begin(s);
    LDBG_LAUNCH_W(W, k_variant_alleles, waves_for(n), 64, s, a);
    tm.end(s);
    rt::stream_sync(s);
    profile_add("variants", tm.ms);
    return res.release();
}

}  // namespace ldbg
