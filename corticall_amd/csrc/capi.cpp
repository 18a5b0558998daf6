// extern "C" surface of libldbg.so (include/ldbg.h).  Every entry point converts C++ exceptions
// into status codes + a thread-local message; there is no CPU fallback behind any of them.
#include <string.h>

#include <memory>

#include "build.h"
#include "cursor.h"
#include "engine_host.h"
#include "linkbuild.h"
#include "mosaic.h"
#include "seeds.h"
#include "select.h"
#include "shard.h"
#include "sw.h"
#include "thread.h"
#include "unitigs.h"
#include "variants.h"

using namespace ldbg;

namespace ldbg {
int64_t sort_ctx_file(const std::string& in_path, const std::string& out_path, int device);
int64_t subset_ctx_file(const std::string& in_path, const int64_t* indices, int64_t n, const std::string& out_path);
int64_t join_ctx_files(const std::vector<std::string>& paths, const std::string& out_path, int device);
std::vector<uint8_t> join_ctx_image(const std::vector<std::string>& paths, int device, bool find_view);
void profile_reset_all();
bool profile_get(const char* family, double* ms, int64_t* n);
}  // namespace ldbg

struct ldbg_graph {
    Graph g;
    ldbg_graph(const std::string& p, const void* img, int64_t n, int dev) : g(p, img, n, dev) {}
    ldbg_graph(const std::string& p, const void* hdr, int64_t hdr_bytes, const void* d_recs, int64_t n_recs, int dev) : g(p, hdr, hdr_bytes, d_recs, n_recs, dev) {}
};
struct ldbg_links {
    Links l;
    ldbg_links(const std::string& p, const Graph& g) : l(p, g) {}
    ldbg_links(const BuiltLinks& b, const Graph& g) : l(b, g) {}
};
struct ldbg_engine {
    Engine e;
    std::unique_ptr<CursorHost> cursor;
    std::unique_ptr<CursorBatchHost> cursor_batch;     // the pool of cursor slots, kept from batch to batch
    explicit ldbg_engine(const ldbg_engine_config& c) : e(c) {}
};
struct ldbg_dfs_result { std::unique_ptr<DfsBatch> b; };
struct ldbg_cursor_result { std::unique_ptr<CursorBatchResult> r; };
struct ldbg_variant_result { std::unique_ptr<VariantResult> r; };
struct ldbg_mosaic_result { std::unique_ptr<MosaicResult> r; };
struct ldbg_sw_result { std::unique_ptr<SwResult> r; };
struct ldbg_unitigs { Unitigs u; ldbg_unitigs(const Graph& g, const int* c, int n) : u(g, c, n) {} };
struct ldbg_selection {
    Selection s;
    ldbg_selection(const Graph& g, const ldbg_record_filter& f, const Graph* q) : s(g, f, q) {}
    ldbg_selection(const Graph& g, int child_colour, const Graph& dirty) : s(g, child_colour, dirty) {}
    explicit ldbg_selection(const Graph& g) : s(g) {}      // filled by variant_seeds
};
struct ldbg_threading {
    Threading t;
    ldbg_threading(const Graph* g, const Graph* rois, const char* bases, const int64_t* offsets, int64_t n, int flags, bool dev, rt::stream_t s)
        : t(g, rois, bases, offsets, n, flags, dev, s) {}
};
struct ldbg_occurrences { Occurrences o; explicit ldbg_occurrences(const Threading& t) : o(t) {} };
struct ldbg_image { ShardImage img; ldbg_image(const Graph& shard, int64_t cap, int64_t global) : img(shard, cap, global) {} };

namespace {
thread_local std::string g_err;
template <class F>
ldbg_status guard(F f) {
    try { f(); return LDBG_OK; }
    catch (const StatusError& e) { g_err = e.what(); return (ldbg_status)e.status; }
    catch (const std::bad_alloc&) { g_err = "out of host memory"; return LDBG_ERR_HIP; }
    catch (const std::exception& e) { g_err = e.what(); return LDBG_ERR_ARG; }
}
// the engine config refers to graphs/links through opaque handles; unwrap them for Engine
ldbg_engine_config unwrap(const ldbg_engine_config& c, std::vector<const ldbg_links*>& keep) {
    ldbg_engine_config u = c;
    u.graph = c.graph ? (const ldbg_graph*)&c.graph->g : nullptr;
    u.rois = c.rois ? (const ldbg_graph*)&c.rois->g : nullptr;
    keep.clear();
    for (int i = 0; i < c.nlinks; i++) keep.push_back(c.links[i] ? (const ldbg_links*)&c.links[i]->l : nullptr);
    u.links = keep.data();
    return u;
}
}  // namespace

extern "C" {

const char* ldbg_last_error(void) { return g_err.c_str(); }
#ifndef LDBG_SRCID
#define LDBG_SRCID "unstamped"
#endif
const char* ldbg_version(void) { return "ldbg 0.2 (gfx950, src " LDBG_SRCID ")"; }
ldbg_status ldbg_device_count(int* count) { *count = rt::device_count(); return LDBG_OK; }

ldbg_status ldbg_kmer_encode(const char* ascii, int k, uint64_t* words_out) {
    return guard([&] {
        if (k <= 0 || k > 128) throw StatusError(LDBG_ERR_ARG, "bad k");
        if (!ascii_to_words_ci(ascii, k, words_out, (k + 31) / 32))        // encodeBinaryKmer takes either case
            throw StatusError(LDBG_ERR_ARG, "Nucleotide is not a valid character nucleotide");
    });
}
ldbg_status ldbg_kmer_decode(const uint64_t* words, int k, char* ascii_out) {
    return guard([&] {
        if (k <= 0 || k > 128) throw StatusError(LDBG_ERR_ARG, "bad k");
        words_to_ascii(words, k, (k + 31) / 32, ascii_out);
        ascii_out[k] = 0;
    });
}

ldbg_status ldbg_sort_ctx(const char* in_path, const char* out_path, int device, int64_t* num_records) {
    return guard([&] { const int64_t n = sort_ctx_file(in_path, out_path, device); if (num_records) *num_records = n; });
}

ldbg_status ldbg_ctx_write_records(const char* in_path, const int64_t* indices, int64_t n, const char* out_path) {
    return guard([&] { subset_ctx_file(in_path, indices, n, out_path); });
}

ldbg_status ldbg_join_ctx(const char* const* in_paths, int n_paths, const char* out_path, int device, int64_t* num_records) {
    return guard([&] {
        std::vector<std::string> paths;
        for (int i = 0; i < n_paths; i++) paths.push_back(in_paths[i]);
        const int64_t n = join_ctx_files(paths, out_path, device);
        if (num_records) *num_records = n;
    });
}

// ---- graph
ldbg_status ldbg_graph_open(const char* path, int device, ldbg_graph** out) {
    return guard([&] { *out = nullptr; *out = new ldbg_graph(path, nullptr, 0, device); });
}
ldbg_status ldbg_graph_open_memory(const void* image, int64_t nbytes, int device, ldbg_graph** out) {
    return guard([&] { *out = nullptr; *out = new ldbg_graph("<memory>", image, nbytes, device); });
}
ldbg_status ldbg_graph_open_device(const void* header, int64_t header_bytes, const void* d_records, int64_t n_records, int device, ldbg_graph** out) {
    return guard([&] { *out = nullptr; *out = new ldbg_graph("<device>", header, header_bytes, d_records, n_records, device); });
}
// ---- graph construction: one device stage (build.cpp) ends with the packed records in device memory; the resident graph is laid
// out from them where they are (the route of ldbg_selection_open_graph), the file form downloads them once
ldbg_status ldbg_graph_build(const ldbg_build_sample* samples, int n_samples, int k, int flags, int device, ldbg_graph** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "build: null output");
        *out = nullptr;
        const BuiltRecords b = build_records(samples, n_samples, k, flags, device);
        *out = new ldbg_graph("<build>", b.header.data(), (int64_t)b.header.size(), b.d_records.get(), b.N, device);
    });
}
ldbg_status ldbg_graph_build_ctx(const ldbg_build_sample* samples, int n_samples, int k, int flags, int device, const char* out_path, int64_t* num_records) {
    return guard([&] {
        if (!out_path) throw StatusError(LDBG_ERR_ARG, "build: null output path");
        const BuiltRecords b = build_records(samples, n_samples, k, flags, device);
        build_write_ctx(b, out_path);
        if (num_records) *num_records = b.N;
    });
}
ldbg_status ldbg_graph_open_collection(const char* const* paths, int n_paths, int find_view, int device, ldbg_graph** out) {
    return guard([&] {
        *out = nullptr;
        std::vector<std::string> ps;
        for (int i = 0; i < n_paths; i++) ps.push_back(paths[i]);
        const std::vector<uint8_t> img = join_ctx_image(ps, device, find_view != 0);
        *out = new ldbg_graph("<collection>", img.data(), (int64_t)img.size(), device);
    });
}
ldbg_status ldbg_graph_close(ldbg_graph* g) { return guard([&] { delete g; }); }
ldbg_status ldbg_graph_info(const ldbg_graph* g, int* k, int* W, int* C, int64_t* N, int* version) {
    return guard([&] {
        if (k) *k = g->g.hdr.k;
        if (W) *W = g->g.hdr.W;
        if (C) *C = g->g.hdr.C;
        if (N) *N = g->g.hdr.num_records;
        if (version) *version = g->g.hdr.version;
    });
}
ldbg_status ldbg_graph_device(const ldbg_graph* g, int* device) { *device = g->g.device; return LDBG_OK; }
ldbg_status ldbg_graph_set_shard(ldbg_graph* g, int is_shard) {
    return guard([&] { g->g.view.java_tiny = (!is_shard && g->g.view.N <= 2) ? 1 : 0; g->g.is_shard = is_shard != 0; });
}
ldbg_status ldbg_graph_sample_name(const ldbg_graph* g, int color, char* buf, int buflen) {
    return guard([&] {
        if (color < 0 || color >= g->g.hdr.C) throw StatusError(LDBG_ERR_ARG, "colour out of range");
        snprintf(buf, buflen, "%s", g->g.hdr.colors[color].sample_name.c_str());
    });
}
ldbg_status ldbg_graph_color_info(const ldbg_graph* g, int color, ldbg_color_info* out, char* name, int buflen) {
    return guard([&] {
        if (color < 0 || color >= g->g.hdr.C) throw StatusError(LDBG_ERR_ARG, "colour out of range");
        const CtxColor& c = g->g.hdr.colors[color];
        out->mean_read_length = c.mean_read_length;
        out->total_sequence = c.total_sequence;
        out->tip_clipping = c.tip_clipping;
        out->low_covg_supernodes_removed = c.low_covg_supernodes_removed;
        out->low_covg_kmers_removed = c.low_covg_kmers_removed;
        out->cleaned_against_graph = c.cleaned_against_graph;
        out->low_cov_supernodes_threshold = c.low_cov_supernodes_threshold;
        out->low_cov_kmer_threshold = c.low_cov_kmer_threshold;
        if (name) snprintf(name, buflen, "%s", c.cleaned_against_graph_name.c_str());
    });
}
ldbg_status ldbg_graph_color_for_sample_name(const ldbg_graph* g, const char* name, int* color) {
    return guard([&] { *color = g->g.color_for_sample_name(name); });
}

ldbg_status ldbg_graph_records_dev(const ldbg_graph* g, int64_t first, int64_t n, uint64_t* d_words, uint32_t* d_cov, uint8_t* d_edges, void* stream) {
    return guard([&] {
        if (first < 0 || n < 0 || first + n > g->g.hdr.num_records) throw StatusError(LDBG_ERR_ARG, "record range outside 0.." + std::to_string(g->g.hdr.num_records));
        rt::set_device(g->g.device);
        g->g.records_dev(first, n, d_words, d_cov, d_edges, stream ? (rt::stream_t)stream : g->g.stream);
    });
}
ldbg_status ldbg_graph_records(const ldbg_graph* g, int64_t first, int64_t n, uint64_t* words, uint32_t* cov, uint8_t* edges) {
    return guard([&] {
        if (first < 0 || n < 0 || first + n > g->g.hdr.num_records) throw StatusError(LDBG_ERR_ARG, "record range outside 0.." + std::to_string(g->g.hdr.num_records));
        if (n == 0) return;
        rt::set_device(g->g.device);
        const int W = g->g.hdr.W, C = g->g.hdr.C;
        rt::stream_t s = g->g.stream;
        uint64_t* dw = (uint64_t*)rt::dmalloc((size_t)n * W * 8);
        uint32_t* dc = cov ? (uint32_t*)rt::dmalloc((size_t)n * C * 4) : nullptr;
        uint8_t* de = edges ? (uint8_t*)rt::dmalloc((size_t)n * C) : nullptr;
        g->g.records_dev(first, n, dw, dc, de, s);
        if (words) rt::d2h(words, dw, (size_t)n * W * 8, s);
        if (cov) rt::d2h(cov, dc, (size_t)n * C * 4, s);
        if (edges) rt::d2h(edges, de, (size_t)n * C, s);
        rt::stream_sync(s);
        rt::dfree(dw); rt::dfree(dc); rt::dfree(de);
    });
}

ldbg_status ldbg_graph_find_dev(const ldbg_graph* g, const uint64_t* d_packed, int64_t n, int64_t* d_idx, uint32_t* d_cov, uint8_t* d_edges, void* stream) {
    return guard([&] {
        rt::set_device(g->g.device);
        g->g.find_dev(d_packed, n, d_idx, d_cov, d_edges, stream ? (rt::stream_t)stream : g->g.stream);
    });
}
ldbg_status ldbg_shard_owner_dev(int k, const uint64_t* d_packed, int64_t n, int world, uint64_t* d_canon, int32_t* d_owner, void* stream) {
    return guard([&] {
        shard_owner_dev(k, d_packed, n, world, d_canon, d_owner, (rt::stream_t)stream);
        rt::stream_sync((rt::stream_t)stream);
    });
}
ldbg_status ldbg_shard_owner(int k, const uint64_t* packed, int64_t n, int world, int device, int32_t* owner) {
    return guard([&] {
        if (n <= 0) return;
        if (rt::device_count() <= device) throw StatusError(LDBG_ERR_HIP, "no HIP device " + std::to_string(device) + " available (libldbg has no CPU fallback)");
        rt::set_device(device);
        const int W = (k + 31) / 32;
        rt::stream_t s = rt::stream_create();
        uint64_t* dq = (uint64_t*)rt::dmalloc((size_t)n * W * 8);
        int32_t* d_o = (int32_t*)rt::dmalloc((size_t)n * 4);
        rt::h2d(dq, packed, (size_t)n * W * 8, s);
        shard_owner_dev(k, dq, n, world, nullptr, d_o, s);
        rt::d2h(owner, d_o, (size_t)n * 4, s);
        rt::stream_sync(s);
        rt::dfree(dq); rt::dfree(d_o);
        rt::stream_destroy(s);
    });
}
ldbg_status ldbg_shard_nbr_queries(const ldbg_graph* g, int64_t first, int64_t n, uint64_t* d_words, uint8_t* d_flips, uint8_t* d_have) {
    return guard([&] { rt::set_device(g->g.device); shard_nbr_queries(g->g, first, n, d_words, d_flips, d_have); });
}
ldbg_status ldbg_shard_set_nbr(ldbg_graph* g, int64_t first, int64_t n, const int32_t* d_owner, const int64_t* d_lidx, const uint8_t* d_flips) {
    return guard([&] { rt::set_device(g->g.device); shard_set_nbr(g->g, first, n, d_owner, d_lidx, d_flips); });
}
// ---- the local image of a hash-sharded table (image.h) and walks over it, one bulk-synchronous round at a time
ldbg_status ldbg_image_create(const ldbg_graph* shard, int64_t cap, int64_t global_records, ldbg_image** out) {
    return guard([&] {
        *out = nullptr;
        if (cap < 1 || cap > ldbg::max_records_per_device()) throw StatusError(LDBG_ERR_ARG, "image capacity out of range");
        *out = new ldbg_image(shard->g, cap, global_records);
    });
}
ldbg_status ldbg_image_destroy(ldbg_image* im) { return guard([&] { delete im; }); }
ldbg_status ldbg_image_graph(ldbg_image* im, ldbg_graph** g) { return guard([&] { *g = reinterpret_cast<ldbg_graph*>(&im->img.graph()); }); }
ldbg_status ldbg_image_row_bytes(const ldbg_image* im, int* bytes) { return guard([&] { *bytes = im->img.row_bytes(); }); }
ldbg_status ldbg_image_clear(ldbg_image* im) { return guard([&] { rt::set_device(im->img.graph().device); im->img.clear(); }); }
static rt::stream_t image_stream(const ldbg_image* im, void* stream) { return stream ? (rt::stream_t)stream : im->img.graph().stream; }
ldbg_status ldbg_image_serve(const ldbg_image* im, int my_rank, const uint64_t* d_keys, int64_t n, uint8_t* d_out, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.serve(my_rank, (const unsigned long long*)d_keys, n, 1, d_out, image_stream(im, stream)); });
}
ldbg_status ldbg_image_serve_chain(const ldbg_image* im, int my_rank, const uint64_t* d_keys, int64_t n, int depth, uint8_t* d_out, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.serve(my_rank, (const unsigned long long*)d_keys, n, depth, d_out, image_stream(im, stream)); });
}
ldbg_status ldbg_image_insert(ldbg_image* im, const ldbg_engine* e, const uint8_t* d_rows, int64_t n, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.insert(e ? &e->e : nullptr, d_rows, n, image_stream(im, stream)); });
}
ldbg_status ldbg_image_lookup(const ldbg_image* im, const uint64_t* d_keys, int64_t n, int32_t* d_slots, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.lookup((const unsigned long long*)d_keys, n, d_slots, image_stream(im, stream)); });
}
ldbg_status ldbg_image_bucket(ldbg_image* im, int world, uint32_t cap_per_owner, uint64_t* d_send, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.bucket(world, cap_per_owner, (unsigned long long*)d_send, image_stream(im, stream)); });
}
ldbg_status ldbg_image_request(ldbg_image* im, const uint64_t* d_keys, int64_t n, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.request((const unsigned long long*)d_keys, n, image_stream(im, stream)); });
}
ldbg_status ldbg_image_reset_requests(ldbg_image* im, void* stream) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.reset_requests(image_stream(im, stream)); });
}
ldbg_status ldbg_image_counters(const ldbg_image* im, int64_t* n_rows, int64_t* n_req, int* overflow) {
    return guard([&] { rt::set_device(im->img.graph().device); im->img.counters(n_rows, n_req, overflow); });
}
ldbg_status ldbg_engine_sharded_walk_begin(ldbg_engine* e, ldbg_image* im, const char* seeds, int64_t n, const int32_t* d_seed_slot, void* stream) {
    return guard([&] { e->e.sharded_walk_begin(im->img, seeds, n, d_seed_slot, (rt::stream_t)stream); });
}
ldbg_status ldbg_engine_sharded_walk_round(ldbg_engine* e, int64_t* d_stats) { return guard([&] { e->e.sharded_walk_round(d_stats); }); }
ldbg_status ldbg_engine_sharded_walk_finish(ldbg_engine* e, int64_t* total_bytes, int64_t* traversed) {
    return guard([&] {
        try { e->e.sharded_walk_finish(total_bytes, traversed); }
        catch (const StatusError& se) {
            // a full per-walk link store: the next batch of this engine gets a larger one (the caller walks the batch again — exactness
            // is never traded away; ldbg_engine_walk_batch_run does the same retry inside the call)
            if (se.status == LDBG_ERR_CAPACITY && std::string(se.what()) == "LINKSTORE_FULL") e->e.link_store_capacity *= 4;
            throw;
        }
    });
}

ldbg_status ldbg_graph_find(const ldbg_graph* g, const uint64_t* packed, int64_t n, int64_t* idx_out, uint32_t* cov_out, uint8_t* edges_out) {
    return guard([&] {
        if (n <= 0) return;
        rt::set_device(g->g.device);
        const int W = g->g.hdr.W, C = g->g.hdr.C;
        rt::stream_t s = g->g.stream;
        uint64_t* dq = (uint64_t*)rt::dmalloc((size_t)n * W * 8);
        int64_t* di = (int64_t*)rt::dmalloc((size_t)n * 8);
        uint32_t* dc = cov_out ? (uint32_t*)rt::dmalloc((size_t)n * C * 4) : nullptr;
        uint8_t* de = edges_out ? (uint8_t*)rt::dmalloc((size_t)n * C) : nullptr;
        rt::h2d(dq, packed, (size_t)n * W * 8, s);
        g->g.find_dev(dq, n, di, dc, de, s);
        rt::d2h(idx_out, di, (size_t)n * 8, s);
        if (cov_out) rt::d2h(cov_out, dc, (size_t)n * C * 4, s);
        if (edges_out) rt::d2h(edges_out, de, (size_t)n * C, s);
        rt::stream_sync(s);
        rt::dfree(dq); rt::dfree(di); rt::dfree(dc); rt::dfree(de);
    });
}
ldbg_status ldbg_graph_find_ascii(const ldbg_graph* g, const char* kmers, int64_t n, int64_t* idx_out, uint32_t* cov_out, uint8_t* edges_out) {
    return guard([&] {
        rt::set_device(g->g.device);
        const int W = g->g.hdr.W, k = g->g.hdr.k, C = g->g.hdr.C;
        if (n <= 0) return;
        std::vector<uint64_t> packed((size_t)n * W);
        std::vector<uint8_t> valid((size_t)n);
        ascii_batch_to_words(kmers, n, k, W, packed.data(), valid.data());      // Q4: a string with a non-ACGT byte never matches
        rt::stream_t s = g->g.stream;
        DevBlocks tmp;
        uint64_t* dq = tmp.get<uint64_t>((size_t)n * W);
        uint8_t* dv = tmp.get<uint8_t>((size_t)n);
        int64_t* di = tmp.get<int64_t>((size_t)n);
        uint32_t* dc = cov_out ? tmp.get<uint32_t>((size_t)n * C) : nullptr;
        uint8_t* de = edges_out ? tmp.get<uint8_t>((size_t)n * C) : nullptr;
        rt::h2d(dq, packed.data(), (size_t)n * W * 8, s);
        rt::h2d(dv, valid.data(), (size_t)n, s);
        g->g.find_dev(dq, n, di, dc, de, s, dv);
        rt::d2h(idx_out, di, (size_t)n * 8, s);
        if (cov_out) rt::d2h(cov_out, dc, (size_t)n * C * 4, s);
        if (edges_out) rt::d2h(edges_out, de, (size_t)n * C, s);
        rt::stream_sync(s);
    });
}

// ---- unitigs
ldbg_status ldbg_graph_unitigs(const ldbg_graph* g, const int* colors, int n_colors, ldbg_unitigs** out) {
    return guard([&] {
        *out = nullptr;
        if (!colors && n_colors > 0) throw StatusError(LDBG_ERR_ARG, "unitigs: null colours");
        *out = new ldbg_unitigs(g->g, colors, n_colors);
    });
}
ldbg_status ldbg_unitigs_info(const ldbg_unitigs* u, int64_t* count, int64_t* total_bases, int64_t* longest, double* build_ms) {
    return guard([&] {
        if (count) *count = u->u.count;
        if (total_bases) *total_bases = u->u.total_bases;
        if (longest) *longest = u->u.longest;
        if (build_ms) *build_ms = u->u.build_ms;
    });
}
ldbg_status ldbg_unitigs_get(const ldbg_unitigs* u, int64_t first, int64_t n, int64_t* offsets, char* bases, int64_t capacity) {
    return guard([&] { u->u.get(first, n, offsets, bases, capacity, false, u->u.graph.stream); });
}
ldbg_status ldbg_unitigs_get_dev(const ldbg_unitigs* u, int64_t first, int64_t n, int64_t* d_offsets, char* d_bases, int64_t capacity, void* stream) {
    return guard([&] { u->u.get(first, n, d_offsets, d_bases, capacity, true, stream ? (rt::stream_t)stream : u->u.graph.stream); });
}
ldbg_status ldbg_unitigs_coverage(const ldbg_unitigs* u, int64_t first, int64_t n, uint32_t* cov) { return guard([&] { u->u.coverage(first, n, cov); }); }
ldbg_status ldbg_unitigs_of_records(const ldbg_unitigs* u, const int64_t* records, int64_t n, int64_t* unitig, int64_t* position, int8_t* orientation) {
    return guard([&] { u->u.of_records(records, n, unitig, position, orientation); });
}
ldbg_status ldbg_unitigs_write_fasta(const ldbg_unitigs* u, const char* path) { return guard([&] { u->u.write_fasta(path); }); }
ldbg_status ldbg_unitigs_write_gfa1(const ldbg_unitigs* u, const char* path, int sample_color, int flags) {
    return guard([&] { u->u.write_gfa1(path, sample_color, flags); });
}
ldbg_status ldbg_unitigs_free(ldbg_unitigs* u) { return guard([&] { delete u; }); }

// ---- record selection
ldbg_status ldbg_graph_select(const ldbg_graph* g, const ldbg_record_filter* filter, ldbg_selection** out) {
    return guard([&] {
        *out = nullptr;
        if (!filter) throw StatusError(LDBG_ERR_ARG, "select: null filter");
        *out = new ldbg_selection(g->g, *filter, nullptr);
    });
}
ldbg_status ldbg_graph_select_lookup(const ldbg_graph* g, const ldbg_record_filter* filter, const ldbg_graph* q, ldbg_selection** out) {
    return guard([&] {
        *out = nullptr;
        if (!filter || !q) throw StatusError(LDBG_ERR_ARG, "select: null filter or query graph");
        *out = new ldbg_selection(g->g, *filter, &q->g);
    });
}
ldbg_status ldbg_selection_count(const ldbg_selection* sel, int64_t* n) { return guard([&] { *n = sel->s.count; }); }
ldbg_status ldbg_selection_indices(const ldbg_selection* sel, int64_t first, int64_t n, int64_t* idx) {
    return guard([&] { sel->s.indices(first, n, idx, false, sel->s.graph.stream); });
}
ldbg_status ldbg_selection_indices_dev(const ldbg_selection* sel, int64_t first, int64_t n, int64_t* d_idx, void* stream) {
    return guard([&] { sel->s.indices(first, n, d_idx, true, stream ? (rt::stream_t)stream : sel->s.graph.stream); });
}
ldbg_status ldbg_selection_write_ctx(const ldbg_selection* sel, const int* colours, int n_colours, const char* header_path, const char* out_path) {
    return guard([&] { sel->s.write_ctx(colours, n_colours, header_path, out_path); });
}
ldbg_status ldbg_selection_open_graph(const ldbg_selection* sel, const int* colours, int n_colours, const char* header_path, ldbg_graph** out) {
    return guard([&] {
        *out = nullptr;
        const std::vector<uint8_t> hdr = sel->s.header(colours, n_colours, header_path);
        const DevRecords d = sel->s.pack(colours, n_colours);
        *out = new ldbg_graph("<selection>", hdr.data(), (int64_t)hdr.size(), d.get(), sel->s.count, sel->s.graph.device);
    });
}
ldbg_status ldbg_selection_free(ldbg_selection* sel) { return guard([&] { delete sel; }); }

// ---- RecoverExcludedKmers: a selection with a join (select.cpp)
ldbg_status ldbg_graph_recover(const ldbg_graph* g, int child_colour, const ldbg_graph* dirty, ldbg_selection** out, int64_t* n_recovered) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "recover: null output");
        *out = nullptr;
        if (!g || !dirty) throw StatusError(LDBG_ERR_ARG, "recover: null graph");
        *out = new ldbg_selection(g->g, child_colour, dirty->g);
        if (n_recovered) *n_recovered = (*out)->s.n_recovered;
    });
}
ldbg_status ldbg_selection_recovered_coverage(const ldbg_selection* sel, int64_t first, int64_t n, int32_t* cov) {
    return guard([&] { sel->s.recovered_coverage(first, n, cov); });
}
ldbg_status ldbg_selection_write_recovered(const ldbg_selection* sel, const char* out_path) {
    return guard([&] {
        if (!out_path) throw StatusError(LDBG_ERR_ARG, "recover: null output path");
        sel->s.write_recovered(out_path);
    });
}
ldbg_status ldbg_selection_open_recovered(const ldbg_selection* sel, ldbg_graph** out) {
    return guard([&] {
        *out = nullptr;
        const std::vector<uint8_t> hdr = sel->s.recovered_header();
        const DevRecords d = sel->s.pack_recovered();
        *out = new ldbg_graph("<recovered>", hdr.data(), (int64_t)hdr.size(), d.get(), sel->s.count, sel->s.graph.device);
    });
}

// ---- links
ldbg_status ldbg_links_open(const char* path, const ldbg_graph* g, ldbg_links** out) {
    return guard([&] { *out = nullptr; *out = new ldbg_links(path, g->g); });
}
// ---- links construction: the device stage (linkbuild.cpp) ends with the records in the file's order on the host; the file form writes
// their text, the resident form binds them as ldbg_links_open binds the records it has parsed
ldbg_status ldbg_links_build_ctp(const ldbg_graph* g, const char* sample_name, const char* bases, const int64_t* offsets, int64_t n_reads, int flags,
                                 const char* out_path, int64_t* num_kmers_with_links, int64_t* num_links) {
    return guard([&] {
        if (!g) throw StatusError(LDBG_ERR_ARG, "links build: null graph");
        if (!out_path) throw StatusError(LDBG_ERR_ARG, "links build: null output path");
        const BuiltLinks b = build_links(g->g, sample_name, bases, offsets, n_reads, flags);
        built_links_write(b, out_path);
        if (num_kmers_with_links) *num_kmers_with_links = (int64_t)b.records.size();
        if (num_links) *num_links = b.num_links;
    });
}
ldbg_status ldbg_links_build(const ldbg_graph* g, const char* sample_name, const char* bases, const int64_t* offsets, int64_t n_reads, int flags, ldbg_links** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "links build: null output");
        *out = nullptr;
        if (!g) throw StatusError(LDBG_ERR_ARG, "links build: null graph");
        const BuiltLinks b = build_links(g->g, sample_name, bases, offsets, n_reads, flags);
        *out = new ldbg_links(b, g->g);
    });
}
// ---- sequences threaded through a graph (thread.cpp)
ldbg_status ldbg_graph_thread(const ldbg_graph* g, const ldbg_graph* rois, const char* bases, const int64_t* offsets, int64_t n_seqs, int flags, ldbg_threading** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "thread: null output");
        *out = nullptr;
        *out = new ldbg_threading(g ? &g->g : nullptr, rois ? &rois->g : nullptr, bases, offsets, n_seqs, flags, false, nullptr);
    });
}
ldbg_status ldbg_graph_thread_dev(const ldbg_graph* g, const ldbg_graph* rois, const void* d_bases, const void* d_offsets, int64_t n_seqs, int flags, void* stream,
                                  ldbg_threading** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "thread: null output");
        *out = nullptr;
        *out = new ldbg_threading(g ? &g->g : nullptr, rois ? &rois->g : nullptr, (const char*)d_bases, (const int64_t*)d_offsets, n_seqs, flags, true, (rt::stream_t)stream);
    });
}
ldbg_status ldbg_threading_info(const ldbg_threading* t, int64_t* n_seqs, int64_t* n_windows, int64_t* n_regions, double* device_ms) {
    return guard([&] {
        if (!t) throw StatusError(LDBG_ERR_ARG, "thread: null threading");
        if (n_seqs) *n_seqs = t->t.n_seqs;
        if (n_windows) *n_windows = t->t.n_windows;
        if (n_regions) *n_regions = t->t.n_regions;
        if (device_ms) *device_ms = t->t.device_ms;
    });
}
ldbg_status ldbg_threading_windows(const ldbg_threading* t, int64_t first, int64_t n, int64_t* rec, uint8_t* info, int32_t* copy_index) {
    return guard([&] {
        if (!t) throw StatusError(LDBG_ERR_ARG, "thread: null threading");
        t->t.windows(first, n, rec, info, copy_index, false, nullptr);
    });
}
ldbg_status ldbg_threading_windows_dev(const ldbg_threading* t, int64_t first, int64_t n, void* d_rec, void* d_info, void* d_copy_index, void* stream) {
    return guard([&] {
        if (!t) throw StatusError(LDBG_ERR_ARG, "thread: null threading");
        t->t.windows(first, n, (int64_t*)d_rec, (uint8_t*)d_info, (int32_t*)d_copy_index, true, (rt::stream_t)stream);
    });
}
ldbg_status ldbg_threading_coverage(const ldbg_threading* t, int colour, int64_t first, int64_t n, int32_t* cov) {
    return guard([&] {
        if (!t) throw StatusError(LDBG_ERR_ARG, "thread: null threading");
        t->t.coverage(colour, first, n, cov);
    });
}
ldbg_status ldbg_threading_summary(const ldbg_threading* t, int64_t first_seq, int64_t n, int64_t* win_start, int32_t* first_hit, int32_t* last_hit, int32_t* n_hits,
                                   int32_t* n_distinct, uint8_t* ends) {
    return guard([&] {
        if (!t) throw StatusError(LDBG_ERR_ARG, "thread: null threading");
        t->t.summary(first_seq, n, win_start, first_hit, last_hit, n_hits, n_distinct, ends);
    });
}
ldbg_status ldbg_threading_regions(const ldbg_threading* t, int64_t* region_offsets, int32_t* start, int32_t* stop, int64_t capacity) {
    return guard([&] {
        if (!t) throw StatusError(LDBG_ERR_ARG, "thread: null threading");
        t->t.regions(region_offsets, start, stop, capacity);
    });
}
ldbg_status ldbg_threading_free(ldbg_threading* t) { return guard([&] { delete t; }); }

// ---- occurrences of a threading and the seed pass (seeds.cpp)
ldbg_status ldbg_threading_occurrences(const ldbg_threading* t, ldbg_occurrences** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "occurrences: null output");
        *out = nullptr;
        if (!t) throw StatusError(LDBG_ERR_ARG, "occurrences: null threading");
        *out = new ldbg_occurrences(t->t);
    });
}
ldbg_status ldbg_occurrences_info(const ldbg_occurrences* o, int64_t* n_records, double* device_ms) {
    return guard([&] {
        if (!o) throw StatusError(LDBG_ERR_ARG, "occurrences: null handle");
        if (n_records) *n_records = o->o.n_records;
        if (device_ms) *device_ms = o->o.device_ms;
    });
}
ldbg_status ldbg_occurrences_get(const ldbg_occurrences* o, int64_t first_rec, int64_t n, uint32_t* count, int64_t* first_window) {
    return guard([&] {
        if (!o) throw StatusError(LDBG_ERR_ARG, "occurrences: null handle");
        o->o.get(first_rec, n, count, first_window, false, nullptr);
    });
}
ldbg_status ldbg_occurrences_get_dev(const ldbg_occurrences* o, int64_t first_rec, int64_t n, void* d_count, void* d_first_window, void* stream) {
    return guard([&] {
        if (!o) throw StatusError(LDBG_ERR_ARG, "occurrences: null handle");
        o->o.get(first_rec, n, (uint32_t*)d_count, (int64_t*)d_first_window, true, (rt::stream_t)stream);
    });
}
ldbg_status ldbg_occurrences_free(ldbg_occurrences* o) { return guard([&] { delete o; }); }
ldbg_status ldbg_graph_variant_seeds(const ldbg_graph* g, const ldbg_seed_filter* filter, ldbg_selection** out, ldbg_seed_counts* counts) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "variant seeds: null output");
        *out = nullptr;
        if (!g) throw StatusError(LDBG_ERR_ARG, "variant seeds: null graph");
        if (!filter) throw StatusError(LDBG_ERR_ARG, "variant seeds: null filter");
        if (filter->n_covered < 0 || filter->n_covered > LDBG_SEED_MAX_COVERED) throw StatusError(LDBG_ERR_ARG, "variant seeds: more covered clauses than the filter holds");
        if (filter->n_unique < 0 || filter->n_unique > LDBG_SEED_MAX_UNIQUE) throw StatusError(LDBG_ERR_ARG, "variant seeds: more unique entries than the filter holds");
        SeedFilter f;
        f.all_zero = filter->all_zero;
        f.n_covered = filter->n_covered;
        for (int j = 0; j < f.n_covered; j++) f.covered[j] = filter->covered[j];
        f.n_unique = filter->n_unique;
        for (int j = 0; j < f.n_unique; j++)
            f.unique[j] = SeedUnique{filter->unique[j].colour, filter->unique[j].occurrences ? &filter->unique[j].occurrences->o : nullptr, (const uint8_t*)filter->unique[j].d_unique};
        std::unique_ptr<ldbg_selection> sel(new ldbg_selection(g->g));
        variant_seeds(sel->s, f, counts);
        *out = sel.release();
    });
}

ldbg_status ldbg_links_close(ldbg_links* l) { return guard([&] { delete l; }); }
ldbg_status ldbg_links_index(const char* in_path, const char* out_path, const char* source, int64_t* num_records) {
    return guard([&] { const int64_t n = links_index_file(in_path, out_path, source ? source : ""); if (num_records) *num_records = n; });
}
ldbg_status ldbg_links_source(const ldbg_links* l, char* buf, int buflen) { return guard([&] { snprintf(buf, buflen, "%s", l->l.source().c_str()); }); }
ldbg_status ldbg_links_info(const ldbg_links* l, int* version, int* num_colors, int* k, int64_t* nkg, int64_t* nkl, int64_t* nl) {
    return guard([&] {
        if (version) *version = l->l.version;
        if (num_colors) *num_colors = l->l.num_colors;
        if (k) *k = l->l.k;
        if (nkg) *nkg = l->l.num_kmers_in_graph;
        if (nkl) *nkl = l->l.num_kmers_with_links;
        if (nl) *nl = l->l.num_links;
    });
}
ldbg_status ldbg_links_sample_name(const ldbg_links* l, int color, char* buf, int buflen) {
    return guard([&] {
        if (color < 0 || color >= (int)l->l.sample_names.size()) throw StatusError(LDBG_ERR_ARG, "colour out of range");
        snprintf(buf, buflen, "%s", l->l.sample_names[color].c_str());
    });
}
ldbg_status ldbg_links_get(const ldbg_links* l, const char* kmer, int* found, char* buf, int64_t buflen) {
    return guard([&] {
        const HostLinksRecord* r = l->l.get(std::string(kmer, l->l.k));
        *found = r ? 1 : 0;
        std::string s;
        if (r) {
            s = r->kmer + " " + std::to_string(r->juncs.size()) + "\n";
            for (auto& j : r->juncs) {
                s += j.is_fw ? "F " : "R ";
                s += std::to_string(j.num_junctions) + " ";
                for (size_t c = 0; c < j.cov.size(); c++) { if (c) s += ","; s += std::to_string(j.cov[c]); }
                s += " " + j.junctions + "\n";
            }
        }
        if ((int64_t)s.size() + 1 > buflen) throw StatusError(LDBG_ERR_CAPACITY, "buffer too small: need " + std::to_string(s.size() + 1));
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

// ---- engine
void ldbg_engine_config_default(ldbg_engine_config* c) {
    memset(c, 0, sizeof(*c));
    c->direction = LDBG_DIR_BOTH;
    c->combination_operator = LDBG_OP_OR;
    c->stopping_rule = LDBG_STOP_CONTIG;
    c->max_branch_length = 75000;
    c->connect_all_neighbors = 0;
    c->strict_java_flip = 1;
}
ldbg_status ldbg_engine_create(const ldbg_engine_config* cfg, ldbg_engine** out) {
    return guard([&] {
        *out = nullptr;
        if (cfg->n_traversal > LDBG_MAX_COLORS || cfg->n_joining > LDBG_MAX_COLORS || cfg->n_recruitment > LDBG_MAX_COLORS || cfg->n_secondary > LDBG_MAX_COLORS)
            throw StatusError(LDBG_ERR_ARG, "too many colours");
        std::vector<const ldbg_links*> keep;
        ldbg_engine_config u = unwrap(*cfg, keep);
        *out = new ldbg_engine(u);
    });
}
ldbg_status ldbg_engine_destroy(ldbg_engine* e) { return guard([&] { delete e; }); }

static ldbg_status walk_batch_run_any(ldbg_engine* e, const char* seeds, int64_t n, int64_t* total_bytes, int64_t* traversed, bool on_device) {
    return guard([&] {
        // a full per-walk link store is retried with a larger one (exactness is never traded away)
        for (int attempt = 0;; attempt++) {
            try { e->e.walk_batch_run(seeds, n, total_bytes, traversed, on_device); return; }
            catch (const StatusError& se) {
                if (se.status == LDBG_ERR_CAPACITY && std::string(se.what()) == "LINKSTORE_FULL" && attempt < 8) { e->e.link_store_capacity *= 4; continue; }
                throw;
            }
        }
    });
}
ldbg_status ldbg_engine_walk_batch_run(ldbg_engine* e, const char* seeds, int64_t n, int64_t* total_bytes, int64_t* traversed) {
    return walk_batch_run_any(e, seeds, n, total_bytes, traversed, false);
}
ldbg_status ldbg_engine_walk_batch_run_device(ldbg_engine* e, const void* d_seeds, int64_t n, int64_t* total_bytes, int64_t* traversed) {
    if (n > 0 && !d_seeds) return guard([&] { throw StatusError(LDBG_ERR_ARG, "ldbg_engine_walk_batch_run_device: null seeds"); });
    return walk_batch_run_any(e, (const char*)d_seeds, n, total_bytes, traversed, true);
}
ldbg_status ldbg_host_alloc(int64_t bytes, void** out) {
    return guard([&] { *out = nullptr; if (bytes < 0) throw StatusError(LDBG_ERR_ARG, "ldbg_host_alloc: negative size"); *out = rt::hmalloc_pinned((size_t)bytes); });
}
ldbg_status ldbg_host_free(void* p) { return guard([&] { rt::hfree_pinned(p); }); }
ldbg_status ldbg_engine_walk_batch_fetch(ldbg_engine* e, char* arena, int64_t cap, int64_t* offsets, int64_t* walk_len) {
    return guard([&] { e->e.walk_batch_fetch(arena, cap, offsets, walk_len); });
}
ldbg_status ldbg_engine_walk_batch(ldbg_engine* e, const char* seeds, int64_t n, char* arena, int64_t cap, int64_t* offsets, int64_t* walk_len, int64_t* traversed) {
    int64_t total = 0;
    ldbg_status st = ldbg_engine_walk_batch_run(e, seeds, n, &total, traversed);
    if (st != LDBG_OK) return st;
    return ldbg_engine_walk_batch_fetch(e, arena, cap, offsets, walk_len);
}
ldbg_status ldbg_engine_walk_vertices(ldbg_engine* e, int64_t walk, int64_t capacity, int64_t* len, uint64_t* words, int64_t* rec, int32_t* copy, int32_t* index) {
    return guard([&] { e->e.walk_vertices(walk, capacity, len, words, rec, copy, index); });
}

ldbg_status ldbg_engine_walk_roi_hits(ldbg_engine* e, int64_t* offsets, uint32_t* hits, int64_t capacity, uint8_t* has_null) {
    return guard([&] { e->e.walk_roi_hits(offsets, hits, capacity, has_null); });
}

ldbg_status ldbg_engine_dfs_batch(ldbg_engine* e, const char* sources, int64_t n, const char* sinks, const int64_t* sink_offsets, ldbg_dfs_result** out) {
    return guard([&] {
        *out = nullptr;
        // a full per-walk link store or frame stack is retried with a larger one (exactness is never traded away)
        for (int attempt = 0;; attempt++) {
            try {
                std::unique_ptr<DfsBatch> b(e->e.dfs_batch(sources, n, sinks, sink_offsets));
                *out = new ldbg_dfs_result{std::move(b)};
                return;
            } catch (const StatusError& se) {
                const std::string what = se.what();
                if (se.status == LDBG_ERR_CAPACITY && what == "LINKSTORE_FULL" && attempt < 8) { e->e.link_store_capacity *= 4; continue; }
                if (se.status == LDBG_ERR_CAPACITY && what == "LOG_FULL" && e->e.dfs_log_blocks < (1 << 20)) { e->e.dfs_log_blocks *= 8; continue; }
                if (se.status == LDBG_ERR_CAPACITY && what == "DEPTH_OVERFLOW" && e->e.dfs_max_depth < 4096) { e->e.dfs_max_depth *= 4; continue; }
                if (se.status == LDBG_ERR_CAPACITY && what == "DEPTH_OVERFLOW")
                    throw StatusError(LDBG_ERR_UNSUPPORTED, "dfs recursion deeper than 4096 branches (the reference overflows its thread stack here)");
                throw;
            }
        }
    });
}
// dfs_batch over the local image of a hash-sharded table: the library runs the bulk-synchronous rounds and calls `round_done` after
// each (the caller exchanges requests and rows there, and returns non-zero once no rank has a search in progress)
ldbg_status ldbg_engine_sharded_dfs_batch(ldbg_engine* e, ldbg_image* im, const char* sources, int64_t n, const char* sinks, const int64_t* sink_offsets,
                                          const int32_t* d_seed_slot, const int32_t* d_sink_slot, int (*round_done)(void*), void* user,
                                          int64_t* d_stats, void* stream, ldbg_dfs_result** out) {
    return guard([&] {
        *out = nullptr;
        if (&im->img.graph() != e->e.graph) throw StatusError(LDBG_ERR_ARG, "the engine was not created on this image's graph");
        ShardedRun sr{&im->img, d_seed_slot, d_sink_slot, round_done, user, d_stats, (rt::stream_t)stream};
        try {
            std::unique_ptr<DfsBatch> b(e->e.dfs_batch(sources, n, sinks, sink_offsets, &sr));
            b->materialize();                         // the vertices' k-mers and coverages live in the image: read them before it changes
            *out = new ldbg_dfs_result{std::move(b)};
        } catch (const StatusError& se) {
            // capacities grow for the next attempt (the caller runs the batch again on every rank: exactness is never traded away)
            const std::string what = se.what();
            if (se.status == LDBG_ERR_CAPACITY && what == "LINKSTORE_FULL") e->e.link_store_capacity *= 4;
            if (se.status == LDBG_ERR_CAPACITY && what == "LOG_FULL" && e->e.dfs_log_blocks < (1 << 20)) e->e.dfs_log_blocks *= 8;
            if (se.status == LDBG_ERR_CAPACITY && what == "DEPTH_OVERFLOW" && e->e.dfs_max_depth < 4096) e->e.dfs_max_depth *= 4;
            throw;
        }
    });
}
static const DfsGraphHost& dfs_at(const ldbg_dfs_result* r, int64_t i) {
    if (!r || !r->b) throw StatusError(LDBG_ERR_ARG, "no dfs result");
    if (i < 0 || i >= (int64_t)r->b->results.size()) throw StatusError(LDBG_ERR_ARG, "dfs result index out of range");
    return r->b->results[(size_t)i];
}
ldbg_status ldbg_dfs_result_sizes(const ldbg_dfs_result* r, int64_t i, int* is_null, int64_t* n_vertices, int64_t* n_edges) {
    return guard([&] {
        const DfsGraphHost& g = dfs_at(r, i);
        if (is_null) *is_null = g.is_null ? 1 : 0;
        if (n_vertices) *n_vertices = g.n_vertices();
        if (n_edges) *n_edges = g.n_edges();
    });
}
ldbg_status ldbg_dfs_result_get(const ldbg_dfs_result* r, int64_t i, uint64_t* kmer_words, int64_t* rec, int32_t* copy_index, int32_t* index,
                                int32_t* edge_src, int32_t* edge_dst, int32_t* edge_color) {
    return guard([&] {
        dfs_at(r, i);
        if (kmer_words) r->b->materialize();
        const DfsGraphHost& g = dfs_at(r, i);
        if (g.packed) { r->b->read_packed(i, rec, copy_index, index, edge_src, edge_dst, edge_color); return; }    // (no k-mers asked for: straight from the packed entries)
        if (kmer_words && !g.words.empty()) memcpy(kmer_words, g.words.data(), g.words.size() * 8);
        for (size_t v = 0; v < g.verts.size(); v++) {
            if (rec) rec[v] = g.verts[v].rec;
            if (copy_index) copy_index[v] = g.verts[v].copy;
            if (index) index[v] = g.verts[v].index;
        }
        for (size_t x = 0; x < g.edges.size(); x++) {
            if (edge_src) edge_src[x] = g.edges[x].src;
            if (edge_dst) edge_dst[x] = g.edges[x].dst;
            if (edge_color) edge_color[x] = g.edges[x].color;
        }
    });
}
ldbg_status ldbg_dfs_result_walk(const ldbg_dfs_result* r, int64_t i, const char* seed, int color, char* contig, int64_t capacity, int64_t* len) {
    return guard([&] {
        dfs_at(r, i);
        const std::string c = r->b->walk_contig(i, seed, color);
        if (len) *len = (int64_t)c.size();
        if ((int64_t)c.size() + 1 > capacity) throw StatusError(LDBG_ERR_CAPACITY, "contig buffer too small: need " + std::to_string(c.size() + 1));
        memcpy(contig, c.c_str(), c.size() + 1);
    });
}
ldbg_status ldbg_dfs_result_merge(ldbg_dfs_result* r, const int64_t* which, int64_t m, ldbg_dfs_result** out) {
    return guard([&] {
        *out = nullptr;
        std::unique_ptr<DfsBatch> b(dfs_merge(*r->b, which, m));
        *out = new ldbg_dfs_result{std::move(b)};
    });
}
ldbg_status ldbg_dfs_result_free(ldbg_dfs_result* r) { delete r; return LDBG_OK; }
ldbg_status ldbg_engine_neighbours_batch(ldbg_engine* e, const char* kmers, int64_t n, int forward, int64_t* offsets, uint64_t* kmer_words, int64_t* rec, int64_t capacity) {
    return guard([&] { e->e.neighbours_batch(kmers, n, forward != 0, offsets, kmer_words, rec, capacity); });
}
ldbg_status ldbg_engine_dfs_kmers_traversed(const ldbg_engine* e, int64_t* n) { return guard([&] { *n = e->e.dfs_traversed(); }); }

// ---- cursor
static CursorHost& cursor_of(ldbg_engine* e) {
    if (!e->cursor) e->cursor.reset(new CursorHost(e->e));
    return *e->cursor;
}
ldbg_status ldbg_engine_assemble(ldbg_engine* e, const char* seed, int64_t capacity, int64_t* len, uint64_t* kmer_words, int64_t* rec) {
    return guard([&] { cursor_of(e).assemble(seed, capacity, len, kmer_words, rec); });
}
ldbg_status ldbg_engine_seek(ldbg_engine* e, const char* kmer) { return guard([&] { cursor_of(e).seek(kmer); }); }
ldbg_status ldbg_engine_has_next(ldbg_engine* e, int* yes) { return guard([&] { *yes = cursor_of(e).has(true) ? 1 : 0; }); }
ldbg_status ldbg_engine_has_previous(ldbg_engine* e, int* yes) { return guard([&] { *yes = cursor_of(e).has(false) ? 1 : 0; }); }
ldbg_status ldbg_engine_next(ldbg_engine* e, char* kmer_out, int64_t* rec_out) { return guard([&] { cursor_of(e).step(true, kmer_out, rec_out); }); }
ldbg_status ldbg_engine_previous(ldbg_engine* e, char* kmer_out, int64_t* rec_out) { return guard([&] { cursor_of(e).step(false, kmer_out, rec_out); }); }

// ---- cursors in batches
static ldbg_status cursor_batch_any(ldbg_engine* e, const char* seeds, int64_t n, bool on_device, int direction, int64_t max_steps, const ldbg_cursor_stop* stop,
                                    ldbg_cursor_result** out) {
    return guard([&] {
        if (!e || !out) throw StatusError(LDBG_ERR_ARG, "cursor batch: null engine or result pointer");
        *out = nullptr;
        if (!e->cursor_batch) e->cursor_batch.reset(new CursorBatchHost(e->e));
        std::unique_ptr<CursorBatchResult> r(e->cursor_batch->run(seeds, n, on_device, direction, max_steps, stop));
        *out = new ldbg_cursor_result{std::move(r)};
    });
}
ldbg_status ldbg_engine_cursor_batch(ldbg_engine* e, const char* seeds, int64_t n, int direction, int64_t max_steps, const ldbg_cursor_stop* stop,
                                     ldbg_cursor_result** out) {
    return cursor_batch_any(e, seeds, n, false, direction, max_steps, stop, out);
}
ldbg_status ldbg_engine_cursor_batch_device(ldbg_engine* e, const void* d_seeds, int64_t n, int direction, int64_t max_steps, const ldbg_cursor_stop* stop,
                                            ldbg_cursor_result** out) {
    return cursor_batch_any(e, (const char*)d_seeds, n, true, direction, max_steps, stop, out);
}
static const CursorBatchResult& cursor_result_of(const ldbg_cursor_result* r) {
    if (!r || !r->r) throw StatusError(LDBG_ERR_ARG, "no cursor result");
    return *r->r;
}
ldbg_status ldbg_cursor_result_sizes(const ldbg_cursor_result* r, int64_t* n_seeds, int64_t* n_vertices, int* kmer_words) {
    return guard([&] {
        const CursorBatchResult& c = cursor_result_of(r);
        if (n_seeds) *n_seeds = c.n;
        if (n_vertices) *n_vertices = c.total;
        if (kmer_words) *kmer_words = c.W;
    });
}
ldbg_status ldbg_cursor_result_get(const ldbg_cursor_result* r, int64_t* offsets, uint64_t* kmer_words, int64_t* rec, int32_t* n_reverse, int32_t* n_forward,
                                   int64_t* seed_rec, uint8_t* end_reverse, uint8_t* end_forward, uint8_t* status) {
    return guard([&] { cursor_result_of(r).get(offsets, kmer_words, rec, n_reverse, n_forward, seed_rec, end_reverse, end_forward, status, false, nullptr); });
}
ldbg_status ldbg_cursor_result_get_dev(const ldbg_cursor_result* r, void* d_offsets, void* d_kmer_words, void* d_rec, void* d_n_reverse, void* d_n_forward,
                                       void* d_seed_rec, void* d_end_reverse, void* d_end_forward, void* d_status, void* stream) {
    return guard([&] {
        cursor_result_of(r).get(d_offsets, d_kmer_words, d_rec, d_n_reverse, d_n_forward, d_seed_rec, d_end_reverse, d_end_forward, d_status, true, (rt::stream_t)stream);
    });
}
ldbg_status ldbg_cursor_result_free(ldbg_cursor_result* r) { delete r; return LDBG_OK; }

// ---- callVariant in batches
static ldbg_status variant_batch_any(ldbg_engine* ce, ldbg_engine* pe, const char* seeds, int64_t n, bool on_device, int stop_colour, int64_t max_steps, uint64_t sum_mask,
                                     ldbg_variant_result** out) {
    return guard([&] {
        if (!ce || !pe || !out) throw StatusError(LDBG_ERR_ARG, "variant batch: null engine or result pointer");
        *out = nullptr;
        if (!ce->cursor_batch) ce->cursor_batch.reset(new CursorBatchHost(ce->e));
        if (!pe->cursor_batch) pe->cursor_batch.reset(new CursorBatchHost(pe->e));
        std::unique_ptr<VariantResult> r(variant_batch(ce->e, *ce->cursor_batch, pe->e, *pe->cursor_batch, seeds, n, on_device, stop_colour, max_steps, sum_mask));
        *out = new ldbg_variant_result{std::move(r)};
    });
}
ldbg_status ldbg_engine_variant_batch(ldbg_engine* child_engine, ldbg_engine* parent_engine, const char* seeds, int64_t n, int stop_colour, int64_t max_steps,
                                      uint64_t sum_mask, ldbg_variant_result** out) {
    return variant_batch_any(child_engine, parent_engine, seeds, n, false, stop_colour, max_steps, sum_mask, out);
}
ldbg_status ldbg_engine_variant_batch_device(ldbg_engine* child_engine, ldbg_engine* parent_engine, const void* d_seeds, int64_t n, int stop_colour, int64_t max_steps,
                                             uint64_t sum_mask, ldbg_variant_result** out) {
    return variant_batch_any(child_engine, parent_engine, (const char*)d_seeds, n, true, stop_colour, max_steps, sum_mask, out);
}
static const VariantResult& variant_result_of(const ldbg_variant_result* r) {
    if (!r || !r->r) throw StatusError(LDBG_ERR_ARG, "no variant result");
    return *r->r;
}
ldbg_status ldbg_variant_result_sizes(const ldbg_variant_result* r, int64_t* n_seeds, int* n_colours, int64_t* allele_bytes, int64_t* n_child_vertices,
                                      int64_t* n_parent_vertices, int* kmer_words) {
    return guard([&] {
        const VariantResult& v = variant_result_of(r);
        if (n_seeds) *n_seeds = v.n;
        if (n_colours) *n_colours = v.n_colours;
        if (allele_bytes) *allele_bytes = v.allele_bytes;
        if (n_child_vertices) *n_child_vertices = v.child ? v.child->total : 0;
        if (n_parent_vertices) *n_parent_vertices = v.parent ? v.parent->total : 0;
        if (kmer_words) *kmer_words = v.W;
    });
}
ldbg_status ldbg_variant_result_get(const ldbg_variant_result* r, const ldbg_variant_arrays* into) {
    return guard([&] {
        if (!into) throw StatusError(LDBG_ERR_ARG, "variant result: null arrays");
        variant_result_of(r).get(*into, false, nullptr);
    });
}
ldbg_status ldbg_variant_result_get_dev(const ldbg_variant_result* r, const ldbg_variant_arrays* into, void* stream) {
    return guard([&] {
        if (!into) throw StatusError(LDBG_ERR_ARG, "variant result: null arrays");
        variant_result_of(r).get(*into, true, (rt::stream_t)stream);
    });
}
ldbg_status ldbg_variant_result_free(ldbg_variant_result* r) { delete r; return LDBG_OK; }

// ---- Tesserae in batches
ldbg_status ldbg_mosaic_align_batch(int device, const ldbg_mosaic_params* p, int64_t n, const char* queries, const int64_t* query_off, const int64_t* target_first,
                                    const char* targets, const int64_t* target_off, ldbg_mosaic_result** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "mosaic: null result pointer");
        *out = nullptr;
        if (!p) throw StatusError(LDBG_ERR_ARG, "mosaic: null parameters");
        std::unique_ptr<MosaicResult> r(mosaic_align_batch(device, *p, n, queries, query_off, target_first, targets, target_off));
        *out = new ldbg_mosaic_result{std::move(r)};
    });
}
static const MosaicResult& mosaic_result_of(const ldbg_mosaic_result* r) {
    if (!r || !r->r) throw StatusError(LDBG_ERR_ARG, "no mosaic result");
    return *r->r;
}
ldbg_status ldbg_mosaic_result_sizes(const ldbg_mosaic_result* r, int64_t* n, int64_t* path_entries) {
    return guard([&] {
        const MosaicResult& m = mosaic_result_of(r);
        if (n) *n = m.n;
        if (path_entries) *path_entries = m.path_off.back();
    });
}
ldbg_status ldbg_mosaic_result_get(const ldbg_mosaic_result* r, const ldbg_mosaic_arrays* into) {
    return guard([&] {
        if (!into) throw StatusError(LDBG_ERR_ARG, "mosaic result: null arrays");
        const MosaicResult& m = mosaic_result_of(r);
        auto copy = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
        copy(into->status, m.status.data(), m.status.size());
        copy(into->llk, m.llk.data(), m.llk.size() * 8);
        copy(into->path_off, m.path_off.data(), m.path_off.size() * 8);
        copy(into->copy, m.copy.data(), m.copy.size() * 4);
        copy(into->state, m.state.data(), m.state.size() * 4);
        copy(into->pos, m.pos.data(), m.pos.size() * 4);
    });
}
ldbg_status ldbg_mosaic_result_free(ldbg_mosaic_result* r) { delete r; return LDBG_OK; }
ldbg_status ldbg_mosaic_tb_roundtrip(int device, double div, int64_t n, const int32_t* who, const int32_t* state, const int32_t* pos, int32_t* out) {
    return guard([&] { mosaic_tb_roundtrip(device, div, n, who, state, pos, out); });
}

// ---- Smith-Waterman in batches
ldbg_status ldbg_sw_align_batch(int device, int64_t n, const char* queries, const int64_t* query_off, const char* subjects, const int64_t* subject_off,
                                ldbg_sw_result** out) {
    return guard([&] {
        if (!out) throw StatusError(LDBG_ERR_ARG, "sw: null result pointer");
        *out = nullptr;
        std::unique_ptr<SwResult> r(sw_align_batch(device, n, queries, query_off, subjects, subject_off));
        *out = new ldbg_sw_result{std::move(r)};
    });
}
static const SwResult& sw_result_of(const ldbg_sw_result* r) {
    if (!r || !r->r) throw StatusError(LDBG_ERR_ARG, "no sw result");
    return *r->r;
}
ldbg_status ldbg_sw_result_sizes(const ldbg_sw_result* r, int64_t* n, int64_t* columns, int64_t* query_letters, int64_t* subject_letters) {
    return guard([&] {
        const SwResult& m = sw_result_of(r);
        if (n) *n = m.n;
        if (columns) *columns = m.col_off.back();
        if (query_letters) *query_letters = m.q_off.back();
        if (subject_letters) *subject_letters = m.s_off.back();
    });
}
ldbg_status ldbg_sw_result_get(const ldbg_sw_result* r, const ldbg_sw_arrays* into) {
    return guard([&] {
        if (!into) throw StatusError(LDBG_ERR_ARG, "sw result: null arrays");
        const SwResult& m = sw_result_of(r);
        auto copy = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
        copy(into->status, m.status.data(), m.status.size());
        copy(into->score, m.score.data(), m.score.size() * 8);
        copy(into->end_q, m.end_q.data(), m.end_q.size() * 4);
        copy(into->end_s, m.end_s.data(), m.end_s.size() * 4);
        copy(into->begin_q, m.begin_q.data(), m.begin_q.size() * 4);
        copy(into->begin_s, m.begin_s.data(), m.begin_s.size() * 4);
        copy(into->aligned_len, m.aligned_len.data(), m.aligned_len.size() * 4);
        copy(into->edits, m.edits.data(), m.edits.size() * 4);
        copy(into->col_off, m.col_off.data(), m.col_off.size() * 8);
        copy(into->cols, m.cols.data(), m.cols.size());
        copy(into->q_off, m.q_off.data(), m.q_off.size() * 8);
        copy(into->q_letters, m.q_letters.data(), m.q_letters.size());
        copy(into->s_off, m.s_off.data(), m.s_off.size() * 8);
        copy(into->s_letters, m.s_letters.data(), m.s_letters.size());
    });
}
ldbg_status ldbg_sw_result_free(ldbg_sw_result* r) { delete r; return LDBG_OK; }

#ifdef LDBG_HOSTSIM
void ldbg_debug_ls(uint64_t* out) {
    auto& d = ldbg::ls_debug();
    out[0] = d.adds; out[1] = d.newkeys; out[2] = d.choices; out[3] = d.scan; out[4] = d.maxn; out[5] = d.steps; out[6] = d.sum_n;
    out[7] = d.runs_a; out[8] = d.runs_b; out[9] = d.run_vertices; out[10] = d.retries; out[11] = d.repeats;
    d = ldbg::LsDebug();
}
#endif
// ---- measurement
#ifdef LDBG_HOSTSIM
// test hook of the host simulation (rt.h): lanes a simulated wavefront runs in lock step (1, 2, 4, ... 64)
extern "C" void ldbg_hostsim_set_lanes(int n) { int v = 1; while (v * 2 <= n && v < 64) v *= 2; ::ldbg::sim::lanes_setting() = v; }
#endif
ldbg_status ldbg_profile_reset(void) { profile_reset_all(); return LDBG_OK; }
ldbg_status ldbg_profile_get(const char* family, double* total_ms, int64_t* launches) {
    profile_get(family, total_ms, launches);
    return LDBG_OK;
}

}  // extern "C"
