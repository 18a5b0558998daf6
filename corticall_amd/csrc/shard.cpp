// The global neighbour index of a shard of a hash-partitioned table: for every local record and each of its 8 possible
// neighbours (4 successors, 4 predecessors of the canonical k-mer) the owner, the record number in the owner's shard and the
// orientation — a routed findRecord per edge, done once when the table is loaded (corticall_amd/distributed.py drives the routing).
// The traversals over the sharded table (image.h / image.cpp) are served from it.
#include <algorithm>

#include "engine_host.h"
#include "image.h"
#include "shard.h"

namespace ldbg {

// ---- neighbour queries of local records: canonical neighbour k-mers for every edge any colour carries
template <int W>
LDBG_KERNEL void k_nbr_queries(GraphView g, int64_t first, int64_t n, uint64_t* words, uint8_t* flips, uint8_t* have_out) {
    for (int64_t t = global_tid(); t < n * 8; t += global_nthreads()) {
        const int64_t i = first + t / 8;
        const unsigned j = (unsigned)(t % 8), b = j & 3u;
        const uint8_t* row = graph_row(g, i);
        uint32_t lo = 0, hi = 0;
        for (int col = 0; col < g.C; col++) { uint32_t e = row[g.edges_off + col]; lo |= e & 0xf; hi |= e >> 4; }
        const bool have = j < 4 ? ((lo >> b) & 1u) != 0 : ((hi >> (3 - b)) & 1u) != 0;
        Kmer<W> x;
        for (int w = 0; w < W; w++) x.w[w] = 0;
        bool f = false;
        if (have) {
            const Kmer<W> c = graph_key<W>(g, i);
            x = kmer_canonical<W>(j < 4 ? kmer_next<W>(c, g.k, b) : kmer_prev<W>(c, g.k, b), g.k, &f);
        }
        for (int w = 0; w < W; w++) words[t * W + w] = kmer_word<W>(x, w);
        flips[t] = f ? 1 : 0;
        have_out[t] = have ? 1 : 0;      // beside the words: at k = 32, 64, ... no bit pattern of the words is free to say "no query"
    }
}
LDBG_KERNEL void k_set_nbrg(uint64_t* nbrg, int64_t first, int64_t n, const int32_t* owner, const int64_t* lidx, const uint8_t* flips) {
    for (int64_t t = global_tid(); t < n * 8; t += global_nthreads())
        nbrg[first * 8 + t] = gid_make(owner[t], lidx[t], flips[t] != 0);
}

void shard_nbr_queries(const Graph& g, int64_t first, int64_t n, uint64_t* d_words, uint8_t* d_flips, uint8_t* d_have) {
    if (n <= 0) return;
    if (first < 0 || first + n > g.view.N) throw StatusError(LDBG_ERR_ARG, "shard_nbr_queries: record range out of bounds");
    rt::stream_t s = g.stream;
    LDBG_LAUNCH_W(g.view.W, k_nbr_queries, grid_for(n * 8), 256, s, g.view, first, n, d_words, d_flips, d_have);
    rt::stream_sync(s);
}

void shard_set_nbr(Graph& g, int64_t first, int64_t n, const int32_t* d_owner, const int64_t* d_lidx, const uint8_t* d_flips) {
    if (n <= 0) return;
    if (first < 0 || first + n > g.view.N) throw StatusError(LDBG_ERR_ARG, "shard_set_nbr: record range out of bounds");
    rt::stream_t s = g.stream;
    if (!g.d_nbrg) {
        g.d_nbrg = rt::dmalloc((size_t)std::max<int64_t>(1, g.view.N) * 64);
        rt::dmemset(g.d_nbrg, 0, (size_t)std::max<int64_t>(1, g.view.N) * 64, s);
    }
    LDBG_LAUNCH(k_set_nbrg, grid_for(n * 8), 256, s, (uint64_t*)g.d_nbrg, first, n, d_owner, d_lidx, d_flips);
    rt::stream_sync(s);
}

}  // namespace ldbg
