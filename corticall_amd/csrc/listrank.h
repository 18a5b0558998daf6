// List ranking by pointer jumping over oriented vertices: every member of a chain learns its head and its distance from it.  The run
// index (runs.cpp) and the unitigs (unitigs.cpp) rank their chains with it; what they do about pure cycles, which never settle, is
// their own.  Internal linkage, as bldpack.h: each source launches its own copy of the kernels.
#pragma once
#include "rt.h"

namespace ldbg {
namespace {

#define LDBG_LIST_NONE 0xFFFFFFFFu     // no predecessor

// pd[a] = ancestor | distance << 32
LDBG_KERNEL void k_rank_init(int64_t n2, const uint32_t* pred, unsigned long long* pd) {
    for (int64_t i = global_tid(); i < n2; i += global_nthreads())
        pd[i] = pred[i] == LDBG_LIST_NONE ? (unsigned long long)i : ((unsigned long long)pred[i] | (1ull << 32));
}
// One round of pointer jumping, in place: (ancestor, distance) is one 8-byte word, so whatever interleaving the other
// threads produce, a pair that is read is an ancestor with its true distance, and the update keeps that true.
LDBG_KERNEL void k_rank_jump(int64_t n2, unsigned long long* pd, unsigned* changed) {
    bool any = false;
    for (int64_t i = global_tid(); i < n2; i += global_nthreads()) {
        const unsigned long long me = LDBG_GLOBAL(unsigned long long, pd)[i];
        const uint32_t p = (uint32_t)me;
        if (p == (uint32_t)i) continue;
        const unsigned long long up = LDBG_GLOBAL(unsigned long long, pd)[p];
        if ((uint32_t)up == p) continue;                   // p is a head
        LDBG_GLOBAL(unsigned long long, pd)[i] = (unsigned long long)(uint32_t)up | (((me >> 32) + (up >> 32)) << 32);
        any = true;
    }
    if (any) *changed = 1u;
}

// rounds after which the longest possible chain of n2 vertices is ranked
int rank_rounds(int64_t n2) {
    int r = 2;
    while ((1ll << r) < n2) r++;
    return r;
}

// Ranks the lists pred[0..n2) gives into pd (pred == nullptr: pd holds partly ranked lists already and they are ranked on).  A chain of
// L vertices is ranked after ceil(log2 L) rounds; members of pure cycles never settle and are cut off after max_rounds.  d_changed: one
// device word of the caller's.
void rank_lists(unsigned long long* pd, const uint32_t* pred, int64_t n2, unsigned* d_changed, int max_rounds, rt::stream_t s) {
    const int grid = grid_for(n2);
    if (pred) LDBG_LAUNCH(k_rank_init, grid, 256, s, n2, pred, pd);
    for (int r = 0; r < max_rounds; r++) {
        rt::dmemset(d_changed, 0, 4, s);
        LDBG_LAUNCH(k_rank_jump, grid, 256, s, n2, pd, d_changed);
        unsigned changed = 0;
        rt::d2h(&changed, d_changed, 4, s);
        rt::stream_sync(s);
        if (!changed) break;
    }
}

}  // namespace
}  // namespace ldbg
