// The uploaded sequence text as 2-bit words with a validity bit per base: the first stage of graph construction (build.cpp) and of
// link construction (linkbuild.cpp), and of threading sequences through a graph (thread.cpp); and the k-mer windows of a batch of
// sequences over that text, as link construction and threading read them.  Internal linkage: each source launches its own copy of the kernels.
#pragma once
#include "kmer.h"
#include "rt.h"

namespace ldbg {
namespace {

// 32 bases per lane: ascii[32 j .. 32 j + 31] -> packed[j], the first base in the top two bits (a k-mer is then a shift of
// consecutive words), and valid[j], bit b: byte 32 j + b is one of ACGTacgt.  The buffer is a whole number of 32-byte pieces.
LDBG_KERNEL void k_bld_pack(const uint8_t* ascii, int64_t nwords, uint64_t* packed, uint32_t* valid) {
    for (int64_t j = global_tid(); j < nwords; j += global_nthreads()) {
        const uint64_t* src = (const uint64_t*)(ascii + 32 * j);
        uint64_t q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = src[i];
        uint64_t acc = 0;
        uint32_t ok = 0;
#pragma unroll
        for (int b = 0; b < 32; b++) {
            const uint32_t u = (uint32_t)(q[b >> 3] >> (8 * (b & 7))) & 0xDFu;          // upper case
            const uint32_t h = (u >> 1) & 3u;                                          // A 0, C 1, T 2, G 3
            acc = (acc << 2) | (uint64_t)(h ^ (h >> 1));                               // A 0, C 1, G 2, T 3
            ok |= (u == 'A' || u == 'C' || u == 'G' || u == 'T' ? 1u : 0u) << b;
        }
        packed[j] = acc;
        valid[j] = ok;
    }
}

// valid[j] bit b is cleared where byte 32 j + b is a lower-case letter: a read is looked up as it is given (the builder of graphs
// upper-cases, TempLinksAssembler and the commands that thread contigs through a graph do not)
LDBG_KERNEL void k_lnk_upper_only(const uint8_t* ascii, int64_t nwords, uint32_t* valid) {
    for (int64_t j = global_tid(); j < nwords; j += global_nthreads()) {
        const uint64_t* src = (const uint64_t*)(ascii + 32 * j);
        uint32_t low = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t q = src[i];
#pragma unroll
            for (int b = 0; b < 8; b++) low |= (uint32_t)((q >> (8 * b + 5)) & 1ull) << (8 * i + b);
        }
        valid[j] &= ~low;
    }
}

// The windows of a batch of sequences over the packed text: sequence r owns the windows [win_start[r], win_start[r + 1]) and its first
// byte is byte seq_beg[r] of the text; M windows in all.  (A sequence may own none: win_start[r] == win_start[r + 1].)
struct WinCtx {
    const uint64_t* packed;
    const uint32_t* valid;
    const int64_t* win_start;      // [nr + 1], win_start[nr] = M
    const int64_t* seq_beg;        // [nr]
    int64_t nr, M;
    int k;
};
// the sequence of window m < M: win_start[r] <= m < win_start[r + 1]
LDBG_DEV int64_t win_seq(const WinCtx& x, int64_t m) {
    int64_t lo = 0, hi = x.nr;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (x.win_start[mid] <= m) lo = mid; else hi = mid;
    }
    return lo;
}
// the k bases that start at byte gp of the text as a k-mer, as given (k_bld_extract's shifts)
template <int W>
LDBG_DEV Kmer<W> win_kmer(const WinCtx& x, int64_t gp) {
    const int64_t E = 2 * (gp + x.k), wi = (E - 1) >> 6;
    const int r = (int)(E - 64 * wi);                  // 2..64: bits of packed word wi that end the k-mer
    uint64_t pw[W + 1];
#pragma unroll
    for (int j = 0; j <= W; j++) pw[j] = wi - j >= 0 ? x.packed[wi - j] : 0ull;
    Kmer<W> a;
#pragma unroll
    for (int j = 0; j < W; j++) a.w[W - 1 - j] = r == 64 ? pw[j] : (pw[j] >> (64 - r)) | (pw[j + 1] << r);
    const int top = 2 * x.k - 64 * (W - 1);
    if (top < 64) a.w[0] &= (1ull << top) - 1ull;
    return a;
}
// are all of them bases (by the validity bits: upper-case ACGT after k_lnk_upper_only)?
LDBG_DEV bool win_valid(const WinCtx& x, int64_t gp) {
    bool ok = true;
    for (int64_t j = gp >> 5; j <= (gp + x.k - 1) >> 5; j++) {
        const int b0 = (int)(std::max<int64_t>(gp, 32 * j) - 32 * j), b1 = (int)(std::min<int64_t>(gp + x.k, 32 * j + 32) - 32 * j);
        const uint32_t mask = (b1 == 32 ? ~0u : (1u << b1) - 1u) & ~((1u << b0) - 1u);
        if (~x.valid[j] & mask) ok = false;
    }
    return ok;
}

LDBG_DEV unsigned bld_base(const uint64_t* packed, int64_t b) { return (unsigned)(packed[b >> 5] >> (62 - 2 * (int)(b & 31))) & 3u; }

}  // namespace
}  // namespace ldbg
