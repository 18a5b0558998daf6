// The uploaded sequence text as 2-bit words with a validity bit per base: the first stage of graph construction (build.cpp) and of
// link construction (linkbuild.cpp).  Internal linkage: each of the two sources launches its own copy of the kernel.
#pragma once
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

LDBG_DEV unsigned bld_base(const uint64_t* packed, int64_t b) { return (unsigned)(packed[b >> 5] >> (62 - 2 * (int)(b & 31))) & 3u; }

}  // namespace
}  // namespace ldbg
