#pragma once
#include <memory>

#include "cursor.h"

namespace ldbg {

// result of one variant batch (ldbg_engine_variant_batch), resident in HBM until it is asked for
struct VariantResult {
    int device = 0, W = 0, k = 0, n_colours = 0;
    int64_t n = 0, allele_bytes = 0;
    void* d_status = nullptr;          // [n] u8, LDBG_VARIANT_*
    void* d_source_rec = nullptr;      // [n] int64
    void* d_dest_rec = nullptr;        // [n] int64
    void* d_n_child = nullptr;         // [n] int32
    void* d_n_parent = nullptr;        // [n] int32
    void* d_st = nullptr;              // [n] int32
    void* d_s0end = nullptr;           // [n] int32
    void* d_s1end = nullptr;           // [n] int32
    void* d_child_sum = nullptr;       // [n][n_colours] int64
    void* d_child_flag = nullptr;      // [n][n_colours] u8
    void* d_parent_sum = nullptr;      // [n] int64
    void* d_parent_flag = nullptr;     // [n] u8
    void* d_allele_offsets = nullptr;  // [2n + 1] int64
    void* d_alleles = nullptr;         // [allele_bytes] ASCII
    std::unique_ptr<CursorBatchResult> child, parent;      // the contigs: the first batch, and the third (the vertices after the source)
    ~VariantResult();
    void get(const ldbg_variant_arrays& a, bool on_device, rt::stream_t s) const;
};

// callVariant of n seeds (ComputeInheritance.java:102-236, the per-seed reading of DESIGN.md §18): the two engines' cursor pools run the
// three batches, the kernels of variants.cpp chain them and call the alleles; everything is queued on the engines' streams
VariantResult* variant_batch(Engine& child, CursorBatchHost& child_pool, Engine& parent, CursorBatchHost& parent_pool, const char* seeds, int64_t n, bool on_device,
                             int stop_colour, int64_t max_steps, uint64_t sum_mask);

}  // namespace ldbg
