// Variant seeds on the device: how often the windows of a threading hit every record of its graph, and getVariantSeeds
// of ComputeAssemblyQuality (J/commands/quality/ComputeAssemblyQuality.java:204-286) and ComputeInheritance
// (J/commands/inheritance/ComputeInheritance.java:238-322) — the records that pass the commands' filter, the string graph over them and
// their declared neighbours, the walk from every vertex of in-degree 0 and out-degree 1.
#pragma once
#include <memory>

#include "devmem.h"
#include "graph.h"
#include "select.h"
#include "thread.h"

namespace ldbg {

// count[r]: the windows of a threading whose record is r; first[r]: the smallest of them (-1: none).  Stands in for
// IndexedReference.find (J/utils/io/reference/IndexedReference.java:90-101).
class Occurrences {
public:
    explicit Occurrences(const Threading& t);
    Occurrences(const Occurrences&) = delete;
    Occurrences& operator=(const Occurrences&) = delete;

    const Graph& graph;
    int64_t n_records = 0;
    double device_ms = 0;

    // records [first, first + n): either output may be null
    void get(int64_t first, int64_t n, uint32_t* count, int64_t* first_window, bool device_out, rt::stream_t s) const;
    const uint32_t* count_dev() const { return d_count_; }      // [n_records] on the graph's device

private:
    DevBlocks own_;                            // holds the two below
    uint32_t* d_count_ = nullptr;              // [n_records]
    unsigned long long* d_first_ = nullptr;    // [n_records] all ones = none: -1 as the int64 it is read as
};

// ldbg_seed_filter with its handles unwrapped
struct SeedUnique { int colour; const Occurrences* occurrences; const uint8_t* d_unique; };
struct SeedFilter {
    uint64_t all_zero = 0;
    int n_covered = 0;
    ldbg_seed_covered covered[LDBG_SEED_MAX_COVERED];
    int n_unique = 0;
    SeedUnique unique[LDBG_SEED_MAX_UNIQUE];
};

// the good seeds of sel.graph become the records of sel (made empty, Selection(g)); counts may be null
void variant_seeds(Selection& sel, const SeedFilter& f, ldbg_seed_counts* counts);

}  // namespace ldbg
