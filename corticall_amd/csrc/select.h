// Record selection on the device: the records of a resident table that satisfy a predicate over their coverages and
// edges, in record order, and those records packed as a graph.  The loop of FindROIs (J/commands/discover/roi/FindROIs.java:30-82),
// FindLowCoverage, FindDust, FindShared (J/commands/prefilter/) and Remove (J/commands/utils/Remove.java:29-86); and the loop of
// RecoverExcludedKmers (J/commands/discover/recover/RecoverExcludedKmers.java:29-108): a selection with a join.
#pragma once
#include <string>
#include <vector>

#include "devmem.h"
#include "graph.h"

namespace ldbg {

#define LDBG_SELECT_CHUNK 4096      // records per chunk: the stretch one wavefront filters, one entry of the scanned counts
#define LDBG_SELECT_MAX_PROJ 32     // colours of a packed record (a .ctx header holds no more)

class Selection {
public:
    // lookup == nullptr: the records of `g` that pass `f`.  Else: the records of `lookup` whose k-mer's record in `g` (findRecord)
    // passes `f`; a k-mer without one is the reference's NullPointerException.
    Selection(const Graph& g, const ldbg_record_filter& f, const Graph* lookup);
    // RecoverExcludedKmers: the records of `g` with coverage in child_colour, and those without it that another colour covers and
    // whose k-mer `dirty` holds with coverage in its colour 0 (dirty.findRecord, Q1 included); cov_ is the child's coverage of each
    // selected record after the patch
    Selection(const Graph& g, int child_colour, const Graph& dirty);
    // no record of `g` yet: compact() fills it (the seed pass, seeds.cpp)
    explicit Selection(const Graph& g) : graph(g) {}
    Selection(const Selection&) = delete;
    Selection& operator=(const Selection&) = delete;

    const Graph& graph;        // the graph whose records the indices number
    int64_t count = 0;
    double select_ms = 0;      // device time of the selection kernels
    int child_colour = -1;     // >= 0: made by the recover constructor
    int64_t n_recovered = 0;   // selected records whose coverage came from `dirty`

    // The records whose bit is set in ballots (bit b of word w: record 64 w + b; one word per 64 records, LDBG_SELECT_CHUNK records per
    // entry of chunk_cnt, which counts them) become the selection: count and the record numbers, ascending.  Adds its device time to
    // select_ms and waits for the stream.
    void compact(const unsigned long long* ballots, const uint32_t* chunk_cnt, rt::stream_t s);
    const uint32_t* records_dev() const { return d_idx_; }     // [count] on the graph's device
    void indices(int64_t first, int64_t n, int64_t* idx, bool device_out, rt::stream_t s) const;
    // the header CortexGraphWriter would write: that of header_path re-serialised (same k, n_colours colours), or the fresh one of
    // FindROIs.makeCortexHeader (:85-105) with the sample names of the projected colours
    std::vector<uint8_t> header(const int* colours, int n_colours, const char* header_path) const;
    // the selected records projected onto `colours`, in the file's record layout, back to back in device memory (count * (8W + 5 n_colours)
    // bytes; nullptr when nothing is selected)
    DevRecords pack(const int* colours, int n_colours) const;
    void write_ctx(const int* colours, int n_colours, const char* header_path, const std::string& out_path) const;

    // ---- a recover selection only (LDBG_ERR_ARG otherwise)
    void recovered_coverage(int64_t first, int64_t n, int32_t* cov) const;
    // makeHeader (RecoverExcludedKmers.java:98-107): version, k and kmerBits of the graph, ONE colour: the child's block
    std::vector<uint8_t> recovered_header() const;
    // what CortexGraphWriter.addRecord writes under that header (CortexGraphWriter.java:106-138: header.getNumColors() colours of the
    // record it is given): colour 0's coverage and edge byte of every selected record — the patched coverage when the child is colour 0
    DevRecords pack_recovered() const;
    void write_recovered(const std::string& out_path) const;

private:
    DevBlocks own_;               // holds the two below
    uint32_t* d_idx_ = nullptr;   // [count] ascending record numbers
    int32_t* d_cov_ = nullptr;    // [count] recover: the child colour's coverage after the patch
    void check_recovered() const;
};

}  // namespace ldbg
