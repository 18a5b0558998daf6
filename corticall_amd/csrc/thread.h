// Sequences threaded through a graph on the device: for every k-mer window of every sequence of a batch, the record of
// its canonical k-mer in a graph and whether a ROI graph holds it; per sequence, what the partition post-filters and Call's first steps
// derive from that.  The inner loop of TrimPartitions (J/commands/discover/call/TrimPartitions.java:35-68), FilterPartitions (:41-140),
// CountNovelKmersInPartitions (:30-61), Coverage (J/commands/discover/display/Coverage.java:29-47), Call.loadChildWalk
// (J/commands/discover/call/Call.java:2358-2381) and Call.getRegions (:2425-2451).
#pragma once
#include <vector>

#include "devmem.h"
#include "graph.h"

namespace ldbg {

// a window's info byte
#define LDBG_WIN_VALID 1u      // all k bytes are upper-case ACGT
#define LDBG_WIN_FLIP 2u       // the reverse complement is the smaller one (by value): the canonical k-mer is the reverse complement
#define LDBG_WIN_PAL 4u        // the window is its own reverse complement
#define LDBG_WIN_ROI 8u        // the canonical k-mer is a record of the ROI graph

class Threading {
public:
    // g and rois: either may be null, not both.  bases / offsets are host memory, or (on_device) memory of the graphs' device.
    Threading(const Graph* g, const Graph* rois, const char* bases, const int64_t* offsets, int64_t n_seqs, int flags, bool on_device, rt::stream_t stream);
    Threading(const Threading&) = delete;
    Threading& operator=(const Threading&) = delete;

    const Graph* graph;        // g (null: every rec is -1)
    int device = 0, flags = 0;
    int64_t n_seqs = 0, n_windows = 0, n_regions = 0;
    double device_ms = 0;

    // windows [first, first + n): any of the three outputs may be null; copy_index needs LDBG_THREAD_COPY_INDEX
    void windows(int64_t first, int64_t n, int64_t* rec, uint8_t* info, int32_t* copy_index, bool device_out, rt::stream_t s) const;
    // getCoverage(colour) of every window's record as a Java int; a window without a record is the reference's NullPointerException
    void coverage(int colour, int64_t first, int64_t n, int32_t* cov) const;
    void summary(int64_t first_seq, int64_t n, int64_t* win_start, int32_t* first_hit, int32_t* last_hit, int32_t* n_hits, int32_t* n_distinct, uint8_t* ends) const;
    void regions(int64_t* region_offsets, int32_t* start, int32_t* stop, int64_t capacity) const;
    const int64_t* rec_dev() const { return d_rec_; }      // [n_windows] on the device (null without windows)

private:
    DevBlocks own_;               // holds the three below
    int64_t* d_rec_ = nullptr;    // [n_windows]
    uint8_t* d_info_ = nullptr;   // [n_windows]
    int32_t* d_copy_ = nullptr;   // [n_windows] with LDBG_THREAD_COPY_INDEX
    // per sequence, and the regions: small next to the windows, downloaded once
    std::vector<int64_t> win_start_, reg_off_;
    std::vector<int32_t> first_, last_, n_hits_, n_distinct_, reg_start_, reg_stop_;
    std::vector<uint8_t> ends_;
    void check_range(int64_t first, int64_t n, int64_t total, const char* what) const;
};

}  // namespace ldbg
