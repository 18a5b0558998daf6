#pragma once
#include <vector>

#include "rt.h"

namespace ldbg {

// result of one Smith-Waterman batch (ldbg_sw_align_batch), on the host: every array is small
struct SwResult {
    int64_t n = 0;
    std::vector<uint8_t> status;       // [n] LDBG_OK or LDBG_ERR_UNSUPPORTED
    std::vector<double> score;         // [n] SWResult.score: half units / 2.0; -1 for the empty result
    std::vector<int32_t> end_q, end_s, begin_q, begin_s;      // [n] 1-based; -1 for the empty result
    std::vector<int32_t> aligned_len, edits;                  // [n]
    std::vector<int64_t> col_off;      // [n + 1]
    std::vector<uint8_t> cols;         // the traceback's columns in alignment order: 0 both letters, 1 gap in the query, 2 gap in the subject
    std::vector<int64_t> q_off, s_off; // [n + 1]
    std::vector<uint8_t> q_letters, s_letters;                // the letters after Sequence.add and filter
    int slices = 0;                    // launches the batch took (the arena budget)
};

#define LDBG_SW_LETTERS "ATGCSWRYKMBVHDN*"    // the order of EDNAFULL's rows; X is code 16
#define LDBG_SW_MIN_REFUSED 107374            // 20000 x min(|q|, |s|) must stay below 2^31

// SmithWaterman.align of n pairs (SmithWaterman.java:89-294 after Sequence.add and EDNAFULL.filter), one wavefront per pair
SwResult* sw_align_batch(int device, int64_t n, const char* queries, const int64_t* query_off, const char* subjects, const int64_t* subject_off);

}  // namespace ldbg
