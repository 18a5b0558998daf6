// The number tools/sw_bench.py sets the device against: the kernel body of corticall_amd/csrc/sw.cpp compiled as plain C++ (-O2, the host
// simulation's shim with one lane per wavefront), run by one thread.  Not part of the product path.
#include <chrono>

#include "../corticall_amd/csrc/sw.h"

namespace ldbg {
void profile_add(const char*, double) {}
}  // namespace ldbg

// per pair: score, and end_q, end_s, begin_q, begin_s, aligned_len, edits in out6[6 i ..]
extern "C" int sw_cpu_align(int64_t n, const char* queries, const int64_t* query_off, const char* subjects, const int64_t* subject_off, double* score, int32_t* out6,
                            double* seconds) {
    try {
        const auto t0 = std::chrono::steady_clock::now();
        ldbg::SwResult* r = ldbg::sw_align_batch(0, n, queries, query_off, subjects, subject_off);
        *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int64_t i = 0; i < n; i++) {
            const size_t j = (size_t)i;
            score[i] = r->score[j];
            int32_t* o = out6 + 6 * i;
            o[0] = r->end_q[j]; o[1] = r->end_s[j]; o[2] = r->begin_q[j]; o[3] = r->begin_s[j]; o[4] = r->aligned_len[j]; o[5] = r->edits[j];
        }
        delete r;
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}
