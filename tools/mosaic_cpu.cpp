// The number tools/mosaic_bench.py sets the device against: the kernel body of corticall_amd/csrc/mosaic.cpp compiled as plain C++ (-O2,
// the host simulation's shim with one lane per wavefront), run by one thread.  Not part of the product path.
#include <chrono>

#include "../corticall_amd/csrc/mosaic.h"

namespace ldbg {
void profile_add(const char*, double) {}
}  // namespace ldbg

extern "C" int mosaic_cpu_align(const ldbg_mosaic_params* p, int64_t n, const char* queries, const int64_t* query_off, const int64_t* target_first, const char* targets,
                                const int64_t* target_off, double* llk, double* seconds) {
    try {
        const auto t0 = std::chrono::steady_clock::now();
        ldbg::MosaicResult* r = ldbg::mosaic_align_batch(0, *p, n, queries, query_off, target_first, targets, target_off);
        *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int64_t i = 0; i < n; i++) llk[i] = r->status[(size_t)i] == LDBG_OK ? r->llk[(size_t)i] : 0.0;
        delete r;
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}
