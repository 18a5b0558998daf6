#pragma once
#include <vector>

#include "rt.h"

namespace ldbg {

// result of one mosaic batch (ldbg_mosaic_align_batch), on the host: the path arrays are small
struct MosaicResult {
    int64_t n = 0;
    std::vector<uint8_t> status;       // [n] LDBG_OK or LDBG_ERR_UNSUPPORTED
    std::vector<double> llk;           // [n]
    std::vector<int64_t> path_off;     // [n + 1]
    std::vector<int32_t> copy, state, pos;
    int slices = 0;                    // launches the batch took (the arena budget)
};

// the traceback value of Tesserae.java:239,270,281,289,299,315 and its three casts of :363-365, in Java's operation order; on the device
// and on the host.  who10_state = who * 10 + state (an int sum in the Java), div = tb_divisor.
LDBG_HOSTDEV double mosaic_tb_encode(int who10_state, int pos, double div) { return (double)who10_state + (double)pos / div; }
LDBG_HOSTDEV void mosaic_tb_decode(double tb, double div, int* who, int* state, int* pos) {
#pragma clang fp contract(off)         // (x * div + 1e-6 must round twice, as the Java does)
    const int w = (int)tb / 10;
    const int s = (int)(tb - (double)(w * 10));
    const double scaled = (tb - (double)(w * 10) - (double)s) * div;
    *who = w; *state = s; *pos = (int)(scaled + 1e-6);
}

// Tesserae.align of n problems (Tesserae.java:95-382: initialize, alignAll up to the traceback), one wavefront per problem
MosaicResult* mosaic_align_batch(int device, const ldbg_mosaic_params& p, int64_t n, const char* queries, const int64_t* query_off, const int64_t* target_first,
                                 const char* targets, const int64_t* target_off);
// encode, then decode, of n triples on the device (the kernel's own functions): out[3n]
void mosaic_tb_roundtrip(int device, double div, int64_t n, const int32_t* who, const int32_t* state, const int32_t* pos, int32_t* out);

}  // namespace ldbg
