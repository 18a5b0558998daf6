// TEST-ONLY stand-alone program over the host simulation's wavefronts (csrc/rt.h): a two-lane kernel whose lanes part ways, lane 0 to a
// fence and lane 1 to a scan.  The simulation must report the divergence and abort; a fence and a scan that shared one collective kind
// would meet at one barrier instead and the program would end with "no divergence seen".
#include <stdio.h>

#include "../../corticall_amd/csrc/rt.h"

namespace ldbg {
LDBG_WAVE_KERNEL void k_fence_or_scan(uint32_t* out) {
    if (wave_lane() == 0) wave_fence();
    else *out = wave_incl_scan_u32(1u);
}
}  // namespace ldbg

int main() {
    uint32_t out = 0;
    ldbg::sim::lanes_setting() = 2;
    LDBG_LAUNCH(ldbg::k_fence_or_scan, 1, 2, nullptr, &out);
    printf("no divergence seen\n");
    return 0;
}
