// Kernel selection on the host (csrc/pt_flavour.h select_megakernel / select_wavefront): the flavour
// id of every combination of pipeline, the options trav, fastrcp, mailbox, bf, fuse (unset, 0, 1) and
// the four scene facts, one per line ("invalid": the launcher answers hipErrorInvalidValue), after
// two lines that list the instantiated flavours.  tests/test_flavour_select.py compares the output
// with tests/golden/flavour_select.txt.
//   c++ -std=c++17 -I brown-cs2240-path-tracer_amd/csrc scripts/flavour_select_harness.cpp -o harness && ./harness
#include <cstdio>

#include "pt_flavour.h"

int main() {
#define PRINT_ID(T) std::printf(" %d", T);
    std::printf("megakernel:");
    PT_MEGA_FLAVOURS(PRINT_ID)
    std::printf("\nwavefront:");
    PT_WF_FLAVOURS(PRINT_ID)
    std::printf("\n");
    for (int wf = 0; wf < 2; ++wf)
        for (int trav = -1; trav < pt::TRAV_BASE_COUNT; ++trav)  // unset, nested .. lean32
            for (int facts = 0; facts < 16; ++facts)  // fast_rcp | mailbox << 1 | big leaves << 2 | pre-resolved table << 3
                for (int fastrcp = -1; fastrcp < 2; ++fastrcp)
                    for (int mailbox = -1; mailbox < 2; ++mailbox)
                        for (int bf = -1; bf < 2; ++bf)
                            for (int fuse = -1; fuse < 2; ++fuse) {
                                pt::LaunchOpts lo;  // as pt_capi_render.hip launch_opts fills it
                                lo.wavefront = wf != 0;
                                lo.set_flavour_opts(trav, fastrcp, mailbox, bf, fuse);
                                const bool f0 = facts & 1, f1 = facts & 2, f2 = facts & 4, f3 = facts & 8;
                                const int id = wf ? pt::select_wavefront(lo, f0, f1, f2, f3) : pt::select_megakernel(lo, f0, f1, f2, f3);
                                if (wf ? pt::wf_instantiated(id) : pt::mega_instantiated(id)) std::printf("%d\n", id);
                                else std::printf("invalid\n");
                            }
    return 0;
}
