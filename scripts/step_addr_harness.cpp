// Stand-alone check of step_addr32_ok (csrc/pt_step_addr.h): when the fused step kernel may address a
// part's queues with 32-bit byte offsets.  Standard C++, no GPU, no library.
//
// usage: step_addr_harness QCAP PATHS [QCAP PATHS ...]   -> one line "QCAP PATHS 0|1" per pair
// (tests/test_step_addr_cpu.py drives it at the 4 GiB boundary).  The boundary is also pinned at
// compile time below.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "pt_step_addr.h"

using pt::step_addr32_ok;

// ray: 32 B per entry, so 2^27 entries span exactly 4 GiB
static_assert(step_addr32_ok((1ull << 27) - 1, 1), "largest offset 2^32 - 32 fits");
static_assert(!step_addr32_ok(1ull << 27, 1), "largest offset 2^32 does not fit");
static_assert(!step_addr32_ok((1ull << 27) + 1, 1), "largest offset 2^32 + 32 does not fit");
// rad: 12 B per path; 357913941 * 12 = 2^32 - 4
static_assert(step_addr32_ok(64, 357913941ull), "largest offset 2^32 - 4 fits");
static_assert(!step_addr32_ok(64, 357913942ull), "largest offset 2^32 + 8 does not fit");
// neither term may hide the other, and the products do not wrap at 64 bits' lower half
static_assert(!step_addr32_ok(1ull << 27, 357913942ull), "both too large");
static_assert(!step_addr32_ok(0xffffffffull, 0xffffffffull), "a uint32_t's largest values");
static_assert(step_addr32_ok(0, 0), "an empty part");

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: %s QCAP PATHS [QCAP PATHS ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 1 < argc; i += 2) {
        char *e0 = nullptr, *e1 = nullptr;
        const uint64_t qcap = std::strtoull(argv[i], &e0, 10), paths = std::strtoull(argv[i + 1], &e1, 10);
        if (*e0 || *e1) {
            std::fprintf(stderr, "not a number: %s %s\n", argv[i], argv[i + 1]);
            return 2;
        }
        std::printf("%" PRIu64 " %" PRIu64 " %d\n", qcap, paths, step_addr32_ok(qcap, paths) ? 1 : 0);
    }
    return 0;
}
