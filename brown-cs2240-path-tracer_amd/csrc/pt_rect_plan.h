// pt_rect_plan.h — the plan of a rectangle-list render (pt_render_rects): the list checked, every
// rectangle's first slot, and the megakernel's block table.  Standard C++ only, no HIP: a
// stand-alone program links pt_rect_plan.cpp (scripts/rect_plan_harness.cpp, tests/test_rects_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pt_hip.h"

namespace pt {

constexpr size_t kMaxRects = 65536;

// One rectangle as the kernels read it (32 bytes): its place in the IMAGE, the slot of its first
// pixel — the pixels of the list are numbered rectangle after rectangle in list order, row-major
// inside each.
struct alignas(16) RectRow {
    uint32_t x0, y0, w, h;
    uint32_t first;
    uint32_t pad[3];
};
static_assert(sizeof(RectRow) == 32, "RectRow is two 16-byte loads");

// One 16 x 16 block of the megakernel's grid: its rectangle and which block of it (bx | by << 16;
// a rectangle has at most 2048 blocks either way)
struct RectBlock { uint32_t rect, bxy; };

struct RectPlan {
    std::vector<RectRow> rows;  // list order
    uint64_t npix = 0;          // pixels per frame: the sum of the areas
    uint64_t nblocks = 0;       // 16 x 16 blocks, every rectangle its own
};

// frame (NULL: the whole W x H image) must lie inside the image, every rectangle inside frame with
// w, h >= 1, 1 <= n <= kMaxRects, and no two rectangles may share a pixel (a sort and a sweep down
// the rows, O(n log n)).  PT_OK, or PT_ERR_INVALID with err naming the offending rectangle(s).
int plan_rects(const pt_window* frame, uint32_t W, uint32_t H, const pt_window* rects, size_t n, RectPlan& plan,
               std::string& err);

// the block table of a plan: nblocks entries, rectangle after rectangle, row-major inside each
void plan_blocks(const RectPlan& plan, std::vector<RectBlock>& blocks);

}  // namespace pt
