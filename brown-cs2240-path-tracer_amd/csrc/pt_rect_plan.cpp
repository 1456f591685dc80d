// pt_rect_plan.cpp — pt_rect_plan.h: a rectangle list checked and planned on the host.
#include "pt_rect_plan.h"

#include <algorithm>
#include <map>

namespace pt {

namespace {

std::string show(const pt_window& r) {
    return "(" + std::to_string(r.x0) + ", " + std::to_string(r.y0) + ", " + std::to_string(r.w) + ", " + std::to_string(r.h) + ")";
}
std::string name(size_t k, const pt_window& r) { return "rects[" + std::to_string(k) + "] = " + show(r); }

int invalid(std::string& err, const std::string& msg) {
    err = msg;
    return PT_ERR_INVALID;
}

}  // namespace

int plan_rects(const pt_window* frame, uint32_t W, uint32_t H, const pt_window* rects, size_t n, RectPlan& plan,
               std::string& err) {
    plan = RectPlan{};
    if (W < 1 || H < 1 || W > 32768 || H > 32768) return invalid(err, "rects: the image's width and height must lie in [1, 32768]");
    const pt_window whole = {0, 0, W, H};
    const pt_window fr = frame ? *frame : whole;
    if (fr.w < 1 || fr.h < 1) return invalid(err, "rects: frame " + show(fr) + ": w and h must be at least 1");
    if ((uint64_t)fr.x0 + fr.w > W || (uint64_t)fr.y0 + fr.h > H)
        return invalid(err, "rects: frame " + show(fr) + " must lie within the image (" + std::to_string(W) + " x " + std::to_string(H) + ")");
    if (n == 0) return invalid(err, "rects: the list is empty (n must be at least 1)");
    if (n > kMaxRects) return invalid(err, "rects: " + std::to_string(n) + " rectangles, at most " + std::to_string(kMaxRects));
    if (!rects) return invalid(err, "rects is NULL");
    plan.rows.resize(n);
    for (size_t k = 0; k < n; ++k) {
        const pt_window& r = rects[k];
        if (r.w < 1 || r.h < 1) return invalid(err, name(k, r) + ": w and h must be at least 1");
        if (r.x0 < fr.x0 || r.y0 < fr.y0 || (uint64_t)r.x0 + r.w > (uint64_t)fr.x0 + fr.w ||
            (uint64_t)r.y0 + r.h > (uint64_t)fr.y0 + fr.h)
            return invalid(err, name(k, r) + " lies outside the frame " + show(fr));
        RectRow& row = plan.rows[k];
        row = RectRow{r.x0, r.y0, r.w, r.h, (uint32_t)plan.npix, {0, 0, 0}};
        // inside the image, so the sums stay below 2^32 as long as the list is disjoint; an
        // overlapping list is rejected below before anything reads them
        plan.npix += (uint64_t)r.w * r.h;
        plan.nblocks += (uint64_t)((r.w + 15) / 16) * ((r.h + 15) / 16);
    }
    // overlap: a sweep down the rows.  A rectangle leaves the open set at the row below its last (before
    // the ones that begin there: sharing an edge is no overlap) and enters it at its first; the open
    // rectangles are disjoint in x, so the newcomer can only meet its neighbours by x0.
    struct Event { uint32_t y, begins, k; };
    std::vector<Event> ev(2 * n);
    for (size_t k = 0; k < n; ++k) {
        ev[2 * k] = Event{rects[k].y0, 1u, (uint32_t)k};
        ev[2 * k + 1] = Event{rects[k].y0 + rects[k].h, 0u, (uint32_t)k};
    }
    std::sort(ev.begin(), ev.end(), [](const Event& a, const Event& b) {
        return a.y != b.y ? a.y < b.y : a.begins != b.begins ? a.begins < b.begins : a.k < b.k;
    });
    std::map<uint32_t, uint32_t> open;  // x0 -> rectangle
    for (const Event& e : ev) {
        const pt_window& r = rects[e.k];
        if (!e.begins) {
            open.erase(r.x0);
            continue;
        }
        size_t other = n;
        const auto next = open.lower_bound(r.x0);
        if (next != open.end() && next->first < r.x0 + r.w) other = next->second;
        if (other == n && next != open.begin()) {
            const auto prev = std::prev(next);
            if (rects[prev->second].x0 + rects[prev->second].w > r.x0) other = prev->second;
        }
        if (other != n) {
            const size_t a = std::min<size_t>(other, e.k), b = std::max<size_t>(other, e.k);
            return invalid(err, name(a, rects[a]) + " and " + name(b, rects[b]) + " overlap");
        }
        open.emplace(r.x0, e.k);
    }
    return PT_OK;
}

void plan_blocks(const RectPlan& plan, std::vector<RectBlock>& blocks) {
    blocks.clear();
    blocks.reserve(plan.nblocks);
    for (size_t k = 0; k < plan.rows.size(); ++k) {
        const RectRow& r = plan.rows[k];
        const uint32_t nx = (r.w + 15) / 16, ny = (r.h + 15) / 16;
        for (uint32_t by = 0; by < ny; ++by)
            for (uint32_t bx = 0; bx < nx; ++bx) blocks.push_back(RectBlock{(uint32_t)k, bx | by << 16});
    }
}

}  // namespace pt
