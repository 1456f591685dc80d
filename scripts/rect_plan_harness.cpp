// rect_plan_harness.cpp — the planner of rectangle-list renders (csrc/pt_rect_plan.cpp) in a
// stand-alone program, so that it runs under -fsanitize=address,undefined without Python or a GPU
// (tests/test_rects_cpu.py builds and runs it).
//
//   rect_plan_harness cases FILE    one case per line: W H fx fy fw fh n, then n times x0 y0 w h
//                                   (fw = 0: no frame).  Prints per case "ok NPIX FIRST..." or
//                                   "invalid MESSAGE".
//   rect_plan_harness random SEED LISTS
//                                   random lists, disjoint by construction or not, against a pairwise
//                                   overlap check and prefix sums done here; prints "lists L accepted A
//                                   rejected R mismatches M".
//   rect_plan_harness ones N        N rectangles of 1 x 1 in a 256-wide image; prints "ok NPIX" or
//                                   "invalid MESSAGE", and the planning time.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "pt_rect_plan.h"

using pt::RectBlock;
using pt::RectPlan;

static bool overlap(const pt_window& a, const pt_window& b) {
    return a.x0 < b.x0 + b.w && b.x0 < a.x0 + a.w && a.y0 < b.y0 + b.h && b.y0 < a.y0 + a.h;
}

// the plan against what it must hold: prefix sums, the pixel count, and a block table that names
// every 16 x 16 block of every rectangle once
static bool plan_holds(const std::vector<pt_window>& r, const RectPlan& plan) {
    if (plan.rows.size() != r.size()) return false;
    uint64_t first = 0, blocks = 0;
    for (size_t k = 0; k < r.size(); ++k) {
        const pt::RectRow& row = plan.rows[k];
        if (row.x0 != r[k].x0 || row.y0 != r[k].y0 || row.w != r[k].w || row.h != r[k].h || row.first != first) return false;
        first += (uint64_t)r[k].w * r[k].h;
        blocks += (uint64_t)((r[k].w + 15) / 16) * ((r[k].h + 15) / 16);
    }
    if (plan.npix != first || plan.nblocks != blocks) return false;
    std::vector<RectBlock> tab;
    pt::plan_blocks(plan, tab);
    if (tab.size() != blocks) return false;
    size_t at = 0;
    for (size_t k = 0; k < r.size(); ++k)
        for (uint32_t by = 0; by < (r[k].h + 15) / 16; ++by)
            for (uint32_t bx = 0; bx < (r[k].w + 15) / 16; ++bx, ++at)
                if (tab[at].rect != k || tab[at].bxy != (bx | by << 16)) return false;
    return true;
}

static int run_cases(const char* path) {
    std::ifstream in(path);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        uint32_t W, H;
        pt_window fr;
        size_t n;
        ss >> W >> H >> fr.x0 >> fr.y0 >> fr.w >> fr.h >> n;
        std::vector<pt_window> r(n);
        for (auto& w : r) ss >> w.x0 >> w.y0 >> w.w >> w.h;
        if (!ss) { std::fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
        RectPlan plan;
        std::string err;
        const int rc = pt::plan_rects(fr.w ? &fr : nullptr, W, H, r.data(), n, plan, err);
        if (rc != PT_OK) { std::printf("invalid %s\n", err.c_str()); continue; }
        if (!plan_holds(r, plan)) { std::printf("broken plan\n"); continue; }
        std::printf("ok %llu", (unsigned long long)plan.npix);
        for (const auto& row : plan.rows) std::printf(" %u", row.first);
        std::printf("\n");
    }
    return 0;
}

static int run_random(uint32_t seed, int lists) {
    std::mt19937 rng(seed);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    int accepted = 0, rejected = 0, mismatches = 0;
    for (int l = 0; l < lists; ++l) {
        const uint32_t W = pick(1, 96), H = pick(1, 96);
        pt_window fr = {0, 0, W, H};
        if (l % 3 == 0) { fr.x0 = pick(0, W - 1); fr.y0 = pick(0, H - 1); fr.w = pick(1, W - fr.x0); fr.h = pick(1, H - fr.y0); }
        std::vector<pt_window> r;
        if (l % 2 == 0) {  // disjoint by construction: some cells of a random grid over the frame, shuffled
            const uint32_t cw = pick(1, 9), ch = pick(1, 9);
            for (uint32_t y = 0; y < fr.h; y += ch)
                for (uint32_t x = 0; x < fr.w; x += cw)
                    if (rng() % 3) r.push_back(pt_window{fr.x0 + x, fr.y0 + y, std::min(cw, fr.w - x), std::min(ch, fr.h - y)});
            std::shuffle(r.begin(), r.end(), rng);
        } else {  // anything inside the frame: most such lists overlap
            const size_t n = pick(1, 12);
            for (size_t k = 0; k < n; ++k) {
                pt_window w;
                w.x0 = fr.x0 + pick(0, fr.w - 1);
                w.y0 = fr.y0 + pick(0, fr.h - 1);
                w.w = pick(1, std::min<uint32_t>(8, fr.x0 + fr.w - w.x0));
                w.h = pick(1, std::min<uint32_t>(8, fr.y0 + fr.h - w.y0));
                r.push_back(w);
            }
        }
        bool clash = false;
        for (size_t a = 0; a < r.size() && !clash; ++a)
            for (size_t b = a + 1; b < r.size() && !clash; ++b) clash = overlap(r[a], r[b]);
        RectPlan plan;
        std::string err;
        const int rc = pt::plan_rects(l % 3 == 0 ? &fr : nullptr, W, H, r.data(), r.size(), plan, err);
        const bool want_ok = !clash && !r.empty();
        if ((rc == PT_OK) != want_ok || (rc == PT_OK && !plan_holds(r, plan)) || (rc != PT_OK && err.empty())) {
            ++mismatches;
            std::printf("list %d: rc %d, expected %s (%s)\n", l, rc, want_ok ? "ok" : "invalid", err.c_str());
        }
        (rc == PT_OK ? accepted : rejected)++;
    }
    std::printf("lists %d accepted %d rejected %d mismatches %d\n", lists, accepted, rejected, mismatches);
    return mismatches ? 1 : 0;
}

static int run_ones(size_t n) {
    std::vector<pt_window> r(n);
    for (size_t k = 0; k < n; ++k) r[k] = pt_window{(uint32_t)((k * 97) % 256), (uint32_t)(k / 256), 1, 1};
    // (k * 97 mod 256 visits every column of a row once: the list is disjoint and in no raster order)
    RectPlan plan;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = pt::plan_rects(nullptr, 256, 32768, r.data(), n, plan, err);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != PT_OK) std::printf("invalid %s\n", err.c_str());
    else std::printf("%s %llu\n", plan_holds(r, plan) ? "ok" : "broken plan", (unsigned long long)plan.npix);
    std::printf("planned in %.1f ms\n", ms);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "cases")) return run_cases(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "random")) return run_random((uint32_t)std::atol(argv[2]), std::atoi(argv[3]));
    if (argc == 3 && !std::strcmp(argv[1], "ones")) return run_ones((size_t)std::atol(argv[2]));
    std::fprintf(stderr, "usage: rect_plan_harness cases FILE | random SEED LISTS | ones N\n");
    return 2;
}
