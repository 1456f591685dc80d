// view_plan_harness.cpp — the planner of view-list renders (csrc/pt_view_plan.cpp, which calls
// csrc/pt_rect_plan.cpp for the destinations' disjointness) in a stand-alone program, so that it runs under
// -fsanitize=address,undefined without Python or a GPU (tests/test_views_cpu.py builds and runs it).
//
//   view_plan_harness cases FILE    one case per line: ATLAS_W ATLAS_H N, then N times
//                                   W H x0 y0 w h MODEL LENS FOCUS DST_X DST_Y FRAME0 RESERVED RR_BITS DIRECT
//                                   (W, H, LENS, FOCUS, DIRECT: floats as strtof reads them, "nan" and "inf"
//                                   included; RR_BITS: meta[45]'s bit pattern).  Prints per case
//                                   "ok NPIX FIRST..." or "invalid MESSAGE".
//   view_plan_harness random SEED LISTS
//                                   random lists, valid by construction or broken in one random way, against
//                                   checks and prefix sums done here; prints "lists L accepted A rejected R
//                                   mismatches M".
//   view_plan_harness ones N        N views of 1 x 1 in a 256-wide atlas; prints "ok NPIX" or
//                                   "invalid MESSAGE".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "pt_view_plan.h"

using pt::ViewPlan;

static pt_view make_view(float W, float H, pt_window win, uint32_t dx, uint32_t dy) {
    pt_view v;
    std::memset(&v, 0, sizeof v);
    v.meta[0] = W; v.meta[1] = H;
    v.meta[45] = 0.9f;
    v.win = win;
    v.dst_x = dx; v.dst_y = dy;
    return v;
}

static bool plan_holds(const std::vector<pt_view>& v, const ViewPlan& plan) {
    if (plan.first.size() != v.size()) return false;
    uint64_t first = 0;
    for (size_t k = 0; k < v.size(); ++k) {
        if (plan.first[k] != first) return false;
        first += (uint64_t)v[k].win.w * v[k].win.h;
    }
    return plan.npix == first;
}

static int run_cases(const char* path) {
    std::ifstream in(path);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::vector<std::string> tok;
        for (std::string t; ss >> t;) tok.push_back(t);
        if (tok.size() < 3) { std::fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
        auto u = [&](size_t i) { return (uint32_t)std::strtoul(tok[i].c_str(), nullptr, 10); };
        auto f = [&](size_t i) { return std::strtof(tok[i].c_str(), nullptr); };
        const uint32_t aw = u(0), ah = u(1);
        const size_t n = u(2);
        if (tok.size() != 3 + 15 * n) { std::fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
        std::vector<pt_view> v(n);
        for (size_t k = 0; k < n; ++k) {
            const size_t b = 3 + 15 * k;
            v[k] = make_view(f(b), f(b + 1), pt_window{u(b + 2), u(b + 3), u(b + 4), u(b + 5)}, u(b + 9), u(b + 10));
            v[k].cam = pt_camera{u(b + 6), f(b + 7), f(b + 8), 0};
            v[k].frame0 = u(b + 11);
            v[k].reserved = u(b + 12);
            const uint32_t rr = u(b + 13);
            std::memcpy(&v[k].meta[45], &rr, sizeof rr);
            v[k].meta[46] = f(b + 14);
        }
        ViewPlan plan;
        std::string err;
        const int rc = pt::plan_views(n ? v.data() : nullptr, n, aw, ah, 1, 1, plan, err);
        if (rc != PT_OK) { std::printf("invalid %s\n", err.c_str()); continue; }
        if (!plan_holds(v, plan)) { std::printf("broken plan\n"); continue; }
        std::printf("ok %llu", (unsigned long long)plan.npix);
        for (const uint32_t fst : plan.first) std::printf(" %u", fst);
        std::printf("\n");
    }
    return 0;
}

static bool overlap(const pt_view& a, const pt_view& b) {
    return a.dst_x < b.dst_x + b.win.w && b.dst_x < a.dst_x + a.win.w && a.dst_y < b.dst_y + b.win.h &&
           b.dst_y < a.dst_y + a.win.h;
}

static int run_random(uint32_t seed, int lists) {
    std::mt19937 rng(seed);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    int accepted = 0, rejected = 0, mismatches = 0;
    for (int l = 0; l < lists; ++l) {
        const uint32_t aw = pick(1, 96), ah = pick(1, 96);
        // destinations: some cells of a random grid over the atlas, shuffled — disjoint by construction
        std::vector<pt_view> v;
        const uint32_t cw = pick(1, 9), ch = pick(1, 9);
        for (uint32_t y = 0; y < ah; y += ch)
            for (uint32_t x = 0; x < aw; x += cw)
                if (rng() % 3) {
                    const uint32_t w = std::min(cw, aw - x), h = std::min(ch, ah - y);
                    const uint32_t W = w + pick(0, 5), H = h + pick(0, 5);
                    pt_view nv = make_view((float)W, (float)H, pt_window{pick(0, W - w), pick(0, H - h), w, h}, x, y);
                    nv.frame0 = pick(0, (1u << 24) - 1);
                    nv.cam.model = pick(0, 3);
                    nv.cam.lens_radius = 0.1f;
                    nv.cam.focus_distance = 2.0f;
                    v.push_back(nv);
                }
        std::shuffle(v.begin(), v.end(), rng);
        bool want_ok = !v.empty();
        if (!v.empty() && l % 2) {  // broken in one way
            pt_view& b = v[rng() % v.size()];
            switch (rng() % 9) {
                case 0: b.reserved = 1; break;
                case 1: b.win.w = 0; break;
                case 2: b.win.x0 = (uint32_t)b.meta[0] - b.win.w + 1; break;
                case 3: b.dst_x = aw - b.win.w + 1; break;
                case 4: b.cam.model = 4; break;
                case 5: b.frame0 = 1u << 24; break;
                case 6: b.meta[0] = 0.5f; break;
                case 7: b.cam = pt_camera{PT_CAMERA_THIN_LENS, -1.0f, 1.0f, 0}; break;
                default: {  // a second view onto one of its pixels
                    pt_view c = make_view(4.0f, 4.0f, pt_window{0, 0, 1, 1}, b.dst_x + b.win.w - 1, b.dst_y + b.win.h - 1);
                    v.push_back(c);
                    break;
                }
            }
            want_ok = false;
        }
        bool clash = false;
        for (size_t a = 0; a < v.size() && !clash; ++a)
            for (size_t b = a + 1; b < v.size() && !clash; ++b) clash = overlap(v[a], v[b]);
        if (clash) want_ok = false;
        ViewPlan plan;
        std::string err;
        const int rc = pt::plan_views(v.empty() ? nullptr : v.data(), v.size(), aw, ah, 1, 1, plan, err);
        if ((rc == PT_OK) != want_ok || (rc == PT_OK && !plan_holds(v, plan)) ||
            (rc != PT_OK && (err.empty() || (!v.empty() && err.find("views[") == std::string::npos)))) {
            ++mismatches;
            std::printf("list %d: rc %d, expected %s (%s)\n", l, rc, want_ok ? "ok" : "invalid", err.c_str());
        }
        (rc == PT_OK ? accepted : rejected)++;
    }
    std::printf("lists %d accepted %d rejected %d mismatches %d\n", lists, accepted, rejected, mismatches);
    return mismatches ? 1 : 0;
}

static int run_ones(size_t n) {
    std::vector<pt_view> v(n);
    // (k * 97 mod 256 visits every column of a row once: the destinations are disjoint, in no raster order)
    for (size_t k = 0; k < n; ++k)
        v[k] = make_view(8.0f, 8.0f, pt_window{(uint32_t)(k % 8), (uint32_t)(k / 8 % 8), 1, 1}, (uint32_t)((k * 97) % 256),
                         (uint32_t)(k / 256));
    ViewPlan plan;
    std::string err;
    const int rc = pt::plan_views(v.data(), n, 256, 32768, 1, 1, plan, err);
    if (rc != PT_OK) std::printf("invalid %s\n", err.c_str());
    else std::printf("%s %llu\n", plan_holds(v, plan) ? "ok" : "broken plan", (unsigned long long)plan.npix);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "cases")) return run_cases(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "random")) return run_random((uint32_t)std::atol(argv[2]), std::atoi(argv[3]));
    if (argc == 3 && !std::strcmp(argv[1], "ones")) return run_ones((size_t)std::atol(argv[2]));
    std::fprintf(stderr, "usage: view_plan_harness cases FILE | random SEED LISTS | ones N\n");
    return 2;
}
