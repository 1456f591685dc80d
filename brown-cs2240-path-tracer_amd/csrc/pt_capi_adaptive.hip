// pt_capi_adaptive.hip — C ABI (include/pt_hip.h): the tile noise estimate, the per-tile mean and the
// adaptive driver.  Host code only; the kernels are pt_image.hip's.
#include <cmath>
#include <algorithm>

#include "pt_capi_internal.h"

using namespace pt;

namespace pt {

static_assert(sizeof(pt_tile_noise) == 16 && sizeof(TileNoise) == 16 && offsetof(pt_tile_noise, max_err) == 8 &&
                  offsetof(TileNoise, max_err) == 8,
              "pt_tile_noise is 16 bytes");

int make_grid(uint32_t w, uint32_t h, size_t row_pitch, uint32_t tile_w, uint32_t tile_h, TileGrid& g) {
    if (w < 1 || h < 1 || w > 32768 || h > 32768) return fail(PT_ERR_INVALID, "tiles: w and h must lie in [1, 32768]");
    if (row_pitch < w) return fail(PT_ERR_INVALID, "row_pitch is smaller than the buffer's width");
    if (row_pitch > 0xffffffffull) return fail(PT_ERR_INVALID, "row_pitch out of range");
    if (tile_w < 1 || tile_h < 1) return fail(PT_ERR_INVALID, "tiles: tile_w and tile_h must be at least 1");
    g = TileGrid{w, h, (uint32_t)row_pitch, tile_w, tile_h, (w - 1) / tile_w + 1, (h - 1) / tile_h + 1};
    return PT_OK;
}
int ensure_tiles(pt_scene* s, size_t T, pt_tile_noise*& d_noise, uint32_t*& d_frames) {
    PT_TRY(s->d_tiles.ensure(T * (sizeof(pt_tile_noise) + sizeof(uint32_t)), "tiles"));
    d_noise = reinterpret_cast<pt_tile_noise*>(s->d_tiles.p);
    d_frames = reinterpret_cast<uint32_t*>(s->d_tiles.p + T * sizeof(pt_tile_noise));
    return PT_OK;
}
static int check_tol(double tol, double floor) {
    if (!(std::isfinite(tol) && tol > 0.0)) return fail(PT_ERR_INVALID, "tol must be finite and > 0");
    if (!(std::isfinite(floor) && floor > 0.0)) return fail(PT_ERR_INVALID, "floor must be finite and > 0");
    return PT_OK;
}
static int check_adaptive(const pt_adaptive& a) {
    if (a.tile_w < 1 || a.tile_h < 1) return fail(PT_ERR_INVALID, "pt_adaptive: tile_w and tile_h must be at least 1");
    if (a.min_frames < 2) return fail(PT_ERR_INVALID, "pt_adaptive: min_frames must be at least 2");
    if (a.step_frames < 1) return fail(PT_ERR_INVALID, "pt_adaptive: step_frames must be at least 1");
    if (a.max_frames < a.min_frames) return fail(PT_ERR_INVALID, "pt_adaptive: max_frames must be at least min_frames");
    if (!(std::isfinite(a.tol) && a.tol > 0.0)) return fail(PT_ERR_INVALID, "pt_adaptive: tol must be finite and > 0");
    if (!(std::isfinite(a.floor) && a.floor > 0.0)) return fail(PT_ERR_INVALID, "pt_adaptive: floor must be finite and > 0");
    if (!(a.noisy_fraction >= 0.0 && a.noisy_fraction < 1.0))
        return fail(PT_ERR_INVALID, "pt_adaptive: noisy_fraction must lie in [0, 1)");
    return PT_OK;
}

// The rectangles of a mask of active tiles (pt_selftest_tile_rects): tile rows top to bottom, the
// maximal runs of active tiles in each; a run with the columns of a rectangle that reached the row
// above extends it, any other opens a new one.  (tx0, ty0, width, height) in tiles, in opening order.
static void tile_rects(const uint8_t* active, uint32_t tx, uint32_t ty, std::vector<std::array<uint32_t, 4>>& out) {
    out.clear();
    std::vector<size_t> open, next;  // rectangles whose last row is the previous / this one
    for (uint32_t y = 0; y < ty; ++y) {
        next.clear();
        const uint8_t* row = active + (size_t)y * tx;
        for (uint32_t x = 0; x < tx;) {
            if (!row[x]) { ++x; continue; }
            uint32_t x1 = x;
            while (x1 < tx && row[x1]) ++x1;
            size_t k = out.size();
            for (size_t c : open)
                if (out[c][0] == x && out[c][2] == x1 - x) k = c;
            if (k == out.size()) out.push_back({x, y, x1 - x, 1u});
            else ++out[k][3];
            next.push_back(k);
            x = x1;
        }
        open.swap(next);
    }
}

}  // namespace pt

extern "C" {

int pt_noise_tiles_async(pt_scene* s, const float* d_accum, const float* d_m2, uint32_t w, uint32_t h, size_t row_pitch,
                         uint32_t tile_w, uint32_t tile_h, const uint32_t* d_frames, double tol, double floor,
                         pt_tile_noise* d_out, void* stream) {
    if (!s || !d_accum || !d_m2 || !d_frames || !d_out) return fail(PT_ERR_INVALID, "null argument");
    TileGrid g{};
    int rc = make_grid(w, h, row_pitch, tile_w, tile_h, g);
    if (rc != PT_OK || (rc = check_tol(tol, floor)) != PT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    HIP_TRY(launch_noise_tiles(d_accum, d_m2, g, d_frames, tol, floor, reinterpret_cast<TileNoise*>(d_out),
                               static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_tile_mean_async(pt_scene* s, const float* d_accum, uint32_t w, uint32_t h, size_t row_pitch, uint32_t tile_w,
                       uint32_t tile_h, const uint32_t* d_frames, float* d_mean, void* stream) {
    if (!s || !d_accum || !d_frames || !d_mean) return fail(PT_ERR_INVALID, "null argument");
    TileGrid g{};
    const int rc = make_grid(w, h, row_pitch, tile_w, tile_h, g);
    if (rc != PT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    HIP_TRY(launch_tile_mean(d_accum, g, d_frames, d_mean, static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_noise_tiles(pt_scene* s, const float* accum, const float* m2, uint32_t w, uint32_t h, uint32_t tile_w,
                   uint32_t tile_h, const uint32_t* frames, double tol, double floor, pt_tile_noise* out) {
    if (!s || !accum || !m2 || !frames || !out) return fail(PT_ERR_INVALID, "null argument");
    TileGrid g{};
    int rc = make_grid(w, h, w, tile_w, tile_h, g);
    if (rc != PT_OK || (rc = check_tol(tol, floor)) != PT_OK) return rc;
    const size_t n = (size_t)w * h * 3, T = (size_t)g.tx * g.ty;
    Blocking b(s);
    pt_tile_noise* d_noise = nullptr;
    uint32_t* d_frames = nullptr;
    if ((rc = b.device()) != PT_OK || (rc = s->d_accum.ensure(n, "accumulator")) != PT_OK ||
        (rc = s->d_m2.ensure(n, "second moments")) != PT_OK || (rc = ensure_tiles(s, T, d_noise, d_frames)) != PT_OK ||
        (rc = b.open()) != PT_OK)
        return rc;
    PT_TRY(b.in(s->d_accum.p, accum, n * sizeof(float)));
    PT_TRY(b.in(s->d_m2.p, m2, n * sizeof(float)));
    PT_TRY(b.in(d_frames, frames, T * sizeof(uint32_t)));
    PT_TRY(pt_noise_tiles_async(s, s->d_accum.p, s->d_m2.p, w, h, w, tile_w, tile_h, d_frames, tol, floor, d_noise, s->stream));
    PT_TRY(b.out(out, d_noise, T * sizeof(pt_tile_noise)));
    return b.finish(Blocking::kNoWatchdog);  // no render of this call: the next call of the scene takes the watchdog
}

int pt_selftest_tile_rects(const uint8_t* active, uint32_t tx, uint32_t ty, uint32_t* rects, size_t cap, size_t* n_out) {
    if (!active || !n_out || (!rects && cap)) return fail(PT_ERR_INVALID, "null argument");
    if (tx < 1 || ty < 1 || (uint64_t)tx * ty > (1ull << 30)) return fail(PT_ERR_INVALID, "tile counts out of range");
    std::vector<std::array<uint32_t, 4>> r;
    tile_rects(active, tx, ty, r);
    *n_out = r.size();
    for (size_t k = 0; k < std::min(cap, r.size()); ++k)
        for (int c = 0; c < 4; ++c) rects[4 * k + c] = r[k][c];
    if (r.size() > cap) return fail(PT_ERR_INVALID, "rects holds fewer rectangles than the mask has (*n_out)");
    return PT_OK;
}

int pt_render_adaptive(pt_scene* s, const float meta[48], const pt_window* win, const pt_adaptive* ad, uint32_t frame0,
                       int max_depth, int mode, float* accum, float* m2, uint32_t* tile_frames, pt_tile_noise* tile_noise,
                       uint8_t* rgba, pt_counters* counters, uint32_t* passes) {
    if (!s || !meta || !ad || !accum || !tile_frames) return fail(PT_ERR_INVALID, "null argument");
    PT_TRY(check_adaptive(*ad));
    if ((uint64_t)frame0 + ad->max_frames > (1ull << 24))
        return fail(PT_ERR_INVALID, "frame0 + max_frames exceeds 2^24 (t_k = u32(f32(k)) would round)");
    FrameParams fp{};
    PT_TRY(make_params(meta, max_depth, fp, win));
    const uint32_t W = fp.win_w, H = fp.win_h;
    TileGrid g{};
    PT_TRY(make_grid(W, H, W, ad->tile_w, ad->tile_h, g));
    const size_t npix = (size_t)W * H, n = 3 * npix, T = (size_t)g.tx * g.ty;
    Blocking b(s, counters);
    pt_tile_noise* d_noise = nullptr;
    uint32_t* d_frames = nullptr;
    int rc;
    if ((rc = b.device()) != PT_OK || (rc = s->d_accum.ensure(n, "accumulator")) != PT_OK ||
        (rc = s->d_m2.ensure(n, "second moments")) != PT_OK || (rc = ensure_tiles(s, T, d_noise, d_frames)) != PT_OK ||
        (rc = b.open()) != PT_OK)
        return rc;
    if (rgba && ((rc = s->d_mean.ensure(n, "tile mean")) != PT_OK ||
                 (rc = s->d_rgba.ensure(4 * npix, "image")) != PT_OK))
        return rc;
    PT_TRY(b.zero(s->d_accum.p, n * sizeof(float)));
    PT_TRY(b.zero(s->d_m2.p, n * sizeof(float)));
    PT_TRY(b.zero(d_frames, T * sizeof(uint32_t)));
    Counters* const d_cnt = b.d_cnt();
    // pass 0: the whole window
    const pt_window whole = {fp.win_x0, fp.win_y0, W, H};
    PT_TRY(render_impl(s, meta, frame0, ad->min_frames, 1, max_depth, mode, true, s->d_accum.p, d_cnt, s->stream, &whole,
                       nullptr, s->d_m2.p));
    std::vector<uint32_t> frames(T, ad->min_frames);
    std::vector<pt_tile_noise> noise(T);
    std::vector<uint8_t> active(T);
    std::vector<std::array<uint32_t, 4>> rects;
    std::vector<pt_window> list;
    uint32_t done = ad->min_frames, npass = 1;  // done: the frames of every tile still active
    for (;;) {
        PT_TRY(b.in(d_frames, frames.data(), T * sizeof(uint32_t)));
        PT_TRY(pt_noise_tiles_async(s, s->d_accum.p, s->d_m2.p, W, H, W, ad->tile_w, ad->tile_h, d_frames, ad->tol, ad->floor,
                                    d_noise, s->stream));
        PT_TRY(b.out(noise.data(), d_noise, T * sizeof(pt_tile_noise)));
        PT_TRY(b.sync(Blocking::kWatchdog));  // once per pass: the verdicts decide the next
        size_t nact = 0;
        for (size_t t = 0; t < T; ++t) {
            active[t] = noise[t].noisy > (uint32_t)(ad->noisy_fraction * noise[t].pixels) && frames[t] < ad->max_frames;
            nact += active[t];
        }
        if (nact == 0) break;
        // the active tiles' next frames: one frame range over the rectangles of the active set, clipped
        // to the window, as ONE list render in place inside the window's buffers
        const uint32_t nf = std::min(ad->step_frames, ad->max_frames - done);
        tile_rects(active.data(), g.tx, g.ty, rects);
        list.clear();
        for (const auto& r : rects) {
            const uint32_t px = r[0] * g.tile_w, py = r[1] * g.tile_h;
            const uint32_t pw = (uint32_t)std::min<uint64_t>((uint64_t)r[2] * g.tile_w, W - px);
            const uint32_t ph = (uint32_t)std::min<uint64_t>((uint64_t)r[3] * g.tile_h, H - py);
            list.push_back(pt_window{fp.win_x0 + px, fp.win_y0 + py, pw, ph});
        }
        for (size_t k = 0; k < list.size(); k += kMaxRects)  // (a list call takes kMaxRects rectangles)
            PT_TRY(render_impl(s, meta, frame0 + done, nf, 1, max_depth, mode, true, s->d_accum.p, d_cnt, s->stream, &whole,
                               nullptr, s->d_m2.p, list.data() + k, std::min(kMaxRects, list.size() - k)));
        for (size_t t = 0; t < T; ++t)
            if (active[t]) frames[t] += nf;
        done += nf;
        ++npass;
    }
    if (rgba) {  // the display transform of the per-tile mean (d_frames holds the final counts)
        PT_TRY(pt_tile_mean_async(s, s->d_accum.p, W, H, W, ad->tile_w, ad->tile_h, d_frames, s->d_mean.p, s->stream));
        PT_TRY(pt_tonemap_async(s, s->d_mean.p, npix, 1, s->d_rgba.p, s->stream));
        PT_TRY(b.out(rgba, s->d_rgba.p, 4 * npix));
    }
    PT_TRY(b.out(accum, s->d_accum.p, n * sizeof(float)));
    if (m2) PT_TRY(b.out(m2, s->d_m2.p, n * sizeof(float)));
    PT_TRY(b.finish(Blocking::kNoWatchdog));  // taken below, after the tiles' results are out
    std::memcpy(tile_frames, frames.data(), T * sizeof(uint32_t));
    if (tile_noise) std::memcpy(tile_noise, noise.data(), T * sizeof(pt_tile_noise));
    if (passes) *passes = npass;
    return take_watchdog(s);
}

}  // extern "C"
