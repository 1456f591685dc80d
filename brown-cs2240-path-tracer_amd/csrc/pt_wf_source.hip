// pt_wf_source.hip — the two ends of a wavefront batch: where its paths come from and where their
// radiance goes, for the five kinds of PathSource (the table in pt_kernels.h).  Owns the slot maps of the
// lists (row_of, rect_of, view_of, slot_path of a rectangle list; the window's is in pt_wf_queue.h, the
// fused kernel makes camera paths with it too), the compaction of the admitted paths (mark_no_path,
// compact_slot, count_generated), the five generate kernels, k_gather_rays and the four accumulate
// kernels, with their launches: launch_generate, launch_accum (pt_wf_stage.h), launch_gather_rays.
#include "pt_wf_queue.h"
#include "pt_wf_stage.h"

namespace pt {

// The last of n rows whose .first is <= q (rows ordered by .first, rows[0].first = 0), by bisection: the
// rectangle or the view that holds pixel q of its list's frame (n <= 65536: at most 17 steps; neighbouring
// lanes nearly always agree on every one)
template <class Row>
__device__ __forceinline__ uint32_t row_of(const Row* rows, uint32_t n, uint32_t q) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rows[mid].first <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The rectangle of a list that holds pixel q of its frame (q < rl.npix), and q's place inside it
__device__ __forceinline__ RectRow rect_of(const RectList& rl, uint32_t q, uint32_t& i, uint32_t& j) {
    const RectRow r = rl.rows[row_of(rl.rows, rl.n, q)];
    const uint32_t k = q - r.first;
    j = k / r.w;
    i = k - j * r.w;
    return r;
}

// slot_path of a rectangle list (pt_render_rects): path id p = f * npix + q with npix the list's
// pixels and q the pixel's position in the concatenation of the rectangles, row-major inside each
__device__ __forceinline__ uint32_t slot_path(uint32_t s, const RectList& rl, uint32_t& x, uint32_t& y, uint32_t& f) {
    f = s / rl.npix;
    uint32_t i, j;
    const RectRow r = rect_of(rl, s - f * rl.npix, i, j);
    x = r.x0 + i;
    y = r.y0 + j;
    return s;
}

// RL: nothing (the window's instances, whose arguments and code stay as they were), or the call's
// RectList (its slot -> pixel map instead of the window's)
template <bool COUNT, class... RL>
__global__ __launch_bounds__(256) void k_wf_generate(FrameParams fp, WfBuffers wb, uint32_t frame0, uint32_t stride,
                                                     uint32_t fbase, uint32_t P, bool raw_salt, Counters* cnt_out,
                                                     RL... rl) {
    static_assert(sizeof...(RL) <= 1, "at most the one rectangle list");
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) {
        wb.ctl[WF_COUNT0] = P;
        wb.ctl[WF_COUNT1] = 0;
    }
    // region layout (k_wf_step_bf, wb.nreg > 0): 64-path batch j goes to region j % nreg
    const uint32_t R = wb.nreg;
    if (R && p < R) {  // counts of region p: its batches j = t, t + R, ... < ceil(P / 64), t = p rq mod R
        const uint32_t nbat = (P + 63) / 64;
        const uint32_t t = (uint32_t)((uint64_t)p * wb.rq % R);
        const uint32_t n = t < nbat ? (nbat - t + R - 1) / R : 0u;
        const uint32_t last = t + (n - 1) * R;
        wb.rcnt[p] = n == 0 ? 0u : n * 64 - ((last == nbat - 1 && (P & 63)) ? 64 - (P & 63) : 0u);
        wb.rcnt[kRegions + p] = 0;
    }
    Counters c = {};
    if (p < P) {  // p: the queue slot; pid: the path made there (slot_path)
        uint32_t x, y, f;
        uint32_t pid;
        if constexpr (sizeof...(RL) > 0) pid = slot_path(p, rl..., x, y, f);
        else pid = slot_path(p, fp, x, y, f);
        const uint32_t t = raw_salt ? frame0 : (uint32_t)(float)(frame0 + (fbase + f) * stride);
        PathState ps;
        Ray r = path_begin(fp, x, y, t, ps);
        const uint32_t j = p / 64;
        const uint32_t i = R ? (uint32_t)((uint64_t)(j % R) * wb.rqi % R) * wb.rstride + (j / R) * 64 + (p & 63) : p;
        store_entry(wb.ext, i, r, pid, ps);
        if (COUNT) { c.samples++; c.ext_queries++; }
    }
    if (COUNT) flush_counters(c, cnt_out);
}

// What the generate kernels that can reject a sample share (k_wf_generate_rays, _cam, _views, _gather): a
// sample that is not admitted makes no queue entry and counts nothing, and the admitted paths are compacted
// into the queue.  The host zeroes the counts appended to before the launch.

// No path for launch slot p: (-0, -0, -0) in its radiance slot, the one value k_wf_accum's
// acc + (L >= 0 ? L : 0) adds without changing a bit of acc (x + -0 = x for every x, -0 included) and that
// no traced path can leave there (a path's L starts at +0 and is only added to)
__device__ __forceinline__ void mark_no_path(const WfBuffers& wb, uint32_t p) {
    float* o = wb.rad + 3 * (size_t)p;
    o[0] = -0.0f; o[1] = -0.0f; o[2] = -0.0f;
}

// The queue slot of launch slot p's path; every thread of the block calls it, adm: this lane has a path
// (the slot of a lane without one means nothing).  NW: the block's waves.  With the fused kernel's regions
// (wb.nreg > 0) the wave's slots are batch p / 64 of k_wf_generate's layout, so its paths take its region's
// next entries, as k_wf_step_bf appends: one atomicAdd per wave on the region's count (a region receives at
// most the batches k_wf_generate gives it, so it holds them).  Otherwise wave counts -> LDS -> prefix by
// the first wave -> one atomicAdd per block on the queue's count (as k_wf_shade compacts).  No atomic when
// nothing is kept; the order of the entries changes no path's result.
template <uint32_t NW>
__device__ __forceinline__ uint32_t compact_slot(const WfBuffers& wb, uint32_t p, bool adm) {
    static_assert(NW <= 64 && (NW & (NW - 1)) == 0, "the first wave scans the wave counts");
    const uint64_t keep = __ballot(adm);
    const uint32_t R = wb.nreg;
    uint32_t slot = 0;
    if (R) {
        if (keep) {  // wave-uniform
            const uint32_t j = __builtin_amdgcn_readfirstlane(p) / 64;
            const uint32_t rg = (uint32_t)((uint64_t)(j % R) * wb.rqi % R);
            uint32_t base = 0;
            if (lane_id() == 0) base = atomicAdd(&wb.rcnt[rg], (uint32_t)__popcll(keep));
            slot = rg * wb.rstride + __shfl(base, 0, 64) + rank_below(keep);
        }
    } else {
        __shared__ uint32_t s_cnt[NW];
        const uint32_t wv = threadIdx.x / 64;
        if (lane_id() == 0) s_cnt[wv] = (uint32_t)__popcll(keep);
        __syncthreads();
        if (threadIdx.x < 64) {
            const uint32_t n = threadIdx.x < NW ? s_cnt[threadIdx.x] : 0u;
            uint32_t incl = n;
#pragma unroll
            for (uint32_t off = 1; off < NW; off <<= 1) {
                const uint32_t v = __shfl_up(incl, off, 64);
                if (lane_id() >= off) incl += v;
            }
            const uint32_t total = __shfl(incl, NW - 1, 64);
            uint32_t base = 0;
            if (threadIdx.x == 0 && total) base = atomicAdd(&wb.ctl[WF_COUNT0], total);
            base = __shfl(base, 0, 64);
            if (threadIdx.x < NW) s_cnt[threadIdx.x] = base + incl - n;
        }
        __syncthreads();
        slot = s_cnt[wv] + rank_below(keep);
    }
    return slot;
}

// the COUNT epilogue: an admitted path is one sample and one extension query
template <bool COUNT>
__device__ __forceinline__ void count_generated(bool adm, Counters* cnt_out) {
    if (COUNT) {
        Counters c = {};
        if (adm) { c.samples++; c.ext_queries++; }
        flush_counters(c, cnt_out);
    }
}

// k_wf_generate for a ray list (pt_query_radiance; RayList, pt_kernels.h): launch slot p < P is sample
// f = p / n of ray i = p - f n, so neighbouring lanes load neighbouring 32-byte rays (two float4 each)
// and seeds.  Path id p — the radiance index k_wf_accum_rays reads.  The path's seed_in is the ray's seed
// for sample 0 of the call and hash1u(seed + s * 16787) for its sample s = sample0 + fbase + f >= 1.
// A ray that is not admitted (ray_admitted) has no path; its radiance slot is left alone (k_wf_accum_rays
// takes the test again).
template <bool COUNT>
__global__ __launch_bounds__(1024) void k_wf_generate_rays(WfBuffers wb, RayList ql, uint32_t sample0, uint32_t fbase,
                                                           uint32_t P, Counters* cnt_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool adm = false;
    Ray r;
    PathState ps;
    if (p < P) {
        const uint32_t f = p / ql.n, i = p - f * ql.n;
        const float4 a = ql.rays[2 * (size_t)i], b = ql.rays[2 * (size_t)i + 1];
        adm = ray_admitted(b.x, b.y, b.z);
        if (adm) {
            const uint32_t s = sample0 + fbase + f, s0 = ql.seeds[i];
            r.o = mk(a.x, a.y, a.z);
            r.d = mk(b.x, b.y, b.z);
            r.inv = r.d;  // not stored: the trace kernels take 1 / d when they unpack the entry
            path_begin_ray(r, s == 0 ? s0 : hash1u(s0 + s * 16787u), ps);
        }
    }
    const uint32_t slot = compact_slot<16>(wb, p, adm);
    if (adm) store_entry(wb.ext, slot, r, p, ps);
    count_generated<COUNT>(adm, cnt_out);
}

// k_wf_generate under a lens camera (LensCam): k_wf_generate's slot maps — the window,
// the rectangle list, raw_salt — with path_begin_model<MODEL> for path_begin; a sample whose direction is
// not admitted has no path (mark_no_path).
template <bool COUNT, uint32_t MODEL, class... RL>
__global__ __launch_bounds__(256) void k_wf_generate_cam(FrameParams fp, LensCam lc, WfBuffers wb, uint32_t frame0,
                                                         uint32_t stride, uint32_t fbase, uint32_t P, bool raw_salt,
                                                         Counters* cnt_out, RL... rl) {
    static_assert(sizeof...(RL) <= 1, "at most the one rectangle list");
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool adm = false;
    Ray r;
    PathState ps;
    if (p < P) {  // p: the launch slot = the path id (slot_path)
        uint32_t x, y, f;
        if constexpr (sizeof...(RL) > 0) (void)slot_path(p, rl..., x, y, f);
        else (void)slot_path(p, fp, x, y, f);
        const uint32_t t = raw_salt ? frame0 : (uint32_t)(float)(frame0 + (fbase + f) * stride);
        adm = path_begin_model<MODEL>(fp, lc, x, y, t, r, ps);
        if (!adm) mark_no_path(wb, p);
    }
    const uint32_t slot = compact_slot<4>(wb, p, adm);
    if (adm) store_entry(wb.ext, slot, r, p, ps);
    count_generated<COUNT>(adm, cnt_out);
}

// The view of a list that holds pixel q of its frame (q < vl.npix)
__device__ __forceinline__ const ViewRow* view_of(const ViewList& vl, uint32_t q) {
    return vl.rows + row_of(vl.rows, vl.n, q);
}

// k_wf_generate for a view list (pt_render_views; ViewList, pt_kernels.h): launch slot
// p < P is pixel q = p - f npix of frame f = p / npix, path id p.  The slot finds its view (view_of), takes
// the row's camera block into a FrameParams of its own — ten float4 loads; a wave inside one view loads one
// address — and begins its path with path_begin (a pinhole row) or path_begin_model of the row's model, at
// pixel (x0 + i, y0 + j) of the view's image and salt u32(f32(frame0_v + (fbase + f) * stride)).  Those
// functions and camera_ray are the other generate kernels' own; a lens row's sample that is not admitted
// has no path (mark_no_path).
template <bool COUNT>
__global__ __launch_bounds__(256) void k_wf_generate_views(ViewList vl, WfBuffers wb, uint32_t stride, uint32_t fbase,
                                                           uint32_t P, Counters* cnt_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool adm = false;
    Ray r;
    PathState ps;
    if (p < P) {  // p: the launch slot = the path id
        const uint32_t f = p / vl.npix, q = p - f * vl.npix;
        const float4* rw = reinterpret_cast<const float4*>(view_of(vl, q));
        const float4 a = rw[0], b = rw[1], c = rw[2], d = rw[3], e = rw[4], g = rw[9];
        const uint32_t k = q - __float_as_uint(a.x), w = __float_as_uint(a.w);
        const uint32_t j = k / w, i = k - j * w;
        const uint32_t x = __float_as_uint(a.y) + i, y = __float_as_uint(a.z) + j;
        const uint32_t t = (uint32_t)(float)(__float_as_uint(b.w) + (fbase + f) * stride);
        FrameParams fp = {};  // the camera fields alone: nothing else is read before the queue entry stands
        fp.W = c.x; fp.H = c.y; fp.inv_w = c.z; fp.inv_h = c.w;
        fp.aspect = d.x; fp.focal = d.y; fp.view_half_h = d.z;
        fp.cam[0] = e.x; fp.cam[1] = e.y; fp.cam[2] = e.z; fp.cam[3] = e.w;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 col = rw[5 + m];
            fp.M[4 * m] = col.x; fp.M[4 * m + 1] = col.y; fp.M[4 * m + 2] = col.z; fp.M[4 * m + 3] = col.w;
        }
        fp.width = __float_as_uint(g.x); fp.height = __float_as_uint(g.y);
        LensCam lc;
        lc.model = __float_as_uint(d.w);
        lc.lens_radius = g.z;
        lc.focus_distance = g.w;
        switch (lc.model) {
            case CAM_THIN_LENS: adm = path_begin_model<CAM_THIN_LENS>(fp, lc, x, y, t, r, ps); break;
            case CAM_ORTHO: adm = path_begin_model<CAM_ORTHO>(fp, lc, x, y, t, r, ps); break;
            case CAM_EQUIRECT: adm = path_begin_model<CAM_EQUIRECT>(fp, lc, x, y, t, r, ps); break;
            default: r = path_begin(fp, x, y, t, ps); adm = true; break;  // the pinhole: every sample has a path
        }
        if (!adm) mark_no_path(wb, p);
    }
    const uint32_t slot = compact_slot<4>(wb, p, adm);
    if (adm) store_entry(wb.ext, slot, r, p, ps);
    count_generated<COUNT>(adm, cnt_out);
}

// k_wf_generate for a gather list (pt_gather; GatherList, pt_kernels.h): launch slot
// p < P is sample f = p / n of point i = p - f n, so neighbouring lanes load neighbouring 32-byte points
// (two float4 each).  Path id p.  The sample's direction is drawn on the spot (gather_ray<MODE>) with
// sd = gather_seed(seed, sample0 + fbase + f) and its path enters with seed_in = hash1u(sd + 7).  A point
// or a sample that is not admitted has no path (mark_no_path), and k_wf_accum_gather skips its slot.
template <bool COUNT, uint32_t MODE>
__global__ __launch_bounds__(1024) void k_wf_generate_gather(WfBuffers wb, GatherList gl, uint32_t sample0, uint32_t fbase,
                                                             uint32_t P, Counters* cnt_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool adm = false;
    Ray r;
    PathState ps;
    if (p < P) {
        const uint32_t f = p / gl.n, i = p - f * gl.n;
        const float4 a = gl.pts[2 * (size_t)i], b = gl.pts[2 * (size_t)i + 1];
        const uint32_t sd = gather_seed(__float_as_uint(a.w), sample0 + fbase + f);
        adm = gather_ray<MODE>(a, b, sd, r);
        if (adm) {
            r.inv = r.d;  // not stored: the trace kernels take 1 / d when they unpack the entry
            path_begin_ray(r, hash1u(sd + 7u), ps);
        } else {
            mark_no_path(wb, p);
        }
    }
    const uint32_t slot = compact_slot<16>(wb, p, adm);
    if (adm) store_entry(wb.ext, slot, r, p, ps);
    count_generated<COUNT>(adm, cnt_out);
}

// One sample of every point as the ray and seed a radiance query takes (pt_gather_rays): pt_ray
// {o, +inf, d, 0} and seed_in; a point or sample that is not admitted gets d = 0 (o = p) and seed 0.
template <uint32_t MODE>
__global__ __launch_bounds__(256) void k_gather_rays(GatherList gl, uint32_t sample, float4* __restrict__ rays,
                                                     uint32_t* __restrict__ seeds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gl.n) return;
    const float4 a = gl.pts[2 * (size_t)i], b = gl.pts[2 * (size_t)i + 1];
    const uint32_t sd = gather_seed(__float_as_uint(a.w), sample);
    Ray r;
    const bool adm = gather_ray<MODE>(a, b, sd, r);
    if (!adm) { r.o = mk(a.x, a.y, a.z); r.d = mk(0.0f, 0.0f, 0.0f); }
    rays[2 * (size_t)i] = make_float4(r.o.x, r.o.y, r.o.z, __uint_as_float(0x7f800000u));
    rays[2 * (size_t)i + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
    seeds[i] = adm ? hash1u(sd + 7u) : 0u;
}

// acc += clamp(radiance) for the batch's frames in order (program-raymarch.ts:283-285); window
// pixel pix = j * win_w + i lives at acc + 3 * (j * row_pitch + i).  m2 (nullable, with accumulate):
// the second moments at the same place, m2 += clamp(L)^2 in the same frame order, so a call's batches
// continue them as they continue acc.  RL: nothing, or the call's RectList — pix is then the pixel's
// position in the list, and its place the frame-relative one of its rectangle's pixel (win_w unused)
template <class... RL>
__global__ __launch_bounds__(256) void k_wf_accum(const float* __restrict__ rad, float* __restrict__ acc, uint32_t npix,
                                                  uint32_t win_w, uint32_t row_pitch, uint32_t F, bool accumulate,
                                                  float* __restrict__ m2, RL... rl) {
    static_assert(sizeof...(RL) <= 1, "at most the one rectangle list");
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    size_t oi;
    if constexpr (sizeof...(RL) > 0) {
        const RectList& l = (rl, ...);
        uint32_t i, j;
        const RectRow r = rect_of(l, pix, i, j);
        oi = 3 * ((size_t)(r.y0 + j - l.fy0) * row_pitch + (r.x0 + i - l.fx0));
    } else {
        const uint32_t j = pix / win_w;
        oi = 3 * ((size_t)j * row_pitch + (pix - j * win_w));
    }
    float* o = acc + oi;
    f3 a = accumulate ? mk(o[0], o[1], o[2]) : mk(0.0f, 0.0f, 0.0f);
    if (m2) {
        float* q = m2 + oi;
        f3 sq = mk(q[0], q[1], q[2]);
        for (uint32_t f = 0; f < F; ++f) {
            const float* r = rad + 3 * ((size_t)f * npix + pix);
            const f3 L = mk(r[0], r[1], r[2]);
            sq = add_clamped_sq(sq, L);
            a = add_clamped(a, L);
        }
        q[0] = sq.x; q[1] = sq.y; q[2] = sq.z;
    } else {
        for (uint32_t f = 0; f < F; ++f) {
            const float* r = rad + 3 * ((size_t)f * npix + pix);
            f3 L = mk(r[0], r[1], r[2]);
            a = accumulate ? add_clamped(a, L) : L;
        }
    }
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
}

// k_wf_accum for a ray list: acc[3 i + c] += clamp(radiance of sample f of ray i), f = 0 .. F - 1 in order;
// one lane owns ray i for the whole batch (no atomics).  A ray that is not admitted has no path, so its
// radiance slots hold nothing: the lane takes the generate kernel's test again and leaves the ray's row
// of acc alone, bit for bit.
__global__ __launch_bounds__(256) void k_wf_accum_rays(const float* __restrict__ rad, float* __restrict__ acc, RayList ql,
                                                       uint32_t F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ql.n) return;
    const float4 b = ql.rays[2 * (size_t)i + 1];
    if (!ray_admitted(b.x, b.y, b.z)) return;
    float* o = acc + 3 * (size_t)i;
    f3 a = mk(o[0], o[1], o[2]);
    for (uint32_t f = 0; f < F; ++f) {
        const float* r = rad + 3 * ((size_t)f * ql.n + i);
        a = add_clamped(a, mk(r[0], r[1], r[2]));
    }
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
}

// k_wf_accum for a gather list: one lane owns point i for the whole batch (no atomics) and adds its F
// samples in order.  COSINE: acc[3 i + c] += clamp(L_c).  SH9: acc[27 i + 9 c + k] = fmaf(clamp(L_c), Y_k,
// acc[..]) with the nine basis values of the sample's direction, drawn again from its seed (sbase: the
// call's sample index of the batch's first sample); the 27 sums stay in registers.  A sample whose
// radiance slot holds k_wf_generate_gather's -0 mark has no path and is skipped outright (fmaf(-0, Y, acc)
// with Y < 0 would turn a -0 word into +0); a point none of whose samples has a path is not written.
template <uint32_t MODE>
__global__ __launch_bounds__(256) void k_wf_accum_gather(const float* __restrict__ rad, float* __restrict__ acc, GatherList gl,
                                                         uint32_t sbase, uint32_t F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gl.n) return;
    constexpr int W = MODE == GATHER_SH9 ? 27 : 3;
    float* o = acc + W * (size_t)i;
    float a[W];
#pragma unroll
    for (int k = 0; k < W; ++k) a[k] = o[k];
    uint32_t seed = 0;
    if constexpr (MODE == GATHER_SH9) seed = __float_as_uint(gl.pts[2 * (size_t)i].w);
    bool any = false;
    for (uint32_t f = 0; f < F; ++f) {
        const float* r = rad + 3 * ((size_t)f * gl.n + i);
        const float lx = r[0], ly = r[1], lz = r[2];
        if (__float_as_uint(lx) == 0x80000000u) continue;  // no path
        any = true;
        const float L[3] = {lx >= 0.0f ? lx : 0.0f, ly >= 0.0f ? ly : 0.0f, lz >= 0.0f ? lz : 0.0f};
        if constexpr (MODE == GATHER_SH9) {
            const f3 d = gather_sphere_dir(gather_seed(seed, sbase + f));
            const float Y[9] = {0.282095f,
                                0.488603f * d.y,
                                0.488603f * d.z,
                                0.488603f * d.x,
                                1.092548f * (d.x * d.y),
                                1.092548f * (d.y * d.z),
                                0.315392f * fmaf(3.0f * d.z, d.z, -1.0f),
                                1.092548f * (d.x * d.z),
                                0.546274f * fmaf(d.x, d.x, -(d.y * d.y))};
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 9; ++k) a[9 * c + k] = fmaf(L[c], Y[k], a[9 * c + k]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] = a[c] + L[c];
        }
    }
    if (!any) return;
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = a[k];
}

// k_wf_accum for a view list: pixel pix of the list (its position in the concatenation of the views'
// windows) is window pixel (i, j) of its view and lives at acc + 3 * ((dst_y + j) * row_pitch + dst_x + i);
// acc += clamp(radiance) for the batch's F frames in order, k_wf_accum's accumulating statements (a sample
// that is not admitted left -0 in its radiance slot, which changes no bit).  A sibling of k_wf_accum, so
// that its instances' code stays as it is.
__global__ __launch_bounds__(256) void k_wf_accum_views(const float* __restrict__ rad, float* __restrict__ acc, ViewList vl,
                                                        uint32_t row_pitch, uint32_t F) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= vl.npix) return;
    const float4* rw = reinterpret_cast<const float4*>(view_of(vl, pix));
    const float4 ra = rw[0], rb = rw[1];
    const uint32_t k = pix - __float_as_uint(ra.x), w = __float_as_uint(ra.w);
    const uint32_t j = k / w, i = k - j * w;
    float* o = acc + 3 * ((size_t)(__float_as_uint(rb.z) + j) * row_pitch + (__float_as_uint(rb.y) + i));
    f3 a = mk(o[0], o[1], o[2]);
    for (uint32_t f = 0; f < F; ++f) {
        const float* r = rad + 3 * ((size_t)f * vl.npix + pix);
        a = add_clamped(a, mk(r[0], r[1], r[2]));
    }
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// A part's camera paths over the window's or a rectangle list's slot map (RL: nothing, or the list):
// k_wf_generate, or under a lens camera k_wf_generate_cam's instance of the model
template <bool COUNT, class... RL>
static void launch_generate_pixels(const PathSource& src, const FrameParams& fp, const WfPart& pt, uint32_t frame0,
                                   uint32_t stride, bool accum, Counters* cnt, const RL&... rl) {
    if (!src.cam) {
        const dim3 ggrid((std::max(pt.P, pt.w.nreg) + 255) / 256);  // a thread per region sets its count
        PT_LAUNCH(KID_WF_GENERATE, pt.st, (k_wf_generate<COUNT, RL...>), ggrid, dim3(256), 0, pt.st, fp, pt.w, frame0, stride,
                  pt.fbase, pt.P, !accum, cnt, rl...);
        return;
    }
    auto kern = k_wf_generate_cam<COUNT, CAM_EQUIRECT, RL...>;
    if (src.cam->model == CAM_THIN_LENS) kern = k_wf_generate_cam<COUNT, CAM_THIN_LENS, RL...>;
    else if (src.cam->model == CAM_ORTHO) kern = k_wf_generate_cam<COUNT, CAM_ORTHO, RL...>;
    PT_LAUNCH(KID_WF_GENERATE, pt.st, kern, dim3((pt.P + 255) / 256), dim3(256), 0, pt.st, fp, *src.cam, pt.w, frame0, stride,
              pt.fbase, pt.P, !accum, cnt, rl...);
}

// A part's first-vertex paths, by the source's kind (the table in pt_kernels.h)
template <bool COUNT>
static void launch_generate_t(const PathSource& src, const FrameParams& fp, const WfPart& pt, uint32_t frame0, uint32_t stride,
                              bool accum, Counters* cnt) {
    const dim3 qgrid((pt.P + 1023) / 1024);
    switch (src.kind) {
        case PathSource::WINDOW: launch_generate_pixels<COUNT>(src, fp, pt, frame0, stride, accum, cnt); break;
        case PathSource::RECTS: launch_generate_pixels<COUNT>(src, fp, pt, frame0, stride, accum, cnt, src.rects); break;
        case PathSource::RAYS:
            PT_LAUNCH(KID_WF_GENERATE, pt.st, (k_wf_generate_rays<COUNT>), qgrid, dim3(1024), 0, pt.st, pt.w, src.rays, frame0,
                      pt.fbase, pt.P, cnt);
            break;
        case PathSource::GATHER: {
            const auto kern = src.gather.mode == GATHER_SH9 ? k_wf_generate_gather<COUNT, GATHER_SH9>
                                                            : k_wf_generate_gather<COUNT, GATHER_COSINE>;
            PT_LAUNCH(KID_WF_GENERATE, pt.st, kern, qgrid, dim3(1024), 0, pt.st, pt.w, src.gather, frame0, pt.fbase, pt.P, cnt);
            break;
        }
        case PathSource::VIEWS:
            PT_LAUNCH(KID_WF_GENERATE, pt.st, (k_wf_generate_views<COUNT>), dim3((pt.P + 255) / 256), dim3(256), 0, pt.st,
                      src.views, pt.w, stride, pt.fbase, pt.P, cnt);
            break;
    }
}

void launch_generate(const PathSource& src, const WfCall& c, const WfPart& pt, bool count) {
    if (count) launch_generate_t<true>(src, c.fp, pt, c.frame0, c.stride, c.accum, c.cnt);
    else launch_generate_t<false>(src, c.fp, pt, c.frame0, c.stride, c.accum, c.cnt);
}

// A batch's radiance (Fb frames of npix paths; sbase: the call's sample index of the first) added to `out`,
// by the source's kind
void launch_accum(const PathSource& src, const FrameParams& fp, const float* rad, uint32_t npix, uint32_t sbase, uint32_t Fb,
                  bool accum, float* out, hipStream_t stream) {
    const dim3 grid((npix + 255) / 256), block(256);
    switch (src.kind) {
        case PathSource::WINDOW:
            PT_LAUNCH(KID_WF_ACCUM, stream, (k_wf_accum<>), grid, block, 0, stream, rad, out, npix, fp.win_w, fp.row_pitch, Fb,
                      accum, src.m2);
            break;
        case PathSource::RECTS:
            PT_LAUNCH(KID_WF_ACCUM, stream, (k_wf_accum<RectList>), grid, block, 0, stream, rad, out, npix, fp.win_w,
                      fp.row_pitch, Fb, accum, src.m2, src.rects);
            break;
        case PathSource::RAYS:
            PT_LAUNCH(KID_WF_ACCUM, stream, k_wf_accum_rays, grid, block, 0, stream, rad, out, src.rays, Fb);
            break;
        case PathSource::GATHER: {
            const auto kern = src.gather.mode == GATHER_SH9 ? k_wf_accum_gather<GATHER_SH9> : k_wf_accum_gather<GATHER_COSINE>;
            PT_LAUNCH(KID_WF_ACCUM, stream, kern, grid, block, 0, stream, rad, out, src.gather, sbase, Fb);
            break;
        }
        case PathSource::VIEWS:
            PT_LAUNCH(KID_WF_ACCUM, stream, k_wf_accum_views, grid, block, 0, stream, rad, out, src.views, fp.row_pitch, Fb);
            break;
    }
}

hipError_t launch_gather_rays(const GatherList& gl, uint32_t sample, void* rays, uint32_t* seeds, hipStream_t stream) {
    if (gl.n == 0 || gl.mode > GATHER_SH9) return hipErrorInvalidValue;
    const dim3 grid((gl.n + 255) / 256), block(256);
    if (gl.mode == GATHER_SH9)
        PT_LAUNCH(KID_GATHER_RAYS, stream, (k_gather_rays<GATHER_SH9>), grid, block, 0, stream, gl, sample,
                  static_cast<float4*>(rays), seeds);
    else
        PT_LAUNCH(KID_GATHER_RAYS, stream, (k_gather_rays<GATHER_COSINE>), grid, block, 0, stream, gl, sample,
                  static_cast<float4*>(rays), seeds);
    return hipGetLastError();
}

}  // namespace pt
