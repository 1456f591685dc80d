// pt_wf_queue.h — the wavefront's queue entries as its kernels read and write them: the device helpers
// every stage shares (pt_wf_source.hip makes the first entries, pt_wf_trace.hip / pt_wf_bf.hip trace them,
// pt_wf_shade.hip / pt_wf_bf.hip shade and compact them).  WfQueue and WfBuffers are in pt_kernels.h; the
// pipeline is described in pt_wavefront.hip.  Owns: the lane helper (rank_below: pt_device.h), the words of
// an entry (pack_dspec, unpack_ray, q_at, ray_at, store_entry, load_entry), the shading point and the
// fused kernels' packed shadow entry, the window's slot -> pixel map (slot_path), and the phase
// statistics macros of the diagnostic builds (the trace statistics' are in pt_device.h).
#pragma once
#include <cstddef>
#include <type_traits>

#include "pt_kernels.h"
#include "pt_path.h"

namespace pt {

// Diagnostic build only (make EXTRA=-DPT_PHASE_STATS=1 OUT_DIR=...; scripts/phase_stats.py): the fused
// kernel's waves time their phases with s_memtime and count, per phase, loop iterations and the
// active lanes at each (the mean over iterations of popcount(exec) / 64 is the phase's lane use for a
// loop whose body issues the same instructions every iteration), summed over waves into
// g_phase_stats[EXT][phase][cycles, iterations, lanes] (pt_wf_bf.hip) at the end of each wave; read by
// pt_phase_stats_read.  Phases (PH_*): the batch's loads, phase 1 (the entries' tests; PH_P1FULL
// counts its iterations past the vote), the replay (PH_REPLAY: its node iterations; PH_RLEAF the
// leaf-hit iterations), the path logic, the append and stores.
#ifndef PT_PHASE_STATS
#define PT_PHASE_STATS 0
#endif
enum { PH_LOAD = 0, PH_P1, PH_P1FULL, PH_REPLAY, PH_RLEAF, PH_SHADE, PH_APPEND, PH_COUNT };
#if PT_PHASE_STATS
struct PhaseAcc {
    uint64_t v[PH_COUNT + 1][3];  // + a scratch row: the start of phase 1
};
__device__ __forceinline__ uint64_t ph_now() { return __builtin_amdgcn_s_memtime(); }
__device__ __forceinline__ void ph_iter(PhaseAcc& pa, int ph) {
    pa.v[ph][1] += 1;
    pa.v[ph][2] += (uint64_t)__builtin_popcountll(__builtin_amdgcn_read_exec());
}
#define PH_PARAM , PhaseAcc& pa
#define PH_PASS , pa
#define PH_ITER(ph) ph_iter(pa, ph)
#else
#define PH_PARAM
#define PH_PASS
#define PH_ITER(ph) ((void)0)
#endif

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t pack_dspec(const PathState& ps) {
    return (uint32_t)ps.depth | (ps.spec ? 0x10000u : 0u);
}
__device__ __forceinline__ void unpack_dspec(uint32_t dw, PathState& ps) {
    ps.depth = (int)(dw & 0xffffu);
    ps.spec = (dw & 0x10000u) != 0;
}
// FAST_INV (the fused kernel's FAST_RCP instances only): 1 / d from ray_inv (pt_math.h), the same bits
template <bool FAST_INV = false>
__device__ __forceinline__ Ray unpack_ray(float4 a, float4 b, uint32_t& p) {
    Ray r;
    r.o = mk(a.x, a.y, a.z);
    r.d = mk(a.w, b.x, b.y);
    r.inv = FAST_INV ? ray_inv(r.d) : rcp3(r.d);
    p = __builtin_bit_cast(uint32_t, b.z);
    return r;
}
// Element i of a queue array.  A32 (the fused kernel's 32-bit instances; pt_step_addr.h says when the
// host may launch them): the wave-uniform base stays in SGPRs and the lane adds a 32-bit BYTE offset
// (global_load/store v_off, s[base:base+1]), so no access costs 64-bit VALU; a neighbour element
// (q_at(..)[1]) rides in the instruction's immediate offset.  Otherwise base + (size_t)i as ever.
template <bool A32, class T>
__device__ __forceinline__ T* q_at(T* base, uint32_t i) {
    if constexpr (A32) return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + (uint32_t)(i * (uint32_t)sizeof(T)));
    else return base + (size_t)i;
}
// the two float4 of entry i of WfQueue::ray (the index doubles in 64 bits in the wide form)
template <bool A32>
__device__ __forceinline__ float4* ray_at(float4* ray, uint32_t i) {
    if constexpr (A32) return reinterpret_cast<float4*>(reinterpret_cast<char*>(ray) + (uint32_t)(i * 32u));
    else return ray + 2 * (size_t)i;
}
// queue entry i <- (ray, path index, path state)
template <bool A32 = false>
__device__ __forceinline__ void store_entry(const WfQueue& Q, uint32_t i, const Ray& r, uint32_t p, const PathState& ps) {
    float4* ray = ray_at<A32>(Q.ray, i);
    ray[0] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
    ray[1] = make_float4(r.d.y, r.d.z, __builtin_bit_cast(float, p), __builtin_bit_cast(float, pack_dspec(ps)));
    *q_at<A32>(Q.q2, i) = make_float4(ps.L.x, ps.L.y, ps.L.z, __builtin_bit_cast(float, ps.seed));
    *q_at<A32>(Q.q3, i) = make_float4(ps.beta.x, ps.beta.y, ps.beta.z, 0.0f);
}
__device__ __forceinline__ Ray load_entry(const WfQueue& Q, uint32_t i, uint32_t& p, PathState& ps) {
    const float4 a = Q.ray[2 * (size_t)i], b = Q.ray[2 * (size_t)i + 1], c = Q.q2[i], d = Q.q3[i];
    unpack_dspec(__builtin_bit_cast(uint32_t, b.w), ps);
    ps.L = mk(c.x, c.y, c.z);
    ps.seed = __builtin_bit_cast(uint32_t, c.w);
    ps.beta = mk(d.x, d.y, d.z);
    return unpack_ray(a, b, p);
}
__device__ __forceinline__ void store_shading_point(const WfBuffers& wb, uint32_t i, const PathState& ps) {
    wb.sp0[i] = make_float4(ps.hp.x, ps.hp.y, ps.hp.z, __builtin_bit_cast(float, ps.mat_id));
    wb.sp1[i] = make_float4(ps.hn.x, ps.hn.y, ps.hn.z, ps.wi.x);
    wb.sp2[i] = make_float2(ps.wi.y, ps.wi.z);
}
__device__ __forceinline__ void load_shading_point(const WfBuffers& wb, uint32_t i, PathState& ps) {
    const float4 a = wb.sp0[i], b = wb.sp1[i];
    const float2 c = wb.sp2[i];
    ps.hp = mk(a.x, a.y, a.z);
    ps.mat_id = __builtin_bit_cast(int, a.w);
    ps.hn = mk(b.x, b.y, b.z);
    ps.wi = mk(b.w, c.x, c.y);
}

// The fused kernels' shadow queue (bf_step_batch, its only writer and reader) holds 88 B per entry
// instead of the 104 B of a ray + path state + shading point: the shadow ray's origin is not
// stored — it is offset = madd(hp, hn, 1e-4), recomputed from the shading point with the very
// operation path_after_ext made it with (the same bits) — and the words are packed into the
// queue's arrays as
//   ray[2i]   = (d.xyz, path)      ray[2i+1] = (depth | spec, L.xyz)   q2 = (seed, beta.xyz)
//   q3        = (hp.xyz, material) sp0      = (hn.xyz, wi.x)          sp2 = (wi.y, wi.z)
// (sp1 unused).  The traversal pipeline (k_wf_trace + k_wf_shade) keeps the full layout above.
template <bool A32 = false>
__device__ __forceinline__ void store_shadow_packed(const WfBuffers& wb, uint32_t i, const Ray& r, uint32_t p,
                                                    const PathState& ps) {
    const WfQueue& Q = wb.shd;
    float4* ray = ray_at<A32>(Q.ray, i);
    ray[0] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_bit_cast(float, p));
    ray[1] = make_float4(__builtin_bit_cast(float, pack_dspec(ps)), ps.L.x, ps.L.y, ps.L.z);
    *q_at<A32>(Q.q2, i) = make_float4(__builtin_bit_cast(float, ps.seed), ps.beta.x, ps.beta.y, ps.beta.z);
    *q_at<A32>(Q.q3, i) = make_float4(ps.hp.x, ps.hp.y, ps.hp.z, __builtin_bit_cast(float, ps.mat_id));
    *q_at<A32>(wb.sp0, i) = make_float4(ps.hn.x, ps.hn.y, ps.hn.z, ps.wi.x);
    *q_at<A32>(wb.sp2, i) = make_float2(ps.wi.y, ps.wi.z);
}
// the ray of a packed shadow entry from its words (a = ray[2i], h = q3, n = sp0)
template <bool FAST_INV = false>
__device__ __forceinline__ Ray unpack_shadow_ray(float4 a, float4 h, float4 n, uint32_t& p) {
    Ray r;
    r.o = madd(mk(h.x, h.y, h.z), mk(n.x, n.y, n.z), 1.0e-4f);  // = path_after_ext's offset, bit for bit
    r.d = mk(a.x, a.y, a.z);
    r.inv = FAST_INV ? ray_inv(r.d) : rcp3(r.d);
    p = __builtin_bit_cast(uint32_t, a.w);
    return r;
}

// The camera path made for queue slot s (the s-th path of a batch part in generation order): its
// frame f, pixel (x, y) of the IMAGE and path id p = f * npix + j * win_w + i over the call's window
// (npix = win_w * win_h, (i, j) = (x - win_x0, y - win_y0)) — row-major within its frame's window,
// the radiance index k_wf_accum reads; slot = path id.  This and pixel_of (pt_kernels.hip) are the
// only places that tie a launch slot to a pixel.
__device__ __forceinline__ uint32_t slot_path(uint32_t s, const FrameParams& fp, uint32_t& x, uint32_t& y, uint32_t& f) {
    const uint32_t W = fp.win_w, npix = W * fp.win_h;
    f = s / npix;
    const uint32_t q = s - f * npix;
    const uint32_t j = q / W;
    y = j + fp.win_y0;
    x = q - j * W + fp.win_x0;
    return s;
}

}  // namespace pt
