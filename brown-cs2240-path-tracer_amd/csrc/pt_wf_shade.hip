// pt_wf_shade.hip — k_wf_shade: the path logic after a traversal (path_after_ext / path_after_shadow,
// pt_path.h) and the compaction of the surviving paths into the other queue, for the flavours whose
// trace kernel does not shade (every one but the fused).  Owns the kernel and launch_shade (pt_wf_stage.h).
#include "pt_wf_queue.h"
#include "pt_wf_stage.h"

namespace pt {

template <bool EXT, bool COUNT>
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade(SceneView sc, FrameParams fp, WfBuffers wb, Counters* cnt_out,
                                                          int bins) {
    // EXT: extension queue -> shadow queue; else shadow queue -> extension queue
    const uint32_t count = wb.ctl[EXT ? WF_COUNT0 : WF_COUNT1];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x * blockDim.x >= count) return;  // whole block past the queue
    const WfQueue& in = EXT ? wb.ext : wb.shd;
    const WfQueue& out = EXT ? wb.shd : wb.ext;
    uint32_t* out_count = &wb.ctl[EXT ? WF_COUNT1 : WF_COUNT0];
    Counters c = {};
    bool more = false;
    uint32_t p = 0;
    Ray r;
    PathState ps;
    if (i < count) {
        r = load_entry(in, i, p, ps);
        const int2 h = wb.hitq[i];
        const float t = __builtin_bit_cast(float, h.y);
        // a trace that gave up (watchdog, reported by the host) leaves stale records: never
        // let one index outside the triangle array
        const int rec = (uint32_t)h.x < (uint32_t)sc.n_tris ? h.x : -1;
        if (EXT) {
            more = path_after_ext(sc, rec, t, r, ps);
            if (more && COUNT) c.shadow_queries++;
        } else {
            load_shading_point(wb, i, ps);
            more = path_after_shadow(sc, fp, rec, t, r, ps);
            if (more && COUNT) c.ext_queries++;
        }
        if (!more) {
            float* o = wb.rad + 3 * (size_t)p;
            o[0] = ps.L.x; o[1] = ps.L.y; o[2] = ps.L.z;
        }
    }
    // compaction of the surviving paths: wave counts -> LDS prefix -> one atomicAdd per block
    __shared__ uint32_t s_cnt[kShadeBlock / 64];
    const uint64_t keep = __ballot(more);
    const uint32_t wv = threadIdx.x / 64;
    if (bins > 1) {  // block-uniform (kernel argument): the block's survivors grouped by a
        // coherence key (PT_SORT): the octant of the new direction (bins = 8), and with bins = 64
        // also the octant of the origin about the scene box's centre.  The block's output stays
        // one contiguous chunk (one atomicAdd), ordered key by key, so the traversal's 32-entry
        // windows hold similar rays.  Only the queue order changes (ranks within a key come from
        // LDS atomics, in any order): every path's result is the same.
        __shared__ uint32_t s_bin[512];
        for (uint32_t b = threadIdx.x; b < 512; b += blockDim.x) s_bin[b] = 0;
        uint32_t key = (r.d.x < 0.0f ? 1u : 0u) | (r.d.y < 0.0f ? 2u : 0u) | (r.d.z < 0.0f ? 4u : 0u);
        if (bins > 8) {  // the origin's cell: octant of the scene box (64 keys) or 4 x 4 x 4 cells (512)
            const Node& root = sc.nodes[0];
            const float lx = fminf(root.lmin[0], root.rmin[0]), hx = fmaxf(root.lmax[0], root.rmax[0]);
            const float ly = fminf(root.lmin[1], root.rmin[1]), hy = fmaxf(root.lmax[1], root.rmax[1]);
            const float lz = fminf(root.lmin[2], root.rmin[2]), hz = fmaxf(root.lmax[2], root.rmax[2]);
            const float q = bins > 64 ? 4.0f : 2.0f;
            auto cell = [&](float v, float lo, float hi) {
                const float c = (v - lo) / fmaxf(hi - lo, 1e-30f) * q;
                return (uint32_t)fminf(fmaxf(c, 0.0f), q - 1.0f);  // NaN -> 0
            };
            const uint32_t sh = bins > 64 ? 2u : 1u;
            key |= (cell(r.o.x, lx, hx) | (cell(r.o.y, ly, hy) << sh) | (cell(r.o.z, lz, hz) << (2 * sh))) << 3;
        }
        __syncthreads();
        const uint32_t rank = more ? atomicAdd(&s_bin[key], 1u) : 0u;
        __syncthreads();
        if (threadIdx.x < 64) {  // exclusive scan of the key counts, 8 per lane
            uint32_t c8[8], n = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { c8[i] = s_bin[8 * threadIdx.x + i]; n += c8[i]; }
            uint32_t incl = n;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t v = __shfl_up(incl, off, 64);
                if (lane_id() >= (uint32_t)off) incl += v;
            }
            const uint32_t total = __shfl(incl, 63, 64);
            uint32_t base = 0;
            if (threadIdx.x == 0 && total) base = atomicAdd(out_count, total);
            base = __shfl(base, 0, 64);
            uint32_t run = base + incl - n;
#pragma unroll
            for (int i = 0; i < 8; ++i) { s_bin[8 * threadIdx.x + i] = run; run += c8[i]; }
        }
        __syncthreads();
        if (more) {
            const uint32_t j = s_bin[key] + rank;
            store_entry(out, j, r, p, ps);
            if (EXT) store_shading_point(wb, j, ps);
        }
        if (COUNT) flush_counters(c, cnt_out);
        return;
    }
    if (lane_id() == 0) s_cnt[wv] = (uint32_t)__popcll(keep);
    __syncthreads();
    if (threadIdx.x < 64) {
        const uint32_t n = threadIdx.x < kShadeBlock / 64 ? s_cnt[threadIdx.x] : 0u;
        uint32_t incl = n;  // inclusive scan of the wave counts
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off, 64);
            if (lane_id() >= (uint32_t)off) incl += v;
        }
        const uint32_t total = __shfl(incl, 63, 64);
        uint32_t base = 0;
        if (threadIdx.x == 0 && total) base = atomicAdd(out_count, total);
        base = __shfl(base, 0, 64);
        if (threadIdx.x < kShadeBlock / 64) s_cnt[threadIdx.x] = base + incl - n;
    }
    __syncthreads();
    if (more) {
        const uint32_t j = s_cnt[wv] + rank_below(keep);
        store_entry(out, j, r, p, ps);
        if (EXT) store_shading_point(wb, j, ps);
    }
    if (COUNT) flush_counters(c, cnt_out);
}

void launch_shade(const SceneView& sc, const WfCall& c, const WfPart& pt, int it, bool count, int sort_bins) {
    const int sblocks = (int)((pt.P + kShadeBlock - 1) / kShadeBlock);
    auto kern = (it & 1) == 0 ? k_wf_shade<true, false> : k_wf_shade<false, false>;
    if (count) kern = (it & 1) == 0 ? k_wf_shade<true, true> : k_wf_shade<false, true>;
    PT_LAUNCH((it & 1) == 0 ? KID_WF_SHADE_EXT : KID_WF_SHADE_SHADOW, pt.st, kern, dim3(sblocks), dim3(kShadeBlock), 0, pt.st,
              sc, c.fp, pt.w, c.cnt, sort_bins);
}

}  // namespace pt
