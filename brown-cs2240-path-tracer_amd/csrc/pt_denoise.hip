// pt_denoise.hip — variance-guided edge-avoiding a-trous filter (pt_hip.h pt_denoise_async).
//
// The a-trous wavelet filter of Dammertz et al. 2010 with the guide weights (normal, albedo, depth)
// of the first hit and the variance-guided luminance weight of SVGF.  pt_hip.h specifies every
// operation; all of it is f32, rounded once, without FMAs (-ffp-contract=off), except the variance of
// the prepare step, which is double as in k_noise_tiles.
//
//   k_denoise_prepare   per pixel: mean colour and variance of the mean from the two accumulators and
//       the pixel's tile's frame count, the mean guides; packed into three float4 planes of w x h
//       pixels — (c.rgb, var), (N.xyz, Z), (A.rgb, 0) — so that a tap is three 16-byte loads.
//   k_atrous<STAGED>    one pass with step s: 25 taps at p + s * (dx, dy), 16 x 16 pixels per
//       workgroup (8 x 8 per wave).  STAGED = false loads the taps from global memory; true first
//       stages the block's (16 + 4 s)^2 region of the three planes in LDS.  Both read the same values
//       in the same order, so they give the same bits.
#include "pt_kernels.h"

#include <atomic>

namespace pt {

constexpr int kDnBlock = 256;
constexpr int kMaxDevices = 64;  // devices whose raised LDS limit launch_atrous remembers

// the lane's pixel: 8 x 8 per wave, 16 x 16 per workgroup (the megakernels' layout)
__device__ __forceinline__ void dn_pixel(uint32_t& i, uint32_t& j, uint32_t& li, uint32_t& lj) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    li = (wv & 1u) * 8u + (lane & 7u);
    lj = (wv >> 1) * 8u + (lane >> 3);
    i = blockIdx.x * 16u + li;
    j = blockIdx.y * 16u + lj;
}

__global__ __launch_bounds__(kDnBlock) void k_denoise_prepare(const float* __restrict__ acc, const float* __restrict__ m2,
                                                             const float4* __restrict__ geo, const float4* __restrict__ alb,
                                                             TileGrid g, const uint32_t* __restrict__ frames, float nf,
                                                             float4* __restrict__ cv, float4* __restrict__ nz,
                                                             float4* __restrict__ ab) {
    uint32_t i, j, li, lj;
    dn_pixel(i, j, li, lj);
    if (i >= g.w || j >= g.h) return;
    const uint32_t n = frames[(j / g.tile_h) * g.tx + i / g.tile_w];
    const size_t p = (size_t)j * g.row_pitch + i, o = 3 * p, q = (size_t)j * g.w + i;
    const float sr = acc[o], sg = acc[o + 1], sb = acc[o + 2];
    const float fn = (float)n;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (n) { c.x = sr / fn; c.y = sg / fn; c.z = sb / fn; }
    if (n >= 2) {
        const double dn = (double)n, dd = dn * (dn - 1.0);
        const double dsr = (double)sr, dsg = (double)sg, dsb = (double)sb;
        const double dr = (double)m2[o] - (dsr * dsr) / dn, dg = (double)m2[o + 1] - (dsg * dsg) / dn,
                     db = (double)m2[o + 2] - (dsb * dsb) / dn;
        const double vr = dr > 0.0 ? dr : 0.0, vg = dg > 0.0 ? dg : 0.0, vb = db > 0.0 ? db : 0.0;
        const double V = (vr + vg) + vb;
        c.w = (float)(V / dd);
    }
    const float4 ge = geo[p], al = alb[p];
    cv[q] = c;
    nz[q] = make_float4(ge.x / nf, ge.y / nf, ge.z / nf, ge.w / nf);
    ab[q] = make_float4(al.x / nf, al.y / nf, al.z / nf, 0.0f);
}

hipError_t launch_denoise_prepare(const float* acc, const float* m2, const float* geo, const float* alb, const TileGrid& g,
                                  const uint32_t* frames, uint32_t feature_frames, float4* cv, float4* nz, float4* ab,
                                  hipStream_t stream) {
    PT_LAUNCH(KID_DENOISE_PREPARE, stream, k_denoise_prepare, dim3((g.w + 15) / 16, (g.h + 15) / 16), dim3(kDnBlock), 0, stream,
              acc, m2, reinterpret_cast<const float4*>(geo), reinterpret_cast<const float4*>(alb), g, frames,
              (float)feature_frames, cv, nz, ab);
    return hipGetLastError();
}

// Staged region of a pass with step s: E = 16 + 4 s pixels a side; each plane's rows are pitch(E)
// 16-byte slots apart, the smallest pitch >= E that is 8 mod 16.  A ds_read_b128 is served in four
// groups of 16 lanes ({0-3, 12-15, 20-27}, ...: four pixels of each of four rows of the wave's 8 x 8
// tile, the column halves alternating as 0, 1, 1, 0 or 1, 0, 0, 1); with the pitch 8 mod 16 their
// slots are {0-3}, {12-15}, {4-7}, {8-11} (mod 16) and cover the 64 banks once: conflict-free.  A
// tap moves every lane's address by the same amount.
__host__ __device__ constexpr uint32_t atrous_extent(uint32_t s) { return 16u + 4u * s; }
__host__ __device__ constexpr uint32_t atrous_pitch(uint32_t s) { return ((atrous_extent(s) + 7u) / 16u) * 16u + 8u; }
constexpr size_t atrous_lds_bytes(uint32_t s) { return (size_t)3 * atrous_extent(s) * atrous_pitch(s) * sizeof(float4); }
static_assert(atrous_pitch(1) == 24 && atrous_pitch(2) == 24 && atrous_pitch(4) == 40 && atrous_pitch(8) == 56, "8 mod 16");
static_assert(atrous_lds_bytes(8) == 129024 && atrous_lds_bytes(8) <= 160 * 1024, "the largest staged pass fits the CU's LDS");

struct AtrousParams {
    uint32_t w, h, s;
    float isn, isa, isz, sigma_l;  // 1 / sigma_n^2, 1 / sigma_a^2, 1 / sigma_z (pt_hip.h), sigma_l
    uint32_t row_pitch;            // of out and var_out, pixels
};

// one tap (pt_hip.h: the order of the operations is the contract)
__device__ __forceinline__ void atrous_tap(const AtrousParams& P, float hw, const float4 cp, const float4 np, const float4 ap,
                                           float lp, float den, const float4 cq, const float4 nq, const float4 aq,
                                           float& sw, float& scr, float& scg, float& scb, float& sv) {
    const float dnx = np.x - nq.x, dny = np.y - nq.y, dnz = np.z - nq.z;
    const float tn = ((dnx * dnx + dny * dny) + dnz * dnz) * P.isn;
    const float dax = ap.x - aq.x, day = ap.y - aq.y, daz = ap.z - aq.z;
    const float ta = ((dax * dax + day * day) + daz * daz) * P.isa;
    const float zs = np.w + nq.w;
    const float tz = (fabsf(np.w - nq.w) / (zs > 1.0e-6f ? zs : 1.0e-6f)) * P.isz;
    const float lq = (cq.x + cq.y) + cq.z;
    const float tl = fabsf(lp - lq) / den;
    float e = (tn + ta) + (tz + tl);
    e = e < 126.0f ? e : 126.0f;
    const float wgt = hw * exp2_p(-e);
    sw += wgt;
    scr += wgt * cq.x;
    scg += wgt * cq.y;
    scb += wgt * cq.z;
    sv += (wgt * wgt) * cq.w;
}

// cv_out (nullable): the next pass's (c, var) plane; out / var_out (nullable): the call's results
// [h][w][3] and [h][w], rows row_pitch pixels apart (the last pass)
template <bool STAGED>
__global__ __launch_bounds__(kDnBlock) void k_atrous(const float4* __restrict__ cv, const float4* __restrict__ nz,
                                                    const float4* __restrict__ ab, AtrousParams P,
                                                    float4* __restrict__ cv_out, float* __restrict__ out,
                                                    float* __restrict__ var_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t i, j, li, lj;
    dn_pixel(i, j, li, lj);
    const int s = (int)P.s, w = (int)P.w, h = (int)P.h;
    const uint32_t E = atrous_extent(P.s), Rp = atrous_pitch(P.s);
    float4* const l_cv = reinterpret_cast<float4*>(smem);
    float4* const l_nz = l_cv + (size_t)E * Rp;
    float4* const l_ab = l_nz + (size_t)E * Rp;
    if (STAGED) {
        // the block's region, origin (16 bx - 2 s, 16 by - 2 s); pixels outside the image are never read
        const int rx0 = (int)(blockIdx.x * 16u) - 2 * s, ry0 = (int)(blockIdx.y * 16u) - 2 * s;
        for (uint32_t k = threadIdx.x; k < E * E; k += kDnBlock) {
            const uint32_t ry = k / E, rx = k - ry * E;
            const int gx = rx0 + (int)rx, gy = ry0 + (int)ry;
            if (gx < 0 || gy < 0 || gx >= w || gy >= h) continue;
            const size_t q = (size_t)gy * P.w + (size_t)gx;
            const uint32_t l = ry * Rp + rx;
            l_cv[l] = cv[q];
            l_nz[l] = nz[q];
            l_ab[l] = ab[q];
        }
        __syncthreads();
    }
    if (i >= P.w || j >= P.h) return;
    const size_t p = (size_t)j * P.w + i;
    const uint32_t lc = (lj + 2u * P.s) * Rp + (li + 2u * P.s);  // the pixel's slot in the staged region
    const float4 cp = STAGED ? l_cv[lc] : cv[p];
    const float4 np = STAGED ? l_nz[lc] : nz[p];
    const float4 ap = STAGED ? l_ab[lc] : ab[p];
    const float lp = (cp.x + cp.y) + cp.z;
    const float den = P.sigma_l * sqrtf(cp.w) + 1.0e-6f;
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sw = 0.0f, scr = 0.0f, scg = 0.0f, scb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)j + s * dy;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)i + s * dx;
            if (qx < 0 || qx >= w) continue;
            float4 cq, nq, aq;
            if (STAGED) {
                const uint32_t l = (uint32_t)((int)lc + (dy * (int)Rp + dx) * s);
                cq = l_cv[l]; nq = l_nz[l]; aq = l_ab[l];
            } else {
                const size_t q = (size_t)qy * P.w + (size_t)qx;
                cq = cv[q]; nq = nz[q]; aq = ab[q];
            }
            atrous_tap(P, hk[dy + 2] * hk[dx + 2], cp, np, ap, lp, den, cq, nq, aq, sw, scr, scg, scb, sv);
        }
    }
    const float4 r = make_float4(scr / sw, scg / sw, scb / sw, sv / (sw * sw));
    if (cv_out) cv_out[p] = r;
    if (out) {
        const size_t o = (size_t)j * P.row_pitch + i;
        out[3 * o] = r.x; out[3 * o + 1] = r.y; out[3 * o + 2] = r.z;
        if (var_out) var_out[o] = r.w;
    }
}

bool atrous_can_stage(uint32_t s) { return s <= 8; }

hipError_t launch_atrous(const float4* cv, const float4* nz, const float4* ab, uint32_t w, uint32_t h, uint32_t s, float isn,
                         float isa, float isz, float sigma_l, bool staged, float4* cv_out, float* out, float* var_out,
                         uint32_t row_pitch, hipStream_t stream) {
    const AtrousParams P{w, h, s, isn, isa, isz, sigma_l, row_pitch};
    const dim3 grid((w + 15) / 16, (h + 15) / 16), block(kDnBlock);
    if (staged) {
        if (!atrous_can_stage(s)) return hipErrorInvalidValue;
        const size_t lds = atrous_lds_bytes(s);
        if (lds > 48 * 1024) {  // near or above the default dynamic limit: raise it for this kernel (126 KiB, s = 8)
            // once per device of the process (the attribute belongs to the function on the current device)
            static std::atomic<bool> raised[kMaxDevices] = {};
            int dev = 0;
            hipError_t e = hipGetDevice(&dev);
            if (e != hipSuccess) return e;
            if (dev < 0 || dev >= kMaxDevices || !raised[dev].load(std::memory_order_acquire)) {
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_atrous<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)atrous_lds_bytes(8));
                if (e != hipSuccess) return e;
                if (dev >= 0 && dev < kMaxDevices) raised[dev].store(true, std::memory_order_release);
            }
        }
        PT_LAUNCH(KID_ATROUS, stream, (k_atrous<true>), grid, block, lds, stream, cv, nz, ab, P, cv_out, out, var_out);
    } else {
        PT_LAUNCH(KID_ATROUS, stream, (k_atrous<false>), grid, block, 0, stream, cv, nz, ab, P, cv_out, out, var_out);
    }
    return hipGetLastError();
}

}  // namespace pt
