// pt_temporal.hip — temporal accumulation: history reprojected across a camera move and blended with the
// current step (pt_hip.h pt_reproject_async), and the denoiser's prepare for a caller
// that already has the mean and its variance (pt_denoise_mean_async).
//
// The temporal stage of SVGF (Schied et al. 2017) for a static scene.  pt_hip.h specifies every
// operation; all of it is f32, rounded once, FMAs exactly where the header writes fmaf
// (-ffp-contract=off), with correctly rounded division and square root.
//
//   k_reproject   one pixel per lane, 8 x 8 per wave and 16 x 16 per workgroup (k_atrous' layout).  The
//       pixel's world point from the current camera's pixel-centre ray and the mean hit distance, its
//       place in the previous image, four bilinear taps of the previous (hist, mom, gbuf) planes — one
//       16-byte load per plane and tap — tested by depth and normal, the exponential blend, three
//       16-byte stores.  A pure gather: no atomics, no LDS, no dependence on the grid.
//       The taps are not staged in LDS: a tile's footprint in the previous image is the tile moved by a
//       per-lane, data-dependent amount (depth parallax), so a staged region would need a bound found by
//       a reduction first and a global-memory path for the lanes outside it, for a reuse of at most
//       four that the vector cache already serves — the four taps of a lane and those of its
//       neighbours in the wave fall on the same few 128-byte lines, three planes x (9 x 9) pixels x 16 B
//       per wave.  The kernel moves ~170 B per pixel and is bound by that traffic.
//   k_denoise_prepare_mean   k_denoise_prepare (pt_denoise.hip) with (c, var) given instead of derived:
//       the same three planes, the guides' lines the same statements.
#include "pt_kernels.h"

namespace pt {

constexpr int kTpBlock = 256;

// the lane's pixel: 8 x 8 per wave, 16 x 16 per workgroup (pt_denoise.hip dn_pixel)
__device__ __forceinline__ void tp_pixel(uint32_t& i, uint32_t& j) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    i = blockIdx.x * 16u + (wv & 1u) * 8u + (lane & 7u);
    j = blockIdx.y * 16u + (wv >> 1) * 8u + (lane >> 3);
}

// prev.* == nullptr: a first step (all three or none: the host checks)
__global__ __launch_bounds__(kTpBlock) void k_reproject(const float* __restrict__ acc, const float* __restrict__ m2,
                                                       const float4* __restrict__ geo, const float4* __restrict__ alb,
                                                       ReprojectParams P, const float4* __restrict__ hist_prev,
                                                       const float4* __restrict__ mom_prev, const float4* __restrict__ gbuf_prev,
                                                       float4* __restrict__ hist, float4* __restrict__ mom,
                                                       float4* __restrict__ gbuf, float* __restrict__ out,
                                                       float* __restrict__ var) {
    uint32_t x, y;
    tp_pixel(x, y);
    if (x >= P.w || y >= P.h) return;
    const size_t p = (size_t)y * P.row_pitch + x, o3 = 3 * p;
    // 1. the current step
    const float fn = (float)P.n;
    const float ckr = acc[o3] / fn, ckg = acc[o3 + 1] / fn, ckb = acc[o3 + 2] / fn;
    const float qkr = m2[o3] / fn, qkg = m2[o3 + 1] / fn, qkb = m2[o3 + 2] / fn;
    const float4 ge = geo[p];
    const float hits = alb[p].w;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, Z = 0.0f;
    if (hits > 0.0f) { nx = ge.x / hits; ny = ge.y / hits; nz = ge.z / hits; Z = ge.w / hits; }
    float cr = ckr, cg = ckg, cb = ckb, qr = qkr, qg = qkg, qb = qkb, N1 = 1.0f, a = 1.0f;
    if (hist_prev && Z > 0.0f) {
        // 2. the world point: camera_ray's chain (pt_device.h) with the jitter at the pixel's centre
        const float gx = (float)x, gy = (float)y;
        const float norm_x = fmaf(gx + 0.5f, P.inv_w, -0.5f);
        const float norm_y = fmaf(((P.H - 1.0f) - gy) + 0.5f, P.inv_h, -0.5f);
        const float vhw = P.view_half_h * P.aspect;
        const float vx = vhw * norm_x, vy = P.view_half_h * norm_y;
        const float* M = P.M;
        const float pz = -P.focal;
        const float px = fmaf(M[12], 1.0f, fmaf(M[8], pz, fmaf(M[4], vy, M[0] * vx)));
        const float py = fmaf(M[13], 1.0f, fmaf(M[9], pz, fmaf(M[5], vy, M[1] * vx)));
        const float pzw = fmaf(M[14], 1.0f, fmaf(M[10], pz, fmaf(M[6], vy, M[2] * vx)));
        const float pw = fmaf(M[15], 1.0f, fmaf(M[11], pz, fmaf(M[7], vy, M[3] * vx)));
        const float dx = px - P.cam[0], dy = py - P.cam[1], dz = pzw - P.cam[2], dw = pw - P.cam[3];
        const float len = sqrtf(fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx))));
        const float Px = fmaf(Z, dx / len, P.cam[0]), Py = fmaf(Z, dy / len, P.cam[1]), Pz = fmaf(Z, dz / len, P.cam[2]);
        // 3. the previous camera
        const float* V = P.pV;
        const float pcx = fmaf(V[12], 1.0f, fmaf(V[8], Pz, fmaf(V[4], Py, V[0] * Px)));
        const float pcy = fmaf(V[13], 1.0f, fmaf(V[9], Pz, fmaf(V[5], Py, V[1] * Px)));
        const float pcz = fmaf(V[14], 1.0f, fmaf(V[10], Pz, fmaf(V[6], Py, V[2] * Px)));
        const float zc = -pcz;
        const float pvx = (pcx * P.pfocal) / zc, pvy = (pcy * P.pfocal) / zc;
        const float pvhw = P.pview_half_h * P.paspect;
        const float u = ((pvx / pvhw) + 0.5f) * P.W - 0.5f;
        const float v = (P.H - 1.0f) - (((pvy / P.pview_half_h) + 0.5f) * P.H - 0.5f);
        const float ex = Px - P.pcam[0], ey = Py - P.pcam[1], ez = Pz - P.pcam[2];
        const float Ze = sqrtf(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
        // 5. in float, before any conversion: a huge or NaN coordinate never becomes an index
        if (zc > 0.0f && u > -1.0f && u < P.W && v > -1.0f && v < P.H) {
            // 4. the taps
            const float fu = floorf(u), fv = floorf(v);
            const float fx = u - fu, fy = v - fv;
            const float gx1 = 1.0f - fx, gy1 = 1.0f - fy;
            const int x0 = (int)fu, y0 = (int)fv;  // in [-1, w - 1] and [-1, h - 1]
            const float tol = P.depth_tol * Ze;
            float sw = 0.0f, scr = 0.0f, scg = 0.0f, scb = 0.0f, sqr = 0.0f, sqg = 0.0f, sqb = 0.0f, sn = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int qx = x0 + i, qy = y0 + j;
                    if (qx < 0 || qy < 0 || qx >= (int)P.w || qy >= (int)P.h) continue;
                    const size_t q = (size_t)qy * P.row_pitch + (size_t)qx;
                    const float4 hq = hist_prev[q], gq = gbuf_prev[q];
                    const float dt = (nx * gq.x + ny * gq.y) + nz * gq.z;
                    if (!(hq.w > 0.0f && gq.w > 0.0f && fabsf(gq.w - Ze) <= tol && dt >= P.normal_min)) continue;
                    const float4 mq = mom_prev[q];
                    const float wgt = (i ? fx : gx1) * (j ? fy : gy1);
                    sw += wgt;
                    scr += wgt * hq.x; scg += wgt * hq.y; scb += wgt * hq.z;
                    sqr += wgt * mq.x; sqg += wgt * mq.y; sqb += wgt * mq.z;
                    sn += wgt * hq.w;
                }
            }
            if (sw > 1.0e-6f) {
                // 6. the blend
                const float chr = scr / sw, chg = scg / sw, chb = scb / sw;
                const float qhr = sqr / sw, qhg = sqg / sw, qhb = sqb / sw;
                const float t = sn / sw + 1.0f;
                N1 = t < P.max_history ? t : P.max_history;
                const float r = 1.0f / N1;
                a = P.alpha > r ? P.alpha : r;
                cr = chr + a * (ckr - chr); cg = chg + a * (ckg - chg); cb = chb + a * (ckb - chb);
                qr = qhr + a * (qkr - qhr); qg = qhg + a * (qkg - qhg); qb = qhb + a * (qkb - qhb);
            }
        }
    }
    hist[p] = make_float4(cr, cg, cb, N1);
    mom[p] = make_float4(qr, qg, qb, 0.0f);
    gbuf[p] = make_float4(nx, ny, nz, Z);
    // 7. the optional outputs
    if (out) { out[o3] = cr; out[o3 + 1] = cg; out[o3 + 2] = cb; }
    if (var) {
        const float dr = qr - cr * cr, dg = qg - cg * cg, db = qb - cb * cb;
        const float vr = dr > 0.0f ? dr : 0.0f, vg = dg > 0.0f ? dg : 0.0f, vb = db > 0.0f ? db : 0.0f;
        const float vv = (((vr + vg) + vb) * a) / fn;
        var[p] = vv == vv ? vv : 0.0f;
    }
}

hipError_t launch_reproject(const float* acc, const float* m2, const float* geo, const float* alb, const ReprojectParams& P,
                            const float4* hist_prev, const float4* mom_prev, const float4* gbuf_prev, float4* hist,
                            float4* mom, float4* gbuf, float* out, float* var, hipStream_t stream) {
    PT_LAUNCH(KID_REPROJECT, stream, k_reproject, dim3((P.w + 15) / 16, (P.h + 15) / 16), dim3(kTpBlock), 0, stream, acc, m2,
              reinterpret_cast<const float4*>(geo), reinterpret_cast<const float4*>(alb), P, hist_prev, mom_prev, gbuf_prev,
              hist, mom, gbuf, out, var);
    return hipGetLastError();
}

// c [h][w][3], var [h][w], geo, alb [h][w][4], rows row_pitch pixels apart -> the denoiser's three dense planes
__global__ __launch_bounds__(kTpBlock) void k_denoise_prepare_mean(const float* __restrict__ c, const float* __restrict__ var,
                                                                  const float4* __restrict__ geo,
                                                                  const float4* __restrict__ alb, uint32_t w, uint32_t h,
                                                                  uint32_t row_pitch, float nf, float4* __restrict__ cv,
                                                                  float4* __restrict__ nz, float4* __restrict__ ab) {
    uint32_t i, j;
    tp_pixel(i, j);
    if (i >= w || j >= h) return;
    const size_t p = (size_t)j * row_pitch + i, o = 3 * p, q = (size_t)j * w + i;
    const float4 ge = geo[p], al = alb[p];
    cv[q] = make_float4(c[o], c[o + 1], c[o + 2], var[p]);
    nz[q] = make_float4(ge.x / nf, ge.y / nf, ge.z / nf, ge.w / nf);
    ab[q] = make_float4(al.x / nf, al.y / nf, al.z / nf, 0.0f);
}

hipError_t launch_denoise_prepare_mean(const float* c, const float* var, const float* geo, const float* alb, uint32_t w,
                                       uint32_t h, uint32_t row_pitch, uint32_t feature_frames, float4* cv, float4* nz,
                                       float4* ab, hipStream_t stream) {
    PT_LAUNCH(KID_DENOISE_PREPARE_MEAN, stream, k_denoise_prepare_mean, dim3((w + 15) / 16, (h + 15) / 16), dim3(kTpBlock), 0,
              stream, c, var, reinterpret_cast<const float4*>(geo), reinterpret_cast<const float4*>(alb), w, h, row_pitch,
              (float)feature_frames, cv, nz, ab);
    return hipGetLastError();
}

}  // namespace pt
