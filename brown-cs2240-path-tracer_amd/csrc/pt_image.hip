// pt_image.hip — on-device display transform.
//
// program-raymarch.ts:295-316 on the accumulator, per pixel, in double like the JS it
// replaces: raw = acc / sample_runs, lum = (r + g + b) / 3, out = raw * (lum / (lum + 1))^0.01,
// u8 = clamp(ToInt32(out * 255)), alpha 255.  The same function as the host pt_tonemap
// (pt_capi.hip); the GPU test checks the two byte for byte.
#include "pt_kernels.h"

#include <algorithm>

namespace pt {

__device__ __forceinline__ int32_t to_int32(double v) {  // ECMAScript ToInt32
    if (!isfinite(v)) return 0;
    double m = fmod(trunc(v), 4294967296.0);
    if (m < 0) m += 4294967296.0;
    return (int32_t)(uint32_t)m;
}
__device__ __forceinline__ uint8_t clamp_u8(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : (uint8_t)v); }

__global__ __launch_bounds__(256) void k_tonemap(const float* __restrict__ acc, size_t npix, uint32_t runs,
                                                uchar4* __restrict__ rgba) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double r = (double)acc[3 * i] / runs, g = (double)acc[3 * i + 1] / runs, b = (double)acc[3 * i + 2] / runs;
    const double lum = (r + g + b) / 3.0;
    const double f = pow(lum / (lum + 1.0), 0.01);
    rgba[i] = make_uchar4(clamp_u8(to_int32(r * f * 255.0)), clamp_u8(to_int32(g * f * 255.0)),
                          clamp_u8(to_int32(b * f * 255.0)), 255);
}

hipError_t launch_tonemap(const float* acc, size_t npix, uint32_t runs, uint8_t* rgba, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    PT_LAUNCH(KID_TONEMAP, stream, k_tonemap, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, acc, npix,
              runs, reinterpret_cast<uchar4*>(rgba));
    return hipGetLastError();
}

// Per-tile noise verdict from the first and second moments (pt_hip.h pt_noise_tiles_async, DESIGN.md
// §5.8).  One workgroup per tile, its threads striding over the tile's pixels; per pixel, in double
// and every operation rounded once (-ffp-contract=off), with S, Q the pixel's acc and m2 and n the
// tile's frames:
//   v_c = max(Q_c - S_c^2 / n, 0) (NaN -> 0), V = (v_r + v_g) + v_b, se = sqrt(V / (n (n - 1))),
//   mu = ((S_r + S_g) + S_b) / n, err = se / max(mu, floor); noisy iff err > tol.
// The tile's count of noisy pixels and the maximum of err (from 0; a NaN never replaces it) do not
// depend on the order of the reduction: wave shuffles, then LDS across the waves, then one store.
constexpr int kNoiseBlock = 256;
__global__ __launch_bounds__(kNoiseBlock) void k_noise_tiles(const float* __restrict__ acc, const float* __restrict__ m2,
                                                            TileGrid g, const uint32_t* __restrict__ frames, double tol,
                                                            double floor, TileNoise* __restrict__ out) {
    __shared__ uint32_t s_cnt[kNoiseBlock / 64];
    __shared__ double s_max[kNoiseBlock / 64];
    const uint32_t t = blockIdx.x, tx = t % g.tx, ty = t / g.tx;
    const uint32_t x0 = tx * g.tile_w, y0 = ty * g.tile_h;
    const uint32_t tw = min(g.tile_w, g.w - x0), th = min(g.tile_h, g.h - y0), npx = tw * th;
    const uint32_t n = frames[t];
    if (n < 2) {  // no variance estimate yet: every pixel counts as noisy
        if (threadIdx.x == 0) out[t] = TileNoise{npx, npx, (double)__builtin_inff()};
        return;
    }
    const double dn = (double)n, dd = dn * (dn - 1.0);
    uint32_t cnt = 0;
    double m = 0.0;
    for (uint32_t k = threadIdx.x; k < npx; k += kNoiseBlock) {
        const uint32_t j = k / tw, i = k - j * tw;
        const size_t o = 3 * ((size_t)(y0 + j) * g.row_pitch + (x0 + i));
        const double sr = (double)acc[o], sg = (double)acc[o + 1], sb = (double)acc[o + 2];
        const double dr = (double)m2[o] - (sr * sr) / dn, dg = (double)m2[o + 1] - (sg * sg) / dn,
                     db = (double)m2[o + 2] - (sb * sb) / dn;
        const double vr = dr > 0.0 ? dr : 0.0, vg = dg > 0.0 ? dg : 0.0, vb = db > 0.0 ? db : 0.0;
        const double V = (vr + vg) + vb;
        const double se = sqrt(V / dd);
        const double mu = ((sr + sg) + sb) / dn;
        const double den = mu > floor ? mu : floor;
        const double err = se / den;
        if (err > tol) ++cnt;
        m = err > m ? err : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        const double o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (lane == 0) { s_cnt[wv] = cnt; s_max[wv] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kNoiseBlock / 64; ++k) {
            cnt += s_cnt[k];
            m = s_max[k] > m ? s_max[k] : m;
        }
        out[t] = TileNoise{cnt, npx, m};
    }
}

hipError_t launch_noise_tiles(const float* acc, const float* m2, const TileGrid& g, const uint32_t* frames, double tol,
                              double floor, TileNoise* out, hipStream_t stream) {
    PT_LAUNCH(KID_NOISE_TILES, stream, k_noise_tiles, dim3(g.tx * g.ty), dim3(kNoiseBlock), 0, stream, acc, m2, g, frames,
              tol, floor, out);
    return hipGetLastError();
}

// mean = acc / (float)frames of the pixel's tile, one f32 division (0 where the tile has no frames);
// mean is laid out like acc
__global__ __launch_bounds__(256) void k_tile_mean(const float* __restrict__ acc, TileGrid g,
                                                  const uint32_t* __restrict__ frames, float* __restrict__ mean) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= g.w * g.h) return;
    const uint32_t j = pix / g.w, i = pix - j * g.w;
    const uint32_t n = frames[(j / g.tile_h) * g.tx + i / g.tile_w];
    const size_t o = 3 * ((size_t)j * g.row_pitch + i);
    const float d = (float)n;
    mean[o] = n ? acc[o] / d : 0.0f;
    mean[o + 1] = n ? acc[o + 1] / d : 0.0f;
    mean[o + 2] = n ? acc[o + 2] / d : 0.0f;
}

hipError_t launch_tile_mean(const float* acc, const TileGrid& g, const uint32_t* frames, float* mean, hipStream_t stream) {
    PT_LAUNCH(KID_TILE_MEAN, stream, k_tile_mean, dim3((g.w * g.h + 255) / 256), dim3(256), 0, stream, acc, g, frames, mean);
    return hipGetLastError();
}

// The accumulator to pinned host memory (pt_readback_async): a copy by a few blocks, each thread
// storing 16-B words straight over PCIe.  The runtime's own copy of a 12 MB accumulator is a blit
// kernel of 512 blocks that holds its CU slots for the whole PCIe transfer (0.2-1.2 ms in a kernel
// trace of the bench, r06m), beside the next step's render; PCIe is the bound either way.
constexpr int kReadbackBlocks = 16;
__global__ __launch_bounds__(256) void k_readback(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4,
                                                  const float* __restrict__ src_tail, float* __restrict__ dst_tail,
                                                  uint32_t ntail) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += step) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < ntail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}
hipError_t launch_readback(const float* d_src, float* h_dst_dev, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t n4 = n / 4;
    const uint32_t ntail = (uint32_t)(n - 4 * n4);
    hipLaunchKernelGGL(k_readback, dim3(kReadbackBlocks), dim3(256), 0, stream, reinterpret_cast<const float4*>(d_src),
                       reinterpret_cast<float4*>(h_dst_dev), n4, d_src + 4 * n4, h_dst_dev + 4 * n4, ntail);
    return hipGetLastError();
}

// dst += src, f32, element-wise (the ordered multi-device reduction of pt_render_multi: partial
// accumulators added onto device 0's in device order)
__global__ __launch_bounds__(256) void k_accum_add(float4* __restrict__ dst, const float4* __restrict__ src, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = dst[i];
        const float4 b = src[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        dst[i] = a;
    }
}
__global__ void k_accum_add_tail(float* __restrict__ dst, const float* __restrict__ src, size_t from, size_t n) {
    const size_t i = from + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

hipError_t launch_accum_add(float* dst, const float* src, size_t n, hipStream_t stream) {
    const size_t n4 = n / 4;
    if (n4) {
        const unsigned blocks = (unsigned)std::min<size_t>((n4 + 255) / 256, 8192);
        hipLaunchKernelGGL(k_accum_add, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<float4*>(dst),
                           reinterpret_cast<const float4*>(src), n4);
    }
    if (n % 4) hipLaunchKernelGGL(k_accum_add_tail, dim3(1), dim3(4), 0, stream, dst, src, n4 * 4, n);
    return hipGetLastError();
}

}  // namespace pt
