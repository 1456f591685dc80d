// pt_path.h — one path of program-raymarch.wgsl:35-303 cut at its two traversal calls.
//
//   path_begin        main() seed chain + camera ray, radiance() prologue and first loop head
//   path_after_ext    after intersect(ray): miss / emission end the path; otherwise NEE
//                     samples a light and the path continues with its SHADOW ray
//   path_after_shadow after intersect(shadow ray): NEE contribution, direct-only exit,
//                     Russian roulette, BSDF; the path continues with its next EXTENSION ray
//
// Both the megakernel (k_regen) and the wavefront kernels call exactly these functions, so
// they execute the same f32 operations in the same order as the oracle's radiance().
#pragma once
#include "pt_device.h"

namespace pt {

struct PathState {
    f3 L, beta;
    f3 hp, hn, wi;  // shading point, its normal, incoming direction (live across the shadow trace)
    uint32_t seed;
    int depth;
    int mat_id;
    bool spec;
};

// NEE contribution once the shadow ray hit an emitter (program-raymarch.wgsl:154-182).
__device__ __forceinline__ f3 nee_contrib(const Mat& m, f3 wi, f3 hp, f3 hn, f3 ldir, f3 beta, const Hit& sh,
                                          const Mat& nm, float inv_ntri) {
    float att = pow2_lit(length(hp - sh.p));
    f3 brdf;
    if (m.Ns == 40.0f) {
        f3 refl = reflect(wi, hn);
        float q = dot(refl, ldir);
        if (q < 0.0f) {
            brdf = (m.Kd * (-q)) / kPI;
        } else {
            float sf = ((m.Ns + 2.0f) * pow_p(q, m.Ns)) / (2.0f * kPI);
            brdf = m.Ks * sf;
        }
    } else {
        brdf = m.Kd_pi;  // = m.Kd / kPI, bit for bit (precomputed per material)
    }
    float d1 = dot(sh.n, -ldir);
    float d2 = dot(hn, ldir);
    f3 c = (beta * nm.Ke) * brdf;
    c = c * d1;
    c = c * d2;
    c = c / att;
    return c * inv_ntri;
}

// BSDF continuation after Russian roulette survived (program-raymarch.wgsl:199-299):
// dielectric (illum 7), mirror (Ns > 500 or Fresnel reflection), Phong-glossy or Lambert.
// In: ray.d = incoming direction.  Out: ray = continuation ray; beta/spec/seed updated.
__device__ __forceinline__ void bsdf_continue(const Mat& m, f3 hp, f3 hn, Ray& ray, f3& beta, bool& spec,
                                              uint32_t& seed, int depth, float rr) {
    bool fresnel_reflect = false;
    if (m.illum == 7.0f) {
        f3 wi = ray.d;
        float cos_i = clampf(dot(wi, hn), -1.0f, 1.0f);
        f3 nn = hn;
        // eta_i, eta_t = 1, 2.5 (entering) or 2.5, 1; the quotients of these constants are folded
        // by the compiler with the same IEEE rounding: q = (eta_i - eta_t) / (eta_i + eta_t),
        // ratio = eta_i / eta_t
        constexpr float kQin = (1.0f - 2.5f) / (1.0f + 2.5f), kQout = (2.5f - 1.0f) / (2.5f + 1.0f);
        constexpr float kRatioIn = 1.0f / 2.5f, kRatioOut = 2.5f / 1.0f;
        const bool entering = cos_i < 0.0f;
        if (entering) {
            cos_i = -cos_i;
        } else {
            nn = -nn;
        }
        float q = entering ? kQin : kQout;
        float r0 = q * q;
        float r_theta = fmaf(1.0f - r0, pow5_lit(1.0f - cos_i), r0);
        seed = hash1u(seed + 7u);
        if (hash1(seed) < r_theta) {
            fresnel_reflect = true;
        } else {
            float ratio = entering ? kRatioIn : kRatioOut;
            float k = fmaf(-(ratio * ratio), fmaf(-cos_i, cos_i, 1.0f), 1.0f);
            float cf = fmaf(ratio, cos_i, -sqrtf(clampf(k, 0.0f, 1.0f)));
            f3 nd = mk(fmaf(cf, nn.x, ratio * wi.x), fmaf(cf, nn.y, ratio * wi.y), fmaf(cf, nn.z, ratio * wi.z));
            ray = ray_eps(hp, nd);
            spec = true;
            beta = beta * (1.0f / rr);
            return;
        }
    }
    if (m.Ns > 500.0f || fresnel_reflect) {
        ray = ray_eps(hp, reflect(ray.d, hn));
        spec = true;
        beta = beta * (1.0f / rr);
        return;
    }
    float pdf;
    f3 nd = sample_hemisphere(hn, seed, pdf);
    Ray nr = ray_eps(hp, nd);
    f3 brdf;
    if (sum3(m.Ks) > 0.0f) {
        f3 refl = reflect(ray.d, hn);
        float q = dot(refl, nr.d);
        if (q < 0.0f) {
            brdf = mk(0.0f, 0.0f, 0.0f);
        } else {
            float sf = m.phong * pow_p(q, m.Ns);  // m.phong = (m.Ns + 2) / (2 kPI)
            brdf = m.Ks * sf;
            if (depth == 0) spec = true;
        }
    } else {
        brdf = m.Kd_pi;  // = m.Kd / kPI, bit for bit (precomputed per material)
    }
    float cosn = dot(nr.d, hn) + 0.0f;  // vec4 dot: + w*w (= +0)
    f3 f = (brdf * cosn) / (pdf * rr);
    beta = beta * f;
    ray = nr;
}

// main() (program-raymarch.wgsl:50-77) + radiance() prologue and first loop head (:115-123)
__device__ __forceinline__ Ray path_begin(const FrameParams& fp, uint32_t x, uint32_t y, uint32_t t, PathState& ps) {
    uint32_t s0;
    Ray ray = camera_ray(fp, x, y, t, s0);
    ps.seed = hash1u(hash1u(hash1u(s0)));
    ps.L = mk(0.0f, 0.0f, 0.0f);
    ps.beta = mk(1.0f, 1.0f, 1.0f);
    ps.hp = ps.hn = ps.wi = mk(0.0f, 0.0f, 0.0f);
    ps.depth = 0;
    ps.mat_id = 0;
    ps.spec = false;
    return ray;
}

// The tail of path_begin for a ray the caller supplies (pt_query_radiance): radiance() entered with
// that ray and seed_in = s0 — the prologue's seed chain and the zeroed path state, the very statements
// of path_begin after camera_ray (which stays as it is: its instances' code does not change).
__device__ __forceinline__ void path_begin_ray(const Ray& ray, uint32_t s0, PathState& ps) {
    (void)ray;  // the first segment is the ray as given: nothing of the state depends on it
    ps.seed = hash1u(hash1u(hash1u(s0)));
    ps.L = mk(0.0f, 0.0f, 0.0f);
    ps.beta = mk(1.0f, 1.0f, 1.0f);
    ps.hp = ps.hn = ps.wi = mk(0.0f, 0.0f, 0.0f);
    ps.depth = 0;
    ps.mat_id = 0;
    ps.spec = false;
}

// A caller's direction is admitted when |d|^2, taken in f32 as fma(dz, dz, fma(dy, dy, dx * dx)), lies
// within 2^-18 of 1; a NaN fails the comparison.
__device__ __forceinline__ bool ray_admitted(float dx, float dy, float dz) {
    const float q = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    return fabsf(q - 1.0f) <= 0x1p-18f;
}

// path_begin under a lens camera (camera_ray_model): the model's ray, the admission test
// a caller's ray takes, and path_begin_ray's state.  false: the direction is not admitted (a lens point
// that coincides with its target gives NaN) — the sample has no path, and ps is not written.
template <uint32_t MODEL>
__device__ __forceinline__ bool path_begin_model(const FrameParams& fp, const LensCam& lc, uint32_t x, uint32_t y, uint32_t t,
                                                 Ray& ray, PathState& ps) {
    uint32_t s0;
    ray = camera_ray_model<MODEL>(fp, lc, x, y, t, s0);
    if (!ray_admitted(ray.d.x, ray.d.y, ray.d.z)) return false;
    path_begin_ray(ray, s0, ps);
    return true;
}

// Irradiance gathers (pt_gather).  A gather point is two float4: (p, seed bits) and
// (n, reserved).  Sample s of a point draws its direction with sd = gather_seed(seed, s) — the radiance
// queries' rule — and its path enters radiance() with seed_in = hash1u(sd + 7), the reference's idiom for
// "the next decision".
constexpr uint32_t GATHER_COSINE = 0, GATHER_SH9 = 1;

__device__ __forceinline__ uint32_t gather_seed(uint32_t seed, uint32_t s) { return s == 0 ? seed : hash1u(seed + s * 16787u); }

// SH9 mode's direction: uniform on the sphere from the sampler's own two numbers
__device__ __forceinline__ f3 gather_sphere_dir(uint32_t sd) {
    float xi1, xi2;
    hash2(sd * 7u + 11u, xi1, xi2);
    const float phi = (2.0f * kPI) * xi1;
    const float z = fmaf(-2.0f, xi2, 1.0f);
    const float r = sqrtf(fmaxf(fmaf(-z, z, 1.0f), 0.0f));
    float sn, cs;
    sincos_p(phi, sn, cs);
    return mk(r * cs, r * sn, z);
}

// The ray of a sample drawn with sd.  COSINE: the point is admitted iff nn = |n|^2 (fma chain) lies in
// [2^-80, 2^80] (a NaN fails); the ray is the reference's diffuse bounce from p about n / sqrt(nn) —
// sample_hemisphere and ray_with_epsilon.  SH9: gather_sphere_dir from p itself, the normal ignored.
// false: the point or the generated direction (ray_admitted) is not admitted, and `ray` is not written.
// ray.inv is not set: the queues do not store it.
template <uint32_t MODE>
__device__ __forceinline__ bool gather_ray(const float4& a, const float4& b, uint32_t sd, Ray& ray) {
    f3 d;
    if constexpr (MODE == GATHER_COSINE) {
        const float nn = fmaf(b.z, b.z, fmaf(b.y, b.y, b.x * b.x));
        if (!(nn >= 0x1p-80f && nn <= 0x1p80f)) return false;
        const float len = sqrtf(nn);
        float pdf;  // not used: the estimator's weight is the constant pi
        d = sample_hemisphere(mk(b.x / len, b.y / len, b.z / len), sd, pdf);
    } else {
        d = gather_sphere_dir(sd);
    }
    if (!ray_admitted(d.x, d.y, d.z)) return false;
    if constexpr (MODE == GATHER_COSINE) ray.o = mk(fmaf(0.001f, d.x, a.x), fmaf(0.001f, d.y, a.y), fmaf(0.001f, d.z, a.z));
    else ray.o = mk(a.x, a.y, a.z);
    ray.d = d;
    return true;
}

// :124-151 after the extension trace.  Returns true when the path continues; `ray` then
// holds the shadow ray and ps the shading point.
__device__ __forceinline__ bool path_after_ext(const SceneView& sc, int rec, float t, Ray& ray, PathState& ps) {
    if (rec < 0) return false;
    Hit h = hit_data(sc, ray, rec, t);
    Mat m = load_mat(sc, h.mat);
    if (sum3(m.Ke) > 0.0f && (ps.depth == 0 || ps.spec)) {
        ps.L = ps.L + ps.beta * m.Ke;
        return false;
    }
    f3 off = madd(h.p, h.n, 1.0e-4f);
    f3 ldir = sample_area_lights(sc, off, ps.seed);
    ps.seed = hash1u(ps.seed + 7u);
    ps.hp = h.p; ps.hn = h.n; ps.wi = ray.d; ps.mat_id = h.mat;
    ray.o = off; ray.d = ldir; ray.inv = rcp3(ldir);
    return true;
}

// :152-299 (+ loop test :118 and head :123) after the shadow trace.  Returns true when
// the path continues; `ray` then holds the next extension ray.
__device__ __forceinline__ bool path_after_shadow(const SceneView& sc, const FrameParams& fp, int rec, float t, Ray& ray,
                                                  PathState& ps) {
    const Mat m = load_mat(sc, ps.mat_id);
    if (rec >= 0) {
        Hit sh = hit_data(sc, ray, rec, t);
        Mat nm = load_mat(sc, sh.mat);
        if (sum3(nm.Ke) > 0.0f) ps.L = ps.L + nee_contrib(m, ps.wi, ps.hp, ps.hn, ray.d, ps.beta, sh, nm, sc.inv_ntri);
        if (fp.direct_only) return false;
    }
    if (hash1(ps.seed) > fp.rr_prob) return false;
    ray.d = ps.wi;
    bsdf_continue(m, ps.hp, ps.hn, ray, ps.beta, ps.spec, ps.seed, ps.depth, fp.rr_prob);
    ps.depth += 1;
    if (ps.depth > fp.max_depth) return false;
    ps.seed = hash1u(ps.seed);
    return true;
}

// program-raymarch.ts:283-285: sample_collector += (v >= 0 ? v : 0)
__device__ __forceinline__ f3 add_clamped(f3 acc, f3 L) {
    return mk(acc.x + (L.x >= 0.0f ? L.x : 0.0f), acc.y + (L.y >= 0.0f ? L.y : 0.0f), acc.z + (L.z >= 0.0f ? L.z : 0.0f));
}

// the second moments beside it: m2 + c * c of the same clamped c, the product rounded to f32 and then
// the sum (the library builds with -ffp-contract=off: no FMA here)
__device__ __forceinline__ f3 add_clamped_sq(f3 m2, f3 L) {
    const float x = L.x >= 0.0f ? L.x : 0.0f, y = L.y >= 0.0f ? L.y : 0.0f, z = L.z >= 0.0f ? L.z : 0.0f;
    return mk(m2.x + x * x, m2.y + y * y, m2.z + z * z);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void flush_counters(const Counters& c, Counters* out) {
    uint64_t v[6] = {c.samples, c.ext_queries, c.shadow_queries, c.nodes, c.tri_tests, c.box_tests};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        uint64_t s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(reinterpret_cast<unsigned long long*>(out) + i, (unsigned long long)s);
    }
}

// Copy the scene span into LDS at `base` (whole workgroup) and point `sc` at it.
__device__ __forceinline__ void stage_scene_lds(SceneView& sc, char* base) {
    const float4* src = reinterpret_cast<const float4*>(sc.nodes);
    float4* dst = reinterpret_cast<float4*>(base);
    for (uint32_t k = threadIdx.x; k < sc.span_bytes / 16u; k += blockDim.x) dst[k] = src[k];
    __syncthreads();
    sc.nodes = reinterpret_cast<const Node*>(base);
    sc.tris = reinterpret_cast<const Tri*>(base + sc.off_tris);
    sc.mats = reinterpret_cast<const Material*>(base + sc.off_mats);
    sc.lights = reinterpret_cast<const Light*>(base + sc.off_lights);
    sc.lmask = reinterpret_cast<const uint64_t*>(base + sc.off_lmask);
    if (sc.bfnarrow) sc.bfnarrow = reinterpret_cast<const BfNode*>(base + sc.off_bfnarrow);
    if (sc.bfnode) {
        sc.bfnode = reinterpret_cast<const BfNode*>(base + sc.off_bfnode);
        sc.bfmap = reinterpret_cast<const int32_t*>(base + sc.off_bfmap);
    }
}

}  // namespace pt
