/* Reference of pt_gather and pt_gather_rays (include/pt_hip.h) for the tests: the oracle's own
 * sample_hemisphere, radiance, po_hash2 and po_sincosf, looped over points and samples with the call's seed
 * rule, admission tests and accumulation.  Built by gather_ref.py into pytest's temporary directory; test
 * infrastructure only. */
#include "../oracle/pt_oracle.c"

enum { GR_COSINE = 0, GR_SH9 = 1 };

/* fmaf(dz, dz, fmaf(dy, dy, dx * dx)) within 2^-18 of 1; a NaN fails */
static int gr_admitted(v4 d) {
    float q = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x));
    return fabsf(q - 1.0f) <= 0x1p-18f;
}

static uint32_t gr_sd(uint32_t seed, uint32_t s) { return s == 0 ? seed : po_hash1u(seed + s * 16787u); }

/* the ray of a sample drawn with sd, whether its direction is admitted or not; 0: the point is not admitted
 * (COSINE: |n|^2 outside [2^-80, 2^80] or NaN) and *ray is not written.  pt: p[3], seed bits, n[3], reserved */
static int gr_draw(const float *pt, int mode, uint32_t sd, ray_t *ray) {
    v4 p = V4(pt[0], pt[1], pt[2], 1.0f);
    if (mode == GR_COSINE) {
        float nn = fmaf(pt[6], pt[6], fmaf(pt[5], pt[5], pt[4] * pt[4]));
        if (!(nn >= 0x1p-80f && nn <= 0x1p80f)) return 0;
        float len = sqrtf(nn), pdf;
        *ray = sample_hemisphere(p, V4(pt[4] / len, pt[5] / len, pt[6] / len, 0.0f), (int32_t)sd, &pdf);
        return 1;
    }
    float xi[2]; po_hash2(sd * 7u + 11u, xi);
    float phi = (2.0f * PI_F) * xi[0];
    float z = fmaf(-2.0f, xi[1], 1.0f);
    float r = sqrtf(fmaxf(fmaf(-z, z, 1.0f), 0.0f));
    float sn, cs; po_sincosf(phi, &sn, &cs);
    ray->p = p;
    ray->d = V4(r * cs, r * sn, z, 0.0f);
    ray->d_inv = inv4(ray->d);
    return 1;
}

EXPORT void gr_sh9_basis(const float *d, float *Y) {
    float x = d[0], y = d[1], z = d[2];
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = 1.092548f * (x * y);
    Y[5] = 1.092548f * (y * z);
    Y[6] = 0.315392f * fmaf(3.0f * z, z, -1.0f);
    Y[7] = 1.092548f * (x * z);
    Y[8] = 0.546274f * fmaf(x, x, -(y * y));
}

EXPORT void gr_set_vertex_normals(int on) { po_set_vertex_normals(on); }

/* the generated directions of sample `sample`, admitted or not (dirs: n x 3; NaN for a point that is not
 * admitted) — for the tests of the admission band */
EXPORT void gr_dirs(const float *pts, uint64_t n, int mode, uint32_t sample, float *dirs) {
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const float *pt = pts + 8 * i;
        ray_t ray;
        if (gr_draw(pt, mode, gr_sd(as_uint(pt[3]), sample), &ray)) {
            dirs[3 * i] = ray.d.x; dirs[3 * i + 1] = ray.d.y; dirs[3 * i + 2] = ray.d.z;
        } else {
            dirs[3 * i] = dirs[3 * i + 1] = dirs[3 * i + 2] = NAN;
        }
    }
}

/* pt_gather_rays: rays n x 8 (o, +inf, d, 0) and seeds; not admitted: d = 0, o = p, seed 0 */
EXPORT void gr_rays(const float *pts, uint64_t n, int mode, uint32_t sample, float *rays, uint32_t *seeds) {
    for (uint64_t i = 0; i < n; i++) {
        const float *pt = pts + 8 * i;
        float *r = rays + 8 * i;
        uint32_t sd = gr_sd(as_uint(pt[3]), sample);
        ray_t ray;
        int ok = gr_draw(pt, mode, sd, &ray) && gr_admitted(ray.d);
        r[3] = INFINITY; r[7] = 0.0f;
        if (ok) {
            r[0] = ray.p.x; r[1] = ray.p.y; r[2] = ray.p.z;
            r[4] = ray.d.x; r[5] = ray.d.y; r[6] = ray.d.z;
            seeds[i] = po_hash1u(sd + 7u);
        } else {
            r[0] = pt[0]; r[1] = pt[1]; r[2] = pt[2];
            r[4] = r[5] = r[6] = 0.0f;
            seeds[i] = 0;
        }
    }
}

/* pt_gather.  pts: n x 8 f32, accum: n x 3 (COSINE) or n x 27 (SH9) in/out.  admitted (nullable): n u32 out,
 * the admitted samples of each point.  cnt (nullable): added to.  miss_ends (nullable): += the paths that
 * ended because an extension ray hit nothing (told apart from an emitter's end as radiance_ref.c does). */
EXPORT void gr_gather(const float *tri, uint32_t tri_len, const float *bvh, uint32_t bvh_len, const float *pts, uint64_t n,
                      float rr_prob, int direct_only, int max_depth, uint32_t sample0, uint32_t nsamples, int mode,
                      float *accum, uint32_t *admitted, po_counters *cnt, uint64_t *miss_ends) {
    scene_t s = {tri, tri_len, bvh, bvh_len};
    po_counters total; memset(&total, 0, sizeof total);
    uint64_t misses = 0;
    const int W = mode == GR_SH9 ? 27 : 3;
#ifdef _OPENMP
#pragma omp parallel
#endif
    {
        po_counters loc; memset(&loc, 0, sizeof loc);
        uint64_t lmiss = 0;
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
        for (int64_t i = 0; i < (int64_t)n; i++) {
            const float *pt = pts + 8 * i;
            float *a = accum + (size_t)W * i;
            uint32_t nadm = 0;
            for (uint32_t k = 0; k < nsamples; k++) {
                uint32_t sd = gr_sd(as_uint(pt[3]), sample0 + k);
                ray_t ray;
                if (!gr_draw(pt, mode, sd, &ray) || !gr_admitted(ray.d)) continue;
                nadm++;
                int32_t seed = (int32_t)po_hash1u(sd + 7u);
                po_counters pc; memset(&pc, 0, sizeof pc);
                v3 L = radiance(&s, ray, seed, rr_prob, direct_only, max_depth, &pc);
                if (pc.ext_queries == pc.shadow_queries + 1) {
                    if (pc.ext_queries == 1) {
                        lmiss += (L.x == 0.0f && L.y == 0.0f && L.z == 0.0f);
                    } else {
                        v3 B = radiance(&s, ray, seed, rr_prob, direct_only, (int)pc.ext_queries - 2, NULL);
                        lmiss += (as_uint(B.x) == as_uint(L.x) && as_uint(B.y) == as_uint(L.y) && as_uint(B.z) == as_uint(L.z));
                    }
                }
                loc.samples++;
                loc.ext_queries += pc.ext_queries; loc.shadow_queries += pc.shadow_queries;
                loc.nodes += pc.nodes; loc.tri_tests += pc.tri_tests; loc.box_tests += pc.box_tests;
                float Lc[3] = {L.x >= 0.0f ? L.x : 0.0f, L.y >= 0.0f ? L.y : 0.0f, L.z >= 0.0f ? L.z : 0.0f};
                if (mode == GR_SH9) {
                    float d[3] = {ray.d.x, ray.d.y, ray.d.z}, Y[9];
                    gr_sh9_basis(d, Y);
                    for (int c = 0; c < 3; c++)
                        for (int j = 0; j < 9; j++) a[9 * c + j] = fmaf(Lc[c], Y[j], a[9 * c + j]);
                } else {
                    a[0] = a[0] + Lc[0]; a[1] = a[1] + Lc[1]; a[2] = a[2] + Lc[2];
                }
            }
            if (admitted) admitted[i] = nadm;
        }
#ifdef _OPENMP
#pragma omp critical
#endif
        {
            total.samples += loc.samples; total.ext_queries += loc.ext_queries; total.shadow_queries += loc.shadow_queries;
            total.nodes += loc.nodes; total.tri_tests += loc.tri_tests; total.box_tests += loc.box_tests;
            misses += lmiss;
        }
    }
    if (cnt) {
        cnt->samples += total.samples; cnt->ext_queries += total.ext_queries; cnt->shadow_queries += total.shadow_queries;
        cnt->nodes += total.nodes; cnt->tri_tests += total.tri_tests; cnt->box_tests += total.box_tests;
    }
    if (miss_ends) *miss_ends += misses;
}
