/* Reference of pt_query_radiance (include/pt_hip.h) for the tests: the oracle's radiance(), looped over
 * rays and samples with the call's seed rule, admission test and clamp-accumulate.  Built by
 * radiance_ref.py into pytest's temporary directory; test infrastructure only. */
#include "../oracle/pt_oracle.c"

/* fmaf(dz, dz, fmaf(dy, dy, dx * dx)) within 2^-18 of 1; a NaN fails */
static int rr_admitted(const float *d) {
    float q = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
    return fabsf(q - 1.0f) <= 0x1p-18f;
}

EXPORT void rr_set_vertex_normals(int on) { po_set_vertex_normals(on); }

EXPORT uint32_t rr_hash1u(uint32_t v) { return po_hash1u(v); }

/* rays: n x 8 f32 (o, tmax, d, reserved), seeds: n, accum: n x 3 in/out.  admitted (nullable): n bytes out.
 * cnt (nullable): added to; samples += admitted rays * nsamples.  miss_ends (nullable): += the paths that
 * ended because an extension ray hit nothing.  Such a path has one extension query more than shadow
 * queries, as has one that ended on an emitter — told apart by running the path again without its last
 * extension query (max_depth = queries - 2 changes nothing before it): a miss leaves L as it was. */
EXPORT void rr_radiance(const float *tri, uint32_t tri_len, const float *bvh, uint32_t bvh_len, const float *rays,
                        const uint32_t *seeds, uint64_t n, float rr_prob, int direct_only, int max_depth,
                        uint32_t nsamples, float *accum, uint8_t *admitted, po_counters *cnt, uint64_t *miss_ends) {
    scene_t s = {tri, tri_len, bvh, bvh_len};
    po_counters total; memset(&total, 0, sizeof total);
    uint64_t misses = 0;
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
            const float *r = rays + 8 * i;
            int ok = rr_admitted(r + 4);
            if (admitted) admitted[i] = (uint8_t)ok;
            if (!ok) continue;
            ray_t ray;
            ray.p = V4(r[0], r[1], r[2], 1.0f);
            ray.d = V4(r[4], r[5], r[6], 0.0f);
            ray.d_inv = inv4(ray.d);
            float *a = accum + 3 * i;
            for (uint32_t k = 0; k < nsamples; k++) {
                uint32_t seed = k == 0 ? seeds[i] : po_hash1u(seeds[i] + k * 16787u);
                po_counters pc; memset(&pc, 0, sizeof pc);
                v3 L = radiance(&s, ray, (int32_t)seed, rr_prob, direct_only, max_depth, &pc);
                if (pc.ext_queries == pc.shadow_queries + 1) {
                    if (pc.ext_queries == 1) {
                        lmiss += (L.x == 0.0f && L.y == 0.0f && L.z == 0.0f);
                    } else {
                        v3 B = radiance(&s, ray, (int32_t)seed, rr_prob, direct_only, (int)pc.ext_queries - 2, NULL);
                        lmiss += (as_uint(B.x) == as_uint(L.x) && as_uint(B.y) == as_uint(L.y) && as_uint(B.z) == as_uint(L.z));
                    }
                }
                loc.samples++;
                loc.ext_queries += pc.ext_queries; loc.shadow_queries += pc.shadow_queries;
                loc.nodes += pc.nodes; loc.tri_tests += pc.tri_tests; loc.box_tests += pc.box_tests;
                a[0] = a[0] + (L.x >= 0.0f ? L.x : 0.0f);
                a[1] = a[1] + (L.y >= 0.0f ? L.y : 0.0f);
                a[2] = a[2] + (L.z >= 0.0f ? L.z : 0.0f);
            }
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
