// pt_capi_selftest.hip — C ABI (include/pt_hip.h): the device selftests and the introspection calls the
// tests use.  Host code only.  A selftest's temporaries are Scratches holding what hipMalloc gave them, so
// every return frees them.
#include "pt_capi_internal.h"

using namespace pt;

extern "C" {

int pt_last_bf_width(void) { return pt::last_bf_width(); }
int pt_last_step_addr(void) { return pt::last_step_addr(); }

int pt_selftest_math(int device, int fn, const float* a, const float* b, float* out, size_t n) {
    if (!a || !b || !out || n == 0 || n > (1u << 28)) return fail(PT_ERR_INVALID, "bad argument");
    if (fn < 0 || fn >= PT_MATH_COUNT_) return fail(PT_ERR_INVALID, "unknown math fn");
    HIP_TRY(hipSetDevice(device));
    Scratch<float> da, db, dout;
    HIP_TRY(hipMalloc(&da.p, n * 4));
    HIP_TRY(hipMalloc(&db.p, n * 4));
    HIP_TRY(hipMalloc(&dout.p, n * 4));
    hipMemcpy(da.p, a, n * 4, hipMemcpyHostToDevice);
    hipMemcpy(db.p, b, n * 4, hipMemcpyHostToDevice);
    hipError_t e = launch_selftest_math(fn, da.p, db.p, dout.p, (int)n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_HIP, hipGetErrorString(e));
    return PT_OK;
}

int pt_selftest_valu(int device, int iters, int reps, int packed, double* ms_out, uint64_t* fma_wave_instr_out) {
    if (iters < 1 || reps < 1 || !ms_out) return fail(PT_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(device));
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const int blocks = cus * 8;  // 8 blocks of 4 waves per CU: 8 waves per SIMD
    Scratch<float> d;
    HIP_TRY(hipMalloc(&d.p, (size_t)blocks * 256 * sizeof(float)));
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = launch_selftest_valu(iters, blocks, packed, d.p, nullptr);  // warm-up (clock ramp)
    if (e == hipSuccess) e = hipEventRecord(a, nullptr);
    for (int r = 0; r < reps && e == hipSuccess; ++r) e = launch_selftest_valu(iters, blocks, packed, d.p, nullptr);
    if (e == hipSuccess) e = hipEventRecord(b, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
    if (e != hipSuccess) return fail(PT_ERR_HIP, hipGetErrorString(e));
    *ms_out = ms;
    // v_fma_f32 / v_pk_fma_f32 wave-instructions of the timed launches: 32 per iteration per wave
    if (fma_wave_instr_out) *fma_wave_instr_out = (uint64_t)reps * blocks * 4 * (uint64_t)iters * 32;
    return PT_OK;
}

int pt_scene_leaf_bvh(const pt_scene* s, int leaf, int32_t* first_record, int32_t* entries, int32_t* nodes) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    if (leaf < 0 || (size_t)leaf >= s->lleaves.size()) return fail(PT_ERR_INVALID, "no such leaf BVH");
    const auto& l = s->lleaves[(size_t)leaf];
    if (first_record) *first_record = l[0];
    if (entries) *entries = l[1];
    if (nodes) *nodes = l[2];
    return PT_OK;
}

int pt_selftest_leaf(pt_scene* s, int leaf, int mode, uint32_t seed, uint32_t nrays, int32_t* out) {
    if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
    if (mode < 0 || (mode > 7 && mode < 16) || mode > 31 || nrays == 0 || nrays > (1u << 24))
        return fail(PT_ERR_INVALID, "bad mode or ray count");
    const bool pass = mode >= 16;
    if (!pass && (leaf < 0 || (size_t)leaf >= s->lleaves.size())) return fail(PT_ERR_INVALID, "no such leaf BVH");
    if (pass && (leaf < 0 || (size_t)leaf >= s->pre.size())) return fail(PT_ERR_INVALID, "no such pre-resolvable leaf");
    if (pass && ((mode >> 2) & 3) >= 2 && (!s->view.pnodes || s->pre[(size_t)leaf].c1 <= s->pre[(size_t)leaf].c0))
        return fail(PT_ERR_INVALID, "the leaf has no pass chunks (option leaf_bvh)");
    HIP_TRY(hipSetDevice(s->device));
    Scratch<int32_t> d;
    HIP_TRY(hipMalloc(&d.p, (size_t)nrays * 6 * sizeof(int32_t)));
    hipError_t e;
    if (pass) {
        SceneView v = s->view;
        v.pre = s->d_pre;
        v.npre = (int32_t)s->pre.size();
        e = launch_selftest_leafpass(v, leaf, mode & 15, seed, nrays, d.p, nullptr);
    } else {
        const auto& l = s->lleaves[(size_t)leaf];
        e = launch_selftest_leaf(s->view, l[0], l[1], mode, seed, nrays, d.p, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(out, d.p, (size_t)nrays * 6 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_HIP, hipGetErrorString(e));
    return PT_OK;
}

int pt_selftest_lights(pt_scene* s, const uint32_t* seeds, const float* points, size_t n, float* out) {
    if (!s || !seeds || !points || !out) return fail(PT_ERR_INVALID, "null argument");
    if (n == 0 || n > (1u << 24)) return fail(PT_ERR_INVALID, "bad sample count");
    HIP_TRY(hipSetDevice(s->device));
    Scratch<uint32_t> dseeds;
    Scratch<float> dpts, dout;
    hipError_t e = hipMalloc(&dseeds.p, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&dpts.p, n * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dout.p, n * 4 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dseeds.p, seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dpts.p, points, n * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_selftest_lights(s->view, dseeds.p, dpts.p, (uint32_t)n, dout.p, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, n * 4 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_HIP, hipGetErrorString(e));
    return PT_OK;
}

int pt_selftest_view_half_h(const float* metas, size_t n, float* out) {
    if (!metas || !out) return fail(PT_ERR_INVALID, "null argument");
    for (size_t i = 0; i < n; ++i) {
        FrameParams fp;
        if (int rc = make_params(metas + 48 * i, 0, fp); rc != PT_OK) return rc;
        out[i] = fp.view_half_h;
    }
    return PT_OK;
}

int pt_selftest_rcp(int device, int steps, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches,
                    uint32_t* failing_bits) {
    if (!mismatches || steps < -1 || steps > 2 || lo_bits > hi_bits || hi_bits >= 0x80000000u)
        return fail(PT_ERR_INVALID, "bad argument");
    if (steps < 0) steps = kRcpSteps;
    HIP_TRY(hipSetDevice(device));
    Scratch<unsigned long long> d;
    HIP_TRY(hipMalloc(&d.p, 2 * sizeof(unsigned long long)));
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMemset(d.p, 0, sizeof(h));
    if (e == hipSuccess) e = launch_selftest_rcp(steps, lo_bits, hi_bits, d.p, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_HIP, hipGetErrorString(e));
    *mismatches = h[0];
    if (failing_bits) *failing_bits = (uint32_t)h[1];
    return PT_OK;
}

}  // extern "C"
