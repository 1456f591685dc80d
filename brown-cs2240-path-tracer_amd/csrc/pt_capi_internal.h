// pt_capi_internal.h — what the C ABI units (pt_capi*.hip) share: the error plumbing, the option snapshot,
// the scene and its self-freeing buffers, the blocking calls' scaffold, and the helpers the units call
// across.  Host code only, not part of the public boundary: no kernel unit includes it.
#pragma once
#include <array>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pt_hip.h"
#include "pt_kernels.h"
#include "pt_scene_layout.h"

namespace pt {

int fail(int code, const std::string& msg);  // sets the thread's pt_last_error (pt_capi.hip)
// a call is about to start the HIP runtime: pt_set_hw_queues comes too late from now on (pt_capi.hip)
void mark_hip_touched();

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return ::pt::fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
// the same for a call of this layer, which has set the error itself
#define PT_TRY(expr)                                          \
    do {                                                      \
        if (const int rc_ = (expr); rc_ != PT_OK) return rc_; \
    } while (0)

// Options (pt_capi.hip holds the table): a snapshot, taken once per call (a concurrent pt_set_option
// affects later calls only).
constexpr int kNumOpts = 40;
int opt_index(const char* name);
// the position of value among the '|'-separated choices of the enum option `name`, -1: none of them
int opt_choice(const char* name, const char* value);
struct Opts {
    std::string v[kNumOpts];
    const std::string& get(const char* name) const {
        static const std::string empty;
        const int i = opt_index(name);
        return i >= 0 ? v[i] : empty;
    }
    bool has(const char* name) const { return !get(name).empty(); }
    long num(const char* name, long def) const { return has(name) ? std::atol(get(name).c_str()) : def; }
    int flag(const char* name, int def) const { return has(name) ? (get(name) == "1" ? 1 : 0) : def; }
    bool is(const char* name, const char* val) const { return get(name) == val; }
};
Opts opts_snapshot();

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A device buffer that frees itself, kept with the scene and grown on demand (cap: T's).  counted
// (nullable): a byte counter that follows what the buffer holds (pt_scene_info::device_bytes).
template <class T>
struct Scratch {
    T* p = nullptr;
    size_t cap = 0;
    uint64_t* const counted;
    explicit Scratch(uint64_t* counter = nullptr) : counted(counter) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { free(); }
    // idle: a buffer a running render may use — the device idles before it is freed, and a failed
    // allocation is reported here, not by a later call
    int ensure(size_t n, const char* what, bool idle = false) {
        if (cap >= n) return PT_OK;
        if (p && idle) hipDeviceSynchronize();
        free();
        if (hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)) != hipSuccess) {
            p = nullptr;
            if (idle) (void)hipGetLastError();
            return fail(PT_ERR_NOMEM, std::string("hipMalloc ") + what);
        }
        cap = n;
        if (counted) *counted += cap * sizeof(T);
        return PT_OK;
    }
    int ensure_idle(size_t n, const char* what) { return ensure(n, what, true); }
    void free() {
        if (p) hipFree(p);
        if (counted) *counted -= cap * sizeof(T);
        p = nullptr;
        cap = 0;
    }
};

// Pinned host words that free themselves, made once and zeroed: the mirrors of the device control words
struct PinnedWords {
    uint32_t* p = nullptr;
    PinnedWords() = default;
    PinnedWords(const PinnedWords&) = delete;
    PinnedWords& operator=(const PinnedWords&) = delete;
    ~PinnedWords() { if (p) hipHostFree(p); }
    int ensure(size_t words, const char* what) {
        if (p) return PT_OK;
        if (hipHostMalloc(reinterpret_cast<void**>(&p), words * sizeof(uint32_t)) != hipSuccess) {
            p = nullptr;
            return fail(PT_ERR_NOMEM, std::string("hipHostMalloc ") + what);
        }
        std::memset(p, 0, words * sizeof(uint32_t));
        return PT_OK;
    }
};

}  // namespace pt

struct pt_history;

// Members free themselves (~pt_scene, with the device set by pt_scene_destroy, which also destroys the
// streams, the events and the profiler).
struct pt_scene {
    int device = 0;
    pt::Scratch<char> d_mem;  // the scene's sections (pt_scene_layout.h plan_sections) and its counters
    pt::SceneView view{};
    pt_scene_info info{};
    hipStream_t stream = nullptr;  // the blocking calls' own (pt::Blocking::open)
    pt::Scratch<float> d_accum;  // scratch for the blocking host-buffer calls
    pt::Counters* d_counters = nullptr;
    pt::Scratch<char> d_wf;  // wavefront path state, allocated on first use
    pt::WfBuffers wf{};
    bool prof_on = false;  // pt_profile_enable
    pt::KernelProfiler prof;
    pt::Scratch<uint8_t> d_rgba;  // pt_render_image scratch
    // scratch of the blocking moments, noise and adaptive calls: second moments, per-tile mean (floats),
    // tile verdicts followed by tile frame counts (bytes)
    pt::Scratch<float> d_m2, d_mean;
    pt::Scratch<char> d_tiles;
    // a rectangle-list render's table (pt_render_rects): the rows, then the megakernel's blocks; written
    // on the call's stream before its first launch, so calls in stream order may share it
    pt::Scratch<char> d_rects;
    // a view-list render's table (pt_render_views): its ViewRows, written like d_rects
    pt::Scratch<char> d_views;
    // the denoiser's four w * h float4 planes (pt_denoise_async: two ping-pong (c, var), (N, Z), (A, 0);
    // counted in info.device_bytes while held), and the scratch of its blocking calls: the guide buffers
    // (geo, then alb) and the filtered variance
    pt::Scratch<float4> d_dn{&info.device_bytes};
    pt::Scratch<float> d_feat, d_var;
    // ray queries (pt_query_*): the blocking calls' rays and results (counted in info.device_bytes while
    // held), the kernels' control words (kQueryCtlWords: a wave that gave up sets the first) and their
    // pinned mirror, copied after every query launch on its stream like h_ctl below
    pt::Scratch<char> d_query{&info.device_bytes};
    pt::Scratch<uint32_t> d_qctl;
    // pt_query_radiance: the blocking call's rays, seeds and accumulator (counted like d_query)
    pt::Scratch<char> d_radq{&info.device_bytes};
    pt::PinnedWords h_qctl;
    pt::WfStreams ws;  // dual-stream wavefront: aux stream + fork/join events (created with d_wf)
    // pinned mirror of the wavefront control words, copied after every wavefront render on its
    // stream: a watchdog flag set by an asynchronous render surfaces once that copy has landed
    // (next call, pt_scene_check) without a synchronisation of its own
    pt::PinnedWords h_ctl;
    pt::Scratch<float> d_rad;  // radiance of finished wavefront paths, three floats each (ensure_rad)
    pt::Scratch<float> d_peer;  // pt_render_multi (ordered reduction): another device's partial accumulator
    int32_t leaf_min = 0;  // leaf BVHs: leaves of at least this many entries have one (0: none)
    std::vector<std::array<int32_t, 3>> lleaves;  // (first record, entries, nodes) per leaf BVH
    // big leaves resolved before the traversal (k_wf_leafpass): the table (device copy in d_mem at
    // d_pre), every leaf's size (largest first), and the result keys (ensure_pres)
    std::vector<pt::PreLeaf> pre;
    // shape_view's choice of the leaf pass: per leaf of pre, probe queries passing its box filter and
    // visiting it (probe_pre_leaves, once, with the camera of the scene's first render that could
    // use the pass), from host copies of the tree, records and lights kept for it
    std::vector<std::array<uint32_t, 2>> pre_probe;
    bool pre_probed = false;
    pt::ProbeCamera pre_cam{};  // the camera pre_probe was taken with (a render with another probes again)
    std::mutex pre_mu;
    std::vector<pt::Node> h_nodes;
    std::vector<pt::Tri> h_tris;
    std::vector<pt::Light> h_lights;
    std::vector<int32_t> leaf_sizes;
    const pt::PreLeaf* d_pre = nullptr;
    pt::Scratch<uint64_t> d_pres;
    pt_camera cam{};  // pt_scene_set_camera, as given after validation (model 0: the pinhole)
    // pt_reproject's scratch (the blocking call's inputs, both sets of planes and outputs; counted in
    // info.device_bytes while held), and the scene's live histories (pt_history_create): pt_scene_destroy
    // frees their buffers and orphans them, so a later call on one is an error, not a fault
    pt::Scratch<float> d_temporal{&info.device_bytes};
    std::vector<pt_history*> histories;
    // a scene made by pt_scene_create_mesh: its packed tree inside d_mem (bytes from the base, floats)
    bool mesh_built = false;
    size_t packed_off = 0, packed_len = 0;
};

namespace pt {

struct ProfScope {  // attach the scene's profiler to this thread for the launches of its scope
    explicit ProfScope(pt_scene* s) { t_prof = s->prof_on ? &s->prof : nullptr; }
    ~ProfScope() { t_prof = nullptr; }
};

// pt_capi_render.hip
// meta -> FrameParams, checked.  win: the window of the image the call renders (NULL: the whole image);
// pitch: pixels between rows of its destination (NULL: the window's width)
int make_params(const float* meta, int max_depth, FrameParams& fp, const pt_window* win = nullptr,
                const size_t* pitch = nullptr);
// the frames frame0 + i * stride, i < nframes, all below 2^24
int check_frames(uint32_t frame0, uint32_t nframes, uint32_t stride);
int shape_view(pt_scene* s, const Opts& o, const FrameParams& fp, int mode, uint64_t paths, SceneView& view);
// an earlier asynchronous call's watchdog flag, once its mirror copy has landed: reported and cleared
int take_watchdog(pt_scene* s);
// the call's LaunchOpts: pt_flavour.h's defaults, the pipeline (AUTO by paths and scene), the options
LaunchOpts launch_opts(const Opts& o, int mode, uint64_t paths, const SceneView& view);
// the wavefront's buffers (s->wf) for a call of nframes frames of npix paths each: one batch's queues and
// radiance — the option wf_paths or the default target, at least two frames when the call has two, halved
// down to one frame's paths when the device is short of memory, then PT_ERR_NOMEM — and the view's leaf keys
int prepare_wavefront(pt_scene* s, const Opts& o, const SceneView& view, uint64_t npix, uint32_t nframes);
// One call's way through the wavefront pipeline, for every kind of PathSource:
//     WfCall c;
//     c.open(s, o, fp, mode, npix, nframes)   shape_view (the leaf pass chosen for fp's camera), launch_opts,
//                                             take_watchdog (an earlier asynchronous call failed)
//     what is the call's own: c.lo forced, its table uploaded
//     c.run(s, o, fp, src, ...)               prepare_wavefront, launch_wavefront, the control words' mirror copy
// npix paths per frame; nframes frames or samples (a single-frame call: 1).  run's fp may be another than
// open's (a view list launches with a reduced one).
struct WfCall {
    SceneView view;
    LaunchOpts lo;
    uint64_t npix = 0;
    uint32_t nframes = 0;
    int open(pt_scene* s, const Opts& o, const FrameParams& fp, int mode, uint64_t paths_per_frame, uint32_t frames);
    int run(pt_scene* s, const Opts& o, const FrameParams& fp, const PathSource& src, uint32_t frame0, uint32_t stride,
            bool accum, float* d_out, Counters* d_cnt, hipStream_t stream) const;
};
// A radiance query's or a gather's call (src: its n rays or points), samples sample0 .. sample0 + nsamples - 1
// added to d_accum.  The render's options, except: the pipeline is the wavefront's whatever `kernel` says
// (there is no megakernel for a list), and the leaf pass — chosen for a render by a probe from its camera —
// is off unless option leaf_pre asks for it (1; 2 means off here).  FrameParams: a 1-row "image" of n paths
// per sample with the call's rr_prob, direct_only and max_depth.
int query_call(pt_scene* s, const PathSource& src, size_t n, uint32_t sample0, uint32_t nsamples, float rr_prob,
               int32_t direct_only, int32_t max_depth, float* d_accum, Counters* d_cnt, hipStream_t stream);
int render_impl(pt_scene* s, const float* meta, uint32_t frame0, uint32_t nframes, uint32_t stride, int max_depth,
                int mode, bool accum, float* d_out, Counters* d_cnt, hipStream_t stream, const pt_window* win = nullptr,
                const size_t* pitch = nullptr, float* d_m2 = nullptr, const pt_window* rects = nullptr, size_t nrects = 0);
// pt_capi_denoise.hip
// the denoiser's parameters: the defaults, the caller's over them (p nullable), checked
int denoise_params(const pt_denoise_params* p, uint32_t feature_frames, pt_denoise_params& out);
// pt_render_features_async's body (pitch NULL: dense)
int features_impl(pt_scene* s, const float* meta, const pt_window* win, const size_t* pitch, uint32_t frame0,
                  uint32_t nframes, uint32_t stride, float* d_geo, float* d_alb, Counters* d_cnt, hipStream_t stream);
// the scene's four denoiser planes for npix pixels, and the a-trous passes over them once prepared
int denoise_planes(pt_scene* s, size_t npix, float4* cv[2], float4*& nz, float4*& ab);
int denoise_passes(const pt_denoise_params& prm, uint32_t w, uint32_t h, uint32_t row_pitch, float4* const cv[2],
                   const float4* nz, const float4* ab, float* d_out, float* d_var_out, hipStream_t stream);
// pt_capi_temporal.hip
// pt_scene_destroy: the scene's histories lose their buffers and their scene
void orphan_histories(pt_scene* s);
// pt_capi_camera.hip
// the scene's camera as a call's launches take it, read once per call: lc filled and returned for a lens
// model, nullptr for the pinhole (the call then launches the pinhole's own kernels)
const LensCam* scene_camera(const pt_scene* s, LensCam& lc);
// pt_capi_adaptive.hip
// the tile grid of the noise, mean and denoise calls, checked (host only)
int make_grid(uint32_t w, uint32_t h, size_t row_pitch, uint32_t tile_w, uint32_t tile_h, TileGrid& g);
// the tile scratch of the blocking calls: T verdicts, then T frame counts
int ensure_tiles(pt_scene* s, size_t T, pt_tile_noise*& d_noise, uint32_t*& d_frames);

inline void add_counters(pt_counters& sum, const pt_counters& c) {
    sum.samples += c.samples; sum.ext_queries += c.ext_queries; sum.shadow_queries += c.shadow_queries;
    sum.nodes += c.nodes; sum.tri_tests += c.tri_tests; sum.box_tests += c.box_tests;
}

// One blocking call of a scene, around the call's _async form on the scene's own stream:
//     Blocking b(s, counters);
//     device(), the scene's scratch, open(); in() / zero(); the _async call on s->stream with d_cnt();
//     out(); finish()
// counters (nullable): the caller's — the scene's device slot is zeroed by open() and copied back by finish().
struct Blocking {
    enum End { kNoWatchdog, kWatchdog };
    pt_scene* const s;
    pt_counters* const counters;
    explicit Blocking(pt_scene* scene, pt_counters* cnt = nullptr) : s(scene), counters(cnt) {}
    Counters* d_cnt() const { return counters ? s->d_counters : nullptr; }
    int device() { HIP_TRY(hipSetDevice(s->device)); return PT_OK; }
    // The blocking calls' own stream, created on first use: asynchronous callers never pay for a
    // stream (HIP multiplexes every stream of the process onto GPU_MAX_HW_QUEUES hardware queues,
    // and an idle extra stream can push the dual-stream wavefront's two onto one queue).
    int open() {
        if (!s->stream && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
            s->stream = nullptr;
            return fail(PT_ERR_HIP, "hipStreamCreate");
        }
        if (counters) HIP_TRY(hipMemsetAsync(s->d_counters, 0, sizeof(Counters), s->stream));
        return PT_OK;
    }
    // bytes in (host to device), zeroed, and out (device to host), in order on the stream
    int in(void* d, const void* h, size_t n) { HIP_TRY(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s->stream)); return PT_OK; }
    int zero(void* d, size_t n) { HIP_TRY(hipMemsetAsync(d, 0, n, s->stream)); return PT_OK; }
    int out(void* h, const void* d, size_t n) { HIP_TRY(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s->stream)); return PT_OK; }
    int sync(End end) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        return end == kWatchdog ? take_watchdog(s) : PT_OK;
    }
    // the counters back, the call's one synchronisation, the watchdog where the call takes it.  add: the
    // device counters are added to the caller's (after the watchdog) instead of overwriting them
    int finish(End end, bool add = false) {
        pt_counters got{};
        if (counters) PT_TRY(out(add ? &got : counters, s->d_counters, sizeof(Counters)));
        PT_TRY(sync(end));
        if (counters && add) add_counters(*counters, got);
        return PT_OK;
    }
};

}  // namespace pt
