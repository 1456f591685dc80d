// pt_query_plan.h — the hand-out arithmetic of the ray-query kernels (pt_query.hip k_query; DESIGN.md
// §5.10): which window a wave fetches next, how long it is, how the wave's position in its current
// window moves and when the wave is done.  Everything here is wave-uniform integer arithmetic in
// __host__ __device__ inline functions and nothing else, so a host program can run the very code the
// kernel runs (scripts/query_plan_harness.cpp includes this file alone).
//
// The batch of n rays is cut into windows of kQueryWin consecutive rays; wave w of N takes the windows
// w, w + N, w + 2N, ... (static interleave: §5.4 measured an atomic hand-out slower).  A wave holds one
// window in LDS and the next one in registers.  At the top of every iteration of its loop the idle
// lanes (mask `need`) take the window's next rays in lane order — lane l takes position
// cur + (set bits of need below l) — and when the window is handed out the wave moves on to the
// prefetched one.  With refill off a wave hands rays out only when all 64 lanes are idle (a whole
// window at once: the scheme of the one-lane-per-pixel kernels).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_QP_HD __host__ __device__ inline
#else
#define PT_QP_HD inline
#endif

namespace pt {

constexpr uint32_t kQueryWin = 64;             // rays per window: one per lane
constexpr uint32_t kQueryNone = 0xffffffffu;   // no window
constexpr uint64_t kQueryMaxRays = 1ull << 30; // per call (ray indices and 2 * index stay below 2^32)
constexpr uint32_t kQueryLaunchRays = 1u << 22;  // per launch: the host cuts a call's batch (pt_query.hip launch_query_t)

// the wave's hand-out state (wave-uniform: SGPRs)
struct QueryWave {
    uint32_t nfetch;  // windows this wave has fetched
    uint32_t base;    // first ray of the current window
    uint32_t wv;      // its length
    uint32_t cur;     // positions [0, cur) of it are handed out
    uint32_t wnx;     // the prefetched window (kQueryNone: the wave has no further one)
    uint32_t nv;      // its length (0 when none)
};

PT_QP_HD uint32_t query_windows(uint32_t n) { return n / kQueryWin + (n % kQueryWin ? 1u : 0u); }

// the window of wave w's k-th fetch, or kQueryNone
PT_QP_HD uint32_t query_fetch(uint32_t k, uint32_t w, uint32_t nwaves, uint32_t nwin) {
    const uint64_t wid = (uint64_t)k * nwaves + w;
    return wid < nwin ? (uint32_t)wid : kQueryNone;
}

// rays of window wid of a batch of n (wid < query_windows(n)): 64, the last one what is left
PT_QP_HD uint32_t query_win_len(uint32_t wid, uint32_t n) {
    const uint32_t left = n - wid * kQueryWin;
    return left < kQueryWin ? left : kQueryWin;
}

// The wave's first two fetches: false when the wave has no window at all.  The caller loads window
// q.base / kQueryWin into LDS and window q.wnx (if any) into registers.
PT_QP_HD bool query_begin(QueryWave& q, uint32_t w, uint32_t nwaves, uint32_t n) {
    const uint32_t nwin = query_windows(n);
    q.nfetch = 0; q.base = 0; q.wv = 0; q.cur = 0; q.wnx = kQueryNone; q.nv = 0;
    const uint32_t w0 = query_fetch(q.nfetch++, w, nwaves, nwin);
    if (w0 == kQueryNone) return false;
    q.base = w0 * kQueryWin;
    q.wv = query_win_len(w0, n);
    q.wnx = query_fetch(q.nfetch++, w, nwaves, nwin);
    q.nv = q.wnx != kQueryNone ? query_win_len(q.wnx, n) : 0u;
    return true;
}

// lanes may take rays in this iteration: some lane is idle, and with refill off all of them are
PT_QP_HD bool query_hands_out(uint64_t need, bool refill) { return refill ? need != 0 : need == ~0ull; }

// the current window is handed out and a prefetched one waits: the wave moves on (the caller then
// stores the prefetched rays into LDS, calls query_advance and loads the new q.wnx into registers)
PT_QP_HD bool query_wants_next(const QueryWave& q) { return q.cur == q.wv && q.nv > 0; }
PT_QP_HD void query_advance(QueryWave& q, uint32_t w, uint32_t nwaves, uint32_t n) {
    q.base = q.wnx * kQueryWin;
    q.wv = q.nv;
    q.cur = 0;
    q.wnx = query_fetch(q.nfetch++, w, nwaves, query_windows(n));
    q.nv = q.wnx != kQueryNone ? query_win_len(q.wnx, n) : 0u;
}

// The idle lanes take positions cur, cur + 1, ... in lane order: the position of an idle lane with
// `rank` idle lanes below it, or kQueryNone when the window has no ray left for it.  Its ray is
// q.base + position and that is also its result's slot.
PT_QP_HD uint32_t query_position(const QueryWave& q, uint32_t rank) {
    const uint32_t k = q.cur + rank;
    return k < q.wv ? k : kQueryNone;
}
// ... and the wave's position after `idle` lanes asked
PT_QP_HD void query_took(QueryWave& q, uint32_t idle) {
    const uint32_t c = q.cur + idle;
    q.cur = c < q.wv ? c : q.wv;
}

// after the hand-out: no lane holds a ray, so none was left to take — every window of the wave is
// handed out and traced (an idle wave always hands out, with refill on or off)
PT_QP_HD bool query_done(const QueryWave& q, uint64_t busy) { return busy == 0 && q.cur == q.wv && q.nv == 0; }

}  // namespace pt
