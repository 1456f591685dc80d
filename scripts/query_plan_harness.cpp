// query_plan_harness.cpp — the hand-out of the ray-query kernels (csrc/pt_query_plan.h, included alone)
// run on the host, one modelled wave after the other, exactly as k_query's loop drives it:
//
//   query_plan_harness <n> <waves> <refill 0|1> <seed>
//
// Every wave keeps 64 lanes.  Per iteration the idle lanes take rays as the kernel hands them out
// (ballot, rank, query_position / query_took, query_wants_next / query_advance), then a seeded random,
// non-empty subset of the busy lanes finishes and each writes its ray's result slot.  Checked: every
// ray index is handed out exactly once and its slot written exactly once, a lane never takes a ray
// while busy, with refill off rays are handed out only to a wholly idle wave, the prefetched window is
// the one the plan names, no index is >= n, and every wave's loop ends within n + windows + 2
// iterations.  Prints "ok n=<n> waves=<w> refill=<r> windows=<k> max_iters=<i>" or a line starting
// with "FAIL".  Meant to be built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_query_plan.h"

using namespace pt;

namespace {

uint64_t g_state;
uint32_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

uint32_t rank_below(uint64_t m, int lane) { return (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1)); }

int fail(const char* what, uint32_t w, uint64_t a = 0, uint64_t b = 0) {
    std::printf("FAIL %s (wave %u: %llu, %llu)\n", what, w, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: query_plan_harness <n> <waves> <refill 0|1> <seed>\n");
        return 2;
    }
    const unsigned long long n64 = std::strtoull(argv[1], nullptr, 10);
    const uint32_t nwaves = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const bool refill = std::atoi(argv[3]) != 0;
    g_state = std::strtoull(argv[4], nullptr, 10);
    if (n64 > kQueryMaxRays || nwaves == 0) return 2;
    const uint32_t n = (uint32_t)n64;
    const uint32_t nwin = query_windows(n);
    if ((uint64_t)nwin * kQueryWin < n || (nwin > 0 && (uint64_t)(nwin - 1) * kQueryWin >= n)) return fail("query_windows", 0, nwin, n);
    std::vector<uint8_t> handed(n, 0), written(n, 0);  // exact sizes: an index >= n is the sanitizer's
    std::vector<uint32_t> win_owner(nwin, kQueryNone);
    const uint64_t bound = (uint64_t)n + nwin + 2;
    uint64_t max_iters = 0;
    for (uint32_t w = 0; w < nwaves; ++w) {
        QueryWave q;
        if (!query_begin(q, w, nwaves, n)) {
            if (w < nwin) return fail("a wave with a window got none", w);
            continue;
        }
        if (w >= nwin) return fail("a wave beyond the windows got one", w);
        uint32_t nfetched = 0;
        auto claim = [&](uint32_t wid) {  // the k-th window a wave claims is k * nwaves + w
            if (wid == kQueryNone) return true;
            if (wid >= nwin || win_owner[wid] != kQueryNone || wid != nfetched * nwaves + w) return false;
            win_owner[wid] = w;
            ++nfetched;
            return true;
        };
        if (!claim(q.base / kQueryWin) || !claim(q.wnx)) return fail("first windows", w, q.base, q.wnx);
        if (q.wv != query_win_len(q.base / kQueryWin, n) || q.wv == 0 || q.wv > kQueryWin) return fail("window length", w, q.wv);
        bool has[64] = {};
        uint32_t idx[64] = {};
        uint64_t iters = 0;
        for (;; ++iters) {
            if (iters > bound) return fail("the loop did not end", w, iters, bound);
            uint64_t need = 0;
            for (int l = 0; l < 64; ++l) need |= has[l] ? 0ull : 1ull << l;
            if (query_hands_out(need, refill)) {
                if (!refill && need != ~0ull) return fail("refill off handed out to a busy wave", w);
                if (query_wants_next(q)) {
                    const uint32_t expect = q.wnx, len = q.nv;
                    query_advance(q, w, nwaves, n);
                    if (q.base != expect * kQueryWin || q.wv != len || q.cur != 0 || len != query_win_len(expect, n))
                        return fail("advance", w, q.base, expect);
                    if (!claim(q.wnx)) return fail("prefetched window", w, q.wnx);
                    if (q.nv != (q.wnx == kQueryNone ? 0u : query_win_len(q.wnx, n))) return fail("prefetched length", w, q.nv);
                }
                const QueryWave before = q;
                for (int l = 0; l < 64; ++l) {
                    if (has[l]) continue;
                    const uint32_t k = query_position(before, rank_below(need, l));
                    if (k == kQueryNone) continue;
                    const uint32_t i = before.base + k;
                    if (i >= n) return fail("ray index out of range", w, i, n);
                    if (handed[i]) return fail("ray handed out twice", w, i);
                    handed[i] = 1;
                    has[l] = true;
                    idx[l] = i;
                }
                query_took(q, (uint32_t)__builtin_popcountll(need));
                if (q.cur > q.wv) return fail("cur past the window", w, q.cur, q.wv);
            }
            uint64_t busy = 0;
            for (int l = 0; l < 64; ++l) busy |= has[l] ? 1ull << l : 0ull;
            if (busy == 0) {
                if (!query_done(q, busy)) return fail("idle wave that is not done", w, q.cur, q.nv);
                break;
            }
            // the traversal: a non-empty random subset of the busy lanes finishes
            uint64_t fin = busy & (((uint64_t)rnd() << 32) | rnd()) & (((uint64_t)rnd() << 32) | rnd());
            if (fin == 0) {  // at least one: the (rnd)-th busy lane
                uint32_t pick = rnd() % (uint32_t)__builtin_popcountll(busy);
                for (int l = 0; l < 64; ++l)
                    if ((busy >> l & 1) && pick-- == 0) fin = 1ull << l;
            }
            for (int l = 0; l < 64; ++l) {
                if (!(fin >> l & 1)) continue;
                if (written[idx[l]]) return fail("result slot written twice", w, idx[l]);
                written[idx[l]] = 1;
                has[l] = false;
            }
        }
        if (iters > max_iters) max_iters = iters;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (handed[i] != 1 || written[i] != 1) return fail("ray never handed out or written", 0, i);
    for (uint32_t k = 0; k < nwin; ++k)
        if (win_owner[k] != k % nwaves) return fail("window owner", win_owner[k], k);
    std::printf("ok n=%u waves=%u refill=%d windows=%u max_iters=%llu\n", n, nwaves, refill ? 1 : 0, nwin,
                (unsigned long long)max_iters);
    return 0;
}
