// pt_build.hip — the LBVH of include/pt_hip.h built on the device (pt_scene_create_mesh): the stages
// in order, one kernel or a few each.
//   1  k_build_bounds, k_build_validate   lo / hi over the vertex section; per-record checks into the error
//                                         word, the flagged records counted
//   2  k_build_keys                       Morton keys (flagged records under an emitter root: their record
//                                         number alone, so that the sort puts them first, in record order),
//                                         key r at position r
//   3  k_build_sort_*                     a stable LSD radix sort of the keys' upper words, four passes of 8 bits
//                                         (the lower word is the record number, which is the input's order)
//   4  k_build_karras                     Karras' per-node construction of the radix tree, with parents
//   5  k_build_depth                      depth by a walk up the parents
//   6  k_build_level, once per depth      child boxes, packed sizes and internal-node counts, bottom-up
//   7  k_build_offsets                    packed offset and device node number by a walk up the parents
//   8  k_build_emit_*                     Node, Tri, tnorm and the packed floats
// No workgroup hands anything to another inside a launch: the bottom-up pass is one launch per depth
// (at most PT_LBVH_MAX_DEPTH - 1 small ones), so a parent reads its children's boxes across a kernel
// boundary — no arrival counters, no fences, nothing that spins.  The only atomics are order-independent
// reductions (min, max, or, add of integers) into the control words.
// A record's indices are clamped before they address anything, so a mesh that fails validation is built
// into a meaningless but harmless tree that the host then discards.
#include <algorithm>

#include "pt_build.h"
#include "pt_kernels.h"  // PT_LAUNCH and the stages' profiler ids

namespace pt {
namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kKeyTree = 1ull << 62;  // set in every Morton key: sorts after the flagged records' keys

__device__ inline uint32_t ord_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}
__device__ inline float ord_val(uint32_t k) { return __uint_as_float(k & 0x80000000u ? k ^ 0x80000000u : ~k); }
__device__ inline float omin(float a, float b) { return ord_key(b) < ord_key(a) ? b : a; }
__device__ inline float omax(float a, float b) { return ord_key(b) > ord_key(a) ? b : a; }

__device__ inline int32_t d_wgsl_i32(float f) {
    if (f != f) return 0;
    if (f >= 2147483647.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)f;
}

// one f32 ulp outward (nextafterf towards -inf / +inf), on the bits
__device__ inline float pad_lo(float v) {
    if (v != v || v == -INFINITY) return v;
    if (v == 0.0f) return __uint_as_float(0x80000001u);
    const uint32_t u = __float_as_uint(v);
    return __uint_as_float(u & 0x80000000u ? u + 1 : u - 1);
}
__device__ inline float pad_hi(float v) {
    if (v != v || v == INFINITY) return v;
    if (v == 0.0f) return __uint_as_float(0x00000001u);
    const uint32_t u = __float_as_uint(v);
    return __uint_as_float(u & 0x80000000u ? u - 1 : u + 1);
}

struct Rec {
    uint32_t v[3];  // vertex numbers, 0-based, clamped into the vertex section
    uint32_t mat;   // clamped
    uint32_t err;
};
__device__ inline Rec load_rec(const BuildMesh& m, uint32_t r) {
    const float* f = m.tri + m.i_start + 4 * (size_t)r;
    Rec o;
    o.err = 0;
    for (int k = 0; k < 3; ++k) {
        const int32_t i = d_wgsl_i32(f[k]);
        if (i < 1 || (uint32_t)i > m.nverts) o.err |= BUILD_ERR_INDEX;
        o.v[k] = (uint32_t)min(max(i, 1), (int32_t)m.nverts) - 1;
    }
    const int32_t mat = d_wgsl_i32(f[3]);
    if (mat < 0 || (uint32_t)mat >= m.nobj) o.err |= BUILD_ERR_MATERIAL;
    o.mat = (uint32_t)min(max(mat, 0), (int32_t)m.nobj - 1);
    return o;
}
__device__ inline const float* vertex(const BuildMesh& m, uint32_t v) { return m.tri + m.v_start + 3 * (size_t)v; }
__device__ inline bool flagged(const BuildMesh& m, uint32_t mat) {
    const float* ke = m.tri + m.m_start + 15 * (size_t)mat + 12;
    const float s = ke[0] + ke[1];
    return s + ke[2] > 0.0f;
}

struct DBox {
    float mn[3], mx[3];
};
__device__ inline void box_add(DBox& b, const float* p, bool first) {
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = first ? p[k] : omin(b.mn[k], p[k]);
        b.mx[k] = first ? p[k] : omax(b.mx[k], p[k]);
    }
}
__device__ inline DBox rec_box(const BuildMesh& m, const Rec& rc) {
    DBox b;
    for (int v = 0; v < 3; ++v) box_add(b, vertex(m, rc.v[v]), v == 0);
    return b;
}
// the box of the records at sorted positions [a, b] (one lane)
__device__ inline DBox range_box(const BuildMesh& m, const unsigned long long* keys, uint32_t a, uint32_t b) {
    DBox bx;
    for (uint32_t p = a; p <= b; ++p) {
        const Rec rc = load_rec(m, (uint32_t)(keys[p] & 0xffffffffull));
        for (int v = 0; v < 3; ++v) box_add(bx, vertex(m, rc.v[v]), p == a && v == 0);
    }
    return bx;
}

// ---- stage 1 ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_build_bounds(BuildMesh m, BuildCtl* ctl) {
    __shared__ uint32_t red[6][kBlock];
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m.nverts; i += gridDim.x * kBlock) {
        const float* p = vertex(m, i);
        for (int k = 0; k < 3; ++k) {
            const float x = p[k];
            if (x != x) continue;
            lo[k] = min(lo[k], ord_key(x));
            hi[k] = max(hi[k], ord_key(x));
        }
    }
    for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = lo[k]; red[3 + k][threadIdx.x] = hi[k]; }
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; ++k) {
                red[k][threadIdx.x] = min(red[k][threadIdx.x], red[k][threadIdx.x + s]);
                red[3 + k][threadIdx.x] = max(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) {
            atomicMin(&ctl->bounds[k], red[k][0]);
            atomicMax(&ctl->bounds[3 + k], red[3 + k][0]);
        }
}

__global__ void __launch_bounds__(kBlock) k_build_validate(BuildMesh m, BuildCtl* ctl) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= m.T) return;
    const Rec rc = load_rec(m, r);
    uint32_t err = rc.err;
    if (!err)
        for (int v = 0; v < 3; ++v) {
            const float* p = vertex(m, rc.v[v]);
            for (int k = 0; k < 3; ++k)
                if (!(fabsf(p[k]) <= 3.402823466e38f)) err |= BUILD_ERR_NONFINITE;
        }
    if (err) atomicOr(&ctl->err, err);
    if (flagged(m, rc.mat)) atomicAdd(&ctl->nlit, 1u);
}

// ---- stage 2 ---------------------------------------------------------------------------------
__device__ inline uint32_t spread10(uint32_t q) {
    q &= 0x3ffu;
    q = (q | q << 16) & 0x030000ffu;
    q = (q | q << 8) & 0x0300f00fu;
    q = (q | q << 4) & 0x030c30c3u;
    q = (q | q << 2) & 0x09249249u;
    return q;
}

__global__ void __launch_bounds__(kBlock) k_build_keys(BuildMesh m, BuildCtl* ctl, unsigned long long* keys, int isolate) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= m.T) return;
    const uint32_t nlit = ctl->nlit;
    const bool iso = isolate && nlit > 0 && nlit < m.T;
    const Rec rc = load_rec(m, r);
    const DBox b = rec_box(m, rc);
    if (iso && flagged(m, rc.mat)) {
        keys[r] = r;
        for (int k = 0; k < 3; ++k) {
            atomicMin(&ctl->ebox[k], ord_key(b.mn[k]));
            atomicMax(&ctl->ebox[3 + k], ord_key(b.mx[k]));
        }
        return;
    }
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = ord_val(ctl->bounds[k]), hi = ord_val(ctl->bounds[3 + k]);
        const float ext = hi - lo;
        const float inv = ext > 0.0f ? 1024.0f / ext : 0.0f;
        const float c = (b.mn[k] + b.mx[k]) * 0.5f;
        const float x = (c - lo) * inv;
        q[k] = x >= 0.0f ? (uint32_t)fminf(x, 1023.0f) : 0u;
    }
    const uint32_t morton = spread10(q[0]) << 2 | spread10(q[1]) << 1 | spread10(q[2]);
    keys[r] = kKeyTree | (unsigned long long)morton << 32 | r;
}

// ---- stage 3 ---------------------------------------------------------------------------------
// keys[r] stands at position r, so a STABLE sort by the upper 32 bits is the sort of the whole key.  One pass
// per 8-bit digit: a histogram per tile of kSortTile keys, an exclusive scan over (digit, tile), and a scatter
// that ranks a tile's keys in their order — within a wave by the lanes below holding the same digit (ballots),
// across the tile's waves and iterations by counts in LDS.
constexpr int kSortItems = 8;
constexpr uint32_t kSortTile = kBlock * kSortItems;
static_assert(kBlock == 256, "one thread per digit value; four waves of 64");

__global__ void __launch_bounds__(kBlock) k_build_sort_hist(const unsigned long long* in, uint32_t n, uint32_t shift, uint32_t* hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t idx = base + k * kBlock + threadIdx.x;
        if (idx < n) atomicAdd(&h[(uint32_t)(in[idx] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[blockIdx.x * 256u + threadIdx.x] = h[threadIdx.x];
}

// exclusive scan over the block's 256 values through LDS; *total: their sum
__device__ inline uint32_t block_excl_scan(uint32_t* lds, uint32_t t, uint32_t mine, uint32_t* total) {
    lds[t] = mine;
    __syncthreads();
    for (uint32_t s = 1; s < 256; s <<= 1) {
        const uint32_t add = t >= s ? lds[t - s] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[255];
    __syncthreads();
    return incl - mine;
}

// Block d takes digit d: hist[tile][d] counts -> each tile's first position within the digit, 256 tiles a
// step; totals[d] = the digit's keys (the scatter adds the digits below)
__global__ void __launch_bounds__(kBlock) k_build_sort_scan(uint32_t* hist, uint32_t ntiles, uint32_t* totals) {
    __shared__ uint32_t lds[256];
    const uint32_t d = blockIdx.x, t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t c = 0; c < ntiles; c += 256) {  // (uniform: the scan's barriers)
        const uint32_t b = c + t;
        const uint32_t v = b < ntiles ? hist[b * 256u + d] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(lds, t, v, &tot);
        if (b < ntiles) hist[b * 256u + d] = carry + ex;
        carry += tot;
    }
    if (t == 0) totals[d] = carry;
}

__global__ void __launch_bounds__(kBlock) k_build_sort_scatter(const unsigned long long* in, unsigned long long* out, uint32_t n,
                                                               uint32_t shift, const uint32_t* hist, const uint32_t* totals) {
    __shared__ uint32_t running[256];
    __shared__ uint32_t cnt[kBlock / 64][256];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    uint32_t all;
    running[t] = block_excl_scan(cnt[0], t, totals[t], &all) + hist[blockIdx.x * 256u + t];
    for (int w = 0; w < kBlock / 64; ++w) cnt[w][t] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (int k = 0; k < kSortItems; ++k) {  // (every lane takes every turn: the ballots and barriers are uniform)
        const uint32_t idx = base + k * kBlock + t;
        const bool valid = idx < n;
        const unsigned long long key = valid ? in[idx] : 0ull;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long b = __ballot(valid && one);
            same &= one ? b : ~b;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) cnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t at = running[d] + rank;
            for (uint32_t w = 0; w < wave; ++w) at += cnt[w][d];
            out[at] = key;
        }
        __syncthreads();
        uint32_t add = 0;
        for (int w = 0; w < kBlock / 64; ++w) { add += cnt[w][t]; cnt[w][t] = 0; }
        running[t] += add;
        __syncthreads();
    }
}

// ---- stages 4-7: the radix tree over keys[E .. T), E = the flagged records under an emitter root ----
struct Radix {
    const unsigned long long* keys;  // the tree's, sorted
    uint32_t n;
    uint32_t E;
    uint32_t base_depth;  // the radix root's
};
__device__ inline Radix radix_of(const BuildMesh& m, const BuildCtl* ctl, const unsigned long long* keys, int isolate) {
    const uint32_t nlit = ctl->nlit;
    const bool iso = isolate && nlit > 0 && nlit < m.T;
    const uint32_t E = iso ? nlit : 0;
    return Radix{keys + E, m.T - E, E, iso ? 2u : 1u};
}
// common leading bits of keys i and j; -1 outside the tree
__device__ inline int delta(const Radix& t, int64_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)t.n) return -1;
    return __clzll((long long)(t.keys[i] ^ t.keys[j]));
}

__global__ void __launch_bounds__(kBlock) k_build_karras(BuildMesh m, BuildCtl* ctl, BuildWork w, int isolate) {
    const Radix t = radix_of(m, ctl, w.keys, isolate);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t.n < 2 || i >= (int64_t)t.n - 1) return;
    const int d = delta(t, i, i + 1) > delta(t, i, i - 1) ? 1 : -1;
    const int dmin = delta(t, i, i - d);
    int64_t lmax = 2;
    while (delta(t, i, i + lmax * d) > dmin) lmax <<= 1;
    int64_t l = 0;
    for (int64_t s = lmax >> 1; s >= 1; s >>= 1)
        if (delta(t, i, i + (l + s) * d) > dmin) l += s;
    const int64_t j = i + l * d;
    const int dnode = delta(t, i, j);
    int64_t s = 0, step = l;
    do {
        step = (step + 1) >> 1;
        if (delta(t, i, i + (s + step) * d) > dnode) s += step;
    } while (step > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t a = d > 0 ? i : j, b = d > 0 ? j : i;
    w.first[i] = (int32_t)a;
    w.last[i] = (int32_t)b;
    w.split[i] = (int32_t)g;
    if (i == 0) w.parent[0] = -1;
    if (a != g) w.parent[g] = (int32_t)i;          // the left child [a, g] is a node
    if (b != g + 1) w.parent[g + 1] = (int32_t)i;  // the right child [g + 1, b] is a node
}

__global__ void __launch_bounds__(kBlock) k_build_depth(BuildMesh m, BuildCtl* ctl, BuildWork w, int isolate) {
    const Radix t = radix_of(m, ctl, w.keys, isolate);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (t.n < 2 || i >= t.n - 1) return;
    uint32_t d = t.base_depth;
    int32_t j = (int32_t)i;
    for (int guard = 0; guard < 128; ++guard) {  // (a radix tree over 63-bit keys is at most 63 deep)
        j = w.parent[j];
        if (j < 0) break;
        ++d;
    }
    w.depth[i] = (uint8_t)min(d, 255u);
}

// a node is an internal node of the tree when it holds more than max_leaf records above the depth cap
__device__ inline bool kept(uint32_t count, uint32_t depth, uint32_t max_leaf) {
    return count > max_leaf && depth < (uint32_t)kLbvhMaxDepth;
}

__global__ void __launch_bounds__(kBlock) k_build_level(BuildMesh m, BuildCtl* ctl, BuildWork w, int isolate, uint32_t max_leaf,
                                                        uint32_t depth) {
    const Radix t = radix_of(m, ctl, w.keys, isolate);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (t.n < 2 || i >= t.n - 1 || w.depth[i] != depth) return;
    const uint32_t a = (uint32_t)w.first[i], b = (uint32_t)w.last[i], g = (uint32_t)w.split[i];
    if (!kept(b - a + 1, depth, max_leaf)) return;
    BuildNodeAux out;
    for (int side = 0; side < 2; ++side) {
        const uint32_t ca = side ? g + 1 : a, cb = side ? b : g, cn = cb - ca + 1;
        DBox bx;
        uint32_t size, kn;
        if (kept(cn, depth + 1, max_leaf)) {  // a node of the level below: this launch's predecessor wrote it
            const BuildNodeAux& c = w.aux[side ? g + 1 : g];
            for (int k = 0; k < 3; ++k) {
                bx.mn[k] = omin(c.box[k], c.box[6 + k]);
                bx.mx[k] = omax(c.box[3 + k], c.box[9 + k]);
            }
            size = 17 + c.size_l + c.size_r;
            kn = 1 + c.kn_l + c.kn_r;
        } else {
            bx = range_box(m, t.keys, ca, cb);
            size = 17 + 4 * cn;
            kn = 0;
        }
        for (int k = 0; k < 3; ++k) { out.box[6 * side + k] = bx.mn[k]; out.box[6 * side + 3 + k] = bx.mx[k]; }
        (side ? out.size_r : out.size_l) = size;
        (side ? out.kn_r : out.kn_l) = kn;
    }
    w.aux[i] = out;
}

__global__ void __launch_bounds__(kBlock) k_build_offsets(BuildMesh m, BuildCtl* ctl, BuildWork w, int isolate, uint32_t max_leaf,
                                                          uint32_t radix_off, uint32_t radix_num) {
    const Radix t = radix_of(m, ctl, w.keys, isolate);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (t.n < 2 || i >= t.n - 1) return;
    if (!kept((uint32_t)(w.last[i] - w.first[i] + 1), w.depth[i], max_leaf)) return;
    uint32_t off = radix_off, num = radix_num;
    int32_t j = (int32_t)i;
    for (int guard = 0; guard < kLbvhMaxDepth; ++guard) {
        const int32_t p = w.parent[j];
        if (p < 0) break;
        const bool right = j != w.split[p];
        off += 17 + (right ? w.aux[p].size_l : 0);
        num += 1 + (right ? w.aux[p].kn_l : 0);
        j = p;
    }
    w.off[i] = off;
    w.num[i] = num;
}

// ---- stage 8 ---------------------------------------------------------------------------------
__device__ inline void put_node_header(float* o, uint32_t off, uint32_t right_off, const float lbox[6], const float rbox[6],
                                       bool lempty) {
    o[0] = 0.0f; o[1] = 0.0f; o[2] = (float)(off + 17); o[3] = (float)right_off; o[4] = -2.0f;
    for (int k = 0; k < 3; ++k) {
        o[5 + k] = lempty ? 0.0f : pad_lo(lbox[k]);
        o[8 + k] = lempty ? 0.0f : pad_hi(lbox[3 + k]);
        o[11 + k] = pad_lo(rbox[k]);
        o[14 + k] = pad_hi(rbox[3 + k]);
    }
}
__device__ inline void put_leaf_header(float* o, uint32_t n) {
    o[0] = 1.0f; o[1] = 0.0f; o[2] = -1.0f; o[3] = -1.0f; o[4] = (float)(4 * n);
    for (int k = 5; k < 17; ++k) o[k] = 0.0f;
}
__device__ inline void node_boxes(Node& nd, const float* o) {  // from a packed node's floats
    for (int k = 0; k < 3; ++k) { nd.lmin[k] = o[5 + k]; nd.lmax[k] = o[8 + k]; nd.rmin[k] = o[11 + k]; nd.rmax[k] = o[14 + k]; }
}

__global__ void __launch_bounds__(kBlock) k_build_emit_nodes(BuildMesh m, BuildCtl* ctl, BuildWork w, int isolate, uint32_t max_leaf,
                                                             Node* nodes, float* packed) {
    __shared__ uint32_t red[2][kBlock];  // the block's largest leaf and deepest node: one atomic each
    const Radix t = radix_of(m, ctl, w.keys, isolate);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t big = 0, deep = 0;
    bool node = t.n >= 2 && i < t.n - 1;
    if (node) node = kept((uint32_t)(w.last[i] - w.first[i] + 1), w.depth[i], max_leaf);
    if (node) {
        const uint32_t a = (uint32_t)w.first[i], b = (uint32_t)w.last[i], g = (uint32_t)w.split[i], depth = w.depth[i];
        const BuildNodeAux ax = w.aux[i];
        const uint32_t off = w.off[i], num = w.num[i];
        float hdr[17];
        put_node_header(hdr, off, off + 17 + ax.size_l, ax.box, ax.box + 6, false);
        for (int k = 0; k < 17; ++k) packed[off + k] = hdr[k];
        Node nd;
        node_boxes(nd, hdr);
        for (int side = 0; side < 2; ++side) {
            const uint32_t ca = side ? g + 1 : a, cb = side ? b : g, cn = cb - ca + 1;
            int32_t ref, cnt;
            if (kept(cn, depth + 1, max_leaf)) {
                ref = (int32_t)(num + 1 + (side ? ax.kn_l : 0));
                cnt = -1;
            } else {
                float* o = packed + off + 17 + (side ? ax.size_l : 0);
                put_leaf_header(o, cn);
                for (uint32_t p = ca; p <= cb; ++p) {
                    const float* f = m.tri + m.i_start + 4 * (size_t)(t.keys[p] & 0xffffffffull);
                    for (int k = 0; k < 4; ++k) o[17 + 4 * (p - ca) + k] = f[k];
                }
                ref = (int32_t)(t.E + ca);
                cnt = (int32_t)cn;
                big = max(big, cn);
            }
            (side ? nd.rref : nd.lref) = ref;
            (side ? nd.rcnt : nd.lcnt) = cnt;
        }
        nodes[num] = nd;
        deep = depth;
    }
    red[0][threadIdx.x] = big;
    red[1][threadIdx.x] = deep;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = max(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (red[0][0]) atomicMax(&ctl->max_leaf, red[0][0]);
        if (red[1][0]) atomicMax(&ctl->max_depth, red[1][0]);
    }
}

// The tree's top where it is not the radix root (an emitter root, or the root of two leaves), and the
// outer bounds: one lane.  The leaves' entries follow from k_build_emit_entries
__global__ void k_build_emit_top(BuildMesh m, BuildCtl* ctl, BuildWork w, BuildCtl lay, Node* nodes, float* packed) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < 6; ++k) packed[k] = ord_val(lay.bounds[k]);
    const uint32_t T = m.T;
    if (lay.iso) {
        const uint32_t E = lay.nlit, n = T - E, right_off = 6 + 17 + 17 + 4 * E;
        float lbox[6], rbox[6];
        for (int k = 0; k < 6; ++k) lbox[k] = ord_val(lay.ebox[k]);
        if (lay.radix_kept) {
            const BuildNodeAux& c = w.aux[0];
            for (int k = 0; k < 3; ++k) { rbox[k] = omin(c.box[k], c.box[6 + k]); rbox[3 + k] = omax(c.box[3 + k], c.box[9 + k]); }
        } else {
            const DBox bx = range_box(m, w.keys, E, T - 1);
            for (int k = 0; k < 3; ++k) { rbox[k] = bx.mn[k]; rbox[3 + k] = bx.mx[k]; }
            put_leaf_header(packed + right_off, n);
        }
        put_node_header(packed + 6, 6, right_off, lbox, rbox, false);
        put_leaf_header(packed + 23, E);
        Node nd;
        node_boxes(nd, packed + 6);
        nd.lref = 0; nd.lcnt = (int32_t)E;
        nd.rref = lay.radix_kept ? 1 : (int32_t)E;
        nd.rcnt = lay.radix_kept ? -1 : (int32_t)n;
        nodes[0] = nd;
        atomicMax(&ctl->max_leaf, lay.radix_kept ? E : max(E, n));
        atomicMax(&ctl->max_depth, 1u);
    } else if (lay.two_leaf) {
        const uint32_t n = T, h = n / 2, right_off = 6 + 17 + 17 + 4 * h;
        const DBox bx = range_box(m, w.keys, 0, n - 1);
        float box[6];
        for (int k = 0; k < 3; ++k) { box[k] = bx.mn[k]; box[3 + k] = bx.mx[k]; }
        put_node_header(packed + 6, 6, right_off, box, box, h == 0);
        put_leaf_header(packed + 23, h);
        put_leaf_header(packed + right_off, n - h);
        Node nd;
        node_boxes(nd, packed + 6);
        nd.lref = 0; nd.lcnt = (int32_t)h;
        nd.rref = (int32_t)h; nd.rcnt = (int32_t)(n - h);
        nodes[0] = nd;
        atomicMax(&ctl->max_leaf, n - h);
        atomicMax(&ctl->max_depth, 1u);
    }
}

// the entries of a leaf of the top: the records at sorted positions [p0, p0 + count) to packed[dst ..]
__global__ void __launch_bounds__(kBlock) k_build_emit_entries(BuildMesh m, BuildWork w, uint32_t p0, uint32_t count, uint32_t dst,
                                                               float* packed) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= count) return;
    const float* f = m.tri + m.i_start + 4 * (size_t)(w.keys[p0 + p] & 0xffffffffull);
    for (int k = 0; k < 4; ++k) packed[dst + 4 * (size_t)p + k] = f[k];
}

// Tri and tnorm per sorted position (decode_tree's arithmetic and its clamped reads of the normal
// section), and the reduction fast_rcp needs: max |e1| |e2| in double, as fast_rcp_holds takes it
__global__ void __launch_bounds__(kBlock) k_build_emit_tris(BuildMesh m, BuildCtl* ctl, BuildWork w, Tri* tris, float4* tnorm) {
    __shared__ unsigned long long red[kBlock];
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long mine = 0;
    if (p < m.T) {
        const uint32_t r = (uint32_t)(w.keys[p] & 0xffffffffull);
        const Rec rc = load_rec(m, r);
        const float *v0 = vertex(m, rc.v[0]), *v1 = vertex(m, rc.v[1]), *v2 = vertex(m, rc.v[2]);
        float e1[3], e2[3];
        for (int q = 0; q < 3; ++q) { e1[q] = v1[q] - v0[q]; e2[q] = v2[q] - v0[q]; }
        Tri t;
        t.q0[0] = v0[0]; t.q0[1] = v0[1]; t.q0[2] = v0[2]; t.q0[3] = e1[0];
        t.q1[0] = e1[1]; t.q1[1] = e1[2]; t.q1[2] = e2[0]; t.q1[3] = e2[1];
        t.e2z = e2[2];
        t.mat = (int32_t)rc.mat;
        t.uid = (int32_t)p;
        t.lbvh = 0;
        tris[p] = t;
        for (int q = 0; q < 3; ++q) {
            const uint32_t at0 = (uint32_t)m.vn_start + rc.v[q] * 3u;
            float nv[3];
            for (uint32_t k = 0; k < 3; ++k) {
                uint32_t u = at0 + k;
                if (u >= m.tri_len) u = m.tri_len - 1;
                nv[k] = m.tri[u];
            }
            tnorm[3 * (size_t)p + q] = make_float4(nv[0], nv[1], nv[2], (q == 0 && (int32_t)(rc.v[2] * 3u) < m.vn_range) ? 1.0f : 0.0f);
        }
        const double a = sqrt((double)e1[0] * e1[0] + (double)e1[1] * e1[1] + (double)e1[2] * e1[2]);
        const double b = sqrt((double)e2[0] * e2[0] + (double)e2[1] * e2[1] + (double)e2[2] * e2[2]);
        const double ab = a * b;
        if (!(a <= 1.7976931348623157e308) || !(b <= 1.7976931348623157e308)) atomicOr(&ctl->edge_nonfinite, 1u);
        mine = ab == ab ? (unsigned long long)__double_as_longlong(ab) : 0ull;  // a >= 0, b >= 0: the bits order as the values
    }
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicMax(&ctl->edge_max, red[0]);
}

inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }
inline int launched() { return hipGetLastError() == hipSuccess ? PT_OK : PT_ERR_HIP; }

}  // namespace

// the sort's per-tile histograms, then the 256 digit totals
size_t build_sort_bytes(uint32_t T) { return (((size_t)T + kSortTile - 1) / kSortTile + 1) * 256 * sizeof(uint32_t); }

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

BuildWork build_carve(char* base, uint32_t T, size_t sort_bytes, size_t* total) {
    BuildWork w{};
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + at : nullptr; at += up256(bytes); return p; };
    const size_t n = T;
    w.ctl = reinterpret_cast<BuildCtl*>(take(sizeof(BuildCtl)));
    w.keys = reinterpret_cast<unsigned long long*>(take(n * 8));
    w.keys_alt = reinterpret_cast<unsigned long long*>(take(n * 8));
    w.sort_tmp = take(sort_bytes);
    w.sort_bytes = sort_bytes;
    w.parent = reinterpret_cast<int32_t*>(take(n * 4));
    w.first = reinterpret_cast<int32_t*>(take(n * 4));
    w.last = reinterpret_cast<int32_t*>(take(n * 4));
    w.split = reinterpret_cast<int32_t*>(take(n * 4));
    w.depth = reinterpret_cast<uint8_t*>(take(n));
    w.aux = reinterpret_cast<BuildNodeAux*>(take(n * sizeof(BuildNodeAux)));
    w.off = reinterpret_cast<uint32_t*>(take(n * 4));
    w.num = reinterpret_cast<uint32_t*>(take(n * 4));
    if (total) *total = at;
    return w;
}

int build_tree(const BuildMesh& m, const BuildWork& w, uint32_t max_leaf, bool isolate, hipStream_t stream) {
    BuildCtl init{};
    for (int k = 0; k < 3; ++k) { init.bounds[k] = init.ebox[k] = 0xffffffffu; init.bounds[3 + k] = init.ebox[3 + k] = 0; }
    // (pageable source: the runtime has read it when the call returns)
    if (hipMemcpyAsync(w.ctl, &init, sizeof init, hipMemcpyHostToDevice, stream) != hipSuccess) return PT_ERR_HIP;
    const int iso = isolate ? 1 : 0;
    const uint32_t T = m.T, gT = blocks_for(T);
    PT_LAUNCH(KID_BUILD_BOUNDS, stream, k_build_bounds, dim3(std::min<uint32_t>(blocks_for(m.nverts), 1024u)), dim3(kBlock), 0, stream, m, w.ctl);
    PT_LAUNCH(KID_BUILD_BOUNDS, stream, k_build_validate, dim3(gT), dim3(kBlock), 0, stream, m, w.ctl);
    PT_LAUNCH(KID_BUILD_KEYS, stream, k_build_keys, dim3(gT), dim3(kBlock), 0, stream, m, w.ctl, w.keys, iso);
    {   // four passes over bits 32..63: keys -> keys_alt -> keys -> keys_alt -> keys
        const uint32_t tiles = (T + kSortTile - 1) / kSortTile;
        uint32_t* hist = static_cast<uint32_t*>(w.sort_tmp);
        uint32_t* totals = hist + (size_t)tiles * 256;
        unsigned long long *a = w.keys, *b = w.keys_alt;
        for (uint32_t shift = 32; shift < 64; shift += 8) {
            PT_LAUNCH(KID_BUILD_SORT, stream, k_build_sort_hist, dim3(tiles), dim3(kBlock), 0, stream, a, T, shift, hist);
            PT_LAUNCH(KID_BUILD_SORT, stream, k_build_sort_scan, dim3(256), dim3(kBlock), 0, stream, hist, tiles, totals);
            PT_LAUNCH(KID_BUILD_SORT, stream, k_build_sort_scatter, dim3(tiles), dim3(kBlock), 0, stream, a, b, T, shift, hist, totals);
            std::swap(a, b);
        }
    }
    if (T >= 2) {
        const uint32_t gN = blocks_for(T - 1);  // the tree holds at most T keys: T - 1 nodes
        PT_LAUNCH(KID_BUILD_KARRAS, stream, k_build_karras, dim3(gN), dim3(kBlock), 0, stream, m, w.ctl, w, iso);
        PT_LAUNCH(KID_BUILD_DEPTH, stream, k_build_depth, dim3(gN), dim3(kBlock), 0, stream, m, w.ctl, w, iso);
        for (uint32_t d = (uint32_t)kLbvhMaxDepth - 1; d >= 1; --d)
            PT_LAUNCH(KID_BUILD_LEVEL, stream, k_build_level, dim3(gN), dim3(kBlock), 0, stream, m, w.ctl, w, iso, max_leaf, d);
    }
    return launched();
}

int build_emit(const BuildMesh& m, const BuildWork& w, const BuildCtl& lay, uint32_t max_leaf, Node* nodes, Tri* tris,
               float4* tnorm, float* packed, hipStream_t stream) {
    const int iso = lay.iso ? 1 : 0;
    const uint32_t T = m.T;
    if (lay.radix_kept) {
        const uint32_t gN = blocks_for(T - 1);
        PT_LAUNCH(KID_BUILD_OFFSETS, stream, k_build_offsets, dim3(gN), dim3(kBlock), 0, stream, m, w.ctl, w, iso, max_leaf, lay.radix_off, lay.radix_num);
        PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_nodes, dim3(gN), dim3(kBlock), 0, stream, m, w.ctl, w, iso, max_leaf, nodes, packed);
    }
    PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_top, dim3(1), dim3(64), 0, stream, m, w.ctl, w, lay, nodes, packed);
    if (lay.iso) {
        const uint32_t E = lay.nlit, n = T - E;
        PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_entries, dim3(blocks_for(E)), dim3(kBlock), 0, stream, m, w, 0u, E, 23u + 17u, packed);
        if (!lay.radix_kept)
            PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_entries, dim3(blocks_for(n)), dim3(kBlock), 0, stream, m, w, E, n,
                               6u + 17u + 17u + 4u * E + 17u, packed);
    } else if (lay.two_leaf) {
        const uint32_t h = T / 2;
        if (h) PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_entries, dim3(blocks_for(h)), dim3(kBlock), 0, stream, m, w, 0u, h, 23u + 17u, packed);
        PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_entries, dim3(blocks_for(T - h)), dim3(kBlock), 0, stream, m, w, h, T - h,
                           6u + 17u + 17u + 4u * h + 17u, packed);
    }
    PT_LAUNCH(KID_BUILD_EMIT, stream, k_build_emit_tris, dim3(blocks_for(T)), dim3(kBlock), 0, stream, m, w.ctl, w, tris, tnorm);
    return launched();
}

}  // namespace pt
