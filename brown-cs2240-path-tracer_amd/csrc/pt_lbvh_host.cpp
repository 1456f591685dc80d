// pt_lbvh_host.cpp — the LBVH of include/pt_hip.h built on the host (standard C++, no GPU): written
// top-down and recursively from the definition there, so that it shares nothing with the device
// builder (pt_build.hip: Karras' per-node construction, level launches) it is compared with byte for
// byte (tests/test_gpu_lbvh.py).  The rules are stated in the header only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pt_hip.h"

namespace {

constexpr int kLbvhMaxDepth = PT_LBVH_MAX_DEPTH;

int32_t wgsl_i32(float f) {  // WGSL i32(f32): truncate toward zero, saturating
    if (std::isnan(f)) return 0;
    if (f >= 2147483647.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)f;
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// the header's total order (-0 < +0)
bool before(float a, float b) {
    const uint32_t x = bits(a), y = bits(b);
    const uint32_t kx = x & 0x80000000u ? ~x : x | 0x80000000u, ky = y & 0x80000000u ? ~y : y | 0x80000000u;
    return kx < ky;
}

struct Box {
    float mn[3], mx[3];
    bool empty = true;
    void add(const float* p) {
        for (int k = 0; k < 3; ++k) {
            if (empty || before(p[k], mn[k])) mn[k] = p[k];
            if (empty || before(mx[k], p[k])) mx[k] = p[k];
        }
        empty = false;
    }
    void add(const Box& o) {
        if (o.empty) return;
        add(o.mn);
        add(o.mx);
    }
};

struct Mesh {
    const float* tri;
    const float* verts;  // the vertex section
    const float* recs;   // the index section
    size_t T;
    const float* vertex(size_t r, int v) const { return verts + 3 * (size_t)(wgsl_i32(recs[4 * r + v]) - 1); }
    Box box_of(size_t r) const {
        Box b;
        for (int v = 0; v < 3; ++v) b.add(vertex(r, v));
        return b;
    }
};

uint32_t spread(uint32_t q) {
    uint32_t m = 0;
    for (int k = 0; k < 10; ++k) m |= ((q >> k) & 1u) << (3 * k);
    return m;
}

int clz64(uint64_t v) {
    int n = 0;
    for (uint64_t bit = 1ull << 63; bit && !(v & bit); bit >>= 1) ++n;
    return n;
}

struct Tree {
    const Mesh& m;
    const std::vector<uint64_t>& key;  // sorted
    uint32_t max_leaf;
    std::vector<float>& out;

    static void pad_box(const Box& b, float* dst) {  // dst holds zeros
        if (b.empty) return;
        for (int k = 0; k < 3; ++k) dst[k] = std::nextafterf(b.mn[k], -INFINITY);
        for (int k = 0; k < 3; ++k) dst[3 + k] = std::nextafterf(b.mx[k], INFINITY);
    }
    // a leaf of the records key[a .. b) (or, keys null, of the records list), its box returned
    Box leaf(const uint64_t* keys, const uint32_t* list, size_t n) {
        Box b;
        out.push_back(1.0f); out.push_back(0.0f); out.push_back(-1.0f); out.push_back(-1.0f); out.push_back((float)(4 * n));
        out.insert(out.end(), 12, 0.0f);
        for (size_t i = 0; i < n; ++i) {
            const size_t r = keys ? (size_t)(keys[i] & 0xffffffffu) : list[i];
            out.insert(out.end(), m.recs + 4 * r, m.recs + 4 * r + 4);
            b.add(m.box_of(r));
        }
        return b;
    }
    // an internal node's header with room for its boxes; returns its offset
    size_t open_node() {
        const size_t o = out.size();
        out.push_back(0.0f); out.push_back(0.0f); out.push_back((float)(o + 17)); out.push_back(-1.0f); out.push_back(-2.0f);
        out.insert(out.end(), 12, 0.0f);
        return o;
    }
    void close_node(size_t o, size_t right_off, const Box& l, const Box& r) {
        out[o + 3] = (float)right_off;
        pad_box(l, &out[o + 5]);
        pad_box(r, &out[o + 11]);
    }
    // the radix node over sorted positions [a, b] at `depth`, whose parent holds parent_n records
    Box node(size_t a, size_t b, int depth, size_t parent_n) {
        const size_t n = b - a + 1;
        if ((n <= max_leaf && parent_n > max_leaf) || depth >= kLbvhMaxDepth || a == b) return leaf(&key[a], nullptr, n);
        const int p = clz64(key[a] ^ key[b]);
        size_t s = a;  // the largest s in [a, b) sharing more than p leading bits with key[a]
        for (size_t lo = a + 1, hi = b - 1; lo <= hi;) {
            const size_t mid = lo + (hi - lo) / 2;
            if (clz64(key[a] ^ key[mid]) > p) { s = mid; lo = mid + 1; } else { hi = mid - 1; }
        }
        const size_t o = open_node();
        const Box l = node(a, s, depth + 1, n);
        const size_t right_off = out.size();
        const Box r = node(s + 1, b, depth + 1, n);
        close_node(o, right_off, l, r);
        Box u = l;
        u.add(r);
        return u;
    }
};

bool header_ok(const float* tri, size_t tri_len, int64_t& nverts, int64_t& nobj, int64_t& v_start, int64_t& i_start,
               int64_t& m_start) {
    if (tri_len < 16 || tri_len > (size_t)INT32_MAX) return false;
    const float nverts_f = tri[0], nobj_f = tri[1];
    if (!(nverts_f >= 0 && nverts_f == std::floor(nverts_f)) || !(nobj_f >= 1 && nobj_f == std::floor(nobj_f))) return false;
    nverts = (int64_t)nverts_f;
    nobj = (int64_t)nobj_f;
    v_start = wgsl_i32(tri[2]);
    i_start = wgsl_i32(tri[3]);
    m_start = wgsl_i32(tri[4]);
    if (v_start < 0 || v_start + 3 * nverts > (int64_t)tri_len) return false;
    if (m_start < 0 || m_start + 15 * nobj > (int64_t)tri_len) return false;
    return i_start >= 16 && i_start <= m_start && (m_start - i_start) % 4 == 0 && m_start - i_start >= 4;
}

}  // namespace

extern "C" int pt_build_defaults(pt_build_params* params) {
    if (!params) return PT_ERR_INVALID;
    *params = pt_build_params{4, 1, 0, 0};
    return PT_OK;
}

extern "C" int pt_bvh_build_lbvh(const float* triangle_data, size_t triangle_len, const pt_build_params* params,
                                 float* bvh_out, size_t bvh_cap, size_t* bvh_len) {
    if (!triangle_data || !bvh_len || (bvh_cap && !bvh_out)) return PT_ERR_INVALID;
    pt_build_params prm;
    pt_build_defaults(&prm);
    if (params) prm = *params;
    if (prm.max_leaf < 1 || prm.max_leaf > 8 || prm.isolate_emitters > 1 || prm.profile > 1 || prm.reserved)
        return PT_ERR_INVALID;
    const float* tri = triangle_data;
    int64_t nverts, nobj, v_start, i_start, m_start;
    if (!header_ok(tri, triangle_len, nverts, nobj, v_start, i_start, m_start)) return PT_ERR_INVALID;
    const Mesh m{tri, tri + v_start, tri + i_start, (size_t)((m_start - i_start) / 4)};
    const size_t T = m.T;
    for (size_t r = 0; r < T; ++r) {
        for (int v = 0; v < 3; ++v) {
            const int32_t i = wgsl_i32(m.recs[4 * r + v]);
            if (i < 1 || i > nverts) return PT_ERR_INVALID;
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(m.vertex(r, v)[k])) return PT_ERR_INVALID;
        }
        const int32_t mat = wgsl_i32(m.recs[4 * r + 3]);
        if (mat < 0 || mat >= nobj) return PT_ERR_INVALID;
    }
    // lo, hi over the vertex section (every axis sees a referenced, finite coordinate)
    Box all;
    bool seen[3] = {false, false, false};
    for (int64_t i = 0; i < nverts; ++i)
        for (int k = 0; k < 3; ++k) {
            const float x = m.verts[3 * i + k];
            if (x != x) continue;
            if (!seen[k] || before(x, all.mn[k])) all.mn[k] = x;
            if (!seen[k] || before(all.mx[k], x)) all.mx[k] = x;
            seen[k] = true;
        }
    // flagged records
    std::vector<uint32_t> lit;
    std::vector<uint64_t> key;
    {
        std::vector<uint8_t> flagged((size_t)nobj);
        for (int64_t o = 0; o < nobj; ++o) {
            const float* ke = tri + m_start + 15 * o + 12;
            const float s = ke[0] + ke[1];
            flagged[(size_t)o] = s + ke[2] > 0.0f;
        }
        size_t nlit = 0;
        for (size_t r = 0; r < T; ++r) nlit += flagged[(size_t)wgsl_i32(m.recs[4 * r + 3])];
        const bool isolate = prm.isolate_emitters && nlit > 0 && nlit < T;
        float inv[3];
        for (int k = 0; k < 3; ++k) {
            const float ext = all.mx[k] - all.mn[k];
            inv[k] = ext > 0 ? 1024.0f / ext : 0.0f;
        }
        for (size_t r = 0; r < T; ++r) {
            if (isolate && flagged[(size_t)wgsl_i32(m.recs[4 * r + 3])]) {
                lit.push_back((uint32_t)r);
                continue;
            }
            const Box b = m.box_of(r);
            uint32_t q[3];
            for (int k = 0; k < 3; ++k) {
                const float c = (b.mn[k] + b.mx[k]) * 0.5f;
                const float x = (c - all.mn[k]) * inv[k];
                q[k] = x >= 0 ? (uint32_t)std::fmin(x, 1023.0f) : 0u;
            }
            const uint32_t morton = spread(q[0]) << 2 | spread(q[1]) << 1 | spread(q[2]);
            key.push_back((uint64_t)morton << 32 | (uint64_t)r);
        }
    }
    std::sort(key.begin(), key.end());
    std::vector<float> out(all.mn, all.mn + 3);
    out.insert(out.end(), all.mx, all.mx + 3);
    Tree t{m, key, prm.max_leaf, out};
    const size_t n = key.size();
    if (!lit.empty()) {  // the emitter root: one leaf of the flagged records, the tree over the rest
        const size_t o = t.open_node();
        const Box l = t.leaf(nullptr, lit.data(), lit.size());
        const size_t right_off = out.size();
        const Box r = t.node(0, n - 1, 2, (size_t)prm.max_leaf + 1);  // the emitter root counts as holding more
        t.close_node(o, right_off, l, r);
    } else if (n <= prm.max_leaf) {  // the layout needs an internal root: two leaves under it
        const size_t o = t.open_node();
        Box l = t.leaf(key.data(), nullptr, n / 2);
        const size_t right_off = out.size();
        Box r = t.leaf(key.data() + n / 2, nullptr, n - n / 2);
        r.add(l);
        if (!l.empty) l = r;
        t.close_node(o, right_off, l, r);
    } else {
        t.node(0, n - 1, 1, n + 1);
    }
    if (out.size() >= (1u << 24)) return PT_ERR_INVALID;  // float offsets exact below 2^24 (packer.ts layout)
    *bvh_len = out.size();
    if (bvh_cap < out.size()) return bvh_cap ? PT_ERR_INVALID : PT_OK;
    std::memcpy(bvh_out, out.data(), out.size() * sizeof(float));
    return PT_OK;
}
