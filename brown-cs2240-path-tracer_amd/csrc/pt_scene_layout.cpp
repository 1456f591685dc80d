// pt_scene_layout.cpp — the host-only scene builder (pt_scene_layout.h): build_layout's stages, in
// the order they depend on each other, and the device section plan.
#include "pt_scene_layout.h"

#include "pt_device.h"  // kStackMax, and pt_math.h's kPI

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>

namespace pt {
namespace {

// the leaf pass's chunks: the builder's leaves of at most PT_PASS_LEAF entries, neighbours merged
// while they fit PT_PASS_MERGE (<= kPassChunkMax; 0: no merging)
#ifndef PT_PASS_LEAF
#define PT_PASS_LEAF kPassChunkMax
#endif
#ifndef PT_PASS_MERGE
#define PT_PASS_MERGE kPassChunkMax
#endif
static_assert(PT_PASS_LEAF <= kPassChunkMax && PT_PASS_MERGE <= kPassChunkMax, "pass chunks fit the pass's loops");
// the leaf remainders' probe (build_leaf_skips): at most 2^24 triangle tests (Glossy ~1.7 M, ~20 ms)
constexpr uint64_t kLeafSkipProbeTests = 1ull << 24;

int fail(std::string& err, const char* msg) {
    err = msg;
    return PT_ERR_SCENE;
}

// WGSL i32(f32): truncate toward zero, saturating.
int32_t wgsl_i32(float f) {
    if (std::isnan(f)) return 0;
    if (f >= 2147483647.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)f;
}

// Reads of the packed triangle buffer with Dawn/Tint robustness (index clamped to len-1),
// as the WGSL reads primitive_0 in sample_area_lights (intersection-logic.wgsl:260-279).
struct Packed {
    const float* p;
    size_t n;
    float at(int32_t i) const {
        uint32_t u = (uint32_t)i;
        if (u >= n) u = (uint32_t)(n - 1);
        return p[u];
    }
};

// the caller's buffers with the checked header fields of triangle_data
struct Input {
    const float *tri, *bvh;
    size_t tri_len, bvh_len;
    int64_t nverts, nobj, v_start, m_start;
};

// what the tree decode leaves for the later stages: each record's leaf entry (i0, i1, i2, material),
// the leaves as (first record, count), and the deepest node
struct Leaves {
    std::vector<std::array<int32_t, 4>> entry;
    std::vector<std::pair<int32_t, int32_t>> ranges;
    uint32_t max_depth = 0;
};

// materials (program-raymarch.wgsl:87-102): Ns Ni illum Ka Kd Ks Ke
void build_materials(const Input& in, HostLayout& L) {
    L.mats.resize((size_t)in.nobj);
    for (int64_t id = 0; id < in.nobj; ++id) {
        const float* m = in.tri + in.m_start + 15 * id;
        Material& o = L.mats[(size_t)id];
        std::memset(&o, 0, sizeof o);
        o.Ns = m[0]; o.Ni = m[1]; o.illum = m[2];
        for (int c = 0; c < 3; ++c) { o.Kd[c] = m[6 + c]; o.Ks[c] = m[9 + c]; o.Ke[c] = m[12 + c]; }
        // the material's constant quotients, once per scene instead of per path and bounce: the
        // same correctly rounded f32 divisions the device would make (no contraction, no FTZ)
        o.kd_pi0 = o.Kd[0] / kPI; o.kd_pi1 = o.Kd[1] / kPI; o.kd_pi2 = o.Kd[2] / kPI;
        o.phong = (o.Ns + 2.0f) / (2.0f * kPI);
    }
    L.info.materials = (uint32_t)in.nobj;
}

bool vertex(const Input& in, int64_t one_based, float out[3]) {
    if (one_based < 1 || one_based > in.nverts) return false;
    const float* v = in.tri + in.v_start + 3 * (one_based - 1);
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
    return true;
}

// BVH: pre-order tree from offset 6 (intersection-logic.wgsl:4-16) -> nodes, one record (and three
// vertex normals) per leaf entry
int decode_tree(const Input& in, HostLayout& L, Leaves& lv, std::string& err) {
    const float *tri = in.tri, *bvh = in.bvh;
    const size_t bvh_len = in.bvh_len;
    const Packed P{tri, in.tri_len};
    if (bvh[6] == 1.0f) return fail(err, "BVH root is a leaf (the reference never builds one)");
    struct Item { int32_t off; int32_t node; int32_t depth; };
    std::vector<Item> work;
    L.nodes.push_back(Node{});
    work.push_back({6, 0, 0});
    const size_t node_cap = bvh_len / 17 + 1;
    while (!work.empty()) {
        Item it = work.back();
        work.pop_back();
        const int32_t o = it.off;
        if (o < 0 || (size_t)o + 17 > bvh_len) return fail(err, "BVH node offset out of range");
        lv.max_depth = std::max<uint32_t>(lv.max_depth, (uint32_t)it.depth);
        Node nd{};
        for (int c = 0; c < 3; ++c) {
            nd.lmin[c] = bvh[o + 5 + c]; nd.lmax[c] = bvh[o + 8 + c];
            nd.rmin[c] = bvh[o + 11 + c]; nd.rmax[c] = bvh[o + 14 + c];
        }
        int32_t child_off[2] = {wgsl_i32(bvh[o + 2]), wgsl_i32(bvh[o + 3])};
        int32_t refs[2], cnts[2];
        for (int side = 0; side < 2; ++side) {
            const int32_t c = child_off[side];
            if (c < 0 || (size_t)c + 17 > bvh_len) return fail(err, "BVH child pointer out of range");
            if (bvh[c] == 1.0f) {  // leaf: (i0,i1,i2,mat) 1-based entries after the 17-float header
                const float nf = bvh[c + 4];
                if (!(nf >= 0) || std::fmod(nf, 4.0f) != 0.0f || (size_t)c + 17 + (size_t)nf > bvh_len)
                    return fail(err, "BVH leaf payload malformed");
                const int32_t n = (int32_t)(nf / 4.0f);
                refs[side] = (int32_t)L.tris.size();
                cnts[side] = n;
                for (int32_t k = 0; k < n; ++k) {
                    const float* e = bvh + c + 17 + 4 * k;
                    float v0[3], v1[3], v2[3];
                    if (!vertex(in, wgsl_i32(e[0]), v0) || !vertex(in, wgsl_i32(e[1]), v1) || !vertex(in, wgsl_i32(e[2]), v2))
                        return fail(err, "BVH leaf references a vertex out of range");
                    const int32_t mat = wgsl_i32(e[3]);
                    if (mat < 0 || mat >= in.nobj) return fail(err, "BVH leaf references a material out of range");
                    Tri t{};
                    float e1[3], e2[3];
                    for (int q = 0; q < 3; ++q) {
                        e1[q] = v1[q] - v0[q];  // ray-triangle-intersection.wgsl:6
                        e2[q] = v2[q] - v0[q];  // :7
                    }
                    tri_set(t, v0, e1, e2);
                    t.mat = mat;
                    t.uid = -1;
                    L.tris.push_back(t);
                    {   // vertex normals at vn_start + i (i = (index - 1) * 3, the vertex offsets;
                        // intersection-logic.wgsl:81-97), reads clamped as Tint's
                        const int32_t vi[3] = {(wgsl_i32(e[0]) - 1) * 3, (wgsl_i32(e[1]) - 1) * 3, (wgsl_i32(e[2]) - 1) * 3};
                        const int32_t vn_start = wgsl_i32(tri[5]), vn_range = wgsl_i32(tri[6]);
                        for (int q = 0; q < 3; ++q)
                            L.tnorm.push_back(make_float4(P.at(vn_start + vi[q]), P.at(vn_start + vi[q] + 1),
                                                          P.at(vn_start + vi[q] + 2),
                                                          (q == 0 && vi[2] < vn_range) ? 1.0f : 0.0f));
                    }
                    lv.entry.push_back({wgsl_i32(e[0]), wgsl_i32(e[1]), wgsl_i32(e[2]), mat});
                }
                lv.ranges.emplace_back(refs[side], n);
                L.info.leaves++;
                L.info.leaf_refs += (uint32_t)n;
                L.info.max_leaf = std::max<uint32_t>(L.info.max_leaf, (uint32_t)n);
            } else {
                if (L.nodes.size() >= node_cap) return fail(err, "BVH is not a tree (node count exceeds buffer)");
                refs[side] = (int32_t)L.nodes.size();
                cnts[side] = -1;
                L.nodes.push_back(Node{});
                work.push_back({c, refs[side], it.depth + 1});
            }
        }
        nd.lref = refs[0]; nd.rref = refs[1]; nd.lcnt = cnts[0]; nd.rcnt = cnts[1];
        L.nodes[(size_t)it.node] = nd;
    }
    L.info.nodes = (uint32_t)L.nodes.size();
    return PT_OK;
}

// The stackless replay tree (BfNode): internal nodes in the reference's visiting order — pre-order
// with the right subtree first — so the next node to visit is always the smallest-numbered pending
// one; and its narrow payload where the scene is small enough.  U: the scene's distinct entries
void build_replay_tree(HostLayout& L, int32_t U) {
    std::vector<int32_t> pre(L.nodes.size(), -1);
    std::vector<int32_t> st{0};
    int32_t next = 0;
    while (!st.empty()) {
        const int32_t n = st.back();
        st.pop_back();
        pre[(size_t)n] = next++;
        L.bfmap.push_back(n);
        const Node& nd = L.nodes[(size_t)n];
        if (nd.lcnt < 0) st.push_back(nd.lref);  // popped after the right subtree
        if (nd.rcnt < 0) st.push_back(nd.rref);
    }
    L.bfnode.resize(L.nodes.size());
    for (size_t i = 0; i < L.bfmap.size(); ++i) {
        const Node& nd = L.nodes[(size_t)L.bfmap[i]];
        BfNode& b = L.bfnode[i];
        for (int c = 0; c < 3; ++c) { b.lmin[c] = nd.lmin[c]; b.lmax[c] = nd.lmax[c]; b.rmin[c] = nd.rmin[c]; b.rmax[c] = nd.rmax[c]; }
        b.lm = nd.lcnt < 0 ? (1ull << 63) | (uint64_t)pre[(size_t)nd.lref] : (nd.lcnt > 0 ? L.lmask[(size_t)nd.lref] : 0ull);
        b.rm = nd.rcnt < 0 ? (1ull << 63) | (uint64_t)pre[(size_t)nd.rref] : (nd.rcnt > 0 ? L.lmask[(size_t)nd.rref] : 0ull);
    }
    // the narrow payload (pt_layout.h): per child the uid set beneath it in the low word
    // (children are numbered after their parents, so a backward sweep has every subtree's
    // union ready), the inner flag and pre-order number in the high word
    if (U > kBfNarrowMax || L.nodes.size() > (size_t)kBfNarrowMax) return;
    std::vector<uint64_t> below(L.nodes.size(), 0);
    auto child_set = [&](int32_t ref, int32_t cnt) {
        return cnt < 0 ? below[(size_t)ref] : (cnt > 0 ? L.lmask[(size_t)ref] : 0ull);
    };
    for (size_t n = L.nodes.size(); n-- > 0;) {
        const Node& nd = L.nodes[n];
        below[n] = child_set(nd.lref, nd.lcnt) | child_set(nd.rref, nd.rcnt);
    }
    L.bfnarrow = L.bfnode;
    for (size_t i = 0; i < L.bfmap.size(); ++i) {
        const Node& nd = L.nodes[(size_t)L.bfmap[i]];
        auto word = [&](int32_t ref, int32_t cnt) {
            const uint64_t hi = cnt < 0 ? (uint64_t)(kBfNarrowInner | (uint32_t)pre[(size_t)ref]) : 0ull;
            return hi << 32 | (child_set(ref, cnt) & 0xffffffffull);
        };
        L.bfnarrow[i].lm = word(nd.lref, nd.lcnt);
        L.bfnarrow[i].rm = word(nd.rref, nd.rcnt);
    }
}

// Mailboxing: a leaf entry tested twice by one query gives the same t both
// times and the closest-hit update is strict-<, so repeats never change the result.  With
// at most 64 distinct entries a query keeps the set it has tested in one 64-bit mask.
// uids follow first appearance (uid_reverse numbers them backwards: tests use it to exercise
// the tie-break of the uid-ordered leaf loop).
void build_mailbox(const Leaves& lv, bool uid_reverse, HostLayout& L) {
    const auto& entry = lv.entry;
    std::map<std::array<int32_t, 4>, int32_t> ids;
    std::vector<int32_t> uid(entry.size());
    std::vector<size_t> first;
    for (size_t r = 0; r < entry.size(); ++r) {
        auto it = ids.find(entry[r]);
        if (it == ids.end()) {
            it = ids.emplace(entry[r], (int32_t)first.size()).first;
            first.push_back(r);
        }
        uid[r] = it->second;
    }
    const int32_t U = (int32_t)first.size();
    L.mailbox = U >= 1 && U <= 64;
    // every record carries its entry's uid (the mailbox scenes renumber below)
    for (size_t r = 0; r < entry.size(); ++r) L.tris[r].uid = uid[r];
    if (!L.mailbox) return;
    for (auto& u : uid) u = uid_reverse ? U - 1 - u : u;
    for (size_t r = 0; r < entry.size(); ++r) L.tris[r].uid = uid[r];
    L.mb_base = (int32_t)L.tris.size();
    std::vector<Tri> uniq((size_t)U);
    for (size_t k = 0; k < first.size(); ++k) uniq[(size_t)uid[first[k]]] = L.tris[first[k]];
    L.tris.insert(L.tris.end(), uniq.begin(), uniq.end());
    std::vector<float4> un(3 * (size_t)U);
    for (size_t k = 0; k < first.size(); ++k)
        for (int q = 0; q < 3; ++q) un[3 * (size_t)uid[first[k]] + q] = L.tnorm[3 * first[k] + q];
    L.tnorm.insert(L.tnorm.end(), un.begin(), un.end());
    L.lmask.assign(std::max<size_t>(1, entry.size()), 0);
    for (const auto& lr : lv.ranges)
        for (int32_t k = 0; k < lr.second; ++k) L.lmask[(size_t)lr.first] |= 1ull << uid[(size_t)(lr.first + k)];
    if (U <= 63 && L.nodes.size() <= 64) build_replay_tree(L, U);
}

// Leaf BVHs (pt_leafbvh.cpp): every leaf of at least leaf_bvh entries (option; 0 = none).  The
// leaf's first record holds root + 1, its second the end of its nodes (Tri::lbvh).  The lean
// traversal's big-leaf step walks them (mailbox scenes: only with option mailbox=0, their default
// kernels test every entry once per ray anyway).
void build_leaf_chunks(Leaves& lv, long lmin, HostLayout& L) {
    if (lmin < 2) return;
    L.leaf_min = (int32_t)std::min<long>(lmin, INT32_MAX);
    std::sort(lv.ranges.begin(), lv.ranges.end());
    for (const auto& lr : lv.ranges) {
        if (lr.second < L.leaf_min || L.lidx.size() + (size_t)lr.second >= (1u << 24)) continue;
        int32_t root = 0, end = 0;
        const size_t slot0 = L.lidx.size();
        build_leaf_bvh(L.tris.data(), lr.first, lr.second, L.lnodes, L.lidx, root, end);
        for (size_t j = slot0; j < L.lidx.size(); ++j) {
            Tri t = L.tris[(size_t)(lr.first + L.lidx[j])];
            t.lbvh = L.lidx[j];
            L.ltris.push_back(t);
        }
        L.tris[(size_t)lr.first].lbvh = root + 1;
        L.tris[(size_t)lr.first + 1].lbvh = end;
        L.lleaves.push_back({lr.first, lr.second, end - root});
    }
    if (L.lleaves.empty()) L.leaf_min = 0;
}

// Leaves that k_wf_leafpass can resolve before the traversal: the kMaxPre largest, each with its
// path of child boxes from the root (node << 1 | side per step; PreLeaf), and their pass chunks
void build_pre_table(HostLayout& L) {
    std::vector<PreLeaf> all;
    // iterative pre-order walk keeping the path: (node, depth) frames, path[depth] = the step in
    std::vector<std::pair<int32_t, std::vector<int32_t>>> st;
    st.push_back({0, {}});
    bool deep = false;
    while (!st.empty()) {
        auto fr = std::move(st.back());
        st.pop_back();
        const Node& nd = L.nodes[(size_t)fr.first];
        for (int side = 1; side >= 0; --side) {
            const int32_t cnt = side ? nd.rcnt : nd.lcnt, ref = side ? nd.rref : nd.lref;
            std::vector<int32_t> p2 = fr.second;
            p2.push_back(fr.first << 1 | side);
            if (cnt >= 0) {
                if (cnt == 0) continue;
                L.leaf_sizes.push_back(cnt);
                if ((int)p2.size() > kMaxPrePath) { deep = true; continue; }
                PreLeaf pl{};
                pl.rec0 = ref;
                pl.n = cnt;
                pl.npath = (int32_t)p2.size();
                for (size_t k = 0; k < p2.size(); ++k) pl.path[k] = p2[k];
                all.push_back(pl);
            } else if (ref >= 0 && (size_t)ref < L.nodes.size()) {
                st.push_back({ref, std::move(p2)});
            }
        }
    }
    std::sort(L.leaf_sizes.begin(), L.leaf_sizes.end(), std::greater<int32_t>());
    std::sort(all.begin(), all.end(), [](const PreLeaf& a, const PreLeaf& b) { return a.n > b.n || (a.n == b.n && a.rec0 < b.rec0); });
    if (!deep) {  // (a leaf below kMaxPrePath steps could be among the largest: no table then)
        for (size_t k = 0; k < all.size() && k < (size_t)kMaxPre; ++k) L.pre.push_back(all[k]);
    }
    // the leaf pass's own chunks (kPassChunkMax entries) of the leaves that have traversal chunks
    std::vector<int32_t> plidx;
    for (PreLeaf& pl : L.pre) {
        pl.c0 = pl.c1 = 0;
        if (L.leaf_min <= 0 || pl.n < L.leaf_min || L.ptris.size() + (size_t)pl.n >= (1u << 24)) continue;
        const size_t slot0 = plidx.size();
        int32_t root = 0, end = 0;
        build_leaf_bvh(L.tris.data(), pl.rec0, pl.n, L.pnodes, plidx, root, end, nullptr, PT_PASS_LEAF, PT_PASS_MERGE);
        for (size_t j = slot0; j < plidx.size(); ++j) {
            Tri t = L.tris[(size_t)(pl.rec0 + plidx[j])];
            t.lbvh = plidx[j];
            L.ptris.push_back(t);
            // the entry's normal in double, rounded (the pass's check allows 1e-5 for it)
            const double e1[3] = {t.q0[3], t.q1[0], t.q1[1]}, e2[3] = {t.q1[2], t.q1[3], t.e2z};
            const double nv[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                                  e1[0] * e2[1] - e1[1] * e2[0]};
            const double ln = std::sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
            const bool ok = ln > 0.0 && std::isfinite(ln);
            L.pnorm.push_back(make_float4(ok ? (float)(nv[0] / ln) : 0.0f, ok ? (float)(nv[1] / ln) : 0.0f,
                                          ok ? (float)(nv[2] / ln) : 0.0f, 0.0f));
        }
        pl.c0 = root;
        pl.c1 = end;
    }
    // the pass's check takes A and B times 1.00001 (pt_leafpass.hip pass_box_skip), rounded up;
    // a degenerate chunk's FLT_MAX stays (its delta is never bounded)
    for (LNode& nd : L.pnodes) {
        auto up5 = [](float v) {
            return v >= FLT_MAX ? v : std::nextafter((float)((double)v * 1.00001), FLT_MAX);
        };
        nd.A = up5(nd.A);
        nd.B = up5(nd.B);
    }
}

// |det| = |e1 . (d x e2)| <= |e1| |e2| |d| with |d| = 1 (every ray direction is normalised or
// a reflection/refraction of unit vectors; non-finite ones give no hit on either path)
bool fast_rcp_holds(const std::vector<Tri>& tris) {
    double emax = 0.0;
    bool finite = true;
    for (const Tri& t : tris) {
        const double e1[3] = {t.q0[3], t.q1[0], t.q1[1]}, e2[3] = {t.q1[2], t.q1[3], t.e2z};
        const double a = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
        const double b = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        finite = finite && std::isfinite(a) && std::isfinite(b);
        emax = std::max(emax, a * b);
    }
    return finite && emax < std::ldexp(1.0, 124);
}

// Light table (intersection-logic.wgsl:217-285): entry k for k in [0, Ntri].
int build_lights(const Input& in, HostLayout& L, std::string& err) {
    const float* tri = in.tri;
    const Packed P{tri, in.tri_len};
    int32_t es[4], ee[4], n[4];
    int32_t ntri = 0;
    for (int s = 0; s < 4; ++s) {
        es[s] = wgsl_i32(tri[8 + 2 * s]);
        ee[s] = wgsl_i32(tri[9 + 2 * s]);
        n[s] = (es[s] != -1) ? (ee[s] - es[s]) / 4 : 0;
        ntri += n[s];
    }
    if (ntri <= 0) return fail(err, "scene has no emissive triangles (sample_area_lights needs one)");
    L.ntri = ntri;
    const int32_t vs = wgsl_i32(P.at(2));
    for (int32_t k = 0; k <= ntri; ++k) {
        int32_t idx;
        if (k < n[0]) idx = k * 4 + es[0];
        else if (k < n[0] + n[1]) idx = (k - n[0]) * 4 + es[1];
        else if (k < n[0] + n[1] + n[2]) idx = (k - n[0] - n[1]) * 4 + es[2];
        else idx = (k - n[0] - n[1] - n[2]) * 4 + es[3];
        Light lt{};
        float* dst[3] = {lt.p0, lt.p1, lt.p2};
        for (int j = 0; j < 3; ++j) {
            const int32_t i = (wgsl_i32(P.at(idx + j)) - 1) * 3;
            for (int c = 0; c < 3; ++c) dst[j][c] = P.at(vs + i + c);
        }
        L.lights.push_back(lt);
    }
    L.info.emissive_tris = (uint32_t)ntri;
    return PT_OK;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

int build_layout(const float* tri, size_t tri_len, const float* bvh, size_t bvh_len, const LayoutOptions& opt,
                 HostLayout& L, std::string& err) {
    if (tri_len < 16 || tri_len > (size_t)INT32_MAX) return fail(err, "triangle_data shorter than its 16-float header");
    if (bvh_len < 6 + 17 || bvh_len > (size_t)INT32_MAX) return fail(err, "bvh_data shorter than bounds + one node");
    const float nverts_f = tri[0], nobj_f = tri[1];
    if (!(nverts_f >= 0 && nverts_f == std::floor(nverts_f)) || !(nobj_f >= 1 && nobj_f == std::floor(nobj_f)))
        return fail(err, "bad vertex/object counts in triangle_data header");
    const Input in{tri, bvh, tri_len, bvh_len, (int64_t)nverts_f, (int64_t)nobj_f, wgsl_i32(tri[2]), wgsl_i32(tri[4])};
    if (in.v_start < 0 || in.v_start + 3 * in.nverts > (int64_t)tri_len) return fail(err, "vertex section out of range");
    if (in.m_start < 0 || in.m_start + 15 * in.nobj > (int64_t)tri_len) return fail(err, "material section out of range");
    L.info.vertices = (uint32_t)in.nverts;
    build_materials(in, L);
    Leaves lv;
    const int rc = decode_tree(in, L, lv, err);
    if (rc != PT_OK) return rc;
    build_mailbox(lv, opt.uid_reverse, L);
    build_leaf_chunks(lv, opt.leaf_bvh, L);
    build_pre_table(L);
    // Leaf remainders (pt_leafskip.cpp; option leaf_skip, read here and per render, default on):
    // scenes without mailbox (their kernels test every distinct entry once per ray anyway).  They
    // append records after the chunk fields above are set
    if (!L.mailbox && opt.leaf_skip)
        build_leaf_skips(L.nodes, L.tris, L.tnorm, L.lights, kLeafSkipMaxLeaf, kLeafSkipProbeTests, L.nalt, &L.skip);
    L.fast_rcp = fast_rcp_holds(L.tris);
    // The device stack parks at most one left child per internal ancestor.
    L.info.max_stack = lv.max_depth + 1;
    if (L.info.max_stack >= (uint32_t)kStackMax) return fail(err, "BVH deeper than the device traversal stack");
    return build_lights(in, L, err);
}

int build_mesh_tables(const float* tri, size_t tri_len, HostLayout& L, std::string& err) {
    if (tri_len < 16 || tri_len > (size_t)INT32_MAX) return fail(err, "triangle_data shorter than its 16-float header");
    const float nverts_f = tri[0], nobj_f = tri[1];
    if (!(nverts_f >= 0 && nverts_f == std::floor(nverts_f)) || !(nobj_f >= 1 && nobj_f == std::floor(nobj_f)))
        return fail(err, "bad vertex/object counts in triangle_data header");
    const Input in{tri, nullptr, tri_len, 0, (int64_t)nverts_f, (int64_t)nobj_f, wgsl_i32(tri[2]), wgsl_i32(tri[4])};
    if (in.v_start < 0 || in.v_start + 3 * in.nverts > (int64_t)tri_len) return fail(err, "vertex section out of range");
    if (in.m_start < 0 || in.m_start + 15 * in.nobj > (int64_t)tri_len) return fail(err, "material section out of range");
    L.info.vertices = (uint32_t)in.nverts;
    build_materials(in, L);
    return build_lights(in, L, err);
}

ScenePlan plan_sections(const HostLayout& L, size_t counters_bytes) {
    ScenePlan p{};
    size_t end = 0;  // the end of the section before, with its minimum size
    // n elements of v, room for at least min_n, starting on the next multiple of align
    auto put = [&](Section s, const auto& v, size_t min_n, size_t align) {
        const size_t elem = sizeof(v[0]);
        p.sec[s] = {v.data(), v.size() * elem, align_up(end, align)};
        end = p.sec[s].off + std::max(min_n, v.size()) * elem;
    };
    put(SEC_NODES, L.nodes, 0, 256);
    put(SEC_TRIS, L.tris, 1, 256);
    put(SEC_MATS, L.mats, 0, 256);
    put(SEC_LIGHTS, L.lights, 0, 256);
    put(SEC_LMASK, L.lmask, 0, 16);
    put(SEC_BFNODE, L.bfnode, 0, 16);
    put(SEC_BFMAP, L.bfmap, 0, 16);
    put(SEC_BFNARROW, L.bfnarrow, 0, 16);
    p.span_end = end;  // the LDS span ends here
    p.off_counters = align_up(end, 256);
    end = p.off_counters + counters_bytes;
    put(SEC_TNORM, L.tnorm, 1, 256);
    put(SEC_LNODES, L.lnodes, 0, 256);
    put(SEC_LTRIS, L.ltris, 1, 256);
    put(SEC_PNODES, L.pnodes, 1, 256);
    put(SEC_PTRIS, L.ptris, 1, 256);
    put(SEC_PNORM, L.pnorm, 1, 256);
    put(SEC_PRE, L.pre, 1, 256);
    put(SEC_NALT, L.nalt, 2, 256);
    p.total = align_up(end, 256);
    return p;
}

}  // namespace pt
