// The instance BVH ("TLAS") of the instanced path tracer ("Path-traced instances"): layout, build steps and stackless
// traversal.  Host-compilable like instance_core.h: tests/host_harness/tlas_shim.cpp runs the build steps serially and the traversal per
// ray; the build kernel (trace_kernels.hip: tlas_build_kernel) runs the same steps in parallel in one workgroup.
//
// Layout.  A complete binary tree in heap order over the usable instances sorted by the Morton code of their world box centre:
//   node 0 is a header, node 1 the root, node k's children 2k and 2k + 1, the leaves P .. 2P - 1 (P = the table's slot count, the
//   next power of two >= n_instances).  Leaf P + j holds the j-th instance of the sorted order; leaves past the usable count are empty.
//   Every node is 32 bytes: an int32 box [lo, hi) in world voxels, then `child` (an internal node: 2k; a leaf: kTlasLeaf | instance
//   index; an empty leaf or a node over empty leaves only: kTlasEmpty) and `escape` (the node a depth-first walk visits after this node's subtree, 0 = the end).
// Boxes.  A leaf's box is its instance's world box (instance_world_span: world voxels, whatever the model's scale) grown by kTlasPad voxels on every side; a parent's box is the
//   union of its children's.  The world-space slab test of a node therefore rejects only rays that no leaf below could report: the
//   walk reports voxels in the model's local space, whose origin rounds differently, and one voxel of padding covers that by orders of
//   magnitude.  A leaf then takes the exact local test (instance_box_entered, inside instance_candidate).
// Order of the result.  Leaves are visited in box order, not index order; closest() still returns the composition rule's answer
//   (instance_core.h: world first, a strictly smaller t wins, ties to the lowest index): an instance below the current winner walks with
//   tmax = nextafter(best_t, +inf) and wins on t < best_t or t == best_t, any other walks with tmax = best_t and wins on t < best_t.
//   A walk with a larger tmax reports the same first voxel whenever that voxel's t is below the smaller one, so each candidate sees what
//   the linear loop would have shown it.
#ifndef BLOK_TLAS_CORE_H
#define BLOK_TLAS_CORE_H

#include "instance_core.h"

#ifdef BLOK_TRACE_HOST_HARNESS
#include <algorithm>
#include <cmath>
#include <vector>
#endif

namespace blok {

constexpr uint32_t kTlasMax = 4096;                 // instances one workgroup sorts in LDS; above it every query takes the linear loop
constexpr uint32_t kTlasLeaf = 0x80000000u, kTlasEmpty = 0xFFFFFFFFu;
constexpr int32_t kTlasPad = 1;
constexpr uint32_t kTlasBuildThreads = 1024;

struct TlasNode {
    int32_t lo[3], hi[3];
    uint32_t child, escape;
};
static_assert(sizeof(TlasNode) == 32, "one TLAS node is 32 bytes");

// Slot count of a table of n instances (a power of two, >= 1), and the node count including the header.
BLOK_HD uint32_t tlas_slots(uint32_t n) { uint32_t p = 1u; while (p < n) p <<= 1; return p; }
BLOK_HD uint32_t tlas_nodes(uint32_t n) { return 2u * tlas_slots(n); }

// Morton code of an instance's world box centre on the fixed int16 lattice: lo + hi lies in [-65536, 65536]; 10 bits per axis.
BLOK_HD uint32_t tlas_spread10(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// The sort key of instance i: (Morton << 32) | i for a usable instance, (0xFFFFFFFF << 32) | i for one that is not (sorted last).
BLOK_HD uint64_t tlas_key(const blok_instance* inst, const ModelDesc* models, uint32_t n_models, uint32_t i) {
    const blok_instance I = inst[i];
    if (I.model >= n_models || !instance_usable(I, models[I.model])) return (0xFFFFFFFFull << 32) | i;
    const ModelDesc M = models[I.model];
    uint32_t code = 0u;
    for (uint32_t a = 0; a < 3u; ++a) {
        int64_t lo, hi;
        instance_world_span(I, M, a, lo, hi);
        const uint32_t c = static_cast<uint32_t>((lo + hi + 65536) >> 7);     // [0, 1024]
        code |= tlas_spread10(c > 1023u ? 1023u : c) << a;
    }
    return (static_cast<uint64_t>(code) << 32) | i;
}
BLOK_HD bool tlas_key_usable(uint64_t key) { return (key >> 32) != 0xFFFFFFFFull; }

// The escape link of heap node k (1 <= k): strip k's trailing one bits (the subtrees it closes), step to the right sibling; 1 = the root = the end.
BLOK_HD uint32_t tlas_escape(uint32_t k) {
    uint32_t e = k;
    while (e & 1u) e >>= 1;
    e += 1u;
    return e == 1u ? 0u : e;
}

BLOK_HD TlasNode tlas_empty_node(uint32_t k, uint32_t child) {
    TlasNode nd;
    for (int a = 0; a < 3; ++a) { nd.lo[a] = 0x7FFFFFFF; nd.hi[a] = static_cast<int32_t>(0x80000000u); }
    nd.child = child; nd.escape = tlas_escape(k);
    return nd;
}
// Leaf P + j from the j-th sorted key.
BLOK_HD TlasNode tlas_leaf(const blok_instance* inst, const ModelDesc* models, uint32_t slots, uint32_t j, uint64_t key) {
    const uint32_t k = slots + j;
    if (!tlas_key_usable(key)) return tlas_empty_node(k, kTlasEmpty);
    const uint32_t i = static_cast<uint32_t>(key);
    const blok_instance I = inst[i];
    const ModelDesc M = models[I.model];
    TlasNode nd;
    for (uint32_t a = 0; a < 3u; ++a) {
        int64_t lo, hi;
        instance_world_span(I, M, a, lo, hi);
        nd.lo[a] = static_cast<int32_t>(lo) - kTlasPad; nd.hi[a] = static_cast<int32_t>(hi) + kTlasPad;
    }
    nd.child = kTlasLeaf | i; nd.escape = tlas_escape(k);
    return nd;
}
// Internal node k from its two children (the refit).  A node over no usable leaf is empty like an empty leaf (kTlasEmpty): its inverted
// box would pass the slab test (fminf / fmaxf of its planes), and the traversal skips it by `child` alone.
BLOK_HD TlasNode tlas_internal(uint32_t k, const TlasNode& l, const TlasNode& r) {
    TlasNode nd;
    for (int a = 0; a < 3; ++a) { nd.lo[a] = l.lo[a] < r.lo[a] ? l.lo[a] : r.lo[a]; nd.hi[a] = l.hi[a] > r.hi[a] ? l.hi[a] : r.hi[a]; }
    nd.child = (l.child == kTlasEmpty && r.child == kTlasEmpty) ? kTlasEmpty : 2u * k; nd.escape = tlas_escape(k);
    return nd;
}
// The header: slot count, usable instances.
BLOK_HD TlasNode tlas_header(uint32_t slots, uint32_t usable) {
    TlasNode nd{};
    nd.child = slots; nd.escape = usable;
    return nd;
}

#ifdef BLOK_TRACE_HOST_HARNESS
// The serial build: keys, sort, leaves, refit, header.  out: tlas_nodes(n) nodes.  n <= kTlasMax.
inline void tlas_build_host(const blok_instance* inst, uint32_t n, const ModelDesc* models, uint32_t n_models, TlasNode* out) {
    const uint32_t P = tlas_slots(n);
    std::vector<uint64_t> keys(P, ~0ull);
    for (uint32_t i = 0; i < n; ++i) keys[i] = tlas_key(inst, models, n_models, i);
    std::sort(keys.begin(), keys.end());           // keys are distinct (they hold the index): any sort is the stable sort
    uint32_t usable = 0;
    for (uint32_t j = 0; j < P; ++j) { out[P + j] = tlas_leaf(inst, models, P, j, keys[j]); usable += tlas_key_usable(keys[j]) ? 1u : 0u; }
    for (uint32_t k = P - 1u; k >= 1u; --k) out[k] = tlas_internal(k, out[2u * k], out[2u * k + 1u]);
    out[0] = tlas_header(P, usable);
}
#endif

// ---- traversal ------------------------------------------------------------------------------------------------------------------
// Everything the path kernel needs of the instances: the table, the model store, the tree (null: the linear loop) and the id plane.
struct TlasScene {
    const blok_instance* instances;
    const ModelDesc* models;
    const TlasNode* nodes;
    uint32_t* ids;                   // may be null: the winning instance of each pixel's first hit
    uint32_t n_instances, n_models;
};

// The world-space slab test of a node's box against [tmin, tmax) (the formula of instance_box_entered, on the padded world box).
BLOK_DEV bool tlas_box_hit(const TlasNode& nd, float vs, const RayIn& r, float ix, float iy, float iz, float tmax) {
    float enter = r.tmin, leave = tmax;
    const auto axis = [&](int32_t lo, int32_t hi, float o, float inv) {
        const float t0 = rn_mul(rn_sub(rn_mul(static_cast<float>(lo), vs), o), inv);
        const float t1 = rn_mul(rn_sub(rn_mul(static_cast<float>(hi), vs), o), inv);
        enter = fmaxf(enter, fminf(t0, t1));
        leave = fminf(leave, fmaxf(t0, t1));
    };
    axis(nd.lo[0], nd.hi[0], r.ox, ix);
    axis(nd.lo[1], nd.hi[1], r.oy, iy);
    axis(nd.lo[2], nd.hi[2], r.oz, iz);
    return enter < leave;
}

// One leaf's candidate under the ordering rule above; best_t / best_id / rec updated when it wins.
BLOK_DEV void tlas_leaf_candidate(const TlasScene& S, float vs, float inv_vs, const RayIn& r, uint32_t i, uint4* stk,
                                  float& best_t, uint32_t& best_id, uint4& rec) {
    const blok_instance I = S.instances[i];
    if (I.model >= S.n_models) return;
    const ModelDesc M = S.models[I.model];
    if (!instance_usable(I, M)) return;
    const bool below = best_id != kInstanceNone && i < best_id;        // (the world, best_id == none, wins every tie)
    const float tmax = below ? nextafterf(best_t, 3.0e38f) : best_t;
    uint4 c;
    if (!instance_candidate(I, M, vs, inv_vs, r, tmax, stk, c)) return;
    const float t = __uint_as_float(c.x);
    if (t < best_t || (below && t == best_t)) { rec = c; best_t = t; best_id = i; }
}

// Closest hit of world ray r over the instances, given the world's answer: best_t = the world hit's t (or r's tmax on a miss), best_id =
// kInstanceNone.  Returns the winning instance (rec = its composed record) or kInstanceNone.
BLOK_DEV uint32_t tlas_closest(const TlasScene& S, float vs, float inv_vs, const RayIn& r, float best_t, uint4* stk, uint4& rec) {
    uint32_t best_id = kInstanceNone;
    if (S.nodes == nullptr) {                                            // above kTlasMax: the linear loop, index order
        for (uint32_t i = 0; i < S.n_instances; ++i) tlas_leaf_candidate(S, vs, inv_vs, r, i, stk, best_t, best_id, rec);
        return best_id;
    }
    const float ix = safe_inv(r.dx), iy = safe_inv(r.dy), iz = safe_inv(r.dz);
    uint32_t k = 1u;
    while (k != 0u) {
        const TlasNode nd = S.nodes[k];
        // a tie of a lower index may still replace the current winner: test the box up to just past best_t
        const float tmax = best_id != kInstanceNone ? nextafterf(best_t, 3.0e38f) : best_t;
        if (nd.child != kTlasEmpty && tlas_box_hit(nd, vs, r, ix, iy, iz, tmax)) {
            if (nd.child & kTlasLeaf) {
                tlas_leaf_candidate(S, vs, inv_vs, r, nd.child & ~kTlasLeaf, stk, best_t, best_id, rec);
                k = nd.escape;
            } else k = nd.child;
        } else k = nd.escape;
    }
    return best_id;
}

// Any hit of r in [r.tmin, r.tmax) over the instances (shadow rays).
BLOK_DEV bool tlas_any(const TlasScene& S, float vs, float inv_vs, const RayIn& r, uint4* stk) {
    uint4 rec;
    const auto usable_hit = [&](uint32_t i) {
        const blok_instance I = S.instances[i];
        if (I.model >= S.n_models) return false;
        const ModelDesc M = S.models[I.model];
        return instance_usable(I, M) && instance_candidate(I, M, vs, inv_vs, r, r.tmax, stk, rec);
    };
    if (S.nodes == nullptr) {
        for (uint32_t i = 0; i < S.n_instances; ++i) if (usable_hit(i)) return true;
        return false;
    }
    const float ix = safe_inv(r.dx), iy = safe_inv(r.dy), iz = safe_inv(r.dz);
    uint32_t k = 1u;
    while (k != 0u) {
        const TlasNode nd = S.nodes[k];
        if (nd.child != kTlasEmpty && tlas_box_hit(nd, vs, r, ix, iy, iz, r.tmax)) {
            if (nd.child & kTlasLeaf) {
                if (usable_hit(nd.child & ~kTlasLeaf)) return true;
                k = nd.escape;
            } else k = nd.child;
        } else k = nd.escape;
    }
    return false;
}

#ifndef BLOK_TRACE_HOST_HARNESS
// Builds the tree of n <= kTlasMax instances into nodes (tlas_nodes(n) of them) on the stream: one workgroup, no host synchronise.
void launch_tlas_build(const blok_instance* instances, uint32_t n, const ModelDesc* models, uint32_t n_models, TlasNode* nodes, hipStream_t stream);
#endif

}  // namespace blok
#endif
