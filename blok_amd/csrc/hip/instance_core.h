// Instanced voxel models (include/blok_hip.h: blok_instance): the device math of the instance kernels (placed_kernels.hip over
// LatticeKind, at the end of this file) and of the path kernel's instance leaves (tlas_core.h).
//
// An instance places a model — its own 64-tree in its own local lattice — at a lattice offset with an axis-aligned orientation (a
// signed permutation of the axes).  Such a transform moves a ray into local space with ONE rounding per axis (the subtraction of the
// offset; a sign change and a permutation are exact), so the local walk is the canonical walk of trace_core.h on a transformed ray and
// the composed record is specified bit for bit:
//   o'_k = s_k * fl(o[axis[k]] - offset[axis[k]] * vs),   d'_k = s_k * d[axis[k]],   tmin, tmax unchanged      (s_k = flip bit k ? -1 : +1)
//   world voxel  w[axis[k]] = flip_k ? offset[axis[k]] - 1 - v'_k : offset[axis[k]] + v'_k;   face 2k + n -> 2 axis[k] + (n ^ flip_k)
// A model carries a scale exponent e (ModelDesc::scale_log2, 0 .. kMaxScaleLog2): one model voxel is a cube of 2^e world voxels.  The ray
// above is unchanged (the offset stays in world voxels); the walk and the local box test take the model's voxel size vm = vs * 2^e and
// 1 / vm, both exact powers of two; t, material and face are unchanged, and the record's voxel is the cell's lowest world voxel:
//   w[axis[k]] = flip_k ? offset[axis[k]] - (v'_k + 1) * 2^e : offset[axis[k]] + v'_k * 2^e
// The shift happens once, in instance_record; the walk never sees it.
// Candidates are taken world first, then instance 0, 1, ...; one replaces the record only with a strictly smaller t, which is what a
// walk with tmax = the best t so far does (the walk's acceptance test is t < tmax).
//
// tests/test_instances_cpu.py compiles this header with trace_core.h for the host (BLOK_TRACE_HOST_HARNESS) through its own shim.
#ifndef BLOK_INSTANCE_CORE_H
#define BLOK_INSTANCE_CORE_H

#include "trace_core.h"
#include "../common/stamp_core.h"

// The limits are checked by the host entries too.
#ifdef BLOK_TRACE_HOST_HARNESS
#define BLOK_HD inline
#else
#define BLOK_HD __host__ __device__ __forceinline__
#endif

namespace blok {

// A model as the kernels see it: its tree (tree.h) and the box of its filled voxels [lo, hi) in WORLD voxels from an instance's offset:
// the model's box in its own voxels times 2^e, scaled once by the store (api_instances.hip), so that an instance's span is an add and the
// local box test is [lo, hi) * vs whatever the scale.  nodes == null: a model no instance of which is traced (any is skipped) — a
// destroyed one, or, in the store's device copy, one whose voxel size vs * 2^e is above kMaxModelVoxelSize in the installed world.
struct ModelDesc {
    const uint4*    nodes;
    const uint32_t* materials;
    uint32_t levels;
    int32_t  origin[3];
    int32_t  lo[3], hi[3];
    uint32_t scale_log2;             // e: one model voxel is 2^e world voxels on a side (zero-initialised: scale 1).  The store keeps
                                     // e <= kMaxScaleLog2 (blok_hip_model_set_scale refuses more)
    uint32_t reserved;               // (the arrays' lengths live on the host side of the store: the kernels never read them)
};
static_assert(sizeof(ModelDesc) == 64, "one model descriptor is 64 bytes");
static_assert(sizeof(blok_instance) == 32, "one instance record is 32 bytes");

constexpr uint32_t kInstanceNone = 0xFFFFFFFFu;
// A hit record's voxel is int16: every instance's world box must lie in [kLatticeMin, kLatticeMax) on every axis.
constexpr int64_t kLatticeMin = -32768, kLatticeMax = 32768;
// The largest scale exponent of a model, and the largest voxel size a model may be walked at (vs * 2^e; the walk is exact up to it).
constexpr uint32_t kMaxScaleLog2 = 8;
constexpr float kMaxModelVoxelSize = 256.0f;

// Component `a` (0, 1, 2) of a triple, by selects: the permutation is data, and an array indexed by it would live in scratch.
BLOK_HD float pick3(uint32_t a, float x, float y, float z) { return a == 0u ? x : (a == 1u ? y : z); }
BLOK_HD int32_t pick3(uint32_t a, int32_t x, int32_t y, int32_t z) { return a == 0u ? x : (a == 1u ? y : z); }
// The local axis k with axis[k] == a.
BLOK_HD uint32_t local_axis(const blok_instance& I, uint32_t a) { return I.axis[0] == a ? 0u : (I.axis[1] == a ? 1u : 2u); }

// The model's voxel size vm = vs * 2^e and its inverse from the world's: vs is a power of two, so adding e to the exponent field is the
// exact product, in integer arithmetic (scalar registers where M and vs are wave-uniform).  e <= kMaxScaleLog2 (the store's invariant).
BLOK_HD float model_voxel_size(const ModelDesc& M, float vs) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, vs) + (M.scale_log2 << 23));
}
BLOK_HD float model_inv_voxel_size(const ModelDesc& M, float inv_vs) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, inv_vs) - (M.scale_log2 << 23));
}

// The instance's world box in world voxels along world axis a: [lo, hi)  (the descriptor's box is in world voxels already).
BLOK_HD void instance_world_span(const blok_instance& I, const ModelDesc& M, uint32_t a, int64_t& lo, int64_t& hi) {
    const uint32_t k = local_axis(I, a);
    const int64_t o = pick3(a, I.offset[0], I.offset[1], I.offset[2]);
    const int64_t mlo = pick3(k, M.lo[0], M.lo[1], M.lo[2]), mhi = pick3(k, M.hi[0], M.hi[1], M.hi[2]);
    const bool f = (I.flip >> k) & 1u;
    lo = f ? o - mhi : o + mlo;
    hi = f ? o - mlo : o + mhi;
}

// The record itself is well formed: axis a permutation of 0, 1, 2, only the three flip bits, reserved words zero.
BLOK_HD bool instance_well_formed(const blok_instance& I) { return stamp::well_formed(I); }

// Everything the blocking entries check, for the kernels (an instance of the device entries that fails it is skipped).
BLOK_HD bool instance_usable(const blok_instance& I, const ModelDesc& M) {
    if (!instance_well_formed(I) || !M.nodes) return false;
    for (uint32_t a = 0; a < 3u; ++a) {
        int64_t lo, hi;
        instance_world_span(I, M, a, lo, hi);
        if (lo < kLatticeMin || hi > kLatticeMax) return false;
    }
    return true;
}

// The limit of a model's voxel size in a world of voxel size vs.  It is a property of the model and the world, not of an instance: the
// host entries ask it per table entry for their messages, and the store asks it once per model when it writes the device copy of the
// descriptors (nodes = null where it fails), so the kernels' instance_usable above needs no more than it did before models had a scale.
BLOK_HD bool model_size_usable(const ModelDesc& M, float vs) { return model_voxel_size(M, vs) <= kMaxModelVoxelSize; }

// The ray in the model's local space (one rounding per axis: the subtraction).  vs: the world's voxel size.
BLOK_DEV float local_origin(const blok_instance& I, float vs, const RayIn& r, uint32_t k) {
    const uint32_t a = I.axis[k];
    // offset * vs: exact (|offset| <= 2^16, vs a power of two)
    const float rel = rn_sub(pick3(a, r.ox, r.oy, r.oz), rn_mul(static_cast<float>(pick3(a, I.offset[0], I.offset[1], I.offset[2])), vs));
    return ((I.flip >> k) & 1u) ? -rel : rel;
}
BLOK_DEV float local_dir(const blok_instance& I, const RayIn& r, uint32_t k) {
    const float d = pick3(I.axis[k], r.dx, r.dy, r.dz);
    return ((I.flip >> k) & 1u) ? -d : d;
}
BLOK_DEV RayIn instance_ray(const blok_instance& I, float vs, const RayIn& r) {
    RayIn t;
    t.ox = local_origin(I, vs, r, 0u); t.oy = local_origin(I, vs, r, 1u); t.oz = local_origin(I, vs, r, 2u);
    t.dx = local_dir(I, r, 0u); t.dy = local_dir(I, r, 1u); t.dz = local_dir(I, r, 2u);
    t.tmin = r.tmin; t.tmax = r.tmax;
    return t;
}

// Does the local ray's interval [tmin, tmax) meet the model's box [lo, hi) * vs (world voxels; the same planes as the model's own box
// times vm = vs * 2^e, bit for bit: a power of two moves from one factor to the other exactly)?  The planes' T are the walk's own formula
// (trace_kernels.h: T = fl(fl(p - o) * inv)), and every voxel's planes lie between the box planes, so a reported voxel's interval is
// inside the box's: the test never rejects a ray the walk would report a voxel for.
BLOK_DEV void box_axis(int32_t lo, int32_t hi, float vs, float o, float d, float& enter, float& leave) {
    const float inv = safe_inv(d);
    const float t0 = rn_mul(rn_sub(rn_mul(static_cast<float>(lo), vs), o), inv);
    const float t1 = rn_mul(rn_sub(rn_mul(static_cast<float>(hi), vs), o), inv);
    enter = fmaxf(enter, fminf(t0, t1));
    leave = fminf(leave, fmaxf(t0, t1));
}
BLOK_DEV bool instance_box_entered(const ModelDesc& M, float vs, const RayIn& r) {
    float enter = r.tmin, leave = r.tmax;
    box_axis(M.lo[0], M.hi[0], vs, r.ox, r.dx, enter, leave);
    box_axis(M.lo[1], M.hi[1], vs, r.oy, r.dy, enter, leave);
    box_axis(M.lo[2], M.hi[2], vs, r.oz, r.dz, enter, leave);
    return enter < leave;
}

// The walk's arguments for a model in a world of voxel size vs (the model's own voxel size and material table; no camera, no outputs).
BLOK_DEV TraceArgs model_args(const ModelDesc& M, float vs, float inv_vs) {
    TraceArgs a{};
    a.nodes = M.nodes;
    a.materials = M.materials;
    a.origin[0] = M.origin[0]; a.origin[1] = M.origin[1]; a.origin[2] = M.origin[2];
    a.levels = M.levels;
    a.voxel_size = model_voxel_size(M, vs); a.inv_voxel_size = model_inv_voxel_size(M, inv_vs);
    return a;
}

// A local hit as a world record (the 16-byte blok_hit layout, trace_core.h: trace_one).  e: the model's scale exponent; the voxel is the
// hit cell's lowest world voxel.  The record keeps its low 16 bits, and those of the wrapping 32-bit sum here are those of the exact
// (64-bit) sum of the rule; a usable instance's cells all lie in the int16 lattice, so nothing is lost.
BLOK_DEV int32_t world_voxel(const blok_instance& I, const HitInfo& h, uint32_t a, uint32_t e) {
    const uint32_t k = local_axis(I, a);
    const uint32_t v = static_cast<uint32_t>(pick3(k, h.vx, h.vy, h.vz)), o = static_cast<uint32_t>(pick3(a, I.offset[0], I.offset[1], I.offset[2]));
    return static_cast<int32_t>(((I.flip >> k) & 1u) ? o - ((v + 1u) << e) : o + (v << e));
}
BLOK_DEV uint4 instance_record(const blok_instance& I, const HitInfo& h, uint32_t e) {
    const uint32_t fk = h.face >> 1, fn = h.face & 1u;
    const uint32_t face = 2u * pick3(fk, int32_t(I.axis[0]), int32_t(I.axis[1]), int32_t(I.axis[2])) + (fn ^ ((I.flip >> fk) & 1u));
    uint4 rec;
    rec.x = __float_as_uint(h.t);
    rec.y = h.material;
    rec.z = (static_cast<uint32_t>(world_voxel(I, h, 0u, e)) & 0xFFFFu) | (static_cast<uint32_t>(world_voxel(I, h, 1u, e)) << 16);
    rec.w = (static_cast<uint32_t>(world_voxel(I, h, 2u, e)) & 0xFFFFu) | (face << 16) | (1u << 24);
    return rec;
}
#ifdef BLOK_TRACE_HOST_HARNESS
// (for the host shims that map records of scale-0 models; device code always says which scale)
inline uint4 instance_record(const blok_instance& I, const HitInfo& h) { return instance_record(I, h, 0u); }
#endif

// One candidate of the path kernel's leaves (tlas_core.h): the instance's walk of world ray r with tmax = best_t.  true (and rec) iff it
// reports a voxel, whose t is then < best_t.  (The primary frame's candidate, with its wave-uniform descriptor, is placed_candidate below.)
BLOK_DEV bool instance_candidate(const blok_instance& I, const ModelDesc& M, float vs, float inv_vs, const RayIn& r, float best_t,
                                 uint4* stk, uint4& rec) {
    RayIn l = instance_ray(I, vs, r);
    l.tmax = best_t;
    if (!instance_box_entered(M, vs, l)) return false;
    // walk() of trace_core.h, piece by piece.  Here the descriptor is per lane (the path kernel's leaves), so vm would be a vector value alive
    // across the walk's loop beside the exponent; the loop itself does not read it, so it is formed again from the exponent behind the loop,
    // for the hit's face — the exponent is then the one value a scaled model keeps alive where a scale-0 model kept none.
    BLOK_STAT(4, 0);                       // a walk begins
    TraceArgs a = model_args(M, vs, inv_vs);
    const WalkRay R = walk_ray(a, l.ox, l.oy, l.oz, safe_inv(l.dx), safe_inv(l.dy), safe_inv(l.dz));
    WalkState s;
    walk_enter(a, R, l.tmin, l.tmax, s);
    walk_loop(a, R, l.tmax, s, stk);
    if (!s.found) return false;
    const uint32_t e = as_written(M.scale_log2);
    a.voxel_size = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, vs) + (e << 23));
    rec = instance_record(I, walk_hit(a, l, R, s), e);
    return true;
}

// ---- screen bins (binning kernel) -----------------------------------------------------------------------------------------------
// Where a world point lands on screen: the solution of  p - pos = lambda fwd + mu right + nu up  (the camera basis need not be orthonormal)
// is lambda = dot(p - pos, cl), mu = dot(p - pos, cu), nu = dot(p - pos, cv) with the rows of the basis' inverse; the pixel of
// (u, v) = (mu, nu) / lambda inverts camera_plane_uv (trace_core.h).
struct BinView {
    float pos[3], cl[3], cu[3], cv[3];
    float sx, bx, sy, by;        // pixel x = u * sx + bx, pixel y = v * sy + by (pixel index space: pixel i's centre at i)
    uint32_t usable;             // 0: the basis is degenerate, every instance covers every bin
};

// The pixel rectangle [x0, x1] x [y0, y1] (inclusive, frame pixels, with a 1-pixel margin) that a world box [lo, hi) * vs may cover;
// false: some corner is at or behind the camera plane (the box may cover anything).
BLOK_DEV bool project_box(const BinView& V, const float lo[3], const float hi[3], float& x0, float& y0, float& x1, float& y1) {
    x0 = y0 = 3.0e38f; x1 = y1 = -3.0e38f;
    for (int c = 0; c < 8; ++c) {
        const float px = ((c & 1) ? hi[0] : lo[0]) - V.pos[0];
        const float py = ((c & 2) ? hi[1] : lo[1]) - V.pos[1];
        const float pz = ((c & 4) ? hi[2] : lo[2]) - V.pos[2];
        const float l = px * V.cl[0] + py * V.cl[1] + pz * V.cl[2];
        const float len = fabsf(px) + fabsf(py) + fabsf(pz);
        if (!(l > 1e-5f * len)) return false;               // at, behind or next to the camera plane (NaN included)
        const float inv = 1.0f / l;
        const float u = (px * V.cu[0] + py * V.cu[1] + pz * V.cu[2]) * inv;
        const float v = (px * V.cv[0] + py * V.cv[1] + pz * V.cv[2]) * inv;
        const float x = u * V.sx + V.bx, y = v * V.sy + V.by;
        x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    x0 -= 1.0f; y0 -= 1.0f; x1 += 1.0f; y1 += 1.0f;        // the margin: rounding of both the rays and this projection stays far below a pixel
    return true;
}

// Arguments of the three instance kernels (placed_kernels.hip).  Bins: one per kBinPixels x kBinPixels pixels of the launch rectangle,
// kBinWords words each: word 0 = the number of instances listed (kBinOverflow: more than kBinCapacity, the bin's pixels test every
// instance), then the instance indices in ascending order.
constexpr uint32_t kBinPixels = 32, kBinWords = 64, kBinCapacity = kBinWords - 1, kBinOverflow = 0xFFFFFFFFu;
struct InstanceArgs {
    TraceArgs world;                     // camera, frame and rectangle, material table, voxel size, tmin / tmax; rays / n_rays (rays kernel)
    const blok_instance* instances;      // device memory, n_instances records
    uint32_t n_instances;
    const ModelDesc* models;             // the context's model store
    uint32_t n_models;
    uint32_t* bins;                      // bins_x * bins_y bins of kBinWords words (per-stream scratch)
    uint32_t bins_x, bins_y;
    BinView view;
    blok_hit* hits;                      // the world pass's records in, the composed records out (never null)
    uint32_t* rgba;                      // may be null: RGBA8 of the pixels an instance won (the world pass wrote the others)
    uint32_t* ids;                       // may be null: the winning instance per pixel / ray, kInstanceNone for the world or a miss
    uint32_t stack_levels;               // LDS stack slots per lane: the deepest live model's levels - 1 (>= 1)
};

// ---- placed models: what the lattice instances and the poses (posed_core.h) share ------------------------------------------------------------
// Both place a model's own tree in the world, take a world ray into the model's local space, walk it there with tmax = the best t so far
// and compose the record; the kernels (placed_kernels.hip) and the host shims (tests/host_harness) state that once, over a KIND.
// A kind is a struct of static functions holding the six things in which the two differ, and nothing else:
//   1. Record / Args, table, count, frame   the record type and where its table lives in the kernels' arguments
//   2. usable                               what the kernels make of a record and its model (the others are skipped)
//   3. local_ray                            world ray -> local ray; false: the ray does not enter (a non-finite component)
//   4. world_box                            the world box the screen bins project; false: the record may cover anything
//   5. Hit, record                          a local hit as the composed record, and the world face shade_rgba takes for it
//   6. owns_ids, id_tag                     who owns the id plane: the lattice pass writes every pixel it visits (kInstanceNone where no
//                                           instance wins), the posed pass only the pixels a pose wins, as BLOK_POSE_ID | index
// Each kind stands behind its own math: LatticeKind here, PoseKind in posed_core.h.
struct LatticeKind {
    using Record = blok_instance;
    using Args = InstanceArgs;
    static BLOK_DEV const InstanceArgs& frame(const Args& a) { return a; }
    static BLOK_DEV const Record* table(const Args& a) { return a.instances; }
    static BLOK_DEV uint32_t count(const Args& a) { return a.n_instances; }
    static BLOK_DEV bool usable(const Record& I, const ModelDesc& M) { return instance_usable(I, M); }
    static BLOK_DEV bool local_ray(const Record& I, float vs, const RayIn& r, RayIn& l) { l = instance_ray(I, vs, r); return true; }
    static BLOK_DEV bool world_box(const Record& I, const ModelDesc& M, float vs, const float*, float flo[3], float fhi[3]) {
        for (uint32_t a = 0; a < 3u; ++a) {
            int64_t lo, hi;
            instance_world_span(I, M, a, lo, hi);
            flo[a] = static_cast<float>(lo) * vs; fhi[a] = static_cast<float>(hi) * vs;
        }
        return true;
    }
    struct Hit {
        uint4 rec{};
        BLOK_DEV uint32_t shade_face() const { return (rec.w >> 16) & 0xFFu; }       // the record's face is a world face
    };
    static BLOK_DEV Hit record(const Record& I, const ModelDesc& M, const HitInfo& h) { return Hit{instance_record(I, h, M.scale_log2)}; }
    static constexpr bool owns_ids = true;
    static constexpr uint32_t id_tag = 0u;
};

// One candidate on the host: the record's walk of world ray r with tmax = best_t; true iff it reports a voxel, whose t is then < best_t
// (hit and best_t are then the candidate's).  The body of the kernels' loop (placed_kernels.hip: compose) from the same kind functions,
// without the wave: there a candidate that no lane's ray enters is skipped by one ballot, and that skip is all the host does not run.
template <class K>
BLOK_DEV bool placed_candidate(const typename K::Record& S, const ModelDesc& M, float vs, float inv_vs, const RayIn& r, float& best_t, uint4* stk,
                               typename K::Hit& hit) {
    RayIn l;
    const bool finite = K::local_ray(S, vs, r, l);
    l.tmax = best_t;
    if (!finite || !instance_box_entered(M, vs, l)) return false;
    const HitInfo h = walk(model_args(M, vs, inv_vs), l, stk);
    if (!h.found) return false;
    hit = K::record(S, M, h);
    best_t = h.t;
    return true;
}

#ifndef BLOK_TRACE_HOST_HARNESS
void launch_instance_bins(const InstanceArgs& args, hipStream_t stream);
void launch_instance_pass(const InstanceArgs& args, hipStream_t stream);
void launch_instance_rays(const InstanceArgs& args, hipStream_t stream);
#endif

}  // namespace blok
#endif
