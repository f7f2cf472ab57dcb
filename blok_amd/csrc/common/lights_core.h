// Emissive voxels as lights: what the host build (host/lights.cpp), the table kernels (hip/lights_kernels.hip) and the lit path loop
// (hip/path_core.h: shade_pixel<…, kLit>) share.  include/blok_hip.h has the contract ("Emissive voxels as lights"); DESIGN.md §32 the rule.
// The table part is integer arithmetic; the sample part is float, every operation rounded separately (no contraction).
#ifndef BLOK_LIGHTS_CORE_H
#define BLOK_LIGHTS_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_LD __host__ __device__ inline
#else
#define BLOK_LD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace blok {
namespace lights {

constexpr uint32_t kSetBits = 65536u, kSetWords = kSetBits / 32u;      // a set of material indices: one bit each
constexpr float kLightEps = 0.004f;                                     // twice the bounce ray's offset: what a light's shadow ray stops short of

// The index a material id reads the material table at (path_core.h, hit.rchit): ids above 65535 read 65535, ids beyond the table read 0.
BLOK_LD uint32_t material_index(uint32_t id, uint32_t n_materials) {
    const uint32_t c = id < 65535u ? id : 65535u;
    return c < n_materials ? c : 0u;
}
// raygen.rgen:158-160 (path_core.h: is_emissive): dot(e, 1) > 0.01, summed left to right.
BLOK_LD bool emissive(const float e[3]) { return ((e[0] * 1.0f + e[1] * 1.0f) + e[2] * 1.0f) > 0.01f; }
BLOK_LD bool in_set(const uint32_t* set, uint32_t i) { return (set[i >> 5] >> (i & 31u)) & 1u; }
// A quad becomes a light iff the material its key maps to glows (`glows`: the set of emissive material indices).
BLOK_LD bool keeps(uint32_t material, const uint32_t* glows, uint32_t n_materials) { return in_set(glows, material_index(material, n_materials)); }

// The set of emissive indices of a material table (host; one evaluation per material).
inline void emissive_set(const blok_material* materials, size_t n_materials, uint32_t* set) {
    for (uint32_t w = 0; w < kSetWords; ++w) set[w] = 0u;
    const size_t n = n_materials < kSetBits ? n_materials : kSetBits;
    for (size_t m = 0; m < n; ++m) if (emissive(materials[m].emission)) set[m >> 5] |= 1u << (m & 31u);
}

// The rules blok_hip_set_lights holds a host table to.  0: fine (then *out_faces = A); else the rule that light *out_index breaks:
// 1 face > 5, 2 du or dv 0, 3 cum is not the running sum, 4 (unsupported) A >= 2^32 or n >= 2^31, 5 a coordinate outside [-32768, 32768].
inline int check_table(const blok_light* t, uint64_t n, uint64_t* out_faces, uint64_t* out_index) {
    uint64_t sum = 0;
    *out_faces = 0; *out_index = 0;
    if (n >= 0x80000000ull) return 4;
    for (uint64_t i = 0; i < n; ++i) {
        const blok_light& l = t[i];
        *out_index = i;
        if (l.face > 5u) return 1;
        if (l.du == 0u || l.dv == 0u) return 2;
        if (sum > 0xFFFFFFFFull) return 4;
        if (l.cum != static_cast<uint32_t>(sum)) return 3;
        const int a = static_cast<int>(l.face >> 1), u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
        for (int c = 0; c < 3; ++c) if (l.lo[c] < -32768 || l.lo[c] > 32768) return 5;
        if (l.du > 65536u || l.dv > 65536u || int64_t(l.lo[u]) + l.du > 32768 || int64_t(l.lo[v]) + l.dv > 32768) return 5;
        sum += static_cast<uint64_t>(l.du) * l.dv;
    }
    if (sum > 0xFFFFFFFFull) return 4;
    *out_faces = sum;
    return 0;
}

// ---- the pick: which unit face a 32-bit random number selects, and its light ----
BLOK_LD uint32_t pick_of(uint32_t r, uint32_t n_faces) { return static_cast<uint32_t>((static_cast<uint64_t>(r) * n_faces) >> 32); }
// The last light whose cum is <= pick (cum[0] = 0, so there is one), n >= 1: 4-byte loads of the records' cum words.
BLOK_LD uint32_t find_light(const blok_light* t, uint32_t n, uint32_t pick) {
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t[mid].cum <= pick) lo = mid; else hi = mid;
    }
    return lo;
}

// The sampled point q on cell `off` of light L (off = pick - L.cum; iu = off % du, iv = off / du) and the light's normal nl = +-e_a.
// World position = lattice x vs; vs is a power of two, so the products are exact.
BLOK_LD void sample_point(const blok_light& L, uint32_t off, float u1, float u2, float vs, float q[3], float nl[3]) {
    const uint32_t iu = off % L.du, iv = off / L.du;
    const uint32_t a = L.face >> 1;
    const int32_t lo_u = a == 0u ? L.lo[1] : L.lo[0], lo_v = a == 2u ? L.lo[1] : L.lo[2], lo_a = a == 0u ? L.lo[0] : (a == 1u ? L.lo[1] : L.lo[2]);
    const float pa = static_cast<float>(lo_a) * vs;
    const float pu = (static_cast<float>(lo_u + static_cast<int32_t>(iu)) + u1) * vs;
    const float pv = (static_cast<float>(lo_v + static_cast<int32_t>(iv)) + u2) * vs;
    q[0] = a == 0u ? pa : pu;
    q[1] = a == 0u ? pu : (a == 1u ? pa : pv);
    q[2] = a == 2u ? pa : pv;
    const float s = (L.face & 1u) ? -1.0f : 1.0f;
    nl[0] = a == 0u ? s : 0.0f; nl[1] = a == 1u ? s : 0.0f; nl[2] = a == 2u ? s : 0.0f;
}

}  // namespace lights
}  // namespace blok
#endif
