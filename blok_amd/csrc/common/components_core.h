// Connected components of a voxel volume (include/blok_hip.h: blok_hip_volume_label_components has the contract).  The one place the
// region's index arithmetic and the union-find live: the kernels (hip/components_kernels.hip) and the host build (host/components.cpp)
// both include this header.  No HIP types.
//
// The union-find is the label array itself: parent[r] <= r, a root has parent[r] == r, and a union links the LARGER root under the
// smaller, so the final root of a tree is the smallest index of its component — the contract's label — whatever the order of the unions.
// `Cells` is how the array is reached: load(i), and fetch_min(i, v) = { old = parent[i]; parent[i] = min(old, v); return old; }.  On the
// host both are plain and serial; on the device both are agent-scope atomics, and unite decides by what fetch_min RETURNED, never by a
// load: a loaded parent may be out of date (it is still an ancestor, parents only ever move towards the root, so find stays right), but
// "was it still a root when I linked it" is something only the atomic knows.
#ifndef BLOK_COMPONENTS_CORE_H
#define BLOK_COMPONENTS_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_COMPONENTS_HD __host__ __device__ __forceinline__
#else
#define BLOK_COMPONENTS_HD inline
#endif

namespace blok {
namespace components {

// A volume's voxel is filled iff its density > 0: zero of either sign, negative values and NaN are empty (the rebuild's rule).
BLOK_COMPONENTS_HD bool filled(float density) { return density > 0.0f; }

// The region, box-local: corner and extents.  cells() < 2^32 is the callers' precondition (BLOK_LABEL_EMPTY must not be an index).
struct Region {
    uint32_t lo[3], ext[3];
};
BLOK_COMPONENTS_HD uint64_t cells(const Region& g) { return static_cast<uint64_t>(g.ext[0]) * g.ext[1] * g.ext[2]; }
// Index of the box-local voxel (x, y, z) of the region, x fastest.
BLOK_COMPONENTS_HD uint32_t index_of(const Region& g, uint32_t x, uint32_t y, uint32_t z) {
    return static_cast<uint32_t>((x - g.lo[0]) + (static_cast<uint64_t>(y - g.lo[1]) + static_cast<uint64_t>(z - g.lo[2]) * g.ext[1]) * g.ext[0]);
}
BLOK_COMPONENTS_HD bool inside(const Region& g, uint32_t x, uint32_t y, uint32_t z) {
    return x - g.lo[0] < g.ext[0] && y - g.lo[1] < g.ext[1] && z - g.lo[2] < g.ext[2];      // (a coordinate below lo wraps and fails)
}
// Region-local coordinates of index r.
BLOK_COMPONENTS_HD void cell_of(const Region& g, uint32_t r, uint32_t& x, uint32_t& y, uint32_t& z) {
    x = r % g.ext[0];
    const uint32_t q = r / g.ext[0];
    y = q % g.ext[1]; z = q / g.ext[1];
}
// Index step to the neighbour at +1 along axis a.
BLOK_COMPONENTS_HD uint32_t stride(const Region& g, uint32_t a) { return a == 0u ? 1u : (a == 1u ? g.ext[0] : g.ext[0] * g.ext[1]); }

// Bit f of blok_component::touches from region-local INCLUSIVE bounds mn, mx: the bounds reach the region's side f.
BLOK_COMPONENTS_HD uint32_t touches(const Region& g, const uint32_t mn[3], const uint32_t mx[3]) {
    uint32_t t = 0;
    for (uint32_t a = 0; a < 3u; ++a) t |= (mx[a] + 1u == g.ext[a] ? 1u : 0u) << (2u * a) | (mn[a] == 0u ? 2u : 0u) << (2u * a);
    return t;
}

template <class Cells>
BLOK_COMPONENTS_HD uint32_t find(const Cells& p, uint32_t r) {
    for (uint32_t q = p.load(r); q != r; q = p.load(r)) r = q;
    return r;
}

template <class Cells>
BLOK_COMPONENTS_HD void unite(const Cells& p, uint32_t a, uint32_t b) {
    for (;;) {
        a = find(p, a); b = find(p, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = p.fetch_min(b, a);
        if (old == b) return;              // b was a root and now hangs under a
        // b had been linked under `old` (< b) in the meantime.  Its cell now holds min(old, a), so one of the two trees has lost its
        // link through b: joining a's with old's restores it, and is what was asked for.
        b = old;
    }
}

}  // namespace components
}  // namespace blok
#endif
