// The resident volume as a sparse brick stream (include/blok_hip.h: blok_hip_volume_encode_bricks has the contract).  The one place the
// stream's rules live: the kernels (hip/bricks_kernels.hip) and the host build (host/bricks.cpp) both include this header.  No HIP types.
// Densities travel as their 32-bit patterns: the stream is a function of bits, never of float comparisons other than the FILLED_ONLY rule.
#ifndef BLOK_BRICKS_CORE_H
#define BLOK_BRICKS_CORE_H
#include <stdint.h>
#include <string.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_BRICKS_HD __host__ __device__ inline
#else
#define BLOK_BRICKS_HD inline
#endif

namespace blok {
namespace bricks {

constexpr uint32_t kUniformDensity = 1u, kUniformMaterial = 2u;      // blok_brick_record::kind
constexpr uint32_t kEncodeFlags = BLOK_BRICKS_FILLED_ONLY, kDecodeFlags = BLOK_BRICKS_KEEP_OTHERS;

BLOK_BRICKS_HD float bits_float(uint32_t bits) { float f; memcpy(&f, &bits, sizeof f); return f; }

// The stored predicate: by default any cell that is not (+0.0f, 0); with FILLED_ONLY the rebuild's rule, density > 0.
BLOK_BRICKS_HD bool stored(uint32_t density_bits, uint32_t id, bool filled_only) {
    return filled_only ? bits_float(density_bits) > 0.0f : (density_bits | id) != 0u;
}

// Bit of cell (x, y, z) of a brick in its mask: the bit order of GpuVolume::d_masks and of brick_lane_voxel.
BLOK_BRICKS_HD uint32_t cell_bit(uint32_t x, uint32_t y, uint32_t z) { return x | (y << 2) | (z << 4); }

// What one plane (density patterns or ids) of a brick comes to, cell after cell in ascending bit order: the first stored value and
// whether every stored value equals it.
struct PlaneDraft {
    uint32_t first = 0u;
    bool any = false, uniform = true;
    BLOK_BRICKS_HD void add(uint32_t value) {
        if (!any) { first = value; any = true; }
        else uniform = uniform && value == first;
    }
};

// A brick's draft from its up to 64 (density bits, id) pairs; cells cut off by the region are never added.
struct BrickDraft {
    uint64_t mask = 0ull;
    PlaneDraft density, material;
    BLOK_BRICKS_HD void add(uint32_t bit, uint32_t density_bits, uint32_t id, bool filled_only) {
        if (!stored(density_bits, id, filled_only)) return;
        mask |= 1ull << bit;
        density.add(density_bits); material.add(id);
    }
    BLOK_BRICKS_HD uint32_t kind() const { return (density.uniform ? kUniformDensity : 0u) | (material.uniform ? kUniformMaterial : 0u); }
};

BLOK_BRICKS_HD uint32_t popcount64(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__popcll(m));
#else
    return static_cast<uint32_t>(__builtin_popcountll(m));
#endif
}

// The record of a stored brick (mask != 0) whose non-uniform planes start at the given payload indices.
BLOK_BRICKS_HD blok_brick_record make_record(uint32_t brick, uint64_t mask, uint32_t kind, uint32_t first_density, uint32_t first_material,
                                             uint32_t density_base, uint32_t material_base) {
    blok_brick_record r;
    r.mask = mask; r.brick = brick; r.kind = kind;
    r.density = (kind & kUniformDensity) ? first_density : density_base;
    r.material = (kind & kUniformMaterial) ? first_material : material_base;
    return r;
}

// Bricks of a region, counted from its lo: nb[a] = ceil(ext[a] / 4).
BLOK_BRICKS_HD void brick_counts(const uint32_t ext[3], uint32_t nb[3]) { for (int a = 0; a < 3; ++a) nb[a] = (ext[a] + 3u) / 4u; }

// The bits of brick (bx, by, bz) that lie inside a region of extents ext (the last brick on an axis may be partial).
BLOK_BRICKS_HD uint64_t region_mask(const uint32_t ext[3], uint32_t bx, uint32_t by, uint32_t bz) {
    const uint32_t wx = ext[0] - 4u * bx < 4u ? ext[0] - 4u * bx : 4u, wy = ext[1] - 4u * by < 4u ? ext[1] - 4u * by : 4u,
                   wz = ext[2] - 4u * bz < 4u ? ext[2] - 4u * bz : 4u;
    const uint64_t row = (1ull << wx) - 1ull;                         // one x row
    uint64_t layer = 0ull;
    for (uint32_t y = 0; y < wy; ++y) layer |= row << (4u * y);
    uint64_t all = 0ull;
    for (uint32_t z = 0; z < wz; ++z) all |= layer << (16u * z);
    return all;
}

// Validation of a host stream (the rules of blok_hip.h).  0: valid.  Otherwise the rule that failed, with *bad_record the first record
// that fails it (rules 1 and 9..12 concern the info alone and leave it at n_bricks).
enum Rule { kValid = 0, kVersion, kFlags, kOrder, kBrickRange, kMaskEmpty, kMaskOutside, kKind, kDensityIndex, kMaterialIndex,
            kTotalDensity, kTotalMaterial, kTotalVoxels, kNullArray, kExtent };
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "version is not 1", "unknown flag bits", "records not strictly ascending by brick", "brick index outside the region's bricks",
                                        "empty mask", "mask bit outside the region", "kind above 3", "density index is not the running sum",
                                        "material index is not the running sum", "n_density differs from what the records imply",
                                        "n_material differs from what the records imply", "n_voxels differs from what the records imply",
                                        "null array with a non-zero count", "region above 2^32 cells"};
    return kText[rule];
}
inline int validate(const blok_bricks_info& info, const blok_brick_record* records, const uint32_t* density_payload, const uint32_t* material_payload,
                    uint64_t* bad_record) {
    *bad_record = info.n_bricks;
    if (info.version != 1u) return kVersion;
    if (info.flags & ~kEncodeFlags) return kFlags;
    if (static_cast<uint64_t>(info.ext[0]) * info.ext[1] > 0xFFFFFFFFull || static_cast<uint64_t>(info.ext[0]) * info.ext[1] * info.ext[2] > 0xFFFFFFFFull) return kExtent;
    if ((info.n_bricks && !records) || (info.n_density && !density_payload) || (info.n_material && !material_payload)) return kNullArray;
    uint32_t nb[3];
    brick_counts(info.ext, nb);
    const uint64_t total = static_cast<uint64_t>(nb[0]) * nb[1] * nb[2];
    uint64_t n_density = 0, n_material = 0, n_voxels = 0;
    for (uint64_t i = 0; i < info.n_bricks; ++i) {
        const blok_brick_record& r = records[i];
        *bad_record = i;
        if (i && r.brick <= records[i - 1].brick) return kOrder;
        if (r.brick >= total) return kBrickRange;
        if (r.mask == 0ull) return kMaskEmpty;
        const uint32_t bx = r.brick % nb[0], by = (r.brick / nb[0]) % nb[1], bz = r.brick / (nb[0] * nb[1]);
        if (r.mask & ~region_mask(info.ext, bx, by, bz)) return kMaskOutside;
        if (r.kind > 3u) return kKind;
        const uint32_t cells = popcount64(r.mask);
        if (!(r.kind & kUniformDensity)) { if (r.density != n_density) return kDensityIndex; n_density += cells; }
        if (!(r.kind & kUniformMaterial)) { if (r.material != n_material) return kMaterialIndex; n_material += cells; }
        n_voxels += cells;
    }
    *bad_record = info.n_bricks;
    if (n_density != info.n_density) return kTotalDensity;
    if (n_material != info.n_material) return kTotalMaterial;
    if (n_voxels != info.n_voxels) return kTotalVoxels;
    return kValid;
}

}  // namespace bricks
}  // namespace blok
#endif
