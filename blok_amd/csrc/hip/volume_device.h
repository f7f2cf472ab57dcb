// What the kernels over the resident volume and over placed models share, each defined once: wave-uniform loads through the scalar cache,
// the keyed brick index, the mask word of a brick in either layout of GpuVolume::d_masks (gpu_build.h), the row segment a wave of a region
// launch owns, and the walk from a model's root to one of its bricks.  The key arithmetic also compiles without HIP (tests/host_harness/cell_key_main.cpp).
#ifndef BLOK_VOLUME_DEVICE_H
#define BLOK_VOLUME_DEVICE_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BLOK_VOLUME_HD __host__ __device__ inline
#else
#define BLOK_VOLUME_HD inline
#endif

namespace blok {

// ---- keyed layout (gpu_build.h: GpuVolume::keyed) -------------------------------------------------------------------------------
// Key of a cell from its coordinates in units of its own size: `digits` 2-bit digit triples, least significant level first
// (x | y << 2 | z << 4 per digit, the tree's child bit order).  A brick's key has levels-1 digits, a level-l cell's levels-l.
BLOK_VOLUME_HD uint64_t cell_key(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t digits) {
    uint64_t key = 0;
    for (uint32_t j = 0; j < digits; ++j)
        key |= static_cast<uint64_t>(((cx >> (2u * j)) & 3u) | (((cy >> (2u * j)) & 3u) << 2) | (((cz >> (2u * j)) & 3u) << 4)) << (6u * j);
    return key;
}
BLOK_VOLUME_HD void key_cell(uint64_t key, uint32_t digits, uint32_t& cx, uint32_t& cy, uint32_t& cz) {
    cx = cy = cz = 0;
    for (uint32_t j = 0; j < digits; ++j) {
        const uint32_t d = static_cast<uint32_t>(key >> (6u * j)) & 63u;
        cx |= (d & 3u) << (2u * j); cy |= ((d >> 2) & 3u) << (2u * j); cz |= (d >> 4) << (2u * j);
    }
}

#if defined(__HIPCC__)

// The brick masks of a volume as a kernel reads them (gpu_build.h: brick_masks_of).  key_digits: keyed brick layout, digits of a brick's
// key (levels - 1); 0 = row-major.
struct BrickMasks {
    const uint64_t* masks;
    uint32_t nbx, nby, key_digits;
    // The mask word of brick (bx, by, bz), in either layout of GpuVolume::d_masks.
    __device__ __forceinline__ uint64_t at(uint32_t bx, uint32_t by, uint32_t bz) const {
        if (key_digits == 0u) return masks[bx + (static_cast<size_t>(bz) * nby + by) * nbx];
        return masks[cell_key(bx, by, bz, key_digits)];
    }
    // What brick coordinate b along `axis` contributes to a brick's index: at(bx, by, bz) = masks[part(bx, 0) + part(by, 1) + part(bz, 2)]
    // in either layout, and part(4 g + k, axis) = part(4 g, axis) + k * part(1, axis) for k < 4 — a walk along an axis computes one part per
    // four bricks.
    __device__ __forceinline__ uint64_t part(uint32_t b, uint32_t axis) const {
        if (key_digits == 0u) return static_cast<uint64_t>(b) * (axis == 0u ? 1ull : axis == 1u ? static_cast<uint64_t>(nbx) : static_cast<uint64_t>(nbx) * nby);
        uint64_t key = 0;
        for (uint32_t j = 0; j < key_digits; ++j) key |= static_cast<uint64_t>((b >> (2u * j)) & 3u) << (6u * j + 2u * axis);
        return key;
    }
};

// Wave `wave` of a launch over a region whose rows along x are cut into segments of 64 cells, `x_chunks` to a row of the `ny` rows of a
// slice: it is segment xc of row (y, z).
__device__ __forceinline__ void row_segment(uint64_t wave, uint32_t x_chunks, uint32_t ny, uint32_t& xc, uint32_t& y, uint32_t& z) {
    xc = static_cast<uint32_t>(wave % x_chunks);
    const uint64_t row = wave / x_chunks;
    y = static_cast<uint32_t>(row % ny); z = static_cast<uint32_t>(row / ny);
}

// ---- wave-uniform loads through the scalar cache ----------------------------------------------------------------------------------------
// A record of a wave-uniform index through the scalar cache (s_load): the arrays read this way — the instance table, the model store, a
// model's nodes, the sweep's placement records and prefix — are read-only while the kernels run, and the compiler cannot know that next to
// the kernels' stores and atomics (trace_core.h: walk_enter_wave does the same for nodes).
// A record whose size is a power of two is one load.  Any other multiple of 16 bytes goes in 16-byte words: a vector type's size and
// alignment round UP to a power of two, so one vector of 24 words would stride the index by 128 bytes, not by the record's 96.
template <class T>
__device__ __forceinline__ T uniform_record(const T* base, uint32_t index) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr uint32_t kWords = sizeof(T) / 4;
    static_assert(sizeof(T) % 4 == 0 && ((kWords & (kWords - 1)) == 0 || sizeof(T) % 16 == 0), "a power of two of 4-byte words, or whole 16-byte words");
    T out;
    if constexpr ((kWords & (kWords - 1)) == 0) {
        typedef uint32_t Words __attribute__((ext_vector_type(kWords)));
        const Words w = reinterpret_cast<const __attribute__((address_space(4))) Words*>(reinterpret_cast<uintptr_t>(base))[__builtin_amdgcn_readfirstlane(index)];
        __builtin_memcpy(&out, &w, sizeof(T));
    } else {
        typedef uint32_t Words4 __attribute__((ext_vector_type(4)));
        const auto* q = reinterpret_cast<const __attribute__((address_space(4))) Words4*>(reinterpret_cast<uintptr_t>(base + __builtin_amdgcn_readfirstlane(index)));
        Words4 w[sizeof(T) / 16];
#pragma unroll
        for (uint32_t i = 0; i < sizeof(T) / 16; ++i) w[i] = q[i];
        __builtin_memcpy(&out, w, sizeof(T));
    }
    return out;
#else
    return base[index];
#endif
}

__device__ __forceinline__ uint32_t uniform_word(const uint32_t* base, uint32_t index) {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(reinterpret_cast<uintptr_t>(base))[__builtin_amdgcn_readfirstlane(index)];
#else
    return base[index];
#endif
}

__device__ __forceinline__ uint64_t uniform_u64(const uint64_t* base, uint32_t index) {
    const uint2 w = uniform_record(reinterpret_cast<const uint2*>(base), index);
    return static_cast<uint64_t>(w.x) | (static_cast<uint64_t>(w.y) << 32);
}

// A 64-bit value every lane holds alike, moved to scalar registers half by half.
// (the builtin returns int: each half goes through uint32_t, or a low word with bit 31 set would sign-extend over the high word)
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32)));
    return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
}

// ---- a model's tree, a wave per brick (tree.h: a node is mask lo, mask hi, index of the first child or of the first material id) --------
__device__ __forceinline__ uint64_t node_mask(const uint4& node) { return static_cast<uint64_t>(node.x) | (static_cast<uint64_t>(node.y) << 32); }

// Root to brick (bx, by, bz), bricks counted from the tree's corner; wave-uniform.  Digit l - 1 of the voxel coordinate is digit l - 2 of
// the brick coordinate.  False: the brick lies in an empty cell of the model, nothing below it.
__device__ __forceinline__ bool model_brick(const uint4* nodes, uint32_t levels, uint32_t bx, uint32_t by, uint32_t bz, uint4& node) {
    node = uniform_record(nodes, 0u);
    for (uint32_t l = levels; l >= 2u; --l) {
        const uint32_t s = 2u * (l - 2u);
        const uint32_t bit = ((bx >> s) & 3u) | (((by >> s) & 3u) << 2) | (((bz >> s) & 3u) << 4);
        const uint64_t mask = node_mask(node);
        if (!((mask >> bit) & 1ull)) return false;
        node = uniform_record(nodes, node.z + static_cast<uint32_t>(__popcll(mask & ((1ull << bit) - 1ull))));
    }
    return true;
}

// The voxel lane b of the brick's wave owns (bit b of the brick's mask), in the model's local coordinates: origin = the tree's corner.
__device__ __forceinline__ void brick_lane_voxel(const int32_t origin[3], uint32_t bx, uint32_t by, uint32_t bz, uint32_t lane, int64_t v[3]) {
    v[0] = int64_t(origin[0]) + int64_t(bx * 4u + (lane & 3u));
    v[1] = int64_t(origin[1]) + int64_t(by * 4u + ((lane >> 2) & 3u));
    v[2] = int64_t(origin[2]) + int64_t(bz * 4u + (lane >> 4));
}

#endif  // __HIPCC__

}  // namespace blok
#endif
