// Procedural terrain as a pure integer function of the world voxel coordinate (include/blok_hip.h: blok_hip_volume_generate_terrain has
// the contract).  The one place its arithmetic lives: the host library (host/terrain.cpp) and the kernels (hip/terrain_kernels.hip)
// both include this header, and so does the benchmark scene G(N, seed) (host/scene.cpp) for the hash it shares with the terrain.
// No HIP types.  Intermediate values are bounded as the contract states, so 32-bit words hold them where they are used here.
#ifndef BLOK_TERRAIN_CORE_H
#define BLOK_TERRAIN_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_TERRAIN_HD __host__ __device__ __forceinline__
#else
#define BLOK_TERRAIN_HD inline
#endif

namespace blok {

// murmur3's 32-bit finaliser over a multiply-xor mix of three coordinates and a seed: the hash of G(N, seed) and of the terrain.
BLOK_TERRAIN_HD uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
BLOK_TERRAIN_HD uint32_t hash3(uint32_t x, uint32_t y, uint32_t z, uint32_t s) {
    return fmix32(x * 0x9E3779B1u ^ y * 0x85EBCA77u ^ z * 0xC2B2AE3Du ^ s);
}

namespace terrain {

constexpr uint32_t kCaveSalt = 0x51ED0000u;       // + octave
constexpr uint32_t kOreSalt = 0x0BE00000u;
constexpr uint32_t kHeightSalt = 0x100u;          // + octave: the y argument of the 2-D lattice's hash
constexpr uint32_t kKnownFlags = BLOK_TERRAIN_SHELL | BLOK_TERRAIN_CLOSE_SIDES | BLOK_TERRAIN_ADD;

// t = f << (16 - c) < 2^16;  s = t^2 (3 * 2^16 - 2 t) >> 32 < 2^16  (the product stays below 2^50)
BLOK_TERRAIN_HD uint32_t fade(uint32_t f, uint32_t c) {
    const uint64_t t = static_cast<uint64_t>(f) << (16u - c);
    return static_cast<uint32_t>((t * t * (196608u - 2u * t)) >> 32);
}
// a, b < 2^16, s <= 2^16: the sum is at most 65535 * 65536 and fits 32 bits
BLOK_TERRAIN_HD uint32_t lerp16(uint32_t a, uint32_t b, uint32_t s) { return (a * (65536u - s) + b * s) >> 16; }

BLOK_TERRAIN_HD uint32_t lattice2(int32_t i, uint32_t salt, int32_t j, uint32_t seed) {
    return hash3(static_cast<uint32_t>(i), kHeightSalt + salt, static_cast<uint32_t>(j), seed) & 0xFFFFu;
}
BLOK_TERRAIN_HD uint32_t lattice3(int32_t i, int32_t j, int32_t k, uint32_t seed_salt) {
    return hash3(static_cast<uint32_t>(i), static_cast<uint32_t>(j), static_cast<uint32_t>(k), seed_salt) & 0xFFFFu;
}
// coordinate + d in the low 32 bits (the lattice wraps with the hash's arguments; no signed overflow at the ends of int32)
BLOK_TERRAIN_HD int32_t step(int32_t i, int32_t d) { return static_cast<int32_t>(static_cast<uint32_t>(i) + static_cast<uint32_t>(d)); }

BLOK_TERRAIN_HD uint32_t noise2(int32_t X, int32_t Z, uint32_t c, uint32_t salt, uint32_t seed) {
    const int32_t i = X >> c, j = Z >> c;
    const uint32_t m = (1u << c) - 1u;
    const uint32_t sx = fade(static_cast<uint32_t>(X) & m, c), sz = fade(static_cast<uint32_t>(Z) & m, c);
    const uint32_t a = lerp16(lattice2(i, salt, j, seed), lattice2(step(i, 1), salt, j, seed), sx);
    const uint32_t b = lerp16(lattice2(i, salt, step(j, 1), seed), lattice2(step(i, 1), salt, step(j, 1), seed), sx);
    return lerp16(a, b, sz);
}

// The eight lattice values of one cell of a 3-D noise; interpolation along x, then y, then z.
struct Cell3 {
    int32_t i, j, k;
    uint32_t g[8];            // bit 0: i + 1, bit 1: j + 1, bit 2: k + 1
};
BLOK_TERRAIN_HD void cell3_load(Cell3& cell, int32_t i, int32_t j, int32_t k, uint32_t seed_salt) {
    cell.i = i; cell.j = j; cell.k = k;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int n = 0; n < 8; ++n) cell.g[n] = lattice3((n & 1) ? step(i, 1) : i, (n & 2) ? step(j, 1) : j, (n & 4) ? step(k, 1) : k, seed_salt);
}
BLOK_TERRAIN_HD uint32_t cell3_eval(const Cell3& cell, int32_t X, int32_t Y, int32_t Z, uint32_t c) {
    const uint32_t m = (1u << c) - 1u;
    const uint32_t sx = fade(static_cast<uint32_t>(X) & m, c), sy = fade(static_cast<uint32_t>(Y) & m, c), sz = fade(static_cast<uint32_t>(Z) & m, c);
    const uint32_t x00 = lerp16(cell.g[0], cell.g[1], sx), x10 = lerp16(cell.g[2], cell.g[3], sx);
    const uint32_t x01 = lerp16(cell.g[4], cell.g[5], sx), x11 = lerp16(cell.g[6], cell.g[7], sx);
    return lerp16(lerp16(x00, x10, sy), lerp16(x01, x11, sy), sz);
}
// A walker along a row or a column keeps the cell it is in: the hashes are taken again only when the voxel leaves it.
BLOK_TERRAIN_HD uint32_t noise3_cached(Cell3& cell, uint32_t& valid, int32_t X, int32_t Y, int32_t Z, uint32_t c, uint32_t seed_salt) {
    const int32_t i = X >> c, j = Y >> c, k = Z >> c;
    if (!valid || i != cell.i || j != cell.j || k != cell.k) { cell3_load(cell, i, j, k, seed_salt); valid = 1u; }
    return cell3_eval(cell, X, Y, Z, c);
}

// H(X, Z): world y of the column's top voxel before caves.  The octaves' weighted sum is below 2^16 * 255.
BLOK_TERRAIN_HD int32_t height(const blok_terrain_params& p, int32_t X, int32_t Z) {
    const uint32_t K = p.height_octaves;
    uint32_t acc = 0;
    for (uint32_t k = 0; k < K; ++k) acc += noise2(X, Z, p.height_cell_log2 - k, k, p.seed) << (K - 1u - k);
    const uint64_t fbm = acc / ((1u << K) - 1u);
    return p.base_height + static_cast<int32_t>((fbm * p.amplitude) >> 16);
}

// The walkers of one evaluator: the cave noise's up to four octaves and the ore noise, each with the cell it last visited.
struct Walker {
    Cell3 cave[4];
    Cell3 ore;
    uint32_t cave_valid[4];      // words, not bools: a per-lane bool kept across a loop costs the kernels a scalar register pair
    uint32_t ore_valid;
};
BLOK_TERRAIN_HD void walker_reset(Walker& w) { for (int k = 0; k < 4; ++k) w.cave_valid[k] = 0u; w.ore_valid = 0u; }
BLOK_TERRAIN_HD uint32_t cave_fbm(const blok_terrain_params& p, Walker& w, int32_t X, int32_t Y, int32_t Z) {
    const uint32_t K = p.cave_octaves;
    uint32_t acc = 0;
    for (uint32_t k = 0; k < 4; ++k)
        if (k < K) acc += noise3_cached(w.cave[k], w.cave_valid[k], X, Y, Z, p.cave_cell_log2 - k, p.seed ^ (kCaveSalt + k)) << (K - 1u - k);
    return acc / ((1u << K) - 1u);
}
// solid(X, Y, Z) given the column's height H
BLOK_TERRAIN_HD bool solid(const blok_terrain_params& p, Walker& w, int32_t X, int32_t Y, int32_t Z, int32_t H) {
    if (Y > H) return false;
    if (p.cave_octaves == 0u || static_cast<int64_t>(Y) > static_cast<int64_t>(H) - static_cast<int64_t>(p.cave_roof)) return true;
    return !(cave_fbm(p, w, X, Y, Z) < p.cave_threshold);
}
// material of a voxel at or under its column's height
BLOK_TERRAIN_HD uint32_t material(const blok_terrain_params& p, Walker& w, int32_t X, int32_t Y, int32_t Z, int32_t H) {
    const uint64_t d = static_cast<uint64_t>(static_cast<int64_t>(H) - static_cast<int64_t>(Y));
    if (d == 0u) return p.surface_material;
    if (d <= p.soil_depth) return p.soil_material;
    return noise3_cached(w.ore, w.ore_valid, X, Y, Z, p.ore_cell_log2, p.seed ^ kOreSalt) > p.ore_threshold ? p.ore_material : p.rock_material;
}

// The limits of the contract that concern the parameters alone.  0 = fine, else the number of the first rule broken.
BLOK_TERRAIN_HD int check_params(const blok_terrain_params& p) {
    if (p.height_octaves < 1u || p.height_octaves > 8u || p.height_cell_log2 > 12u || p.height_octaves > p.height_cell_log2 + 1u) return 1;
    if (p.cave_octaves > 4u || p.cave_cell_log2 > 12u || p.cave_octaves > p.cave_cell_log2 + 1u) return 2;
    if (p.ore_cell_log2 > 12u) return 3;
    if (p.cave_threshold > 65536u || p.ore_threshold > 65536u) return 4;
    if (p.amplitude > 65536u) return 5;
    if (p.base_height > (1 << 24) || p.base_height < -(1 << 24)) return 6;
    uint32_t bits;
    __builtin_memcpy(&bits, &p.density, 4);
    if ((bits & 0x7F800000u) == 0x7F800000u || !(p.density > 0.0f)) return 7;      // infinite or NaN; zero or negative
    if (p.flags & ~kKnownFlags) return 8;
    if ((p.flags & BLOK_TERRAIN_CLOSE_SIDES) && !(p.flags & BLOK_TERRAIN_SHELL)) return 9;
    return 0;
}

}  // namespace terrain
}  // namespace blok
#endif
