// Per-ray work of the dense-grid kernel (dense_kernels.hip): the two-level DDA over the tiled id grid, from the axis setup to the
// packed hit record, and the tile / in-tile cell arithmetic of the tiling.  As trace_core.h, written against a handful of HIP device
// intrinsics so that tests/host_harness/dense_shim.cpp compiles the same text for the host (BLOK_TRACE_HOST_HARNESS) to run it
// against the CPU reference and under sanitizers.  The shipped library never builds or calls the host form.
#ifndef BLOK_DENSE_CORE_H
#define BLOK_DENSE_CORE_H

#include "trace_core.h"

// Optional hooks, defined only by the host harness: the axis of every step, and the tile index before every read that it addresses (the
// harness ends a walk whose tile lies outside the grid instead of reading there).
#ifndef BLOK_DENSE_STEP
#define BLOK_DENSE_STEP(axis)
#endif
#ifndef BLOK_DENSE_TILE
#define BLOK_DENSE_TILE(tile)
#endif

namespace blok {

// ---- tiling: ids[z][y][x] of an nx x ny x nz grid -> 8x8x8-cell tiles of 512 words, tile (bx, by, bz) row-major over tx x ty x tz ----
// the tile that holds grid cell (x, y, z), and the cell's word inside it
BLOK_DEV uint32_t dense_tile_of(uint32_t x, uint32_t y, uint32_t z, uint32_t tx, uint32_t ty) { return (x >> 3) + tx * ((y >> 3) + ty * (z >> 3)); }
BLOK_DEV uint32_t dense_cell_in_tile(uint32_t x, uint32_t y, uint32_t z) { return (x & 7u) | ((y & 7u) << 3) | ((z & 7u) << 6); }
// the inverse: grid cell of word c of tile `tile`
BLOK_DEV void dense_cell_of(uint32_t tile, uint32_t c, uint32_t tx, uint32_t ty, uint32_t& x, uint32_t& y, uint32_t& z) {
    const uint32_t bx = tile % tx, by = (tile / tx) % ty, bz = tile / (tx * ty);
    x = bx * 8u + (c & 7u); y = by * 8u + ((c >> 3) & 7u); z = bz * 8u + (c >> 6);
}
// the id a tile holds for grid cell (x, y, z): cells beyond the grid inside the last tiles are 0
BLOK_DEV uint32_t dense_source_id(const uint32_t* ids, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t x, uint32_t y, uint32_t z) {
    return (x < nx && y < ny && z < nz) ? ids[(static_cast<size_t>(z) * ny + y) * nx + x] : 0u;
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------------
struct DenseGrid {
    int32_t origin[3];             // grid corner (voxelSize 1)
    uint32_t tx, ty, tz;           // tiles per axis
    const uint32_t* tiled;         // ids, 8x8x8-cell tiles of 512 words
};

struct DAxis {
    float o, inv, sgn, c;      // as trace_core.h: Axis
    float f;                   // mirrored coordinate 2^23 + q of the current cell / tile corner
    float tF;                  // T of its far plane
    uint32_t n;                // padded extent (multiple of 8) on this axis
    bool neg;
};

BLOK_DEV float dplane(const DAxis& a, float f) { return rn_mul(rn_sub(exact_fma(a.sgn, f, a.c), a.o), a.inv); }

// the slab [q, q + step) of `count` slabs starting at a.f that holds the ray at tS: counts interior planes with T <= tS by
// bisection (T is monotone in q); sets a.f and a.tF (t_far comes in as the far plane of the whole span)
BLOK_DEV void denter(DAxis& a, uint32_t count, float step, float tS) {
    uint32_t lo = 0u, hi = count - 1u;                   // the answer lies in [lo, hi]
    float t_hi = a.tF;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        const float t = dplane(a, a.f + static_cast<float>(mid) * step);
        if (t <= tS) lo = mid; else { hi = mid - 1u; t_hi = t; }
    }
    a.f += static_cast<float>(lo) * step;
    a.tF = t_hi;
}

// Walks one ray over the grid.  bits(w): word w of the tile occupancy bits (the kernel's LDS copy or the global array).  true: `rec` is
// the packed 16-byte hit record (material id in rec.y, face in bits 16..23 of rec.w); false: a miss, rec untouched.
template <typename Bits>
BLOK_DEV bool dense_walk(const RayIn& r, const DenseGrid& G, const Bits& bits, uint4& rec) {
    DAxis ax[3];
    const float org[3] = {r.ox, r.oy, r.oz}, dir[3] = {r.dx, r.dy, r.dz};
    const uint32_t dims[3] = {G.tx * 8u, G.ty * 8u, G.tz * 8u};
    float t_in = r.tmin, t_out = r.tmax;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        DAxis& x = ax[a];
        x.o = org[a]; x.inv = safe_inv(dir[a]); x.neg = !(x.inv > 0.0f); x.n = dims[a];
        x.sgn = x.neg ? -1.0f : 1.0f;
        x.c = static_cast<float>(G.origin[a] + (x.neg ? static_cast<int>(x.n) : 0)) + (x.neg ? kCoordBias : -kCoordBias);
        x.f = kCoordBias;
        x.tF = dplane(x, kCoordBias + static_cast<float>(x.n));
        t_in = fmaxf(t_in, dplane(x, kCoordBias));
        t_out = fminf(t_out, x.tF);
    }
    if (!(t_in < t_out)) return false;
    float tCur = t_in;
    // tile level first: the tile that holds the ray at tCur
#pragma unroll
    for (int a = 0; a < 3; ++a) denter(ax[a], ax[a].n / 8u, 8.0f, tCur);
    uint32_t lvl = 1u;
    bool found = false;
    uint32_t id = 0u;
    for (;;) {
        // un-mirrored cell coordinates of the current corner
        uint32_t cell[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t q = __float_as_uint(ax[a].f) & 0x7FFFFFu;
            cell[a] = ax[a].neg ? ax[a].n - (lvl ? 8u : 1u) - q : q;
        }
        const uint32_t tile = dense_tile_of(cell[0], cell[1], cell[2], G.tx, G.ty);
        BLOK_DENSE_TILE(tile);
        if (lvl == 1u) {
            const uint32_t word = bits(tile >> 5);
            if ((word >> (tile & 31u)) & 1u) {
                // occupied tile: the cell inside it that holds the ray at tCur
#pragma unroll
                for (int a = 0; a < 3; ++a) denter(ax[a], 8u, 1.0f, tCur);
                lvl = 0u;
                continue;
            }
        } else {
            id = G.tiled[static_cast<size_t>(tile) * 512u + dense_cell_in_tile(cell[0], cell[1], cell[2])];
        }
        const float tExit = fminf(fminf(ax[0].tF, ax[1].tF), ax[2].tF);
        if (lvl == 0u && id != 0u) {
            if (tCur < fminf(tExit, r.tmax)) { found = true; break; }          // the canonical predicate (trace_kernels.h)
        }
        // step across the nearest far plane (x, then y, then z on ties)
        tCur = tExit;
        if (!(tCur < r.tmax)) break;
        const int s = ax[0].tF == tExit ? 0 : (ax[1].tF == tExit ? 1 : 2);
        BLOK_DENSE_STEP(s);
        const float size = lvl ? 8.0f : 1.0f;
        float fs = 0.0f; uint32_t ns = 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a == s) { ax[a].f += size; fs = ax[a].f; ns = ax[a].n; }
        }
        const uint32_t qs = __float_as_uint(fs) & 0x7FFFFFu;
        if (qs >= ns) break;                                                   // left the grid
        if (lvl == 0u && (qs & 7u) == 0u) {
            // crossed into another tile: back to tile level, corner aligned to the tile
            lvl = 1u;
#pragma unroll
            for (int a = 0; a < 3; ++a) ax[a].f = __uint_as_float(__float_as_uint(ax[a].f) & ~7u);
        }
        const float far = lvl ? 8.0f : 1.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) ax[a].tF = dplane(ax[a], ax[a].f + far);
    }
    if (!found) return false;
    int v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int q = static_cast<int>(__float_as_uint(ax[a].f) & 0x7FFFFFu);
        v[a] = ax[a].neg ? G.origin[a] + static_cast<int>(ax[a].n) - q - 1 : G.origin[a] + q;
    }
    const float hx = rn_add(r.ox, rn_mul(r.dx, tCur)), hy = rn_add(r.oy, rn_mul(r.dy, tCur)), hz = rn_add(r.oz, rn_mul(r.dz, tCur));
    const float ex = rn_sub(hx, rn_add(static_cast<float>(v[0]), 0.5f)), ey = rn_sub(hy, rn_add(static_cast<float>(v[1]), 0.5f)),
                ez = rn_sub(hz, rn_add(static_cast<float>(v[2]), 0.5f));
    const float gx = fabsf(ex), gy = fabsf(ey), gz = fabsf(ez);
    uint32_t face;                                                             // getHitFace, intersect.rint:58-68
    if (gx >= gy && gx >= gz) face = ex > 0.0f ? 0u : 1u;
    else if (gy >= gz)        face = ey > 0.0f ? 2u : 3u;
    else                      face = ez > 0.0f ? 4u : 5u;
    rec.x = __float_as_uint(tCur);
    rec.y = id;
    rec.z = (static_cast<uint32_t>(v[0]) & 0xFFFFu) | (static_cast<uint32_t>(v[1]) << 16);
    rec.w = (static_cast<uint32_t>(v[2]) & 0xFFFFu) | (face << 16) | (1u << 24);
    return true;
}

}  // namespace blok
#endif
