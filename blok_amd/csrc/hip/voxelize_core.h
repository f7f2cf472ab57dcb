// Mesh voxelization into the resident volume (include/blok_hip.h: blok_hip_volume_voxelize_mesh): the exact integer tests of the
// kernels in voxelize_kernels.hip.  Compiled for the host too (tests/host_harness/voxelize_shim.cpp, BLOK_VOX_HOST_HARNESS).
//
// Every coordinate is snapped to 1/256 voxel: q = rint(x * 256) (round half to even; x * 256 is exact in float), a 64-bit integer.
// A triangle is kept as its first vertex v0 and the two other vertices relative to it (w1 = v1 - v0, w2 = v2 - v0); every test point
// is taken relative to v0 too.  Bounds (E = 2048 * 256 = 2^19, the largest accepted extent of a triangle on an axis):
//   |w|, |edge| <= 2^19;   normal n = w1 x w2: |n_i| <= 2 * 2^19 * 2^19 = 2^39;
//   a voxel or brick box tested against the triangle lies at most 2^19 + 2^11 from v0 per axis, so its doubled centre c2 = 2 lo + size
//   has |c2_i| < 2^20 + 2^13;  the plane test's n . c2 is then below 3 * 2^39 * (2^20 + 2^13) < 1.52 * 2^60 < 2^61, and the edge axes'
//   terms below 2^42.  Column tests (solid mode): edge functions below 2^40, the crossing's numerator below 2^60.  All exact in int64.
#ifndef BLOK_VOXELIZE_CORE_H
#define BLOK_VOXELIZE_CORE_H

#include <stdint.h>

#ifdef BLOK_VOX_HOST_HARNESS
#include <cmath>
#define BLOK_VOX_HD inline
#else
#include <hip/hip_runtime.h>
#define BLOK_VOX_HD __host__ __device__ __forceinline__
#endif

namespace blok {
namespace vox {

constexpr int64_t kSub = 256;                       // snapping steps per voxel
constexpr int64_t kMaxExtent = 2048 * kSub;         // largest snapped extent of one triangle on an axis
constexpr float kMaxCoord = 8388608.0f;             // 2^23: the largest accepted |coordinate|

BLOK_VOX_HD bool coord_ok(float x) { return x == x && x <= kMaxCoord && x >= -kMaxCoord; }      // (NaN fails the first, +-inf the others)
BLOK_VOX_HD int64_t snap(float x) {
#ifdef BLOK_VOX_HOST_HARNESS
    return static_cast<int64_t>(std::rint(x * 256.0f));
#else
    return static_cast<int64_t>(rintf(x * 256.0f));
#endif
}
BLOK_VOX_HD int64_t abs64(int64_t a) { return a < 0 ? -a : a; }
BLOK_VOX_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
BLOK_VOX_HD int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
BLOK_VOX_HD int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }     // b > 0
BLOK_VOX_HD int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }                                               // b > 0

// Voxels whose closed cube [i, i + 1] meets the closed snapped interval [lo, hi] (world voxel indices).
BLOK_VOX_HD int64_t voxel_lo(int64_t lo) { return floor_div(lo - 1, kSub); }
BLOK_VOX_HD int64_t voxel_hi(int64_t hi) { return floor_div(hi, kSub); }

struct Tri {
    int64_t v0[3];      // snapped first vertex
    int64_t w1[3];      // snapped second and third vertex, relative to v0
    int64_t w2[3];
};

BLOK_VOX_HD void normal(const Tri& t, int64_t n[3]) {
    n[0] = t.w1[1] * t.w2[2] - t.w1[2] * t.w2[1];
    n[1] = t.w1[2] * t.w2[0] - t.w1[0] * t.w2[2];
    n[2] = t.w1[0] * t.w2[1] - t.w1[1] * t.w2[0];
}

// Does axis a separate the triangle (doubled: 0, 2 w1, 2 w2) from the box of doubled centre c2 and half extent h (doubled: the box's
// edge)?  Closed sets: touching does not separate.  A zero axis never separates.
BLOK_VOX_HD bool separates(int64_t ax, int64_t ay, int64_t az, const Tri& t, const int64_t c2[3], int64_t h) {
    const int64_t p1 = 2 * (ax * t.w1[0] + ay * t.w1[1] + az * t.w1[2]);
    const int64_t p2 = 2 * (ax * t.w2[0] + ay * t.w2[1] + az * t.w2[2]);
    const int64_t lo = min64(0, min64(p1, p2)), hi = max64(0, max64(p1, p2));
    const int64_t c = ax * c2[0] + ay * c2[1] + az * c2[2];
    const int64_t r = h * (abs64(ax) + abs64(ay) + abs64(az));
    return lo > c + r || hi < c - r;
}

// Separating-axis test of the closed snapped triangle against the closed cube [lo, lo + size]^3 (lo relative to v0, snapped units):
// the three box normals, the triangle's normal and the nine cross products of its edges with the box axes.  Exact.
BLOK_VOX_HD bool box_overlaps(const Tri& t, const int64_t lo[3], int64_t size) {
    for (int a = 0; a < 3; ++a) {
        const int64_t tmin = min64(0, min64(t.w1[a], t.w2[a])), tmax = max64(0, max64(t.w1[a], t.w2[a]));
        if (tmin > lo[a] + size || tmax < lo[a]) return false;
    }
    const int64_t c2[3] = {2 * lo[0] + size, 2 * lo[1] + size, 2 * lo[2] + size};
    int64_t n[3];
    normal(t, n);
    if (separates(n[0], n[1], n[2], t, c2, size)) return false;
    const int64_t e[3][3] = {{t.w1[0], t.w1[1], t.w1[2]},
                             {t.w2[0] - t.w1[0], t.w2[1] - t.w1[1], t.w2[2] - t.w1[2]},
                             {-t.w2[0], -t.w2[1], -t.w2[2]}};
    for (int k = 0; k < 3; ++k) {
        if (separates(0, e[k][2], -e[k][1], t, c2, size)) return false;      // e x (1, 0, 0)
        if (separates(-e[k][2], 0, e[k][0], t, c2, size)) return false;      // e x (0, 1, 0)
        if (separates(e[k][1], -e[k][0], 0, t, c2, size)) return false;      // e x (0, 0, 1)
    }
    return true;
}

// Solid mode.  Does the column point (Y, Z) (relative to v0) lie in the triangle's yz projection?  Zero-area projections never count.
// The projection is oriented counter-clockwise first; a point on an edge counts iff the edge (dy, dz) has dz < 0, or dz == 0 and dy < 0.
// That is the answer for the point moved by (+e, -e^2), e -> 0: a point on no edge line, so a column through an edge or vertex shared
// by a closed edge-manifold mesh counts exactly as a column beside it.
BLOK_VOX_HD bool column_inside(const Tri& t, int64_t Y, int64_t Z) {
    const int64_t nx = t.w1[1] * t.w2[2] - t.w1[2] * t.w2[1];
    if (nx == 0) return false;
    int64_t py[3] = {0, t.w1[1], t.w2[1]}, pz[3] = {0, t.w1[2], t.w2[2]};
    if (nx < 0) { const int64_t y = py[1], z = pz[1]; py[1] = py[2]; pz[1] = pz[2]; py[2] = y; pz[2] = z; }
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1;
        const int64_t dy = py[k1] - py[k], dz = pz[k1] - pz[k];
        const int64_t E = dy * (Z - pz[k]) - dz * (Y - py[k]);
        if (E < 0) return false;
        if (E == 0 && !(dz < 0 || (dz == 0 && dy < 0))) return false;
    }
    return true;
}

// Solid mode: the first voxel i whose centre lies at or beyond the triangle's crossing of the column (Y, Z) along +x, for a column
// that column_inside() accepted.  Voxel i's centre is at base + 256 i (relative to v0; base = origin_x * 256 + 128 - v0.x).
BLOK_VOX_HD int64_t crossing_voxel(const Tri& t, int64_t Y, int64_t Z, int64_t base) {
    int64_t n[3];
    normal(t, n);
    if (n[0] < 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    // smallest i with n . (base + 256 i, Y, Z) >= 0; base is brought into (-256, 0] first so that no product leaves int64
    const int64_t i0 = floor_div(-base, kSub);
    const int64_t b = base + kSub * i0;
    const int64_t R = -(n[1] * Y + n[2] * Z) - n[0] * b;
    return i0 + ceil_div(R, kSub * n[0]);
}

}  // namespace vox
}  // namespace blok
#endif
