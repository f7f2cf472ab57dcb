// Mesh voxelization into the resident volume (gpu_build.h: gpu_volume_voxelize; include/blok_hip.h: blok_hip_volume_voxelize_mesh).
// The exact tests are in voxelize_core.h; DESIGN.md §12 has the contract and the measured cost.
//
//   1. vox_setup_kernel, a lane per triangle: limits, snapping, the triangle's candidate bricks and (solid mode) columns.  The
//      candidates are brick columns along the dominant axis of the triangle's plane (for a segment or point: of one plane through it),
//      K <= 4 bricks deep where that plane crosses them: not the triangle's whole brick box.  Two scans of the counts; one read-back of totals and
//      errors — nothing is written before it.
//   2. vox_pair_kernel, a wave per (triangle, brick) candidate, lane = voxel: __ballot of the exact test is the pair's brick mask, ORed
//      into a mask per brick of the mesh's box (8 B per 64 voxels); the first wave to touch a brick lists it.  With per-triangle
//      materials a second pass takes atomicMin of the triangle index into the touched voxels' ids (set to ~0 in between).  Launched in
//      batches of a fixed number of pairs: a mesh of a million one-voxel triangles and one of twelve huge ones both fill the chip with
//      waves of the same size.
//   3. solid mode: vox_column_kernel, a lane per (triangle, column) crossing, toggles one bit of a bit volume over the mesh's box;
//      vox_prefix_kernel takes the prefix XOR of every row; vox_interior_kernel writes the interior voxels that are not on the surface.
//   4. vox_finalize_kernel, a wave per listed brick: density and material of the surface voxels.
//   5. gpu_volume_commit over the box of the written voxels: masks, occupancy words and dirty flags as blok_hip_volume_set_voxels leaves them.
// Only integer atomics (Or, Min, Xor, Add): the result depends on the inputs alone.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "voxelize_core.h"

namespace blok {

namespace {

using vox::Tri;

struct TriRec {
    Tri t;
    int32_t blo[3], bhi[3];      // box-local bricks the triangle's voxel box covers (inclusive)
    uint32_t d, K, nu, pad0;
    int32_t jlo, klo;            // solid mode: first column (box-local y, z)
    uint32_t nj, pad;
};

constexpr uint32_t kSpread = 256;                     // copies of the reduction words (one per workgroup residue): no hot address
constexpr uint64_t kPairBatch = 1ull << 22;           // waves per surface launch
constexpr uint64_t kColumnBatch = 1ull << 26;         // lanes per column launch
enum : uint32_t { kErrIndex = 1u, kErrCoord = 2u, kErrExtent = 4u };

struct SetupArgs {
    const float* pos; uint64_t n_vertices;
    const uint32_t* tris; uint32_t n_tris;
    int64_t O[3];                // box origin, snapped units
    int32_t n[3];                // box size
    int32_t origin[3];
    uint32_t solid;
    TriRec* rec; uint64_t* pair_count; uint64_t* col_count;
    uint32_t* error; int32_t* mesh_box;    // [kSpread][8]: world voxel lo[3] (min), hi[3] (max, inclusive)
};

// The plane the candidate bricks are culled by: the triangle's own, or for a degenerate triangle (a segment or a point after snapping) one
// plane that contains it — the cross product of its longest edge with the axis that edge is shortest along.  Only the enumeration of
// candidates uses it; the exact test decides.
__device__ inline void cull_normal(const Tri& t, int64_t n[3]) {
    vox::normal(t, n);
    if (n[0] != 0 || n[1] != 0 || n[2] != 0) return;
    const int64_t e[3][3] = {{t.w1[0], t.w1[1], t.w1[2]}, {t.w2[0], t.w2[1], t.w2[2]}, {t.w2[0] - t.w1[0], t.w2[1] - t.w1[1], t.w2[2] - t.w1[2]}};
    int64_t s[3] = {0, 0, 0}, best = -1;
    for (int k = 0; k < 3; ++k) {
        const int64_t l = vox::abs64(e[k][0]) + vox::abs64(e[k][1]) + vox::abs64(e[k][2]);
        if (l > best) { best = l; s[0] = e[k][0]; s[1] = e[k][1]; s[2] = e[k][2]; }
    }
    if (best == 0) { n[0] = 0; n[1] = 0; n[2] = 1; return; }              // a point: any plane through it
    const int64_t ax = vox::abs64(s[0]), ay = vox::abs64(s[1]), az = vox::abs64(s[2]);
    if (ax <= ay && ax <= az) { n[0] = 0; n[1] = s[2]; n[2] = -s[1]; }     // s x (1, 0, 0)
    else if (ay <= az) { n[0] = -s[2]; n[1] = 0; n[2] = s[0]; }            // s x (0, 1, 0)
    else { n[0] = s[1]; n[1] = -s[0]; n[2] = 0; }                          // s x (0, 0, 1)
}

__global__ __launch_bounds__(256) void vox_setup_kernel(const SetupArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_tris) return;
    a.pair_count[i] = 0; a.col_count[i] = 0;
    int64_t q[3][3];
    uint32_t err = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t vi = a.tris[3ull * i + k];
        if (vi >= a.n_vertices) { err |= kErrIndex; continue; }
        for (int c = 0; c < 3; ++c) {
            const float x = a.pos[3ull * vi + c];
            if (!vox::coord_ok(x)) err |= kErrCoord;
            else q[k][c] = vox::snap(x);
        }
    }
    if (!err)
        for (int c = 0; c < 3; ++c)
            if (vox::max64(q[0][c], vox::max64(q[1][c], q[2][c])) - vox::min64(q[0][c], vox::min64(q[1][c], q[2][c])) > vox::kMaxExtent) err |= kErrExtent;
    if (err) { atomicOr(a.error, err); return; }
    TriRec r{};
    for (int c = 0; c < 3; ++c) { r.t.v0[c] = q[0][c]; r.t.w1[c] = q[1][c] - q[0][c]; r.t.w2[c] = q[2][c] - q[0][c]; }
    int64_t lo[3], hi[3], vlo[3], vhi[3];
    bool inside = true;
    for (int c = 0; c < 3; ++c) {
        lo[c] = vox::min64(q[0][c], vox::min64(q[1][c], q[2][c])); hi[c] = vox::max64(q[0][c], vox::max64(q[1][c], q[2][c]));
        vlo[c] = vox::voxel_lo(lo[c]); vhi[c] = vox::voxel_hi(hi[c]);
        const int64_t b0 = vox::max64(vlo[c] - a.origin[c], 0), b1 = vox::min64(vhi[c] - a.origin[c], int64_t(a.n[c]) - 1);
        if (b0 > b1) inside = false;
        r.blo[c] = static_cast<int32_t>(b0 >> 2); r.bhi[c] = static_cast<int32_t>(b1 >> 2);
    }
    int32_t* box = a.mesh_box + 8u * (blockIdx.x % kSpread);
    for (int c = 0; c < 3; ++c) { atomicMin(box + c, static_cast<int32_t>(vlo[c])); atomicMax(box + 3 + c, static_cast<int32_t>(vhi[c])); }
    int64_t n[3];
    vox::normal(r.t, n);
    if (inside) {
        int64_t m[3];
        cull_normal(r.t, m);
        {
            const int64_t ax = vox::abs64(m[0]), ay = vox::abs64(m[1]), az = vox::abs64(m[2]);
            r.d = ax >= ay && ax >= az ? 0u : (ay >= az ? 1u : 2u);
            // the plane's range of d over a brick column's footprint (1024 x 1024 snapped units); +8: margin for the double rounding
            const int64_t nd = r.d == 0 ? ax : (r.d == 1 ? ay : az);
            const double span = static_cast<double>(ax + ay + az - nd) * 1024.0 / static_cast<double>(nd);
            const int32_t depth = r.d == 0 ? r.bhi[0] - r.blo[0] : (r.d == 1 ? r.bhi[1] - r.blo[1] : r.bhi[2] - r.blo[2]);
            r.K = static_cast<uint32_t>(std::min<double>(std::floor((span + 8.0) / 1024.0) + 2.0, double(depth + 1)));
        }
        // (u, v) = the two other axes, in order
        const uint32_t nbx = uint32_t(r.bhi[0] - r.blo[0] + 1), nby = uint32_t(r.bhi[1] - r.blo[1] + 1), nbz = uint32_t(r.bhi[2] - r.blo[2] + 1);
        r.nu = r.d == 0 ? nby : nbx;
        a.pair_count[i] = uint64_t(r.nu) * uint64_t(r.d == 2 ? nby : nbz) * r.K;
    }
    if (a.solid && n[0] != 0) {
        // columns whose centre (j + 1/2, k + 1/2) lies in the triangle's yz range; none when every crossing lies right of the box
        const int64_t j0 = vox::max64(vox::ceil_div(lo[1] - a.O[1] - 128, 256), 0), j1 = vox::min64(vox::floor_div(hi[1] - a.O[1] - 128, 256), a.n[1] - 1);
        const int64_t k0 = vox::max64(vox::ceil_div(lo[2] - a.O[2] - 128, 256), 0), k1 = vox::min64(vox::floor_div(hi[2] - a.O[2] - 128, 256), a.n[2] - 1);
        const bool right = lo[0] > a.O[0] + 256 * (int64_t(a.n[0]) - 1) + 128;
        if (j0 <= j1 && k0 <= k1 && !right) {
            r.jlo = static_cast<int32_t>(j0); r.klo = static_cast<int32_t>(k0); r.nj = static_cast<uint32_t>(j1 - j0 + 1);
            a.col_count[i] = uint64_t(j1 - j0 + 1) * uint64_t(k1 - k0 + 1);
        }
    }
    a.rec[i] = r;
}

__device__ inline uint32_t find_triangle(const uint64_t* scan, uint32_t n, uint64_t p) {     // first t with scan[t] > p (inclusive sums)
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (scan[mid] > p) hi = mid; else lo = mid + 1; }
    return lo;
}

// The same for a whole wave looking up one p: 64 probes per step (log64 instead of log2 dependent loads).
__device__ inline uint32_t find_triangle_wave(const uint64_t* scan, uint32_t n, uint64_t p) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = n - 1;                          // scan[hi] > p
    while (lo < hi) {
        const uint32_t step = (hi - lo + 64u) / 64u;
        const uint32_t probe = min(lo + lane * step, hi);
        const uint64_t b = __ballot(scan[probe] > p);
        if (b == 0ull) { lo = __shfl(probe, 63) + 1u; continue; }
        const int f = __ffsll(static_cast<unsigned long long>(b)) - 1;
        const uint32_t below = __shfl(probe, f > 0 ? f - 1 : 0);
        hi = __shfl(probe, f);
        if (f > 0) lo = below + 1u;
    }
    return lo;
}

struct Region { int32_t b0[3]; uint32_t nb[3]; };       // bricks of the mesh's box: the per-brick mask scratch
struct PairArgs {
    const TriRec* rec; const uint64_t* scan; uint32_t n_tris;
    int64_t O[3]; int32_t n[3];
    Region reg; uint64_t* smask; uint32_t* list; uint32_t* n_list;
    uint32_t* ids; uint32_t phase;                     // 0: masks and the brick list; 1: atomicMin of the triangle index into ids
};

__global__ __launch_bounds__(256) void vox_pair_kernel(const PairArgs a, uint64_t first, uint64_t end) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p = first + uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (p >= end) return;                                                // (whole waves)
    const uint32_t ti = find_triangle_wave(a.scan, a.n_tris, p);
    const uint64_t local = p - (ti ? a.scan[ti - 1] : 0ull);
    const TriRec& r = a.rec[ti];
    const Tri t = r.t;
    const uint32_t d = r.d, u = d == 0 ? 1u : 0u, v = d == 2 ? 1u : 2u;
    const uint64_t col = local / r.K;
    const uint32_t off = static_cast<uint32_t>(local % r.K);
    int32_t b[3];
    b[u] = r.blo[u] + static_cast<int32_t>(col % r.nu);
    b[v] = r.blo[v] + static_cast<int32_t>(col / r.nu);
    {
        int64_t n[3];
        cull_normal(t, n);
        const double nd = static_cast<double>(n[d]);
        double dlo = 1e300, dhi = -1e300;
        for (int c = 0; c < 4; ++c) {
            const int64_t U = a.O[u] + 1024 * (int64_t(b[u]) + (c & 1)) - t.v0[u], V = a.O[v] + 1024 * (int64_t(b[v]) + (c >> 1)) - t.v0[v];
            const double x = -(static_cast<double>(n[u]) * static_cast<double>(U) + static_cast<double>(n[v]) * static_cast<double>(V)) / nd;
            dlo = fmin(dlo, x); dhi = fmax(dhi, x);
        }
        const double tlo = static_cast<double>(vox::min64(0, vox::min64(t.w1[d], t.w2[d]))), thi = static_cast<double>(vox::max64(0, vox::max64(t.w1[d], t.w2[d])));
        dlo = fmax(dlo, tlo); dhi = fmin(dhi, thi);
        const double base = static_cast<double>(t.v0[d] - a.O[d]);
        const int64_t bf = static_cast<int64_t>(floor((base + dlo - 2.0) / 1024.0)), bl = static_cast<int64_t>(floor((base + dhi + 2.0) / 1024.0));
        const int64_t bd = vox::max64(bf, r.blo[d]) + off;
        if (bd > vox::min64(bl, r.bhi[d])) return;
        b[d] = static_cast<int32_t>(bd);
    }
    const int64_t blo[3] = {a.O[0] + 1024 * int64_t(b[0]) - t.v0[0], a.O[1] + 1024 * int64_t(b[1]) - t.v0[1], a.O[2] + 1024 * int64_t(b[2]) - t.v0[2]};
    if (!vox::box_overlaps(t, blo, 1024)) return;                       // (wave-uniform)
    const int32_t x = 4 * b[0] + int32_t(lane & 3u), y = 4 * b[1] + int32_t((lane >> 2) & 3u), z = 4 * b[2] + int32_t(lane >> 4);
    bool hit = false;
    if (x < a.n[0] && y < a.n[1] && z < a.n[2]) {
        const int64_t vlo[3] = {blo[0] + 256 * int64_t(lane & 3u), blo[1] + 256 * int64_t((lane >> 2) & 3u), blo[2] + 256 * int64_t(lane >> 4)};
        hit = vox::box_overlaps(t, vlo, 256);
    }
    const uint64_t mask = __ballot(hit);
    if (mask == 0ull) return;
    if (a.phase == 0) {
        if (lane == 0) {
            const uint32_t g = uint32_t(b[0] - a.reg.b0[0]) + a.reg.nb[0] * (uint32_t(b[1] - a.reg.b0[1]) + a.reg.nb[1] * uint32_t(b[2] - a.reg.b0[2]));
            const unsigned long long old = atomicOr(reinterpret_cast<unsigned long long*>(a.smask + g), static_cast<unsigned long long>(mask));
            if (old == 0ull) a.list[atomicAdd(a.n_list, 1u)] = g;
        }
    } else if (hit) {
        atomicMin(a.ids + (static_cast<size_t>(z) * a.n[1] + y) * a.n[0] + x, ti);
    }
}

__device__ inline void brick_of(const Region& reg, uint32_t g, int32_t b[3]) {
    b[0] = reg.b0[0] + int32_t(g % reg.nb[0]); b[1] = reg.b0[1] + int32_t((g / reg.nb[0]) % reg.nb[1]); b[2] = reg.b0[2] + int32_t(g / (reg.nb[0] * reg.nb[1]));
}

// The touched voxels' ids to ~0 before the atomicMin pass (per-triangle materials).
__global__ __launch_bounds__(256) void vox_clear_ids_kernel(const Region reg, const uint64_t* smask, const uint32_t* list, uint32_t n_list, int32_t nx, int32_t ny,
                                                            uint32_t* ids) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= n_list) return;
    const uint32_t g = list[w];
    if (!((smask[g] >> lane) & 1ull)) return;
    int32_t b[3];
    brick_of(reg, g, b);
    ids[(static_cast<size_t>(4 * b[2] + int32_t(lane >> 4)) * ny + 4 * b[1] + int32_t((lane >> 2) & 3u)) * nx + 4 * b[0] + int32_t(lane & 3u)] = 0xFFFFFFFFu;
}

// Workgroup reduction of the written voxels' box and count, then one set of atomics into copy blockIdx % kSpread.
struct Written { uint32_t* box; unsigned long long* count; };          // box: [kSpread][8] lo[3] (min), hi[3] (max, exclusive)
__device__ inline void reduce_written(const Written& wr, bool on, int32_t x, int32_t y, int32_t z) {
    __shared__ uint32_t s_box[6];
    __shared__ unsigned long long s_n;
    if (threadIdx.x < 3u) { s_box[threadIdx.x] = 0xFFFFFFFFu; s_box[3 + threadIdx.x] = 0u; }
    if (threadIdx.x == 0) s_n = 0ull;
    __syncthreads();
    const uint64_t n = __popcll(__ballot(on));
    // the wave's box by butterfly shuffles first: one lane per wave touches the shared words (a lane each serialises 64-fold)
    uint32_t b[6] = {on ? uint32_t(x) : 0xFFFFFFFFu, on ? uint32_t(y) : 0xFFFFFFFFu, on ? uint32_t(z) : 0xFFFFFFFFu,
                     on ? uint32_t(x) + 1u : 0u, on ? uint32_t(y) + 1u : 0u, on ? uint32_t(z) + 1u : 0u};
    if (n)
        for (int s = 1; s < 64; s <<= 1)
            for (int c = 0; c < 6; ++c) {
                const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(b[c]), s));
                b[c] = c < 3 ? (o < b[c] ? o : b[c]) : (o > b[c] ? o : b[c]);
            }
    if ((threadIdx.x & 63u) == 0 && n) {
        for (int c = 0; c < 3; ++c) { atomicMin(s_box + c, b[c]); atomicMax(s_box + 3 + c, b[3 + c]); }
        atomicAdd(&s_n, static_cast<unsigned long long>(n));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) {
        uint32_t* box = wr.box + 8u * (blockIdx.x % kSpread);
        for (int c = 0; c < 3; ++c) { atomicMin(box + c, s_box[c]); atomicMax(box + 3 + c, s_box[3 + c]); }
        atomicAdd(wr.count + (blockIdx.x % kSpread), s_n);
    }
}

// The surface voxels: density, and the material (per-triangle: of the lowest-indexed triangle, whose index the ids hold).
__global__ __launch_bounds__(256) void vox_finalize_kernel(const Region reg, const uint64_t* smask, const uint32_t* list, uint32_t n_list, int32_t nx, int32_t ny,
                                                           float* density, uint32_t* ids, const uint32_t* tri_mats, uint32_t material, float value, const Written wr) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    bool on = false;
    int32_t b[3] = {0, 0, 0};
    if (w < n_list) {
        const uint32_t g = list[w];
        on = (smask[g] >> lane) & 1ull;
        brick_of(reg, g, b);
    }
    const int32_t x = 4 * b[0] + int32_t(lane & 3u), y = 4 * b[1] + int32_t((lane >> 2) & 3u), z = 4 * b[2] + int32_t(lane >> 4);
    if (on) {
        const size_t i = (static_cast<size_t>(z) * ny + y) * nx + x;
        density[i] = value;
        ids[i] = tri_mats ? tri_mats[ids[i]] : material;
    }
    reduce_written(wr, on, x, y, z);
}

struct ColumnArgs {
    const TriRec* rec; const uint64_t* scan; uint32_t n_tris;
    int64_t O[3]; int32_t nx;
    int32_t m0[3]; uint32_t ry, words;       // bit volume: x in [m0.x, nx), rows (y, z) from m0.y / m0.z, ry rows per z
    uint32_t* bits;
};

__global__ __launch_bounds__(256) void vox_column_kernel(const ColumnArgs a, uint64_t first, uint64_t end) {
    const uint64_t p = first + uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (p >= end) return;
    const uint32_t ti = find_triangle(a.scan, a.n_tris, p);
    const uint64_t local = p - (ti ? a.scan[ti - 1] : 0ull);
    const TriRec& r = a.rec[ti];
    const int32_t j = r.jlo + int32_t(local % r.nj), k = r.klo + int32_t(local / r.nj);
    const Tri t = r.t;
    const int64_t Y = a.O[1] + 256 * int64_t(j) + 128 - t.v0[1], Z = a.O[2] + 256 * int64_t(k) + 128 - t.v0[2];
    if (!vox::column_inside(t, Y, Z)) return;
    int64_t i = vox::crossing_voxel(t, Y, Z, a.O[0] + 128 - t.v0[0]);
    if (i >= a.nx) return;
    if (i < a.m0[0]) i = a.m0[0];                                        // crossings left of the box count
    const uint32_t bit = static_cast<uint32_t>(i - a.m0[0]);
    const uint64_t row = uint64_t(k - a.m0[2]) * a.ry + uint32_t(j - a.m0[1]);
    atomicXor(a.bits + row * a.words + (bit >> 5), 1u << (bit & 31u));
}

__global__ __launch_bounds__(256) void vox_prefix_kernel(uint32_t* bits, uint64_t rows, uint32_t words) {
    const uint64_t row = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (row >= rows) return;
    uint32_t* w = bits + row * words;
    uint32_t carry = 0;
    for (uint32_t i = 0; i < words; ++i) {
        uint32_t x = w[i];
        x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
        x ^= carry;
        w[i] = x;
        carry = (x >> 31) ? 0xFFFFFFFFu : 0u;
    }
}

// The interior voxels that are not surface voxels: density and `material`.
__global__ __launch_bounds__(256) void vox_interior_kernel(const ColumnArgs a, int32_t ny, uint64_t rows, const Region reg, const uint64_t* smask,
                                                           float* density, uint32_t* ids, uint32_t material, float value, const Written wr) {
    const uint64_t tid = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t wx = static_cast<uint32_t>(a.nx - a.m0[0]);
    const uint64_t row = tid / wx;
    const uint32_t bx = static_cast<uint32_t>(tid % wx);
    bool on = false;
    int32_t x = 0, y = 0, z = 0;
    if (row < rows) {
        x = a.m0[0] + int32_t(bx); y = a.m0[1] + int32_t(row % a.ry); z = a.m0[2] + int32_t(row / a.ry);
        on = (a.bits[row * a.words + (bx >> 5)] >> (bx & 31u)) & 1u;
        if (on) {
            const int32_t b[3] = {(x >> 2) - reg.b0[0], (y >> 2) - reg.b0[1], (z >> 2) - reg.b0[2]};
            if (b[0] >= 0 && b[1] >= 0 && b[2] >= 0 && uint32_t(b[0]) < reg.nb[0] && uint32_t(b[1]) < reg.nb[1] && uint32_t(b[2]) < reg.nb[2]) {
                const uint32_t g = uint32_t(b[0]) + reg.nb[0] * (uint32_t(b[1]) + reg.nb[1] * uint32_t(b[2]));
                if ((smask[g] >> ((x & 3) | ((y & 3) << 2) | ((z & 3) << 4))) & 1ull) on = false;      // a surface voxel: vox_finalize_kernel writes it
            }
        }
        if (on) {
            const size_t i = (static_cast<size_t>(z) * ny + y) * a.nx + x;
            density[i] = value;
            ids[i] = material;
        }
    }
    reduce_written(wr, on, x, y, z);
}

hipError_t inclusive_scan(DeviceMem& mem, const uint64_t* in, uint64_t* out, uint32_t n) {
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceScan::InclusiveSum(nullptr, bytes, in, out, static_cast<int>(n));
    if (e != hipSuccess) return e;
    uint8_t* temp;
    if ((e = mem.alloc(&temp, bytes)) != hipSuccess) return e;
    return hipcub::DeviceScan::InclusiveSum(temp, bytes, in, out, static_cast<int>(n));
}

uint32_t blocks(uint64_t n, uint64_t per) { return static_cast<uint32_t>((n + per - 1) / per); }

}  // namespace

GpuBuildStatus gpu_volume_voxelize(GpuVolume* v, const float* positions, size_t n_vertices, const uint32_t* triangles, size_t n_triangles,
                                   const uint32_t* triangle_materials, uint32_t material, float density, bool solid, uint64_t* out_n_voxels,
                                   bool* invalid, std::string* why) {
    *invalid = false;
    if (out_n_voxels) *out_n_voxels = 0;
    if (!cells_fit_32_bits(v, "voxelize", why)) return GpuBuildStatus::Unsupported;
    if (n_triangles > 0x7FFFFFFFull) { *why = "voxelize: more than 2^31 triangles"; return GpuBuildStatus::Unsupported; }
    if (n_triangles == 0) return GpuBuildStatus::Ok;
    const uint32_t nt = static_cast<uint32_t>(n_triangles);
    DeviceMem mem;
    float* d_pos; uint32_t *d_tris, *d_mats = nullptr, *d_error; TriRec* d_rec; uint64_t *d_pairs, *d_cols, *d_pair_scan, *d_col_scan; int32_t* d_mesh_box;
    BLOK_GPU_TRY(mem.alloc(&d_pos, 3 * n_vertices)); BLOK_GPU_TRY(mem.alloc(&d_tris, 3 * n_triangles)); BLOK_GPU_TRY(mem.alloc(&d_rec, n_triangles));
    BLOK_GPU_TRY(mem.alloc(&d_pairs, n_triangles)); BLOK_GPU_TRY(mem.alloc(&d_cols, n_triangles)); BLOK_GPU_TRY(mem.alloc(&d_pair_scan, n_triangles)); BLOK_GPU_TRY(mem.alloc(&d_col_scan, n_triangles));
    BLOK_GPU_TRY(mem.alloc(&d_error, 1)); BLOK_GPU_TRY(mem.alloc(&d_mesh_box, 8 * kSpread));
    if (n_vertices) BLOK_GPU_TRY(hipMemcpy(d_pos, positions, 3 * n_vertices * sizeof(float), hipMemcpyHostToDevice));
    BLOK_GPU_TRY(hipMemcpy(d_tris, triangles, 3 * n_triangles * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (triangle_materials) {
        BLOK_GPU_TRY(mem.alloc(&d_mats, n_triangles));
        BLOK_GPU_TRY(hipMemcpy(d_mats, triangle_materials, n_triangles * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    {
        std::vector<int32_t> init(8 * kSpread);
        for (uint32_t s = 0; s < kSpread; ++s) for (int c = 0; c < 3; ++c) { init[8 * s + c] = INT32_MAX; init[8 * s + 3 + c] = INT32_MIN; }
        BLOK_GPU_TRY(hipMemcpy(d_mesh_box, init.data(), init.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        BLOK_GPU_TRY(hipMemset(d_error, 0, sizeof(uint32_t)));
    }
    SetupArgs s{};
    s.pos = d_pos; s.n_vertices = n_vertices; s.tris = d_tris; s.n_tris = nt;
    const int32_t dims[3] = {int32_t(v->nx), int32_t(v->ny), int32_t(v->nz)};
    for (int c = 0; c < 3; ++c) { s.O[c] = int64_t(v->origin[c]) * vox::kSub; s.n[c] = dims[c]; s.origin[c] = v->origin[c]; }
    s.solid = solid; s.rec = d_rec; s.pair_count = d_pairs; s.col_count = d_cols; s.error = d_error; s.mesh_box = d_mesh_box;
    hipLaunchKernelGGL(vox_setup_kernel, dim3(blocks(nt, 256)), dim3(256), 0, nullptr, s);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(inclusive_scan(mem, d_pairs, d_pair_scan, nt));
    if (solid) BLOK_GPU_TRY(inclusive_scan(mem, d_cols, d_col_scan, nt));
    uint32_t error = 0; uint64_t n_pairs = 0, n_cols = 0;
    std::vector<int32_t> mb(8 * kSpread);
    BLOK_GPU_TRY(hipMemcpy(&error, d_error, sizeof(uint32_t), hipMemcpyDeviceToHost));
    BLOK_GPU_TRY(hipMemcpy(&n_pairs, d_pair_scan + nt - 1, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (solid) BLOK_GPU_TRY(hipMemcpy(&n_cols, d_col_scan + nt - 1, sizeof(uint64_t), hipMemcpyDeviceToHost));
    BLOK_GPU_TRY(hipMemcpy(mb.data(), d_mesh_box, mb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (error) {
        *invalid = true;
        *why = (error & kErrIndex) ? "voxelize: vertex index out of range" : (error & kErrCoord) ? "voxelize: vertex coordinate not finite or beyond 2^23"
                                                                              : "voxelize: triangle extent exceeds 2048 voxels";
        return GpuBuildStatus::Unsupported;
    }
    // the mesh's box, clamped to the volume (box-local): the region of the brick-mask scratch and of the bit volume
    int32_t m0[3], m1[3];
    for (int c = 0; c < 3; ++c) {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (uint32_t k = 0; k < kSpread; ++k) { lo = std::min<int64_t>(lo, mb[8 * k + c]); hi = std::max<int64_t>(hi, mb[8 * k + 3 + c]); }
        m0[c] = static_cast<int32_t>(std::clamp<int64_t>(lo - v->origin[c], 0, dims[c]));
        m1[c] = static_cast<int32_t>(std::clamp<int64_t>(hi + 1 - v->origin[c], 0, dims[c]));
    }
    if (m0[0] >= m1[0] && !solid) return GpuBuildStatus::Ok;
    Region reg{};
    uint64_t reg_bricks = 1;
    for (int c = 0; c < 3; ++c) {
        reg.b0[c] = m0[c] >> 2;
        reg.nb[c] = m1[c] > m0[c] ? static_cast<uint32_t>(((m1[c] - 1) >> 2) - reg.b0[c] + 1) : 0u;
        reg_bricks *= reg.nb[c];
    }
    uint64_t* d_smask; uint32_t *d_list, *d_n_list, *d_box; unsigned long long* d_count;
    const uint64_t list_cap = std::max<uint64_t>(std::min(n_pairs, reg_bricks), 1);
    BLOK_GPU_TRY(mem.alloc(&d_smask, reg_bricks)); BLOK_GPU_TRY(mem.alloc(&d_list, list_cap)); BLOK_GPU_TRY(mem.alloc(&d_n_list, 1));
    BLOK_GPU_TRY(mem.alloc(&d_box, 8 * kSpread)); BLOK_GPU_TRY(mem.alloc(&d_count, kSpread));
    BLOK_GPU_TRY(hipMemset(d_smask, 0, std::max<uint64_t>(reg_bricks, 1) * sizeof(uint64_t)));
    BLOK_GPU_TRY(hipMemset(d_n_list, 0, sizeof(uint32_t)));
    BLOK_GPU_TRY(hipMemset(d_count, 0, kSpread * sizeof(unsigned long long)));
    {
        std::vector<uint32_t> init(8 * kSpread);
        for (uint32_t k = 0; k < kSpread; ++k) for (int c = 0; c < 3; ++c) { init[8 * k + c] = 0xFFFFFFFFu; init[8 * k + 3 + c] = 0u; }
        BLOK_GPU_TRY(hipMemcpy(d_box, init.data(), init.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    const Written wr{d_box, d_count};
    PairArgs pa{};
    pa.rec = d_rec; pa.scan = d_pair_scan; pa.n_tris = nt;
    for (int c = 0; c < 3; ++c) { pa.O[c] = s.O[c]; pa.n[c] = dims[c]; }
    pa.reg = reg; pa.smask = d_smask; pa.list = d_list; pa.n_list = d_n_list; pa.ids = v->d_ids; pa.phase = 0;
    for (uint64_t f = 0; f < n_pairs; f += kPairBatch) {
        const uint64_t e = std::min(n_pairs, f + kPairBatch);
        hipLaunchKernelGGL(vox_pair_kernel, dim3(blocks(e - f, 4)), dim3(256), 0, nullptr, pa, f, e);
        BLOK_GPU_TRY(hipGetLastError());
    }
    uint32_t n_list = 0;
    BLOK_GPU_TRY(hipMemcpy(&n_list, d_n_list, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (std::getenv("BLOK_VOXELIZE_STATS"))         // diagnostic (scripts/voxelize_timing.py): the work lists' sizes
        std::fprintf(stderr, "[voxelize] triangles %u pairs %llu pair_launches %llu touched_bricks %u columns %llu\n", nt, static_cast<unsigned long long>(n_pairs),
                     static_cast<unsigned long long>((n_pairs + kPairBatch - 1) / kPairBatch), n_list, static_cast<unsigned long long>(n_cols));
    if (solid && n_cols && m0[0] < dims[0] && m0[1] < m1[1] && m0[2] < m1[2]) {
        ColumnArgs ca{};
        ca.rec = d_rec; ca.scan = d_col_scan; ca.n_tris = nt; ca.nx = dims[0];
        for (int c = 0; c < 3; ++c) { ca.O[c] = s.O[c]; ca.m0[c] = m0[c]; }
        ca.ry = static_cast<uint32_t>(m1[1] - m0[1]);
        ca.words = static_cast<uint32_t>((dims[0] - m0[0] + 31) / 32);
        const uint64_t rows = uint64_t(ca.ry) * uint64_t(m1[2] - m0[2]);
        BLOK_GPU_TRY(mem.alloc(&ca.bits, rows * ca.words));
        BLOK_GPU_TRY(hipMemset(ca.bits, 0, rows * ca.words * sizeof(uint32_t)));
        for (uint64_t f = 0; f < n_cols; f += kColumnBatch) {
            const uint64_t e = std::min(n_cols, f + kColumnBatch);
            hipLaunchKernelGGL(vox_column_kernel, dim3(blocks(e - f, 256)), dim3(256), 0, nullptr, ca, f, e);
            BLOK_GPU_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(vox_prefix_kernel, dim3(blocks(rows, 256)), dim3(256), 0, nullptr, ca.bits, rows, ca.words);
        BLOK_GPU_TRY(hipGetLastError());
        hipLaunchKernelGGL(vox_interior_kernel, dim3(blocks(rows * uint64_t(dims[0] - m0[0]), 256)), dim3(256), 0, nullptr, ca, dims[1], rows, reg, d_smask,
                           v->d_density, v->d_ids, material, density, wr);
        BLOK_GPU_TRY(hipGetLastError());
    }
    if (n_list) {
        if (d_mats) {
            hipLaunchKernelGGL(vox_clear_ids_kernel, dim3(blocks(n_list, 4)), dim3(256), 0, nullptr, reg, d_smask, d_list, n_list, dims[0], dims[1], v->d_ids);
            BLOK_GPU_TRY(hipGetLastError());
            pa.phase = 1;
            for (uint64_t f = 0; f < n_pairs; f += kPairBatch) {
                const uint64_t e = std::min(n_pairs, f + kPairBatch);
                hipLaunchKernelGGL(vox_pair_kernel, dim3(blocks(e - f, 4)), dim3(256), 0, nullptr, pa, f, e);
                BLOK_GPU_TRY(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(vox_finalize_kernel, dim3(blocks(n_list, 4)), dim3(256), 0, nullptr, reg, d_smask, d_list, n_list, dims[0], dims[1],
                           v->d_density, v->d_ids, d_mats, material, density, wr);
        BLOK_GPU_TRY(hipGetLastError());
    }
    std::vector<uint32_t> box(8 * kSpread);
    std::vector<unsigned long long> counts(kSpread);
    BLOK_GPU_TRY(hipMemcpy(box.data(), d_box, box.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    BLOK_GPU_TRY(hipMemcpy(counts.data(), d_count, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
    uint64_t written = 0;
    for (uint32_t k = 0; k < kSpread; ++k) {
        written += counts[k];
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], box[8 * k + c]); hi[c] = std::max(hi[c], box[8 * k + 3 + c]); }
    }
    if (out_n_voxels) *out_n_voxels = written;
    if (!written) return GpuBuildStatus::Ok;
    const GpuBuildStatus st = gpu_volume_commit(v, lo, hi, Edit::MayFill, why);
    BLOK_GPU_TRY(hipDeviceSynchronize());
    return st;
}

}  // namespace blok
