// Models resampled into the resident volume through an affine map (gpu_build.h: gpu_volume_stamp_affine; include/blok_hip.h:
// blok_hip_volume_stamp_affine).  The rule is ../common/affine_core.h's, shared with the host build.
//
// stamp_kernels.hip pushes model voxels forward, which is hole-free only for a bijection of the lattice.  This kernel runs over the
// DESTINATION cells and pulls: every cell asks the model's tree which voxel lies under its centre.  The two costs of pulling — a tree read
// per cell, and visits to the model's empty space — are met by never looking per cell at what a whole wave can decide:
//   1. cull (host): the region in coarse tiles of 64^3 cells; the exact interval of P over a tile (affine::tile_interval) against the
//      model's voxel box.  The launch covers the box of the surviving tiles; no survivor, no launch.
//   2. a wave per tile of 64 x 4 x 4 cells (shapes_kernels.hip's tile): lane = one x, over sixteen (y, z) rows, so every store instruction
//      of a wave writes one contiguous 256-byte run of density and one of ids.
//   3. wave-uniform descent: the tile's exact interval; gone if it misses the model's box.  While the whole interval lies inside ONE child
//      of the current node the wave descends together — 16-byte node records through the scalar cache — and is gone as soon as that child's
//      mask bit is clear.  Under magnification most waves end inside one brick, many inside one voxel (then the material is one scalar load).
//   4. per-lane descent from that common ancestor for the lane's own voxel: mask bit, popcount rank, child; at the brick the rank into the
//      material array.  Under minification the lanes part early and the node reads are gathers: inherent to the operation.  A row whose
//      own interval misses the model's box is skipped by a scalar branch.
//   5. KEEP adds one coalesced density load per row.  Written cells: a ballot per row, one 64-bit add per wave, spread over kCountSlots words.
// Placements are launched in table order on the null stream, each followed by its gpu_volume_commit; the call's one wait is the counters'.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/affine_core.h"

namespace blok {

namespace {

namespace A = affine;
namespace S = stamp;

constexpr uint32_t kTile[3] = {64, 4, 4};                 // a wave's tile in cells, counted from the volume's corner
constexpr uint32_t kCoarse = 64;                          // the host cull's tile edge
constexpr uint32_t kCountSlots = 32, kSlotWords = 8;      // stamp_kernels.hip's slots: one counter per 64 bytes

struct AffineArgs {
    const uint4* nodes; const uint32_t* materials;
    uint32_t levels;
    int32_t blo[3], bhi[3];         // the box of the model's voxels, counted from the tree's corner, inside the tree's cube
    A::Frame frame;                 // P' of a box-local cell, model coordinates counted from the tree's corner
    uint32_t lo[3], hi[3];          // the cells to visit, box-local, half open, not empty
    uint32_t t0[3], nt[3], n_tiles; // their tiles: the first one and the tiles per axis
    uint32_t nx, ny;
    float* density; uint32_t* ids;
    int mode; float value;
    unsigned long long* counts;     // kCountSlots * kSlotWords
};

__device__ __forceinline__ uint32_t child_bit(uint32_t u0, uint32_t u1, uint32_t u2, uint32_t s) {
    return ((u0 >> s) & 3u) | (((u1 >> s) & 3u) << 2) | (((u2 >> s) & 3u) << 4);
}

// From `node`, whose cell is 4^level voxels wide and holds voxel u (tree coordinates), down to the voxel: false = u is empty; true = filled,
// and with want_material its id.
__device__ __forceinline__ bool lane_descend(const uint4* nodes, const uint32_t* materials, uint4 node, uint32_t level, uint32_t u0, uint32_t u1,
                                             uint32_t u2, bool want_material, uint32_t& material) {
    for (uint32_t l = level; l >= 1u; --l) {
        const uint32_t bit = child_bit(u0, u1, u2, 2u * (l - 1u));
        const uint64_t mask = node_mask(node);
        if (!((mask >> bit) & 1ull)) return false;
        const uint32_t at = node.z + static_cast<uint32_t>(__popcll(mask & ((1ull << bit) - 1ull)));
        if (l == 1u) { material = want_material ? materials[at] : 0u; return true; }
        node = nodes[at];
    }
    return false;
}

__global__ __launch_bounds__(256) void affine_kernel(const AffineArgs a) {
    const uint32_t tile = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= a.n_tiles) return;
    // the tile, cut with the cells to visit (never empty: the tiles are those of [lo, hi))
    const uint32_t ti[3] = {tile % a.nt[0], tile / a.nt[0] % a.nt[1], tile / a.nt[0] / a.nt[1]};
    uint32_t corner[3], tl[3], th[3], ext[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        corner[k] = (a.t0[k] + ti[k]) * kTile[k];
        tl[k] = max(corner[k], a.lo[k]); th[k] = min(corner[k] + kTile[k], a.hi[k]);
        ext[k] = th[k] - tl[k];
    }
    int64_t Plo[3], Phi[3];
    A::tile_interval(a.frame, tl, ext, Plo, Phi);
    if (!A::meets(Plo, Phi, a.blo, a.bhi)) return;                // wholly outside the model's box
    // wave-uniform descent: for as long as the whole interval lies in one child
    uint4 node = uniform_record(a.nodes, 0u);
    uint32_t level = a.levels;                                    // `node`'s cell is 4^level voxels wide
    uint32_t whole_material = 0u;
    bool whole = false;                                           // the tile lies inside one filled voxel
    {
        const int64_t size = int64_t(1) << (2u * a.levels);
        const int64_t l0 = A::voxel(Plo[0]), l1 = A::voxel(Plo[1]), l2 = A::voxel(Plo[2]);
        const int64_t h0 = A::voxel(Phi[0]), h1 = A::voxel(Phi[1]), h2 = A::voxel(Phi[2]);
        if (l0 >= 0 && l1 >= 0 && l2 >= 0 && h0 < size && h1 < size && h2 < size) {
            const uint32_t u0 = static_cast<uint32_t>(l0), u1 = static_cast<uint32_t>(l1), u2 = static_cast<uint32_t>(l2);
            const uint32_t differ = (u0 ^ static_cast<uint32_t>(h0)) | (u1 ^ static_cast<uint32_t>(h1)) | (u2 ^ static_cast<uint32_t>(h2));
            while (level >= 1u) {
                const uint32_t s = 2u * (level - 1u);
                if (differ >> s) break;                           // the interval's ends part at this level
                const uint32_t bit = child_bit(u0, u1, u2, s);
                const uint64_t mask = node_mask(node);
                if (!((mask >> bit) & 1ull)) return;              // the whole tile samples an empty cell of the model
                const uint32_t at = node.z + static_cast<uint32_t>(__popcll(mask & ((1ull << bit) - 1ull)));
                --level;
                if (level == 0u) { whole = true; whole_material = a.mode == BLOK_STAMP_ERASE ? 0u : uniform_word(a.materials, at); break; }
                node = uniform_record(a.nodes, at);
            }
        }
    }
    const uint32_t x = corner[0] + lane;
    const bool in_x = x >= tl[0] && x < th[0];
    int64_t Px[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Px[k] = a.frame.base[k] + int64_t(a.frame.m[k][0]) * int64_t(x);
    uint32_t written = 0;
    for (uint32_t z = tl[2]; z < th[2]; ++z) {
        for (uint32_t y = tl[1]; y < th[1]; ++y) {
            bool hit = in_x;
            uint32_t material = whole_material;
            if (!whole) {
                const uint32_t row_lo[3] = {tl[0], y, z}, row_ext[3] = {ext[0], 1u, 1u};
                int64_t Rlo[3], Rhi[3];
                A::tile_interval(a.frame, row_lo, row_ext, Rlo, Rhi);
                if (!A::meets(Rlo, Rhi, a.blo, a.bhi)) continue;   // wave-uniform: this row misses the model's box
                int64_t u[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    u[k] = A::voxel(Px[k] + (int64_t(a.frame.m[k][1]) * int64_t(y) + int64_t(a.frame.m[k][2]) * int64_t(z)));
                    hit = hit && u[k] >= int64_t(a.blo[k]) && u[k] < int64_t(a.bhi[k]);
                }
                if (hit) hit = lane_descend(a.nodes, a.materials, node, level, static_cast<uint32_t>(u[0]), static_cast<uint32_t>(u[1]),
                                            static_cast<uint32_t>(u[2]), a.mode != BLOK_STAMP_ERASE, material);
            }
            const size_t cell = x + (static_cast<size_t>(z) * a.ny + y) * a.nx;
            bool wrote = false;
            if (hit) {
                const float present = a.mode == BLOK_STAMP_KEEP ? a.density[cell] : 0.0f;
                float d; uint32_t m;
                wrote = S::apply(a.mode, a.value, material, present, d, m);
                if (wrote) { a.density[cell] = d; a.ids[cell] = m; }
            }
            written += static_cast<uint32_t>(__popcll(__ballot(wrote)));
        }
    }
    if (lane == 0u && written) atomicAdd(a.counts + (tile % kCountSlots) * kSlotWords, static_cast<unsigned long long>(written));
}

}  // namespace

GpuBuildStatus gpu_volume_stamp_affine(GpuVolume* v, const StampModel* models, const blok_affine* records, uint32_t n_records, const uint32_t lo[3],
                                       const uint32_t hi[3], int mode, float density, uint64_t* out_n_voxels, std::string* why) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!cells_fit_32_bits(v, "stamp_affine", why)) return GpuBuildStatus::Unsupported;
    if (n_records == 0 || lo[0] >= hi[0] || lo[1] >= hi[1] || lo[2] >= hi[2]) return GpuBuildStatus::Ok;
    DeviceMem mem;
    unsigned long long* d_counts;
    BLOK_GPU_TRY(mem.alloc(&d_counts, kCountSlots * kSlotWords));
    BLOK_GPU_TRY(hipMemsetAsync(d_counts, 0, kCountSlots * kSlotWords * sizeof(unsigned long long), nullptr));
    for (uint32_t i = 0; i < n_records; ++i) {
        const StampModel& M = models[i];
        AffineArgs a{};
        a.nodes = M.nodes; a.materials = M.materials; a.levels = M.levels;
        a.frame = A::frame(records[i], v->origin, M.origin);
        const int64_t size = int64_t(1) << (2u * M.levels);
        bool empty = false;
        for (int k = 0; k < 3; ++k) {
            a.blo[k] = static_cast<int32_t>(std::max<int64_t>(int64_t(M.lo[k]) - M.origin[k], 0));
            a.bhi[k] = static_cast<int32_t>(std::min<int64_t>(int64_t(M.hi[k]) - M.origin[k], size));
            empty = empty || a.blo[k] >= a.bhi[k];
        }
        if (empty) continue;
        // 1. the cull: the box of the coarse tiles whose exact interval meets the model's box, in cells cut with the region
        uint32_t slo[3] = {hi[0], hi[1], hi[2]}, shi[3] = {lo[0], lo[1], lo[2]};
        bool any = false;
        for (uint32_t z0 = lo[2] / kCoarse * kCoarse; z0 < hi[2]; z0 += kCoarse)
            for (uint32_t y0 = lo[1] / kCoarse * kCoarse; y0 < hi[1]; y0 += kCoarse)
                for (uint32_t x0 = lo[0] / kCoarse * kCoarse; x0 < hi[0]; x0 += kCoarse) {
                    const uint32_t c0[3] = {x0, y0, z0};
                    uint32_t tl[3], th[3], ext[3];
                    for (int k = 0; k < 3; ++k) { tl[k] = std::max(c0[k], lo[k]); th[k] = std::min(c0[k] + kCoarse, hi[k]); ext[k] = th[k] - tl[k]; }
                    int64_t Plo[3], Phi[3];
                    A::tile_interval(a.frame, tl, ext, Plo, Phi);
                    if (!A::meets(Plo, Phi, a.blo, a.bhi)) continue;
                    any = true;
                    for (int k = 0; k < 3; ++k) { slo[k] = std::min(slo[k], tl[k]); shi[k] = std::max(shi[k], th[k]); }
                }
        if (!any) continue;                                       // no cell of the region samples the model's box: nothing written, not an error
        uint64_t n_tiles = 1;
        for (int k = 0; k < 3; ++k) {
            a.lo[k] = slo[k]; a.hi[k] = shi[k];
            a.t0[k] = slo[k] / kTile[k];
            a.nt[k] = (shi[k] - 1u) / kTile[k] - a.t0[k] + 1u;
            n_tiles *= a.nt[k];
        }
        a.n_tiles = static_cast<uint32_t>(n_tiles);               // (at most cells / 1024 + the ragged ends: far below 2^32)
        a.nx = v->nx; a.ny = v->ny;
        a.density = v->d_density; a.ids = v->d_ids; a.mode = mode; a.value = density; a.counts = d_counts;
        hipLaunchKernelGGL(affine_kernel, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
        // this record's box alone: two far-apart pastes must not refresh what lies between them
        const GpuBuildStatus st = gpu_volume_commit(v, slo, shi, mode != BLOK_STAMP_ERASE ? Edit::MayFill : Edit::OnlyClears, why);
        if (st != GpuBuildStatus::Ok) return st;
    }
    std::vector<unsigned long long> counts(kCountSlots * kSlotWords);
    BLOK_GPU_TRY(hipMemcpy(counts.data(), d_counts, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));      // the call's one wait: behind every launch above
    uint64_t written = 0;
    for (uint32_t s = 0; s < kCountSlots; ++s) written += counts[s * kSlotWords];
    if (out_n_voxels) *out_n_voxels = written;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
