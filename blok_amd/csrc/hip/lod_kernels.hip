// The resident volume reduced to a pyramid of coarser levels (gpu_build.h: gpu_volume_reduce; include/blok_hip.h: blok_hip_volume_reduce
// has the contract; the rule lives in ../common/lod_core.h, shared with the host build).
//
// Level 1: a wave owns 64 consecutive level-1 cells of one row of the level's grid (row_segment), that is 128 voxels along x of 2 x 2 voxel
//   rows.  Those lie in at most 33 bricks along x of at most 2 x 2 brick rows (the box origin is arbitrary: a coarse cell may straddle
//   bricks on every axis).  Per brick row, lane k < 34 takes brick k of the run: its mask word and, where that holds a voxel, its six
//   neighbours', in either layout (BrickMasks::part: three parts per lane and wave, the brick row's six scalar), never the densities, and
//   from them the brick's exposed cells in one bit-parallel step (lod::brick_exposed); a brick row is computed once for the voxel rows
//   that share it.  Each lane then fetches the four bits of its voxel row from the lane that holds
//   its brick (one shuffle per child).  Ids are loaded only where a child is filled — a wave over empty masks loads none — as the
//   contiguous run of the wave's 128 voxels, each lane its pair, in one 8-byte load where the pair is aligned.
// Level 1 of blok_hip_terrain_reduce (gpu_terrain_reduce) comes from the terrain function instead, with no volume behind
//   it: terrain_lod_kernel below, over the tile arithmetic of ../common/terrain_lod_core.h.  Everything after level 1 is shared
//   (reduce_levels).
// Levels 2 .. K: a lane per cell, eight children read from the planes below (lod::cell_above), nothing else.
// Counts: per wave two ballots and two shuffle sums, then one atomic instruction of four lanes into one of kSlots rows of the level's four
//   counters; the host adds the rows.  No wave waits for another; nothing is allocated beyond the snapshot and the counters.
// Everything is on the null stream, behind earlier edits.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/lod_core.h"
#include "../common/terrain_lod_core.h"

namespace blok {

namespace {

namespace K = lod;
namespace T = terrain;
namespace TL = terrain_lod;

constexpr uint32_t kSlots = 64u, kCounters = 4u;      // per level: kSlots rows of (cells with n > 0, cells with e > 0, sum of n, sum of e)

// Called by every lane of a wave with its cell's n and e (0 for a lane without a cell).
__device__ __forceinline__ void count_wave(uint32_t n, uint32_t e, uint64_t wave, unsigned long long* counters) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_filled = static_cast<uint32_t>(__popcll(__ballot(n != 0u))), n_exposed = static_cast<uint32_t>(__popcll(__ballot(e != 0u)));
    if (!n_filled) return;                                  // (wave-uniform; e <= n)
    uint32_t sum_n = n, sum_e = e;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum_n += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum_n), d));
        sum_e += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum_e), d));
    }
    if (lane < kCounters) {
        const uint32_t value = lane == 0u ? n_filled : lane == 1u ? n_exposed : lane == 2u ? sum_n : sum_e;
        if (value) atomicAdd(counters + (wave % kSlots) * kCounters + lane, static_cast<unsigned long long>(value));
    }
}

struct Level1Args {
    BrickMasks masks;
    const uint32_t* ids;
    uint32_t dims[3], nb[3];
    uint32_t lo[3], hi[3];                            // the region, box-local
    int32_t base[3];                                  // box-local voxel of child 0 of the grid's first cell: lo or lo - 1 per axis
    uint32_t cext[3], x_chunks, flags;
    uint64_t n_waves;
    uint16_t* n; uint16_t* e; uint32_t* id;
    unsigned long long* counters;
};

__global__ __launch_bounds__(256) void lod_level1_kernel(const Level1Args a) {
    const uint64_t wave = blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;                          // (a whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t xc, cy, cz;
    row_segment(wave, a.x_chunks, a.cext[1], xc, cy, cz);
    // (a wave's segment is the same in every lane: in scalar registers, what depends on it alone — the voxel rows, their brick rows and
    // those bricks' parts of the mask index — is scalar work)
    xc = __builtin_amdgcn_readfirstlane(xc); cy = __builtin_amdgcn_readfirstlane(cy); cz = __builtin_amdgcn_readfirstlane(cz);
    const uint32_t cx = xc * 64u + lane;
    const bool live = cx < a.cext[0];
    const int32_t wx0 = a.base[0] + static_cast<int32_t>(xc * 128u);      // the wave's first voxel along x; -1 only in front of the box
    const uint32_t bx0 = wx0 < 0 ? 0u : static_cast<uint32_t>(wx0) >> 2;
    const int32_t x0 = wx0 + static_cast<int32_t>(2u * lane);             // the lane's pair: x0, x0 + 1
    // a brick's index is the sum of its three coordinates' parts (BrickMasks::part): the lane's brick and its two neighbours along x once
    // per wave, the brick row's and its neighbours' along y and z once per brick row
    const uint32_t bx = bx0 + lane;
    const bool has_brick = lane < 34u && bx < a.nb[0];
    uint64_t px[3] = {0ull, 0ull, 0ull};
    if (has_brick) { px[0] = a.masks.part(bx - 1u, 0u); px[1] = a.masks.part(bx, 0u); px[2] = a.masks.part(bx + 1u, 0u); }      // (a part of a brick beyond the grid is never used)
    uint32_t fbits = 0u, ebits = 0u, ids[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t held_by = 0xFFFFFFFFu, held_bz = 0xFFFFFFFFu;
    uint64_t m = 0ull, open = 0ull;                         // of brick bx0 + lane of brick row (held_by, held_bz)
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const int32_t vy = a.base[1] + static_cast<int32_t>(2u * cy + (r & 1u)), vz = a.base[2] + static_cast<int32_t>(2u * cz + (r >> 1));
        if (vy < static_cast<int32_t>(a.lo[1]) || vy >= static_cast<int32_t>(a.hi[1]) || vz < static_cast<int32_t>(a.lo[2]) || vz >= static_cast<int32_t>(a.hi[2]))
            continue;                                       // (wave-uniform) a voxel row outside the region contributes nothing
        const uint32_t y = static_cast<uint32_t>(vy), z = static_cast<uint32_t>(vz);
        if ((y >> 2) != held_by || (z >> 2) != held_bz) {
            held_by = y >> 2; held_bz = z >> 2;
            m = 0ull; open = 0ull;
            const uint64_t py[3] = {a.masks.part(held_by - 1u, 1u), a.masks.part(held_by, 1u), a.masks.part(held_by + 1u, 1u)};
            const uint64_t pz[3] = {a.masks.part(held_bz - 1u, 2u), a.masks.part(held_bz, 2u), a.masks.part(held_bz + 1u, 2u)};
            const auto at = [&](uint32_t qx, uint32_t qy, uint32_t qz) { return a.masks.masks[px[qx - bx + 1u] + py[qy - held_by + 1u] + pz[qz - held_bz + 1u]]; };
            if (has_brick) open = K::brick_exposed(at, bx, held_by, held_bz, a.nb, a.dims, &m);
        }
        const uint32_t shift = ((y & 3u) << 2) | ((z & 3u) << 4);
        const uint32_t row_bits = (static_cast<uint32_t>(m >> shift) & 15u) | ((static_cast<uint32_t>(open >> shift) & 15u) << 4);
        uint32_t f[2], e[2];
#pragma unroll
        for (uint32_t dx = 0; dx < 2u; ++dx) {
            const int32_t vx = x0 + static_cast<int32_t>(dx);
            const bool in = live && vx >= static_cast<int32_t>(a.lo[0]) && vx < static_cast<int32_t>(a.hi[0]);
            const uint32_t from = in ? (static_cast<uint32_t>(vx) >> 2) - bx0 : 0u;      // < 34
            const uint32_t bits = static_cast<uint32_t>(__shfl(static_cast<int>(row_bits), static_cast<int>(from)));
            f[dx] = in ? (bits >> (static_cast<uint32_t>(vx) & 3u)) & 1u : 0u;
            e[dx] = in ? (bits >> (4u + (static_cast<uint32_t>(vx) & 3u))) & 1u : 0u;
        }
        fbits |= (f[0] | (f[1] << 1)) << (2u * r);
        ebits |= (e[0] | (e[1] << 1)) << (2u * r);
        if (f[0] | f[1]) {                                  // (a filled child lies in the region, so x0 + dx < dims[0] where f[dx])
            const size_t at0 = (static_cast<size_t>(z) * a.dims[1] + y) * a.dims[0] + static_cast<size_t>(static_cast<int64_t>(x0));
            if (f[0] && f[1] && !(at0 & 1u)) {
                const uint2 pair = *reinterpret_cast<const uint2*>(a.ids + at0);
                ids[2u * r] = pair.x; ids[2u * r + 1u] = pair.y;
            } else {
                if (f[0]) ids[2u * r] = a.ids[at0];
                if (f[1]) ids[2u * r + 1u] = a.ids[at0 + 1u];
            }
        }
    }
    uint32_t cn[8], ce[8];
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) { cn[c] = (fbits >> c) & 1u; ce[c] = (ebits >> c) & 1u; }
    uint32_t n, e, id;
    K::cell_of(cn, ce, ids, a.flags, &n, &e, &id);
    if (live) {
        const uint64_t i = cx + a.cext[0] * (cy + static_cast<uint64_t>(a.cext[1]) * cz);
        a.n[i] = static_cast<uint16_t>(n); a.e[i] = static_cast<uint16_t>(e); a.id[i] = id;
    }
    count_wave(n, e, wave, a.counters);
}

struct LevelArgs {
    K::Below below;
    uint32_t cext[3], flags;
    uint64_t n_cells;
    uint16_t* n; uint16_t* e; uint32_t* id;
    unsigned long long* counters;
};

__global__ __launch_bounds__(256) void lod_level_kernel(const LevelArgs a) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t n = 0u, e = 0u, id = 0u;
    if (i < a.n_cells) {
        const uint32_t cx = static_cast<uint32_t>(i % a.cext[0]);
        const uint64_t row = i / a.cext[0];
        K::cell_above(a.below, cx, static_cast<uint32_t>(row % a.cext[1]), static_cast<uint32_t>(row / a.cext[1]), a.flags, &n, &e, &id);
        a.n[i] = static_cast<uint16_t>(n); a.e[i] = static_cast<uint16_t>(e); a.id[i] = id;
    }
    count_wave(n, e, i >> 6, a.counters);
}

// ---- level 1 from the terrain function (gpu_terrain_reduce) --------------------------------------------------------------------------------
// count_wave for lanes that have each added up several cells: four sums per lane, four shuffle sums and the same one atomic instruction.
__device__ __forceinline__ void count_lanes(uint32_t n_filled, uint32_t n_exposed, uint32_t sum_n, uint32_t sum_e, uint64_t wave, unsigned long long* counters) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n_filled += static_cast<uint32_t>(__shfl_xor(static_cast<int>(n_filled), d));
        n_exposed += static_cast<uint32_t>(__shfl_xor(static_cast<int>(n_exposed), d));
        sum_n += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum_n), d));
        sum_e += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum_e), d));
    }
    if (lane < kCounters) {
        const uint32_t value = lane == 0u ? n_filled : lane == 1u ? n_exposed : lane == 2u ? sum_n : sum_e;
        if (value) atomicAdd(counters + (wave % kSlots) * kCounters + lane, static_cast<unsigned long long>(value));
    }
}

struct TerrainLodArgs {
    blok_terrain_params p;
    int32_t lo[3], hi[3];                             // the region, world voxels
    int32_t base[3];                                  // world voxel of child 0 of the grid's first cell: 2 clo, even
    uint32_t cext[3], flags;
    uint16_t* n; uint16_t* e; uint32_t* id;
    unsigned long long* counters;
};

// A workgroup owns a tile (terrain_lod_core.h): kTileX x kTileZ columns, kSlab rows, 32 x 32 x 8 level-1 cells.
//   1. a lane per column of the tile and of its halo (kCols = 1188 columns, 4.6 per lane; the halo is 14 % of them, and its columns take
//      no ore): the height, then one walk up the rows with terrain::solid, the column left in LDS as a word and two halo bits;
//   2. a lane per column of the tile: the exposed word from six words; a tile without a filled voxel stores zeros and is done;
//   3. the same lanes: the ore noise for the voxels whose id can vote (terrain_lod::voters), rising along y;
//   4. a lane per 2 x 2 columns walks up its 32 cells (terrain_lod::cell): lanes 0 .. 31 of a wave store 32 consecutive cells of one
//      row of the grid, lanes 32 .. 63 those of the next row along z, in each of the three planes; the counts are added up per lane and
//      leave the wave once (count_lanes).
// Every noise evaluation sits in a loop that is not unrolled (terrain_lod::column_solid, column_ore).
__global__ __launch_bounds__(256) void terrain_lod_kernel(const TerrainLodArgs a) {
    __shared__ uint64_t s_solid[TL::kCols];
    __shared__ int32_t s_height[TL::kCols];
    __shared__ uint8_t s_halo[TL::kCols];
    __shared__ uint64_t s_exposed[TL::kInner], s_ore[TL::kInner];
    const blok_terrain_params& p = a.p;
    const int32_t x0 = a.base[0] + static_cast<int32_t>(blockIdx.x * TL::kTileX), y0 = a.base[1] + static_cast<int32_t>(blockIdx.y * TL::kSlab),
                  z0 = a.base[2] + static_cast<int32_t>(blockIdx.z * TL::kTileZ);
    const int32_t grow = (a.flags & BLOK_LOD_SEAMLESS) ? 1 : 0;      // the evaluated box: the region, under SEAMLESS grown by a voxel
    T::Walker w;
#pragma unroll 1
    for (uint32_t c = threadIdx.x; c < TL::kCols; c += 256u) {
        const uint32_t hx = c % TL::kColsX, hz = c / TL::kColsX;
        const int32_t X = x0 - 1 + static_cast<int32_t>(hx), Z = z0 - 1 + static_cast<int32_t>(hz);
        const bool corner = (hx == 0u || hx == TL::kColsX - 1u) && (hz == 0u || hz == TL::kColsZ - 1u);      // nobody's neighbour
        TL::Column col = TL::outside();
        int32_t H = 0;
        if (!corner && X >= a.lo[0] - grow && X < a.hi[0] + grow && Z >= a.lo[2] - grow && Z < a.hi[2] + grow) {
            H = T::height(p, X, Z);
            T::walker_reset(w);
            col = TL::column_solid(p, w, X, Z, H, y0, a.lo[1] - grow, a.hi[1] + grow);
        }
        s_solid[c] = col.solid; s_height[c] = H; s_halo[c] = static_cast<uint8_t>(col.halo);
    }
    __syncthreads();
    const uint64_t rows = TL::rows_in(y0, a.lo[1], a.hi[1]);
    // column i of the tile (x fastest): its index among the halo'd columns, and its filled word
    const auto halo_index = [](uint32_t i) { return (i % TL::kTileX + 1u) + (i / TL::kTileX + 1u) * TL::kColsX; };
    const auto filled_of = [&](uint32_t i) -> uint64_t {
        const int32_t X = x0 + static_cast<int32_t>(i % TL::kTileX), Z = z0 + static_cast<int32_t>(i / TL::kTileX);
        return (X >= a.lo[0] && X < a.hi[0] && Z >= a.lo[2] && Z < a.hi[2]) ? s_solid[halo_index(i)] & rows : 0ull;
    };
    int any = 0;
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < TL::kInner; i += 256u) {
        const uint32_t c = halo_index(i);
        const uint64_t filled = filled_of(i);
        const TL::Column col{s_solid[c], s_halo[c]};
        s_exposed[i] = TL::exposed(filled, col, s_solid[c - 1u], s_solid[c + 1u], s_solid[c - TL::kColsX], s_solid[c + TL::kColsX]);
        any |= filled != 0ull;
    }
    any = __syncthreads_or(any);
    const uint32_t cx = blockIdx.x * (TL::kTileX / 2u) + (threadIdx.x & 31u), cz = blockIdx.z * (TL::kTileZ / 2u) + (threadIdx.x >> 5);
    const uint32_t cy0 = blockIdx.y * (TL::kSlab / 2u);
    const bool live = cx < a.cext[0] && cz < a.cext[2];
    const uint64_t at0 = cx + a.cext[0] * (cy0 + static_cast<uint64_t>(a.cext[1]) * cz);
    if (!any) {                                                 // (the whole workgroup) above the heights, or in a cave: zeros, no count
        if (live)
            for (uint32_t pair = 0; pair < TL::kSlab / 2u && cy0 + pair < a.cext[1]; ++pair) {
                const uint64_t i = at0 + static_cast<uint64_t>(a.cext[0]) * pair;
                a.n[i] = 0u; a.e[i] = 0u; a.id[i] = 0u;
            }
        return;
    }
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < TL::kInner; i += 256u) {
        const uint32_t c = halo_index(i);
        const uint64_t cell_exposed = s_exposed[i] | s_exposed[i ^ 1u] | s_exposed[i ^ TL::kTileX] | s_exposed[i ^ 1u ^ TL::kTileX];
        uint64_t soil, deep;
        TL::depth_words(s_height[c], y0, p.soil_depth, &soil, &deep);
        const uint64_t want = TL::voters(filled_of(i), s_exposed[i], cell_exposed, a.flags) & deep;
        T::walker_reset(w);
        s_ore[i] = TL::column_ore(p, w, x0 + static_cast<int32_t>(i % TL::kTileX), z0 + static_cast<int32_t>(i / TL::kTileX), s_height[c], y0, want);
    }
    __syncthreads();
    TL::Words col[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t i = 2u * (threadIdx.x & 31u) + (q & 1u) + (2u * (threadIdx.x >> 5) + (q >> 1)) * TL::kTileX;
        col[q].filled = filled_of(i); col[q].exposed = s_exposed[i]; col[q].ore = s_ore[i];
        TL::depth_words(s_height[halo_index(i)], y0, p.soil_depth, &col[q].soil, &col[q].deep);
    }
    uint32_t n_filled = 0u, n_exposed = 0u, sum_n = 0u, sum_e = 0u;
#pragma unroll 1
    for (uint32_t pair = 0; pair < TL::kSlab / 2u; ++pair) {
        if (!live || cy0 + pair >= a.cext[1]) break;
        uint32_t n, e, id;
        TL::cell(col, pair, p, a.flags, &n, &e, &id);
        const uint64_t i = at0 + static_cast<uint64_t>(a.cext[0]) * pair;
        a.n[i] = static_cast<uint16_t>(n); a.e[i] = static_cast<uint16_t>(e); a.id[i] = id;
        n_filled += n ? 1u : 0u; n_exposed += e ? 1u : 0u; sum_n += n; sum_e += e;
    }
    count_lanes(n_filled, n_exposed, sum_n, sum_e, (blockIdx.x + gridDim.x * (blockIdx.y + static_cast<uint64_t>(gridDim.y) * blockIdx.z)) * 4ull + (threadIdx.x >> 6), a.counters);
}

}  // namespace

void gpu_lod_free(GpuLod* l) {
    if (l->d_planes) (void)hipFree(l->d_planes);
    *l = GpuLod{};
}

namespace {

// What every producer of a pyramid shares: the snapshot and the counters allocated and cleared, level 1 by `level1` (which launches its
// kernel over the level's planes and counter rows), levels 2 .. K from the planes below, the counts added into the info.  out->info is
// the plan, counts zero; on a failure nothing is kept.
struct Level1Planes {
    const blok_lod_level& L;
    uint16_t* n; uint16_t* e; uint32_t* id;
    unsigned long long* counters;
};
template <class Level1>
GpuBuildStatus reduce_levels(uint32_t levels, uint32_t flags, GpuLod* out, std::string* why, const Level1& level1) {
    blok_lod_info& info = out->info;
    const uint64_t bytes = K::total_bytes(info);
    if (!bytes) return GpuBuildStatus::Ok;
    DeviceMem mem;
    uint8_t* d_planes;
    unsigned long long* d_counters;
    const uint32_t n_counters = levels * kSlots * kCounters;
    BLOK_GPU_TRY(mem.alloc(&d_planes, bytes));
    BLOK_GPU_TRY(mem.alloc(&d_counters, static_cast<uint64_t>(n_counters)));
    BLOK_GPU_TRY(hipMemsetAsync(d_counters, 0, n_counters * sizeof(unsigned long long), nullptr));
    // (edits are enqueued on the null stream, and so is this: it reads the masks and the ids they leave)
    for (uint32_t j = 1; j <= levels; ++j) {
        const blok_lod_level& L = info.level[j - 1u];
        uint8_t* at = d_planes + K::level_offset(info, j);
        uint16_t* d_n = reinterpret_cast<uint16_t*>(at + K::plane_offset(L.n_cells, 0u));
        uint16_t* d_e = reinterpret_cast<uint16_t*>(at + K::plane_offset(L.n_cells, 1u));
        uint32_t* d_id = reinterpret_cast<uint32_t*>(at + K::plane_offset(L.n_cells, 2u));
        unsigned long long* counters = d_counters + static_cast<size_t>(j - 1u) * kSlots * kCounters;
        if (j == 1u) {
            level1(Level1Planes{L, d_n, d_e, d_id, counters});
        } else {
            LevelArgs a{};
            a.below = K::below_of(info, j, d_planes);
            for (int k = 0; k < 3; ++k) a.cext[k] = L.cext[k];
            a.flags = flags; a.n_cells = L.n_cells;
            a.n = d_n; a.e = d_e; a.id = d_id; a.counters = counters;
            hipLaunchKernelGGL(lod_level_kernel, dim3(blocks_for(L.n_cells)), dim3(256), 0, nullptr, a);
        }
        BLOK_GPU_TRY(hipGetLastError());
    }
    std::vector<unsigned long long> counts(n_counters);
    BLOK_GPU_TRY(hipMemcpy(counts.data(), d_counters, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost));      // the call's wait
    for (uint32_t j = 1; j <= levels; ++j) {
        blok_lod_level& L = info.level[j - 1u];
        for (uint32_t s = 0; s < kSlots; ++s) {
            const unsigned long long* row = counts.data() + (static_cast<size_t>(j - 1u) * kSlots + s) * kCounters;
            L.n_filled += row[0]; L.n_exposed += row[1]; L.sum_n += row[2]; L.sum_e += row[3];
        }
    }
    mem.release(d_planes);
    out->d_planes = d_planes;
    return GpuBuildStatus::Ok;
}

}  // namespace

GpuBuildStatus gpu_volume_reduce(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t levels, uint32_t flags, GpuLod* out,
                                 std::string* why) {
    *out = GpuLod{};
    if (!cells_fit_32_bits(v, "volume_reduce", why)) return GpuBuildStatus::Unsupported;
    K::plan(v->origin, lo, hi, levels, flags, &out->info);
    return reduce_levels(levels, flags, out, why, [&](const Level1Planes& to) {
        const blok_lod_level& L = to.L;
        Level1Args a{};
        a.masks = brick_masks_of(*v); a.ids = v->d_ids;
        a.dims[0] = v->nx; a.dims[1] = v->ny; a.dims[2] = v->nz; a.nb[0] = v->nbx; a.nb[1] = v->nby; a.nb[2] = v->nbz;
        for (int k = 0; k < 3; ++k) {
            a.lo[k] = lo[k]; a.hi[k] = hi[k]; a.cext[k] = L.cext[k];
            a.base[k] = static_cast<int32_t>(2 * int64_t(L.clo[k]) - v->origin[k]);
        }
        a.x_chunks = (L.cext[0] + 63u) / 64u; a.flags = flags;
        a.n_waves = static_cast<uint64_t>(a.x_chunks) * L.cext[1] * L.cext[2];      // at most 2^32 / 8 cells: 2^27 blocks
        a.n = to.n; a.e = to.e; a.id = to.id; a.counters = to.counters;
        hipLaunchKernelGGL(lod_level1_kernel, dim3(static_cast<uint32_t>((a.n_waves + 3u) / 4u)), dim3(256), 0, nullptr, a);
    });
}

GpuBuildStatus gpu_terrain_reduce(const blok_terrain_params& params, const int32_t lo[3], const int32_t hi[3], uint32_t levels, uint32_t flags,
                                  GpuLod* out, std::string* why) {
    *out = GpuLod{};
    TL::plan(lo, hi, levels, flags, &out->info);
    return reduce_levels(levels, flags, out, why, [&](const Level1Planes& to) {
        const blok_lod_level& L = to.L;
        TerrainLodArgs a{};
        a.p = params; a.flags = flags;
        for (int k = 0; k < 3; ++k) { a.lo[k] = lo[k]; a.hi[k] = hi[k]; a.base[k] = 2 * L.clo[k]; a.cext[k] = L.cext[k]; }
        a.n = to.n; a.e = to.e; a.id = to.id; a.counters = to.counters;
        // (extents of at most 65536 voxels: at most 1025 x 1025 x 4097 tiles)
        const dim3 grid((2u * L.cext[0] + TL::kTileX - 1u) / TL::kTileX, (2u * L.cext[1] + TL::kSlab - 1u) / TL::kSlab, (2u * L.cext[2] + TL::kTileZ - 1u) / TL::kTileZ);
        hipLaunchKernelGGL(terrain_lod_kernel, grid, dim3(256), 0, nullptr, a);
    });
}

}  // namespace blok
