// Procedural terrain into the resident volume (gpu_build.h: gpu_volume_generate_terrain; include/blok_hip.h:
// blok_hip_volume_generate_terrain).  The arithmetic is ../common/terrain_core.h; DESIGN.md §13 has the contract and the measured cost.
//
// terrain_kernel, a lane per (x, z) column of the region, consecutive lanes along x, a workgroup per 256 columns and kRows rows of y:
//   - the column's height (and, for SHELL, the four neighbouring columns') is taken once and stays in registers while the lane walks up
//     its rows; without caves a voxel is two compares against them;
//   - the 3-D noises keep the lattice cell they are in (terrain::Walker): eight hashes when the walk enters a cell, lerps inside it;
//   - a wave writes 64 consecutive voxels of a row with one 256-byte store per array;
//   - SHELL with caves judges the six neighbours by the function: the rows above and below roll through the walk (the loop starts two
//     rows early), the x and z neighbours are evaluated, by one loop, only for a solid voxel that nothing has exposed yet.
// Every noise evaluation sits in a loop that is not unrolled, so each variant holds one copy of the cave and ore code (registers:
// DESIGN.md §13).  The count and the box of the filled voxels are reduced per wave with shuffles, per workgroup through LDS, then one
// lane takes seven integer atomics into one of kSpread copies.  gpu_volume_commit over the written box leaves masks, occupancy words and
// dirty flags.
// (The same function reduced straight to coarse levels, with no volume written: blok_hip_terrain_reduce, lod_kernels.hip: terrain_lod_kernel.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/terrain_core.h"

namespace blok {

namespace {

namespace T = terrain;

constexpr uint32_t kSpread = 16;        // copies of the reduction words (one lane per workgroup adds to them)
constexpr uint32_t kRows = 64;          // y rows per workgroup
constexpr uint32_t kWords = 8;          // per copy: count lo, count hi (one uint64), x/y/z min, x/y/z max (exclusive)

struct TerrainArgs {
    blok_terrain_params p;
    float* density; uint32_t* ids;
    int32_t origin[3];
    uint32_t nx, ny;
    uint32_t lo[3], hi[3];              // region, box-local, half-open
    uint32_t n_items;                   // columns of the region: (hi[0] - lo[0]) * (hi[2] - lo[2])
    uint32_t* words;                    // [kSpread][kWords]
};

template <bool kShell, bool kCaves>
__global__ __launch_bounds__(256) void terrain_kernel(const TerrainArgs a) {
    const blok_terrain_params& p = a.p;
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    uint32_t cnt = 0, ymin = 0xFFFFFFFFu, ymax = 0, lx = 0, lz = 0;
    if (item < a.n_items) {
        const uint32_t row_x = a.hi[0] - a.lo[0];
        lx = a.lo[0] + item % row_x;
        lz = a.lo[2] + item / row_x;
        const uint32_t y0 = a.lo[1] + blockIdx.y * kRows, y1 = min(a.hi[1], y0 + kRows);
        const int32_t X = a.origin[0] + static_cast<int32_t>(lx), Z = a.origin[2] + static_cast<int32_t>(lz);
        const bool add = (p.flags & BLOK_TERRAIN_ADD) != 0u, closed = (p.flags & BLOK_TERRAIN_CLOSE_SIDES) != 0u;
        // the column's height and, for SHELL, its four neighbours' (q = 1..4: x - 1, x + 1, z - 1, z + 1); "never solid" for a column
        // that CLOSE_SIDES shuts out
        int32_t H = 0, Hn[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int q = 0; q < (kShell ? 5 : 1); ++q) {
            const int32_t dx = q == 1 ? -1 : q == 2 ? 1 : 0, dz = q == 3 ? -1 : q == 4 ? 1 : 0;
            const int32_t cx = static_cast<int32_t>(lx) + dx, cz = static_cast<int32_t>(lz) + dz;
            const bool shut = closed && (cx < static_cast<int32_t>(a.lo[0]) || cx >= static_cast<int32_t>(a.hi[0]) || cz < static_cast<int32_t>(a.lo[2]) || cz >= static_cast<int32_t>(a.hi[2]));
            const int32_t h = shut ? INT32_MIN : T::height(p, X + dx, Z + dz);
            if (q == 0) H = h;
            if (q == 1) Hn[0] = h;
            if (q == 2) Hn[1] = h;
            if (q == 3) Hn[2] = h;
            if (q == 4) Hn[3] = h;
        }
        // SHELL without caves: the voxel under a solid one is solid, so a voxel is exposed from the lowest neighbouring top + 1 upwards
        const int32_t from = kShell ? min(H, min(min(Hn[0], Hn[1]), min(Hn[2], Hn[3])) + 1) : INT32_MIN;
        T::Walker w;
        T::walker_reset(w);
        bool below = false, here = false;
        // SHELL with caves starts two rows early: the first two trips only fill `below` and `here`
        const int32_t first = static_cast<int32_t>(y0) - ((kShell && kCaves) ? 2 : 0);
#pragma unroll 1
        for (int32_t ly = first; ly < static_cast<int32_t>(y1); ++ly) {
            const int32_t Y = a.origin[1] + ly;
            bool fill;
            if constexpr (!kCaves) fill = Y <= H && Y >= from;
            else if constexpr (!kShell) fill = T::solid(p, w, X, Y, Z, H);
            else {
                // one evaluation site: q = 0 is the voxel above, q = 1..4 the x and z neighbours of a solid voxel nothing has exposed yet
                bool above = false, candidate = false, exposed = false;
#pragma unroll 1
                for (int q = 0; q < 5; ++q) {
                    if (q > 0 && (!candidate || exposed)) continue;      // (a `break` here costs the compiler 30 more scalar registers)
                    const int32_t dx = q == 1 ? -1 : q == 2 ? 1 : 0, dz = q == 3 ? -1 : q == 4 ? 1 : 0;
                    const int32_t h = q == 0 ? H : q == 1 ? Hn[0] : q == 2 ? Hn[1] : q == 3 ? Hn[2] : Hn[3];
                    const bool s = T::solid(p, w, X + dx, Y + (q == 0 ? 1 : 0), Z + dz, h);
                    if (q == 0) { above = s; candidate = ly >= static_cast<int32_t>(y0) && here; exposed = !above || !below; }
                    else exposed = !s;
                }
                fill = candidate && exposed;
                below = here; here = above;
                if (ly < static_cast<int32_t>(y0)) continue;
            }
            const size_t at = (static_cast<size_t>(lz) * a.ny + static_cast<uint32_t>(ly)) * a.nx + lx;
            if (fill) {
                a.density[at] = p.density;
                a.ids[at] = T::material(p, w, X, Y, Z, H);
                ++cnt; ymin = min(ymin, static_cast<uint32_t>(ly)); ymax = max(ymax, static_cast<uint32_t>(ly) + 1u);
            } else if (!add) {
                a.density[at] = 0.0f;
                a.ids[at] = 0u;
            }
        }
    }
    // the filled voxels' count and box: per wave, per workgroup, then one lane's atomics
    uint32_t xmin = 0xFFFFFFFFu, xmax = 0, zmin = 0xFFFFFFFFu, zmax = 0;
    if (cnt) { xmin = lx; xmax = lx + 1u; zmin = lz; zmax = lz + 1u; }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        xmin = min(xmin, static_cast<uint32_t>(__shfl_xor(xmin, o))); xmax = max(xmax, static_cast<uint32_t>(__shfl_xor(xmax, o)));
        ymin = min(ymin, static_cast<uint32_t>(__shfl_xor(ymin, o))); ymax = max(ymax, static_cast<uint32_t>(__shfl_xor(ymax, o)));
        zmin = min(zmin, static_cast<uint32_t>(__shfl_xor(zmin, o))); zmax = max(zmax, static_cast<uint32_t>(__shfl_xor(zmax, o)));
    }
    __shared__ uint32_t part[4][7];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { part[wave][0] = cnt; part[wave][1] = xmin; part[wave][2] = ymin; part[wave][3] = zmin; part[wave][4] = xmax; part[wave][5] = ymax; part[wave][6] = zmax; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0, lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            total += part[k][0];
            for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], part[k][1 + c]); hi[c] = max(hi[c], part[k][4 + c]); }
        }
        if (total) {
            uint32_t* slot = a.words + ((blockIdx.x + 7u * blockIdx.y) % kSpread) * kWords;
            atomicAdd(reinterpret_cast<unsigned long long*>(slot), static_cast<unsigned long long>(total));
            for (int c = 0; c < 3; ++c) { atomicMin(slot + 2 + c, lo[c]); atomicMax(slot + 5 + c, hi[c]); }
        }
    }
}

}  // namespace

GpuBuildStatus gpu_volume_generate_terrain(GpuVolume* v, const blok_terrain_params& params, const uint32_t lo[3], const uint32_t hi[3],
                                           uint64_t* out_n_voxels, std::string* why) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!cells_fit_32_bits(v, "generate_terrain", why)) return GpuBuildStatus::Unsupported;
    if (lo[0] >= hi[0] || lo[1] >= hi[1] || lo[2] >= hi[2]) return GpuBuildStatus::Ok;
    TerrainArgs a{};
    a.p = params; a.density = v->d_density; a.ids = v->d_ids; a.nx = v->nx; a.ny = v->ny;
    for (int c = 0; c < 3; ++c) { a.origin[c] = v->origin[c]; a.lo[c] = lo[c]; a.hi[c] = hi[c]; }
    const uint64_t items = static_cast<uint64_t>(hi[0] - lo[0]) * (hi[2] - lo[2]);
    a.n_items = static_cast<uint32_t>(items);                    // (below 2^32: the volume has fewer cells than that)
    std::vector<uint32_t> words(kSpread * kWords, 0u);
    for (uint32_t k = 0; k < kSpread; ++k) for (int c = 0; c < 3; ++c) words[k * kWords + 2 + c] = 0xFFFFFFFFu;
    DeviceMem mem;
    BLOK_GPU_TRY(mem.alloc(&a.words, words.size()));
    BLOK_GPU_TRY(hipMemcpy(a.words, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    const dim3 grid(static_cast<uint32_t>((items + 255u) / 256u), (hi[1] - lo[1] + kRows - 1u) / kRows);
    const bool shell = params.flags & BLOK_TERRAIN_SHELL, caves = params.cave_octaves != 0u;
    if (shell && caves) hipLaunchKernelGGL((terrain_kernel<true, true>), grid, dim3(256), 0, nullptr, a);
    else if (shell) hipLaunchKernelGGL((terrain_kernel<true, false>), grid, dim3(256), 0, nullptr, a);
    else if (caves) hipLaunchKernelGGL((terrain_kernel<false, true>), grid, dim3(256), 0, nullptr, a);
    else hipLaunchKernelGGL((terrain_kernel<false, false>), grid, dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(hipMemcpy(words.data(), a.words, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t written = 0;
    uint32_t flo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, fhi[3] = {0, 0, 0};
    for (uint32_t k = 0; k < kSpread; ++k) {
        written += static_cast<uint64_t>(words[k * kWords]) | (static_cast<uint64_t>(words[k * kWords + 1]) << 32);
        for (int c = 0; c < 3; ++c) { flo[c] = std::min(flo[c], words[k * kWords + 2 + c]); fhi[c] = std::max(fhi[c], words[k * kWords + 5 + c]); }
    }
    if (out_n_voxels) *out_n_voxels = written;
    // replace mode rewrote the whole region; ADD touched the filled voxels only (an empty box when nothing was filled)
    const bool add = params.flags & BLOK_TERRAIN_ADD;
    const GpuBuildStatus st = gpu_volume_commit(v, add ? flo : lo, add ? fhi : hi, written ? Edit::MayFill : Edit::OnlyClears, why);
    BLOK_GPU_TRY(hipDeviceSynchronize());
    return st;
}

}  // namespace blok
