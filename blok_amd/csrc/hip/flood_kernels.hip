// The flood of the resident volume from seeds and the edits that threshold it (gpu_build.h: gpu_volume_flood_field /
// gpu_volume_edit_by_flood; include/blok_hip.h: blok_hip_volume_flood_field has the contract; the rules live in ../common/flood_core.h,
// shared with the host build; DESIGN.md §20 has the argument for the rounds and their bound).
//
// The field is label-correcting rounds over the bricks of the region's brick cover (the bricks that hold a region cell):
//   classify. a lane per cover brick, 64 bricks along x per wave: the brick's 64-bit passable word, clipped to the region, from the brick
//      masks alone in either layout (BrickMasks::at) — with SAME_MATERIAL a wave per brick and a lane per cell, from the densities and the
//      ids.  Every later kernel sees only passable words: one flood path for all modes.
//   working field. brick-major tiles of 64 x uint16 = 128 bytes per cover brick, cell x + 4 y + 16 z of the brick at lane's place: a wave
//      owns a brick, a lane a cell, a tile is one 128-byte access per wave instruction.  It starts as FAR everywhere.
//   seeds. a lane per listed seed (a lane per brick of a face's brick layer for the SEED_FACE bits, from the passable words): zeros into the
//      tiles, and the seed bricks into the first list.  A brick enters a list once: one stamp word per brick, claimed by an atomic
//      exchange with the list's number; the claimed bricks of a wave are appended with one atomic add.
//   rounds. a launch over the list of active bricks, a wave per brick.  The wave loads its tile and, for the cells on the brick's faces, the
//      facing cells of the six neighbours' tiles; relaxes d = min(d, neighbour + 1) over its passable cells through lane shuffles until a
//      ballot says nothing changed; stores the tile if it changed; and for every face on which a cell changed whose facing cell is
//      passable, claims the neighbour for the next list.  No wave waits for another: a neighbour's value read in the same launch is from
//      before or after that launch's store, either is the length of a real path, and whoever lowers a face cell queues its reader again.
//      The host reads the next list's count after every round and stops at zero — at the latest after max_steps + 2 rounds (§20).
//   finish. a workgroup per 16 bricks along x: the tiles transposed through LDS into the x-fastest snapshot, counted by ballots, a sum per
//      workgroup in LDS, one atomic per workgroup and counter.
// The edit is field_edit.h's, with the flood rule.
// Everything is on the null stream, behind earlier edits.  The working field, the words, the stamps and the lists live for the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "field_edit.h"
#include "../common/flood_core.h"

namespace blok {

namespace {

namespace F = flood;

constexpr uint32_t kNoBrick = 0xFFFFFFFFu;

// The region (box-local, half open, non-empty) and its brick cover: bricks b0 .. b0 + nb of the volume, cover brick (cx, cy, cz) at
// cx + nb[0] * (cy + nb[1] * cz).
struct Cover {
    uint32_t lo[3], hi[3];
    uint32_t b0[3], nb[3];
};

// The bits of the cells of cover brick (cx, cy, cz) that lie in the region.
__device__ __forceinline__ uint32_t axis_bits(uint32_t brick, uint32_t lo, uint32_t hi) {
    const int32_t l = max(static_cast<int32_t>(lo) - static_cast<int32_t>(4u * brick), 0), h = min(static_cast<int32_t>(hi) - static_cast<int32_t>(4u * brick), 4);
    return h > l ? ((1u << h) - 1u) & ~((1u << l) - 1u) : 0u;
}
__device__ __forceinline__ uint64_t region_word(const Cover& c, uint32_t cx, uint32_t cy, uint32_t cz) {
    const uint32_t xm = axis_bits(c.b0[0] + cx, c.lo[0], c.hi[0]), ym = axis_bits(c.b0[1] + cy, c.lo[1], c.hi[1]), zm = axis_bits(c.b0[2] + cz, c.lo[2], c.hi[2]);
    uint32_t plane = 0u;
#pragma unroll
    for (uint32_t y = 0; y < 4u; ++y) if ((ym >> y) & 1u) plane |= xm << (4u * y);
    uint64_t word = 0ull;
#pragma unroll
    for (uint32_t z = 0; z < 4u; ++z) if ((zm >> z) & 1u) word |= static_cast<uint64_t>(plane) << (16u * z);
    return word;
}
// The bits of a brick's cells whose coordinate along `axis` is k.
__device__ __forceinline__ uint64_t layer_word(uint32_t axis, uint32_t k) {
    return axis == 0u ? 0x1111111111111111ull << k : axis == 1u ? 0x000F000F000F000Full << (4u * k) : 0xFFFFull << (16u * k);
}

// The lanes of a wave that `add` append their values to a list with one atomic add.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_append(bool add, uint32_t value, uint32_t* list, uint32_t* count, uint32_t capacity) {
    const uint64_t adders = __ballot(add);
    if (!adders) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(adders))) - 1u;
    uint32_t base = 0u;
    if (lane == leader) base = atomicAdd(count, static_cast<uint32_t>(__popcll(adders)));
    base = static_cast<uint32_t>(__shfl(static_cast<int>(base), static_cast<int>(leader)));
    if (add) {
        const uint32_t slot = base + static_cast<uint32_t>(__popcll(adders & ((1ull << lane) - 1ull)));
        if (slot < capacity) list[slot] = value;                  // (a brick enters a list once: the list never fills; the test keeps a defect in bounds)
    }
}

// ---- classify ---------------------------------------------------------------------------------------------------------------------------
struct ClassifyArgs {
    BrickMasks masks;
    const float* density; const uint32_t* ids;                    // SAME_MATERIAL only
    uint32_t nx, ny;
    Cover c;
    uint32_t flags, material;
    uint32_t x_chunks;
    uint64_t n_waves;
    uint64_t* pass;
};

__global__ __launch_bounds__(256) void flood_classify_kernel(const ClassifyArgs a) {
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t xc, cy, cz;
    row_segment(wave, a.x_chunks, a.c.nb[1], xc, cy, cz);
    const uint32_t cx = 64u * xc + lane;
    if (cx >= a.c.nb[0]) return;
    const uint64_t m = a.masks.at(a.c.b0[0] + cx, a.c.b0[1] + cy, a.c.b0[2] + cz);
    a.pass[cx + static_cast<size_t>(a.c.nb[0]) * (cy + static_cast<size_t>(a.c.nb[1]) * cz)] = F::passable_word(m, a.flags) & region_word(a.c, cx, cy, cz);
}

// SAME_MATERIAL: a wave per cover brick, a lane per cell (n_waves = the cover's bricks).
__global__ __launch_bounds__(256) void flood_classify_material_kernel(const ClassifyArgs a) {
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t cx = static_cast<uint32_t>(wave % a.c.nb[0]);
    const uint64_t row = wave / a.c.nb[0];
    const uint32_t cy = static_cast<uint32_t>(row % a.c.nb[1]), cz = static_cast<uint32_t>(row / a.c.nb[1]);
    const uint32_t x = 4u * (a.c.b0[0] + cx) + (lane & 3u), y = 4u * (a.c.b0[1] + cy) + ((lane >> 2) & 3u), z = 4u * (a.c.b0[2] + cz) + (lane >> 4);
    bool p = false;
    if (x >= a.c.lo[0] && x < a.c.hi[0] && y >= a.c.lo[1] && y < a.c.hi[1] && z >= a.c.lo[2] && z < a.c.hi[2]) {      // (the region lies in the box)
        const size_t cell = x + y * static_cast<size_t>(a.nx) + z * (static_cast<size_t>(a.nx) * a.ny);
        p = F::passable(F::filled(a.density[cell]), a.ids[cell], a.flags, a.material);
    }
    const uint64_t word = __ballot(p);
    if (lane == 0u) a.pass[wave] = word;
}

// ---- seeds ------------------------------------------------------------------------------------------------------------------------------
struct SeedArgs {
    Cover c;
    const uint32_t* xyz; uint32_t n;                              // listed seeds, box-local, inside the region
    uint32_t axis, layer_brick, layer_cell, nu, nv, u_chunks;     // a face: the cover brick layer along `axis`, the cells' coordinate in it, the layer's extent
    uint64_t n_waves;
    const uint64_t* pass;
    uint16_t* tiles;
    uint32_t* stamp; uint32_t* list; uint32_t* count;
    uint32_t n_cover;
};

__global__ __launch_bounds__(256) void flood_seeds_kernel(const SeedArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool claim = false;
    uint32_t brick = 0u;
    if (i < a.n) {
        const uint32_t x = a.xyz[3u * i], y = a.xyz[3u * i + 1u], z = a.xyz[3u * i + 2u];
        brick = (x / 4u - a.c.b0[0]) + a.c.nb[0] * ((y / 4u - a.c.b0[1]) + a.c.nb[1] * (z / 4u - a.c.b0[2]));
        const uint32_t bit = (x & 3u) | ((y & 3u) << 2) | ((z & 3u) << 4);
        if ((a.pass[brick] >> bit) & 1ull) {
            a.tiles[static_cast<size_t>(brick) * 64u + bit] = 0u;
            claim = atomicExch(&a.stamp[brick], 1u) != 1u;
        }
    }
    wave_append(claim, brick, a.list, a.count, a.n_cover);
}

__global__ __launch_bounds__(256) void flood_face_seeds_kernel(const SeedArgs a) {
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t u = 64u * static_cast<uint32_t>(wave % a.u_chunks) + lane, v = static_cast<uint32_t>(wave / a.u_chunks);
    bool claim = false;
    uint32_t brick = 0u;
    if (u < a.nu) {
        // (u runs along axis + 1, v along axis + 2, cyclically)
        const uint32_t px = a.axis == 0u ? a.layer_brick : a.axis == 1u ? v : u, py = a.axis == 0u ? u : a.axis == 1u ? a.layer_brick : v,
                       pz = a.axis == 0u ? v : a.axis == 1u ? u : a.layer_brick;
        brick = px + a.c.nb[0] * (py + a.c.nb[1] * pz);
        uint64_t word = a.pass[brick] & layer_word(a.axis, a.layer_cell);
        if (word) {
            while (word) {                                        // at most 16 cells
                const uint32_t bit = static_cast<uint32_t>(__ffsll(static_cast<long long>(word))) - 1u;
                word &= word - 1ull;
                a.tiles[static_cast<size_t>(brick) * 64u + bit] = 0u;
            }
            claim = atomicExch(&a.stamp[brick], 1u) != 1u;
        }
    }
    wave_append(claim, brick, a.list, a.count, a.n_cover);
}

// ---- a round ----------------------------------------------------------------------------------------------------------------------------
struct RoundArgs {
    uint32_t nb[3];
    const uint64_t* pass;
    uint16_t* tiles;
    uint32_t* stamp;
    const uint32_t* list; uint32_t n_active;
    uint32_t* next_list; uint32_t* next_count; uint32_t next_stamp;
    uint32_t max_steps;
    uint32_t first;                                               // the round over the seed bricks: every value they hold is news to their neighbours
    uint32_t n_cover;
};

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t from) { return static_cast<uint32_t>(__shfl(static_cast<int>(v), static_cast<int>(from))); }

__global__ __launch_bounds__(256) void flood_round_kernel(const RoundArgs a) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= a.n_active) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = uniform_word(a.list, w);                   // (written by an earlier launch, read-only in this one)
    const uint32_t cx = c % a.nb[0], cy = (c / a.nb[0]) % a.nb[1], cz = c / (a.nb[0] * a.nb[1]);
    const uint64_t pass = a.pass[c];
    const bool mine = (pass >> lane) & 1ull;
    // lane f < 6 holds neighbour f (blok_hit::face numbering): its cover brick and its passable word
    uint32_t nbi = kNoBrick, nbp_lo = 0u, nbp_hi = 0u;
    if (lane < 6u) {
        const uint32_t axis = lane >> 1;
        const bool plus = !(lane & 1u);
        const uint32_t stride = axis == 0u ? 1u : axis == 1u ? a.nb[0] : a.nb[0] * a.nb[1];
        const uint32_t at = axis == 0u ? cx : axis == 1u ? cy : cz, n = axis == 0u ? a.nb[0] : axis == 1u ? a.nb[1] : a.nb[2];
        if (plus ? at + 1u < n : at > 0u) {
            nbi = plus ? c + stride : c - stride;
            const uint64_t p = a.pass[nbi];
            nbp_lo = static_cast<uint32_t>(p); nbp_hi = static_cast<uint32_t>(p >> 32);
        }
    }
    // per axis, a cell on a face of the brick has one neighbour outside it: the facing cell of the neighbour's tile
    uint32_t halo = F::kFar;
    uint32_t face[3];
    bool open[3];
#pragma unroll
    for (uint32_t ax = 0; ax < 3u; ++ax) {
        const uint32_t k = (lane >> (2u * ax)) & 3u, span = 3u << (2u * ax);
        const bool outer = k == 0u || k == 3u;
        face[ax] = 2u * ax + (k == 0u ? 1u : 0u);
        const uint32_t facing = k == 0u ? lane + span : lane - span;      // (meaningful when outer)
        const uint32_t from = outer ? face[ax] : 0u;
        const uint32_t ni = lane_value(nbi, from);
        const uint64_t np = static_cast<uint64_t>(lane_value(nbp_lo, from)) | (static_cast<uint64_t>(lane_value(nbp_hi, from)) << 32);
        open[ax] = outer && mine && ni != kNoBrick && ((np >> (facing & 63u)) & 1ull);
        if (open[ax]) halo = min(halo, static_cast<uint32_t>(a.tiles[static_cast<size_t>(ni) * 64u + facing]));
    }
    const uint32_t d0 = a.tiles[static_cast<size_t>(c) * 64u + lane];      // (FAR wherever the cell is impassable: nothing ever writes those)
    uint32_t d = d0;
    // Bellman-Ford inside the brick: a chain enters from the halo and runs through at most 63 in-brick steps, so sweep 65 changes nothing
    for (uint32_t sweep = 0; sweep < 65u; ++sweep) {
        uint32_t best = halo;
#pragma unroll
        for (uint32_t ax = 0; ax < 3u; ++ax) {
            const uint32_t k = (lane >> (2u * ax)) & 3u, s = 1u << (2u * ax);
            const uint32_t up = lane_value(d, (lane + s) & 63u), down = lane_value(d, (lane - s) & 63u);
            if (k < 3u) best = min(best, up);
            if (k > 0u) best = min(best, down);
        }
        const uint32_t now = mine ? F::relax(d, best, a.max_steps) : d;
        const bool changed = now != d;
        d = now;
        if (!__ballot(changed)) break;
    }
    if (__ballot(d != d0)) a.tiles[static_cast<size_t>(c) * 64u + lane] = static_cast<uint16_t>(d);      // the whole tile: one 128-byte store
    const bool moved = d != d0 || (a.first && d != F::kFar);
    uint32_t faces = 0u;
#pragma unroll
    for (uint32_t f = 0; f < 6u; ++f)
        if (__ballot(moved && open[f >> 1] && face[f >> 1] == f)) faces |= 1u << f;
    const bool want = lane < 6u && ((faces >> lane) & 1u);       // (then nbi is a brick: a cell was open towards it)
    const bool claim = want && atomicExch(&a.stamp[nbi], a.next_stamp) != a.next_stamp;
    wave_append(claim, nbi, a.next_list, a.next_count, a.n_cover);
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kFinishBricks = 16u;                           // cover bricks along x per workgroup: 64 cells, a lane each when writing

struct FinishArgs {
    Cover c;
    const uint64_t* pass;
    const uint16_t* tiles;
    uint16_t* out; uint32_t ext[3];
    uint32_t x_chunks;
    uint64_t* counts;                                             // [0] D == 0, [1] 0 < D <= K, [2] passable with FAR, [3] the largest D
};

__global__ __launch_bounds__(256) void flood_finish_kernel(const FinishArgs a) {
    __shared__ uint16_t s_row[16][4u * kFinishBricks];
    __shared__ uint32_t s_count[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t xc = blockIdx.x % a.x_chunks, cy = (blockIdx.x / a.x_chunks) % a.c.nb[1], cz = blockIdx.x / (a.x_chunks * a.c.nb[1]);
    if (t < 4u) s_count[t] = 0u;
    // thread t loads row r = y + 4 z of brick b of the chunk: four cells along x, 8 bytes
    const uint32_t b = t / 16u, r = t % 16u, cx = kFinishBricks * xc + b;
    uint32_t v[4] = {F::kFar, F::kFar, F::kFar, F::kFar};
    uint32_t bits = 0u;
    if (cx < a.c.nb[0]) {
        const size_t brick = cx + static_cast<size_t>(a.c.nb[0]) * (cy + static_cast<size_t>(a.c.nb[1]) * cz);
        const uint2 q = *reinterpret_cast<const uint2*>(a.tiles + brick * 64u + 4u * r);
        v[0] = q.x & 0xFFFFu; v[1] = q.x >> 16; v[2] = q.y & 0xFFFFu; v[3] = q.y >> 16;
        bits = static_cast<uint32_t>(a.pass[brick] >> (4u * r)) & 0xFu;
    }
    uint32_t n_seed = 0u, n_reached = 0u, n_unreached = 0u, far = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        s_row[r][4u * b + i] = static_cast<uint16_t>(v[i]);
        n_seed += static_cast<uint32_t>(__popcll(__ballot(v[i] == 0u)));
        n_reached += static_cast<uint32_t>(__popcll(__ballot(v[i] != 0u && v[i] != F::kFar)));
        n_unreached += static_cast<uint32_t>(__popcll(__ballot(v[i] == F::kFar && ((bits >> i) & 1u))));
        if (v[i] != F::kFar) far = max(far, v[i]);
    }
#pragma unroll
    for (uint32_t s = 32u; s >= 1u; s >>= 1) far = max(far, lane_value(far, lane ^ s));
    __syncthreads();
    if (lane == 0u) {
        if (n_seed) atomicAdd(&s_count[0], n_seed);
        if (n_reached) atomicAdd(&s_count[1], n_reached);
        if (n_unreached) atomicAdd(&s_count[2], n_unreached);
        if (far) atomicMax(&s_count[3], far);
    }
    // wave w writes rows 4 w .. 4 w + 3, a lane per x: 128 contiguous bytes per wave instruction
    const uint32_t x = 4u * (a.c.b0[0] + kFinishBricks * xc) + lane;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t row = 4u * wave + i;
        const uint32_t y = 4u * (a.c.b0[1] + cy) + (row & 3u), z = 4u * (a.c.b0[2] + cz) + (row >> 2);
        if (x >= a.c.lo[0] && x < a.c.hi[0] && y >= a.c.lo[1] && y < a.c.hi[1] && z >= a.c.lo[2] && z < a.c.hi[2])
            a.out[(x - a.c.lo[0]) + static_cast<size_t>(a.ext[0]) * ((y - a.c.lo[1]) + static_cast<size_t>(a.ext[1]) * (z - a.c.lo[2]))] = s_row[row][lane];
    }
    __syncthreads();
    if (t < 3u && s_count[t]) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + t), static_cast<unsigned long long>(s_count[t]));
    if (t == 3u && s_count[3]) atomicMax(reinterpret_cast<unsigned long long*>(a.counts + 3), static_cast<unsigned long long>(s_count[3]));
}

}  // namespace

GpuBuildStatus gpu_volume_flood_field(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], const int32_t* seeds_xyz, uint64_t n_seeds,
                                      uint32_t max_steps, uint32_t flags, uint32_t material, GpuFlood* out, std::string* why) {
    uint32_t ext[3];
    GpuBuildStatus begun;
    const bool has_cells = gpu_field_begin(v, "flood_field", lo, hi, flags, out, ext, &begun, why);
    blok_flood_info& info = out->info;
    info.max_steps = max_steps;
    if (!has_cells) return begun;
    Cover c{};
    for (int k = 0; k < 3; ++k) { c.lo[k] = lo[k]; c.hi[k] = hi[k]; c.b0[k] = lo[k] / 4u; c.nb[k] = (hi[k] - 1u) / 4u - c.b0[k] + 1u; }
    const uint64_t cells = static_cast<uint64_t>(ext[0]) * ext[1] * ext[2];
    const uint64_t n_cover64 = static_cast<uint64_t>(c.nb[0]) * c.nb[1] * c.nb[2];      // at most the volume's bricks: below 2^31 (gpu_volume_create)
    const uint32_t n_cover = static_cast<uint32_t>(n_cover64);
    DeviceMem mem;
    uint16_t *d_tiles, *d_field;
    uint64_t *d_pass, *d_counts;
    uint32_t *d_stamp, *d_list[2], *d_count, *d_seeds = nullptr;
    BLOK_GPU_TRY(mem.alloc(&d_tiles, n_cover64 * 64u));
    BLOK_GPU_TRY(mem.alloc(&d_pass, n_cover64));
    BLOK_GPU_TRY(mem.alloc(&d_stamp, n_cover64));
    BLOK_GPU_TRY(mem.alloc(&d_list[0], n_cover64));
    BLOK_GPU_TRY(mem.alloc(&d_list[1], n_cover64));
    BLOK_GPU_TRY(mem.alloc(&d_count, 2u));
    BLOK_GPU_TRY(mem.alloc(&d_counts, 4u));
    BLOK_GPU_TRY(mem.alloc(&d_field, cells));
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    BLOK_GPU_TRY(hipMemsetAsync(d_tiles, 0xFF, n_cover64 * 64u * sizeof(uint16_t), nullptr));      // FAR everywhere
    BLOK_GPU_TRY(hipMemsetAsync(d_stamp, 0, n_cover64 * sizeof(uint32_t), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(d_count, 0, 2u * sizeof(uint32_t), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(d_counts, 0, 4u * sizeof(uint64_t), nullptr));
    ClassifyArgs ca{};
    ca.masks = brick_masks_of(*v); ca.density = v->d_density; ca.ids = v->d_ids; ca.nx = v->nx; ca.ny = v->ny;
    ca.c = c; ca.flags = flags; ca.material = material; ca.pass = d_pass;
    if (F::same_material(flags)) {
        ca.n_waves = n_cover64;
        hipLaunchKernelGGL(flood_classify_material_kernel, dim3(static_cast<uint32_t>((ca.n_waves + 3u) / 4u)), dim3(256), 0, nullptr, ca);
    } else {
        ca.x_chunks = (c.nb[0] + 63u) / 64u;
        ca.n_waves = static_cast<uint64_t>(ca.x_chunks) * c.nb[1] * c.nb[2];
        hipLaunchKernelGGL(flood_classify_kernel, dim3(static_cast<uint32_t>((ca.n_waves + 3u) / 4u)), dim3(256), 0, nullptr, ca);
    }
    BLOK_GPU_TRY(hipGetLastError());
    SeedArgs sa{};
    sa.c = c; sa.pass = d_pass; sa.tiles = d_tiles; sa.stamp = d_stamp; sa.list = d_list[0]; sa.count = d_count; sa.n_cover = n_cover;
    // the listed seeds (inside the region: the entry has checked them), box-local, a million at a time
    constexpr uint64_t kSeedChunk = 1ull << 20;
    if (n_seeds) BLOK_GPU_TRY(mem.alloc(&d_seeds, 3u * std::min(n_seeds, kSeedChunk)));
    std::vector<uint32_t> local;
    for (uint64_t at = 0; at < n_seeds; at += kSeedChunk) {
        const uint64_t n = std::min(kSeedChunk, n_seeds - at);
        local.resize(3u * n);
        for (uint64_t i = 0; i < 3u * n; ++i) local[i] = static_cast<uint32_t>(int64_t(seeds_xyz[3u * at + i]) - v->origin[i % 3u]);
        BLOK_GPU_TRY(hipMemcpy(d_seeds, local.data(), local.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        sa.xyz = d_seeds; sa.n = static_cast<uint32_t>(n);
        hipLaunchKernelGGL(flood_seeds_kernel, dim3(static_cast<uint32_t>((n + 255u) / 256u)), dim3(256), 0, nullptr, sa);
        BLOK_GPU_TRY(hipGetLastError());
        if (at + kSeedChunk < n_seeds) BLOK_GPU_TRY(hipDeviceSynchronize());      // the next chunk overwrites d_seeds
    }
    for (uint32_t f = 0; f < 6u; ++f) {
        if (!F::seeds_face(flags, f)) continue;
        const uint32_t axis = F::face_axis(f), cell = F::face_layer(f, lo[axis], hi[axis]);
        sa.axis = axis; sa.layer_brick = cell / 4u - c.b0[axis]; sa.layer_cell = cell & 3u;
        sa.nu = c.nb[(axis + 1u) % 3u]; sa.nv = c.nb[(axis + 2u) % 3u]; sa.u_chunks = (sa.nu + 63u) / 64u;
        sa.n_waves = static_cast<uint64_t>(sa.u_chunks) * sa.nv;
        hipLaunchKernelGGL(flood_face_seeds_kernel, dim3(static_cast<uint32_t>((sa.n_waves + 3u) / 4u)), dim3(256), 0, nullptr, sa);
        BLOK_GPU_TRY(hipGetLastError());
    }
    // the rounds: the host reads the next list's count after each (one small wait per round), and stops at the bound of DESIGN.md §20
    uint32_t count = 0u;
    BLOK_GPU_TRY(hipMemcpy(&count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
    RoundArgs ra{};
    for (int k = 0; k < 3; ++k) ra.nb[k] = c.nb[k];
    ra.pass = d_pass; ra.tiles = d_tiles; ra.stamp = d_stamp; ra.max_steps = max_steps; ra.n_cover = n_cover;
    for (uint32_t r = 0; count != 0u; ++r) {
        if (r >= max_steps + 2u) { *why = "flood_field: the rounds did not end within max_steps + 2"; return GpuBuildStatus::Internal; }
        const uint32_t cur = r & 1u, nxt = cur ^ 1u;
        BLOK_GPU_TRY(hipMemsetAsync(d_count + nxt, 0, sizeof(uint32_t), nullptr));
        ra.list = d_list[cur]; ra.n_active = std::min(count, n_cover); ra.next_list = d_list[nxt]; ra.next_count = d_count + nxt;
        ra.next_stamp = r + 2u; ra.first = r == 0u ? 1u : 0u;
        hipLaunchKernelGGL(flood_round_kernel, dim3((ra.n_active + 3u) / 4u), dim3(256), 0, nullptr, ra);
        BLOK_GPU_TRY(hipGetLastError());
        out->rounds += 1u; out->visits += ra.n_active;
        BLOK_GPU_TRY(hipMemcpy(&count, d_count + nxt, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    FinishArgs fa{};
    fa.c = c; fa.pass = d_pass; fa.tiles = d_tiles; fa.out = d_field; fa.counts = d_counts;
    for (int k = 0; k < 3; ++k) fa.ext[k] = ext[k];
    fa.x_chunks = (c.nb[0] + kFinishBricks - 1u) / kFinishBricks;
    hipLaunchKernelGGL(flood_finish_kernel, dim3(static_cast<uint32_t>(static_cast<uint64_t>(fa.x_chunks) * c.nb[1] * c.nb[2])), dim3(256), 0, nullptr, fa);
    BLOK_GPU_TRY(hipGetLastError());
    uint64_t counts[4] = {0, 0, 0, 0};
    BLOK_GPU_TRY(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));      // (the call's last wait)
    info.n_seed = counts[0]; info.n_reached = counts[1]; info.n_unreached = counts[2]; info.farthest = static_cast<uint32_t>(counts[3]);
    mem.release(d_field);
    out->d_field = d_field;
    return GpuBuildStatus::Ok;
}

GpuBuildStatus gpu_volume_edit_by_flood(GpuVolume* v, const GpuFlood* field, int op, uint32_t d, float density, uint32_t material,
                                        uint64_t* out_n_voxels, std::string* why) {
    return edit_by_field(v, "edit_by_flood", field_edit::flood_rule(op, d, density, material), field->lo, field->info.ext, field->d_field,
                         F::op_fills(op), out_n_voxels, why);
}

}  // namespace blok
