// A table of shapes applied to the resident volume in one pass (gpu_build.h: gpu_volume_apply_shapes; include/blok_hip.h:
// blok_hip_volume_apply_shapes).  The rules are ../common/shapes_core.h's, shared with the host build.
//   1. host: every shape's voxel box (shapes::bounds) cut with the volume's; shapes that miss the box are dropped; the rest are uploaded
//      once, and the index in the uploaded table is the order.
//   2. bin: over the tiles (64 x 4 x 4 cells: 16 bricks, 16 rows of 64 cells along x) of the joined cut box, a wave per tile.  The lanes
//      stride over the shapes 64 at a time testing box overlap; a ballot gives each survivor its rank by a prefix popcount, so a tile's
//      list comes out in table order with no sort and no atomics.  One pass counts, one exclusive scan (hipcub) of
//      (non-empty << 32 | count) gives the lists' offsets and ranks the non-empty tiles, a second pass fills.  The list's length is known
//      on the host beforehand (the tiles each box overlaps), so nothing is read back in between.
//   3. apply: a wave per non-empty tile (the grid is the host's upper bound; waves past the device's count leave at once).  A lane owns
//      cell x of each of the tile's 16 rows, a z slice of 4 rows at a time: 4 density and 4 id loads of 256 contiguous bytes per wave,
//      kept in registers; the tile's list is walked per slice with wave-uniform loads (the shape in scalar registers, only c per lane),
//      slices and rows a shape's extent misses skipped by a scalar branch; inside rule and operation in registers; at most one store
//      per cell and array, only where a bit changed.  (All 16 rows in registers at once took 256 VGPRs and spilled scalars.)
//      Writes are counted per lane, summed over the wave, one 64-bit add per wave spread over kCountSlots words.  No wave waits for another.
//   4. commit: the shapes whose brick-aligned boxes overlap, transitively, form a group (host; a sweep along the joined box's longest
//      axis); one gpu_volume_commit per group over its joined box, MayFill if the group holds a shape that can fill.
// The call's one wait is the download of the counters.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/shapes_core.h"

namespace blok {

namespace {

namespace S = shapes;

constexpr uint32_t kTile[3] = {64, 4, 4}, kSlice = 4;      // a tile in cells; the rows of one z slice of it
constexpr uint32_t kCountSlots = 32, kSlotWords = 8;      // one counter per 64 bytes: the waves' adds do not all meet at one address

struct alignas(16) ShapeBox { uint32_t lo[3], hi[3], pad[2]; };      // a shape's voxel box cut with the volume's: box-local, half open, not empty
static_assert(sizeof(ShapeBox) == 32 && sizeof(blok_shape) == 64, "two and four 16-byte words");

struct TileGrid {
    uint32_t t0[3], nt[3];          // the tiles of the joined box: first tile and tiles per axis, in tiles from the volume's corner
    uint32_t n_tiles;
};

__device__ __forceinline__ void tile_corner(const TileGrid& g, uint32_t tile, uint32_t lo[3]) {
    lo[0] = (g.t0[0] + tile % g.nt[0]) * kTile[0];
    lo[1] = (g.t0[1] + tile / g.nt[0] % g.nt[1]) * kTile[1];
    lo[2] = (g.t0[2] + tile / g.nt[0] / g.nt[1]) * kTile[2];
}

struct BinArgs {
    const ShapeBox* boxes; uint32_t n_shapes;
    TileGrid grid;
    uint64_t* words;                // count pass: out, (list not empty) << 32 | list length per tile; fill pass: in, their exclusive scan
    uint32_t* list; uint32_t list_capacity;
    uint32_t* tiles;                // the non-empty tiles, in order
};

template <bool kFill>
__global__ __launch_bounds__(256) void shapes_bin_kernel(const BinArgs a) {
    const uint32_t tile = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= a.grid.n_tiles) return;
    uint32_t lo[3];
    tile_corner(a.grid, tile, lo);
    const uint64_t before = kFill ? a.words[tile] : 0ull;
    uint32_t total = 0;
    for (uint32_t first = 0; first < a.n_shapes; first += 64u) {
        const uint32_t i = first + lane;
        bool hit = false;
        if (i < a.n_shapes) {
            const uint4 w0 = reinterpret_cast<const uint4*>(a.boxes + i)[0];
            const uint2 w1 = reinterpret_cast<const uint2*>(a.boxes + i)[2];
            // lo x y z, hi x | hi y z
            hit = w0.x < lo[0] + kTile[0] && w0.w > lo[0] && w0.y < lo[1] + kTile[1] && w1.x > lo[1] && w0.z < lo[2] + kTile[2] && w1.y > lo[2];
        }
        const uint64_t votes = __ballot(hit);
        if (kFill && hit) {
            const uint32_t at = static_cast<uint32_t>(before) + total + static_cast<uint32_t>(__popcll(votes & ((1ull << lane) - 1ull)));
            if (at < a.list_capacity) a.list[at] = i;               // (the capacity is the host's own count of the same test)
        }
        total += static_cast<uint32_t>(__popcll(votes));
    }
    if (lane != 0u) return;
    if (!kFill) a.words[tile] = total ? (1ull << 32) | total : 0ull;
    else if (total) a.tiles[before >> 32] = tile;
}

struct ApplyArgs {
    const blok_shape* shapes;
    const uint64_t* words;          // grid.n_tiles + 1: (non-empty tiles before) << 32 | list entries before; the last one holds the totals
    const uint32_t* tiles; const uint32_t* list;
    TileGrid grid;
    int32_t origin[3];
    uint32_t nx, ny, nz;
    float* density; uint32_t* ids;
    unsigned long long* counts;     // kCountSlots * kSlotWords
};

__device__ __forceinline__ uint32_t float_bits(float f) { return __float_as_uint(f); }

__global__ __launch_bounds__(256) void shapes_apply_kernel(const ApplyArgs a) {
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wave >= static_cast<uint32_t>(uniform_u64(a.words, a.grid.n_tiles) >> 32)) return;
    const uint32_t tile = uniform_word(a.tiles, wave);
    const uint32_t first = static_cast<uint32_t>(uniform_u64(a.words, tile)), count = static_cast<uint32_t>(uniform_u64(a.words, tile + 1u)) - first;
    uint32_t lo[3];
    tile_corner(a.grid, tile, lo);
    const uint32_t x = lo[0] + lane;
    const bool in_x = x < a.nx;
    const int64_t cx = 2 * (int64_t(a.origin[0]) + x) + 1;
    // the tile's 16 rows, a slice of 4 at a time: row r of slice zi is (y, z) = (lo y + r, lo z + zi); rows past the box's end do not exist
    uint32_t wrote = 0;
#pragma unroll 1
    for (uint32_t zi = 0; zi < kTile[2]; ++zi) {
        const uint32_t z = lo[2] + zi;
        if (z >= a.nz) break;
        const int64_t cz = 2 * (int64_t(a.origin[2]) + z) + 1;
        float d[kSlice], d_was[kSlice];
        uint32_t m[kSlice], m_was[kSlice];
#pragma unroll
        for (uint32_t r = 0; r < kSlice; ++r) {
            const uint32_t y = lo[1] + r;
            d[r] = 0.0f; m[r] = 0u;
            if (in_x && y < a.ny) {
                const size_t cell = x + (static_cast<size_t>(z) * a.ny + y) * a.nx;
                d[r] = a.density[cell]; m[r] = a.ids[cell];
            }
            d_was[r] = d[r]; m_was[r] = m[r];
        }
        for (uint32_t k = 0; k < count; ++k) {
            const blok_shape s = uniform_record(a.shapes, uniform_word(a.list, first + k));
            int64_t y0, y1, z0, z1;
            S::extent(s, 2, z0, z1);
            if (cz < z0 || cz > z1) continue;                     // wave-uniform: a scalar branch
            S::extent(s, 1, y0, y1);
#pragma unroll
            for (uint32_t r = 0; r < kSlice; ++r) {
                const uint32_t y = lo[1] + r;
                const int64_t cy = 2 * (int64_t(a.origin[1]) + y) + 1;
                if (y >= a.ny || cy < y0 || cy > y1) continue;   // wave-uniform too
                if (in_x && S::inside(s, cx, cy, cz)) wrote += S::apply(s, d[r], m[r]) ? 1u : 0u;
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < kSlice; ++r) {
            const uint32_t y = lo[1] + r;
            if (!(in_x && y < a.ny)) continue;
            const size_t cell = x + (static_cast<size_t>(z) * a.ny + y) * a.nx;
            if (float_bits(d[r]) != float_bits(d_was[r])) a.density[cell] = d[r];
            if (m[r] != m_was[r]) a.ids[cell] = m[r];
        }
    }
#pragma unroll
    for (uint32_t step = 32u; step; step >>= 1) wrote += __shfl_xor(wrote, step);      // (at most 64 lanes x 16 rows x 65536 shapes: below 2^32)
    if (lane == 0u && wrote) atomicAdd(a.counts + (tile % kCountSlots) * kSlotWords, static_cast<unsigned long long>(wrote));
}

// Union-find over the shapes' brick-aligned boxes.
uint32_t find_root(std::vector<uint32_t>& parent, uint32_t i) {
    while (parent[i] != i) { parent[i] = parent[parent[i]]; i = parent[i]; }
    return i;
}

}  // namespace

GpuBuildStatus gpu_volume_apply_shapes(GpuVolume* v, const blok_shape* shapes, uint32_t n_shapes, uint64_t* out_n_written, std::string* why) {
    if (out_n_written) *out_n_written = 0;
    if (!cells_fit_32_bits(v, "apply_shapes", why)) return GpuBuildStatus::Unsupported;
    // 1. the shapes that meet the box, in table order, with their cut boxes
    const int64_t dims[3] = {v->nx, v->ny, v->nz};
    std::vector<blok_shape> kept;
    std::vector<ShapeBox> boxes;
    uint32_t jlo[3] = {v->nx, v->ny, v->nz}, jhi[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n_shapes; ++i) {
        int64_t lo[3], hi[3];
        S::bounds(shapes[i], lo, hi);
        ShapeBox b{};
        bool empty = false;
        for (int k = 0; k < 3; ++k) {
            const int64_t l = std::max<int64_t>(lo[k] - v->origin[k], 0), h = std::min<int64_t>(hi[k] - v->origin[k], dims[k]);
            if (l >= h) { empty = true; break; }
            b.lo[k] = static_cast<uint32_t>(l); b.hi[k] = static_cast<uint32_t>(h);
        }
        if (empty) continue;                                      // wholly outside, or between two voxel centres: nothing written, not an error
        for (int k = 0; k < 3; ++k) { jlo[k] = std::min(jlo[k], b.lo[k]); jhi[k] = std::max(jhi[k], b.hi[k]); }
        kept.push_back(shapes[i]);
        boxes.push_back(b);
    }
    const uint32_t n = static_cast<uint32_t>(kept.size());
    if (!n) return GpuBuildStatus::Ok;
    // 2. the tiles of the joined box, and the length of all lists: the tiles each box overlaps
    TileGrid grid{};
    uint64_t n_tiles = 1, entries = 0;
    for (int k = 0; k < 3; ++k) {
        grid.t0[k] = jlo[k] / kTile[k];
        grid.nt[k] = (jhi[k] - 1u) / kTile[k] - grid.t0[k] + 1u;
        n_tiles *= grid.nt[k];
    }
    grid.n_tiles = static_cast<uint32_t>(n_tiles);                // (at most cells / 1024 + the ragged ends: far below 2^32)
    for (const ShapeBox& b : boxes) {
        uint64_t t = 1;
        for (int k = 0; k < 3; ++k) t *= (b.hi[k] - 1u) / kTile[k] - b.lo[k] / kTile[k] + 1u;
        entries += t;
    }
    if (entries > 0xFFFFFFFFull) { *why = "apply_shapes: the tiles' shape lists hold more than 2^32 entries"; return GpuBuildStatus::Unsupported; }
    const uint32_t n_waves = static_cast<uint32_t>(std::min<uint64_t>(n_tiles, entries));      // no more tiles than that have a list
    DeviceMem mem;
    blok_shape* d_shapes; ShapeBox* d_boxes; uint64_t* d_words; uint32_t *d_list, *d_tiles; unsigned long long* d_counts; unsigned char* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_shapes, n));
    BLOK_GPU_TRY(mem.alloc(&d_boxes, n));
    BLOK_GPU_TRY(mem.alloc(&d_words, n_tiles + 1u));
    BLOK_GPU_TRY(mem.alloc(&d_list, entries));
    BLOK_GPU_TRY(mem.alloc(&d_tiles, n_waves));
    BLOK_GPU_TRY(mem.alloc(&d_counts, kCountSlots * kSlotWords));
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, d_words, d_words, static_cast<int>(n_tiles + 1u)));
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipMemcpy(d_shapes, kept.data(), n * sizeof(blok_shape), hipMemcpyHostToDevice));
    BLOK_GPU_TRY(hipMemcpy(d_boxes, boxes.data(), n * sizeof(ShapeBox), hipMemcpyHostToDevice));
    BLOK_GPU_TRY(hipMemsetAsync(d_counts, 0, kCountSlots * kSlotWords * sizeof(unsigned long long), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(d_words + n_tiles, 0, sizeof(uint64_t), nullptr));
    BinArgs bin{};
    bin.boxes = d_boxes; bin.n_shapes = n; bin.grid = grid; bin.words = d_words; bin.list = d_list; bin.list_capacity = static_cast<uint32_t>(entries); bin.tiles = d_tiles;
    const uint32_t bin_blocks = (grid.n_tiles + 3u) / 4u;
    hipLaunchKernelGGL(shapes_bin_kernel<false>, dim3(bin_blocks), dim3(256), 0, nullptr, bin);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_words, d_words, static_cast<int>(n_tiles + 1u)));
    hipLaunchKernelGGL(shapes_bin_kernel<true>, dim3(bin_blocks), dim3(256), 0, nullptr, bin);
    BLOK_GPU_TRY(hipGetLastError());
    // 3. apply
    ApplyArgs ap{};
    ap.shapes = d_shapes; ap.words = d_words; ap.tiles = d_tiles; ap.list = d_list; ap.grid = grid;
    for (int k = 0; k < 3; ++k) ap.origin[k] = v->origin[k];
    ap.nx = v->nx; ap.ny = v->ny; ap.nz = v->nz; ap.density = v->d_density; ap.ids = v->d_ids; ap.counts = d_counts;
    hipLaunchKernelGGL(shapes_apply_kernel, dim3((n_waves + 3u) / 4u), dim3(256), 0, nullptr, ap);
    BLOK_GPU_TRY(hipGetLastError());
    // 4. one commit per group of shapes whose brick-aligned boxes overlap, transitively: two far-apart shapes do not refresh what lies
    // between them.  Sorted by the low end along the joined box's longest axis, a box is compared with the ones that start before it ends.
    for (ShapeBox& b : boxes)
        for (int k = 0; k < 3; ++k) { b.lo[k] &= ~3u; b.hi[k] = std::min<uint32_t>((b.hi[k] + 3u) & ~3u, static_cast<uint32_t>(dims[k])); }
    int axis = 0;
    for (int k = 1; k < 3; ++k) if (jhi[k] - jlo[k] > jhi[axis] - jlo[axis]) axis = k;
    std::vector<uint32_t> order(n), parent(n);
    std::iota(order.begin(), order.end(), 0u);
    std::iota(parent.begin(), parent.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) { return boxes[p].lo[axis] < boxes[q].lo[axis]; });
    for (uint32_t p = 0; p < n; ++p) {
        const ShapeBox& bp = boxes[order[p]];
        for (uint32_t q = p + 1u; q < n && boxes[order[q]].lo[axis] < bp.hi[axis]; ++q) {
            const ShapeBox& bq = boxes[order[q]];
            bool meet = true;
            for (int k = 0; k < 3; ++k) meet = meet && bp.lo[k] < bq.hi[k] && bq.lo[k] < bp.hi[k];
            if (meet) parent[find_root(parent, order[q])] = find_root(parent, order[p]);
        }
    }
    std::vector<int32_t> group_of(n, -1);
    std::vector<ShapeBox> groups;                                 // (pad[0]: the group may fill)
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t root = find_root(parent, i);
        if (group_of[root] < 0) { group_of[root] = static_cast<int32_t>(groups.size()); groups.push_back(boxes[i]); groups.back().pad[0] = 0u; }
        ShapeBox& g = groups[static_cast<size_t>(group_of[root])];
        for (int k = 0; k < 3; ++k) { g.lo[k] = std::min(g.lo[k], boxes[i].lo[k]); g.hi[k] = std::max(g.hi[k], boxes[i].hi[k]); }
        g.pad[0] |= S::may_fill(kept[i]) ? 1u : 0u;
    }
    for (const ShapeBox& g : groups) {
        const GpuBuildStatus st = gpu_volume_commit(v, g.lo, g.hi, g.pad[0] ? Edit::MayFill : Edit::OnlyClears, why);
        if (st != GpuBuildStatus::Ok) return st;
    }
    std::vector<unsigned long long> counts(kCountSlots * kSlotWords);
    BLOK_GPU_TRY(hipMemcpy(counts.data(), d_counts, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));      // the call's one wait: behind every launch above
    uint64_t written = 0;
    for (uint32_t s = 0; s < kCountSlots; ++s) written += counts[s * kSlotWords];
    if (out_n_written) *out_n_written = written;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
