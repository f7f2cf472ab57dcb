// Connected components of the resident volume (gpu_build.h: gpu_volume_label_components; include/blok_hip.h:
// blok_hip_volume_label_components).  Index arithmetic and union-find are ../common/components_core.h; DESIGN.md §16 has the contract.
//
// Integer work on the brick masks (no density read) and on the label array, which is the union-find's parent array:
//   1. brick_label_kernel: a wave per brick that meets the region.  The brick's 64-bit mask, cut to the region, is flooded bit-parallel:
//      seed = lowest set bit, grow by the six shifts until stable, peel, repeat — wave-uniform 64-bit integer work.  Lane b stores voxel
//      b's first parent: the region index of the lowest voxel of its in-brick component (BLOK_LABEL_EMPTY for an empty cell).  Every cell
//      of the region is written exactly once, so the array needs no clearing.
//   2. brick_merge_kernel: a wave per brick, lanes 0..47 = the 3 x 16 voxel pairs that face each other across the brick's +x, +y, +z
//      sides; where both voxels are filled (two mask bits), components::unite through agent-scope atomics.
//   3. flatten_kernel: a lane per cell, label = find(label); per row of 64 cells the ballot of "is a root", and the row's counts of
//      filled cells and roots packed into one word.  One exclusive scan of those words (hipcub) ranks every root: the records come out
//      sorted by label without a sort, and its last entry holds both totals — the one word the host reads before it sizes the table.
//   4. record_init_kernel / record_kernel / record_finish_kernel: counts and bounds.  Waves take rows in a grid-stride loop and keep the
//      label they are following, with per-lane bounds, in registers; the run is reduced across the wave and flushed (one 64-bit add, six
//      min / max) only when a row no longer holds that label, and at the end.  The other labels of a mixed row are reduced and flushed
//      on the spot.  A volume that is one component costs each wave seven atomics in all.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/components_core.h"

namespace blok {

namespace {

namespace K = components;

struct LabelArgs {
    BrickMasks bricks;
    K::Region g;
    uint32_t b0[3], nb[3];              // the bricks that meet the region: [b0, b0 + nb)
    uint32_t* labels;
};

// The parent array as the kernels reach it while other waves change it: both accesses go to the device's point of coherence.
struct DeviceCells {
    uint32_t* parent;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v) const { return atomicMin(parent + i, v); }
};

// The bits of brick (bx, by, bz) whose voxels lie inside the region: one 4-bit mask per axis, spread over the word.
__device__ __forceinline__ uint64_t region_cut(const K::Region& g, uint32_t bx, uint32_t by, uint32_t bz) {
    uint64_t X = 0, Y = 0, Z = 0;
    for (uint32_t i = 0; i < 4u; ++i) {
        if (bx * 4u + i - g.lo[0] < g.ext[0]) X |= 0x1111111111111111ull << i;
        if (by * 4u + i - g.lo[1] < g.ext[1]) Y |= 0x000F000F000F000Full << (4u * i);
        if (bz * 4u + i - g.lo[2] < g.ext[2]) Z |= 0xFFFFull << (16u * i);
    }
    return X & Y & Z;
}

// One step of the flood: every set bit spreads to its six face neighbours inside the brick (the masks stop the shifts from wrapping
// across the brick's x and y faces; across z the shift leaves the word).
__device__ __forceinline__ uint64_t grow(uint64_t s) {
    return s | ((s & ~0x8888888888888888ull) << 1) | ((s & ~0x1111111111111111ull) >> 1) |
           ((s & ~0xF000F000F000F000ull) << 4) | ((s & ~0x000F000F000F000Full) >> 4) | (s << 16) | (s >> 16);
}

__device__ __forceinline__ bool brick_of_wave(const LabelArgs& a, uint64_t n_bricks, uint32_t& bx, uint32_t& by, uint32_t& bz) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 4u + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    if (t >= n_bricks) return false;
    bx = a.b0[0] + static_cast<uint32_t>(t % a.nb[0]);
    by = a.b0[1] + static_cast<uint32_t>((t / a.nb[0]) % a.nb[1]);
    bz = a.b0[2] + static_cast<uint32_t>(t / (static_cast<uint64_t>(a.nb[0]) * a.nb[1]));
    return true;
}

__global__ __launch_bounds__(256) void brick_label_kernel(const LabelArgs a, uint64_t n_bricks) {
    uint32_t bx, by, bz;
    if (!brick_of_wave(a, n_bricks, bx, by, bz)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t m = uniform64(a.bricks.at(bx, by, bz) & region_cut(a.g, bx, by, bz));
    uint32_t first = 0u;                                         // bit of the lowest voxel of this lane's in-brick component
    if (m != ~0ull) {                                            // (a full brick is one component: no loop)
        uint64_t rest = m;
        while (rest) {
            uint64_t s = rest & (0ull - rest);
            for (;;) {
                const uint64_t t = grow(s) & rest;
                if (t == s) break;
                s = t;
            }
            if ((s >> lane) & 1ull) first = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(s))) - 1u;
            rest &= ~s;
        }
    }
    const uint32_t x = bx * 4u + (lane & 3u), y = by * 4u + ((lane >> 2) & 3u), z = bz * 4u + (lane >> 4);
    if (!K::inside(a.g, x, y, z)) return;
    const uint32_t parent = K::index_of(a.g, bx * 4u + (first & 3u), by * 4u + ((first >> 2) & 3u), bz * 4u + (first >> 4));
    a.labels[K::index_of(a.g, x, y, z)] = ((m >> lane) & 1ull) ? parent : BLOK_LABEL_EMPTY;
}

__global__ __launch_bounds__(256) void brick_merge_kernel(const LabelArgs a, uint64_t n_bricks) {
    uint32_t bx, by, bz;
    if (!brick_of_wave(a, n_bricks, bx, by, bz)) return;
    const uint32_t lane = threadIdx.x & 63u, d = lane >> 4, j = lane & 15u;
    const uint64_t m = uniform64(a.bricks.at(bx, by, bz) & region_cut(a.g, bx, by, bz));
    if (!m || d == 3u) return;
    const uint32_t qx = bx + (d == 0u ? 1u : 0u), qy = by + (d == 1u ? 1u : 0u), qz = bz + (d == 2u ? 1u : 0u);
    if (qx >= a.b0[0] + a.nb[0] || qy >= a.b0[1] + a.nb[1] || qz >= a.b0[2] + a.nb[2]) return;      // no brick of the region on that side
    const uint64_t mq = a.bricks.at(qx, qy, qz) & region_cut(a.g, qx, qy, qz);
    // voxel j of the side: the two coordinates other than d, lower axis first
    const uint32_t u = j & 3u, w = j >> 2;
    const uint32_t x = d == 0u ? 3u : u, y = d == 1u ? 3u : (d == 0u ? u : w), z = d == 2u ? 3u : w;
    const uint32_t mine = x | (y << 2) | (z << 4);
    const uint32_t theirs = (d == 0u ? 0u : x) | ((d == 1u ? 0u : y) << 2) | ((d == 2u ? 0u : z) << 4);
    if (!((m >> mine) & 1ull) || !((mq >> theirs) & 1ull)) return;
    const uint32_t r = K::index_of(a.g, bx * 4u + x, by * 4u + y, bz * 4u + z);
    K::unite(DeviceCells{a.labels}, r, r + K::stride(a.g, d));
}

__global__ __launch_bounds__(256) void flatten_kernel(uint32_t* labels, uint64_t n, uint64_t n_rows, uint64_t* root_bits, uint64_t* packed) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    uint32_t root = BLOK_LABEL_EMPTY;
    if (r < n) {
        const uint32_t parent = labels[r];
        if (parent != BLOK_LABEL_EMPTY) {
            root = K::find(DeviceCells{labels}, parent);
            if (root != parent) labels[r] = root;                // (still an ancestor for every wave that reads it meanwhile)
        }
    }
    const uint64_t roots = __ballot(root != BLOK_LABEL_EMPTY && root == r), filled = __ballot(root != BLOK_LABEL_EMPTY);
    const uint64_t row = r >> 6;
    if ((threadIdx.x & 63u) == 0u && row < n_rows) {
        root_bits[row] = roots;
        packed[row] = (static_cast<uint64_t>(__popcll(filled)) << 32) | static_cast<uint64_t>(__popcll(roots));
    }
}

__device__ __forceinline__ uint32_t rank_of(const uint64_t* root_bits, const uint64_t* row_base, uint32_t root) {
    return static_cast<uint32_t>(row_base[root >> 6]) + static_cast<uint32_t>(__popcll(root_bits[root >> 6] & ((1ull << (root & 63u)) - 1ull)));
}

// While the counts are gathered a record holds region-local INCLUSIVE bounds in lo / hi.
__global__ __launch_bounds__(256) void record_init_kernel(const uint64_t* root_bits, const uint64_t* row_base, uint64_t n, blok_component* records) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (r >= n || !((root_bits[r >> 6] >> (r & 63u)) & 1ull)) return;
    blok_component c;
    c.label = static_cast<uint32_t>(r); c.touches = 0u; c.n_voxels = 0u;
    for (int a = 0; a < 3; ++a) { c.lo[a] = 0x7FFFFFFF; c.hi[a] = 0; }
    records[rank_of(root_bits, row_base, static_cast<uint32_t>(r))] = c;
}

struct RecordArgs {
    const uint32_t* labels; const uint64_t* root_bits; const uint64_t* row_base;
    K::Region g;
    uint64_t n, n_rows;
    blok_component* records;
};

// Adds what the wave's lanes hold for `label` (lanes without a share hold the neutral values) to the label's record.
__device__ __forceinline__ void flush_run(const RecordArgs& a, uint32_t label, uint32_t lane, const uint32_t mn[3], const uint32_t mx[3], uint32_t count) {
    uint32_t lo[3] = {mn[0], mn[1], mn[2]}, hi[3] = {mx[0], mx[1], mx[2]}, c = count;
    for (int o = 32; o > 0; o >>= 1) {
        for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo[k]), o))); hi[k] = max(hi[k], static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi[k]), o))); }
        c += static_cast<uint32_t>(__shfl_xor(static_cast<int>(c), o));
    }
    if (lane != 0u || !c) return;
    blok_component* rec = a.records + rank_of(a.root_bits, a.row_base, label);
    for (int k = 0; k < 3; ++k) { atomicMin(&rec->lo[k], static_cast<int>(lo[k])); atomicMax(&rec->hi[k], static_cast<int>(hi[k])); }
    atomicAdd(reinterpret_cast<unsigned long long*>(&rec->n_voxels), static_cast<unsigned long long>(c));
}

__global__ __launch_bounds__(256) void record_kernel(const RecordArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6), n_waves = static_cast<uint64_t>(gridDim.x) * 4u;
    const uint32_t none[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, zero[3] = {0u, 0u, 0u};
    uint32_t cur = BLOK_LABEL_EMPTY;                             // the label this wave follows (wave-uniform)
    uint32_t mn[3] = {none[0], none[1], none[2]}, mx[3] = {0u, 0u, 0u}, count = 0u;      // this lane's share of its run
    for (uint64_t row = wave; row < a.n_rows; row += n_waves) {
        const uint64_t r = row * 64u + lane;
        const uint32_t lab = r < a.n ? a.labels[r] : BLOK_LABEL_EMPTY;
        uint64_t active = __ballot(lab != BLOK_LABEL_EMPTY);
        if (!active) continue;
        uint32_t c[3] = {0u, 0u, 0u};
        if (lab != BLOK_LABEL_EMPTY) K::cell_of(a.g, static_cast<uint32_t>(r), c[0], c[1], c[2]);
        uint64_t votes = cur != BLOK_LABEL_EMPTY ? __ballot(lab == cur) : 0ull;
        if (!votes) {                                            // the run has ended: flush it and follow the row's first label
            if (cur != BLOK_LABEL_EMPTY) flush_run(a, cur, lane, mn, mx, count);
            for (int k = 0; k < 3; ++k) { mn[k] = none[k]; mx[k] = 0u; }
            count = 0u;
            cur = static_cast<uint32_t>(__shfl(static_cast<int>(lab), __ffsll(static_cast<unsigned long long>(active)) - 1));
            votes = __ballot(lab == cur);
        }
        if (lab == cur) {
            for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], c[k]); mx[k] = max(mx[k], c[k]); }
            ++count;
        }
        active &= ~votes;
        while (active) {                                         // a mixed row: its other labels, one after the other
            const uint32_t other = static_cast<uint32_t>(__shfl(static_cast<int>(lab), __ffsll(static_cast<unsigned long long>(active)) - 1));
            const bool share = lab == other;
            flush_run(a, other, lane, share ? c : none, share ? c : zero, share ? 1u : 0u);
            active &= ~__ballot(share);
        }
    }
    if (cur != BLOK_LABEL_EMPTY) flush_run(a, cur, lane, mn, mx, count);
}

__global__ __launch_bounds__(256) void record_finish_kernel(blok_component* records, uint64_t n_records, const K::Region g, int32_t ox, int32_t oy, int32_t oz) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n_records) return;
    blok_component c = records[i];
    const uint32_t mn[3] = {static_cast<uint32_t>(c.lo[0]), static_cast<uint32_t>(c.lo[1]), static_cast<uint32_t>(c.lo[2])};
    const uint32_t mx[3] = {static_cast<uint32_t>(c.hi[0]), static_cast<uint32_t>(c.hi[1]), static_cast<uint32_t>(c.hi[2])};
    const int32_t o[3] = {ox, oy, oz};
    c.touches = K::touches(g, mn, mx);
    for (int a = 0; a < 3; ++a) {
        c.lo[a] = o[a] + static_cast<int32_t>(g.lo[a] + mn[a]);
        c.hi[a] = o[a] + static_cast<int32_t>(g.lo[a] + mx[a] + 1u);
    }
    records[i] = c;
}

}  // namespace

void gpu_components_free(GpuComponents* c) {
    if (c->d_labels) (void)hipFree(c->d_labels);
    if (c->d_records) (void)hipFree(c->d_records);
    if (c->d_root_bits) (void)hipFree(c->d_root_bits);
    if (c->d_row_base) (void)hipFree(c->d_row_base);
    *c = GpuComponents{};
}

GpuBuildStatus gpu_volume_label_components(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], GpuComponents* out, std::string* why) {
    *out = GpuComponents{};
    if (!cells_fit_32_bits(v, "label_components", why)) return GpuBuildStatus::Unsupported;
    LabelArgs a{};
    for (int k = 0; k < 3; ++k) { a.g.lo[k] = lo[k]; a.g.ext[k] = hi[k] > lo[k] ? hi[k] - lo[k] : 0u; out->lo[k] = lo[k]; out->ext[k] = a.g.ext[k]; }
    const uint64_t n = K::cells(a.g);
    if (n > 0xFFFFFFFFull) { *why = "label_components: region of 2^32 cells"; return GpuBuildStatus::Unsupported; }
    if (n == 0) { out->ext[0] = out->ext[1] = out->ext[2] = 0u; return GpuBuildStatus::Ok; }
    a.bricks = brick_masks_of(*v);
    for (int k = 0; k < 3; ++k) { a.b0[k] = lo[k] / 4u; a.nb[k] = (hi[k] + 3u) / 4u - a.b0[k]; }
    const uint64_t n_bricks = static_cast<uint64_t>(a.nb[0]) * a.nb[1] * a.nb[2];
    const uint64_t n_rows = (n + 63u) / 64u;
    DeviceMem mem;
    uint64_t *d_root_bits, *d_packed, *d_row_base;
    BLOK_GPU_TRY(mem.alloc(&a.labels, n));
    BLOK_GPU_TRY(mem.alloc(&d_root_bits, n_rows));
    BLOK_GPU_TRY(mem.alloc(&d_packed, n_rows + 1u));
    BLOK_GPU_TRY(mem.alloc(&d_row_base, n_rows + 1u));
    BLOK_GPU_TRY(hipMemsetAsync(d_packed + n_rows, 0, sizeof(uint64_t), nullptr));
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    const dim3 brick_grid(static_cast<uint32_t>((n_bricks + 3u) / 4u));
    hipLaunchKernelGGL(brick_label_kernel, brick_grid, dim3(256), 0, nullptr, a, n_bricks);
    BLOK_GPU_TRY(hipGetLastError());
    hipLaunchKernelGGL(brick_merge_kernel, brick_grid, dim3(256), 0, nullptr, a, n_bricks);
    BLOK_GPU_TRY(hipGetLastError());
    hipLaunchKernelGGL(flatten_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, a.labels, n, n_rows, d_root_bits, d_packed);
    BLOK_GPU_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, d_packed, d_row_base, static_cast<int>(n_rows + 1u)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_packed, d_row_base, static_cast<int>(n_rows + 1u)));
    uint64_t totals = 0;
    BLOK_GPU_TRY(hipMemcpy(&totals, d_row_base + n_rows, sizeof(totals), hipMemcpyDeviceToHost));
    const uint64_t n_components = totals & 0xFFFFFFFFull, n_voxels = totals >> 32;
    blok_component* d_records = nullptr;
    if (n_components) {
        BLOK_GPU_TRY(mem.alloc(&d_records, n_components));
        hipLaunchKernelGGL(record_init_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, d_root_bits, d_row_base, n, d_records);
        BLOK_GPU_TRY(hipGetLastError());
        RecordArgs r{};
        r.labels = a.labels; r.root_bits = d_root_bits; r.row_base = d_row_base; r.g = a.g; r.n = n; r.n_rows = n_rows; r.records = d_records;
        hipLaunchKernelGGL(record_kernel, dim3(static_cast<uint32_t>(std::min<uint64_t>((n_rows + 3u) / 4u, 2048u))), dim3(256), 0, nullptr, r);
        BLOK_GPU_TRY(hipGetLastError());
        hipLaunchKernelGGL(record_finish_kernel, dim3(blocks_for(n_components)), dim3(256), 0, nullptr, d_records, n_components, a.g,
                           v->origin[0], v->origin[1], v->origin[2]);
        BLOK_GPU_TRY(hipGetLastError());
    }
    BLOK_GPU_TRY(hipDeviceSynchronize());
    mem.release(a.labels); mem.release(d_root_bits); mem.release(d_row_base); mem.release(d_records);
    out->d_labels = a.labels; out->d_root_bits = d_root_bits; out->d_row_base = d_row_base; out->d_records = d_records;
    out->n_cells = n; out->n_components = n_components; out->n_voxels = n_voxels;
    return GpuBuildStatus::Ok;
}

GpuBuildStatus gpu_components_find(const GpuComponents* c, uint32_t label, blok_component* out, bool* found, std::string* why) {
    *found = false;
    if (label >= c->n_cells) return GpuBuildStatus::Ok;
    uint32_t at = 0;
    BLOK_GPU_TRY(hipMemcpy(&at, c->d_labels + label, sizeof(at), hipMemcpyDeviceToHost));
    if (at != label) return GpuBuildStatus::Ok;                  // not a root: no record carries this label
    uint64_t bits = 0, base = 0;
    BLOK_GPU_TRY(hipMemcpy(&bits, c->d_root_bits + (label >> 6), sizeof(bits), hipMemcpyDeviceToHost));
    BLOK_GPU_TRY(hipMemcpy(&base, c->d_row_base + (label >> 6), sizeof(base), hipMemcpyDeviceToHost));
    const uint64_t rank = (base & 0xFFFFFFFFull) + static_cast<uint64_t>(__builtin_popcountll(bits & ((1ull << (label & 63u)) - 1ull)));
    BLOK_GPU_TRY(hipMemcpy(out, c->d_records + rank, sizeof(*out), hipMemcpyDeviceToHost));
    *found = true;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
