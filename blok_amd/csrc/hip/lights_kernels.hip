// The light table from the quads snapshot (gpu_build.h: gpu_lights_from_quads; include/blok_hip.h: blok_hip_lights_from_quads).  The
// predicates are ../common/lights_core.h; DESIGN.md §32 has the contract.
// Behind it, the table of a MODEL's exposed emissive unit faces from its own tree (gpu_model_lights; blok_hip_model_lights)
// and the per-launch prefix of an instance table over those tables (launch_instance_lights_prefix); and the light grid over the world's
// table (gpu_light_grid_build; blok_hip_build_light_grid).
//
// A lane per quad, two passes and one scan between them; no sort, no atomics, integer arithmetic only:
//   1. lights_count_kernel: a quad is kept iff its key's material index is in the emissive set.  One ballot gives the wave's number of
//      kept quads, one reduction their unit faces: a pair per wave.
//   2. an exclusive scan of the pairs (hipcub); its last entry is the totals, the one thing the host reads before it allocates the result.
//   3. lights_write_kernel: the same test; a kept quad's slot is its wave's offset plus its rank in the ballot, its cum the wave's face
//      offset plus the faces of the kept lanes before it (a scan over the wave by shuffles).  The order is the quads' order by construction.
// The owned set: every kept quad stores 1 to the byte of its material index (all writers of a byte write the same value), and
// lights_pack_kernel packs the 65536 bytes into the 2048 words the path loop tests.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "instance_core.h"
#include "../common/lights_core.h"

namespace blok {

namespace {

namespace L = lights;

struct WaveSum { unsigned long long n, faces; };
struct WaveSumAdd {
    __host__ __device__ WaveSum operator()(const WaveSum& a, const WaveSum& b) const { return WaveSum{a.n + b.n, a.faces + b.faces}; }
};

struct LightArgs {
    const blok_quad* quads; uint32_t n_quads;
    const uint32_t* glows; uint32_t n_materials;
    WaveSum* sums;                      // per wave of the grid, + 1: counts, then (scanned in place) offsets; the last is the totals
    blok_light* out;
    uint8_t* owned_bytes;               // [kSetBits]
};

__device__ __forceinline__ uint32_t lane_of() { return threadIdx.x & 63u; }

// the quad of this lane (zeros beyond the end) and whether it becomes a light
__device__ __forceinline__ bool kept_quad(const LightArgs& a, uint32_t i, uint4& head, uint4& tail) {
    head = make_uint4(0u, 0u, 0u, 0u); tail = head;
    if (i >= a.n_quads) return false;
    const uint4* rec = reinterpret_cast<const uint4*>(a.quads + i);      // 32-byte records in a hipMalloc'ed array: 16-byte aligned
    head = rec[0]; tail = rec[1];                                         // lo[3], du | dv, material, face, reserved
    return L::keeps(tail.y, a.glows, a.n_materials);
}

__global__ __launch_bounds__(256) void lights_count_kernel(const LightArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint4 head, tail;
    const bool keep = kept_quad(a, i, head, tail);
    unsigned long long faces = keep ? static_cast<unsigned long long>(head.w) * tail.x : 0ull;
    for (int off = 32; off > 0; off >>= 1) faces += __shfl_down(faces, off);
    const unsigned long long kept = __ballot(keep);
    if (lane_of() == 0u) a.sums[blockIdx.x * 4u + (threadIdx.x >> 6)] = WaveSum{static_cast<unsigned long long>(__popcll(kept)), faces};
}

__global__ __launch_bounds__(256) void lights_write_kernel(const LightArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint4 head, tail;
    const bool keep = kept_quad(a, i, head, tail);
    const unsigned long long mine = keep ? static_cast<unsigned long long>(head.w) * tail.x : 0ull;
    unsigned long long upto = mine;                                       // inclusive scan over the wave
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const unsigned long long t = __shfl_up(upto, off);
        if (lane_of() >= off) upto += t;
    }
    const unsigned long long kept = __ballot(keep);
    if (!keep) return;
    const WaveSum base = a.sums[blockIdx.x * 4u + (threadIdx.x >> 6)];
    const unsigned long long at = base.n + static_cast<unsigned long long>(__popcll(kept & ((1ull << lane_of()) - 1ull)));
    tail.w = static_cast<uint32_t>(base.faces + (upto - mine));           // (the host has checked the total: it fits)
    uint4* rec = reinterpret_cast<uint4*>(a.out + at);
    rec[0] = head; rec[1] = tail;
    a.owned_bytes[L::material_index(tail.y, a.n_materials)] = 1u;
}

__global__ __launch_bounds__(256) void lights_pack_kernel(const uint8_t* bytes, uint32_t* words) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= L::kSetWords) return;
    uint32_t bits = 0u;
    for (uint32_t b = 0; b < 32u; ++b) bits |= (bytes[w * 32u + b] ? 1u : 0u) << b;
    words[w] = bits;
}

}  // namespace

GpuBuildStatus gpu_lights_from_quads(const blok_quad* d_quads, uint64_t n_quads, const uint32_t* d_glows, uint32_t n_materials, uint32_t* d_owned,
                                     GpuLights* out, std::string* why) {
    *out = GpuLights{};
    if (n_quads >= 0xFFFFFF00ull) { *why = "lights_from_quads: 2^32 or more quads in the snapshot"; return GpuBuildStatus::Unsupported; }
    BLOK_GPU_TRY(hipMemsetAsync(d_owned, 0, L::kSetWords * sizeof(uint32_t), nullptr));
    if (n_quads == 0) { BLOK_GPU_TRY(hipDeviceSynchronize()); return GpuBuildStatus::Ok; }
    LightArgs a{};
    a.quads = d_quads; a.n_quads = static_cast<uint32_t>(n_quads); a.glows = d_glows; a.n_materials = n_materials;
    const uint32_t blocks = blocks_for(n_quads), waves = blocks * 4u;
    DeviceMem mem;
    BLOK_GPU_TRY(mem.alloc(&a.sums, waves + 1u));
    BLOK_GPU_TRY(mem.alloc(&a.owned_bytes, L::kSetBits));
    BLOK_GPU_TRY(hipMemsetAsync(a.sums + waves, 0, sizeof(WaveSum), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(a.owned_bytes, 0, L::kSetBits, nullptr));
    hipLaunchKernelGGL(lights_count_kernel, dim3(blocks), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, temp_bytes, a.sums, a.sums, WaveSumAdd{}, WaveSum{0ull, 0ull}, static_cast<int>(waves + 1u)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveScan(d_temp, temp_bytes, a.sums, a.sums, WaveSumAdd{}, WaveSum{0ull, 0ull}, static_cast<int>(waves + 1u)));
    WaveSum total{};
    BLOK_GPU_TRY(hipMemcpy(&total, a.sums + waves, sizeof(total), hipMemcpyDeviceToHost));
    if (total.n >= 0x80000000ull || total.faces > 0xFFFFFFFFull) {
        *why = "lights_from_quads: 2^31 or more lights, or 2^32 or more unit faces";
        return GpuBuildStatus::Unsupported;
    }
    if (total.n) {
        BLOK_GPU_TRY(mem.alloc(&a.out, total.n));
        hipLaunchKernelGGL(lights_write_kernel, dim3(blocks), dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
        hipLaunchKernelGGL(lights_pack_kernel, dim3(L::kSetWords / 256u), dim3(256), 0, nullptr, a.owned_bytes, d_owned);
        BLOK_GPU_TRY(hipGetLastError());
        BLOK_GPU_TRY(hipDeviceSynchronize());
        mem.release(a.out);
        out->d_lights = a.out;
    }
    out->n = static_cast<uint32_t>(total.n); out->n_faces = total.faces;
    return GpuBuildStatus::Ok;
}

// ---- a model's table (lights_core.h: brick_lights, brick_write_lights) ----------------------------------------------------------------------
// A lane per brick, two passes and one scan between them, no atomics: the count pass leaves each brick's number of records, the scan turns
// them into offsets (its last entry the total, the one thing the host reads before it allocates), the write pass forms the bricks' masks
// again and writes each brick's records from its offset on, ranks by popcounts.  A brick's exposure is bit-parallel from its mask and its
// six neighbours', found by a descent of the model's tree.
namespace {

struct LoadNode {
    const uint4* nodes;
    __device__ __forceinline__ L::Node operator()(uint32_t i) const { const uint4 w = nodes[i]; return L::Node{w.x | (static_cast<uint64_t>(w.y) << 32), w.z}; }
};
using DeviceModelTree = L::ModelTree<LoadNode>;

struct ModelLightArgs {
    DeviceModelTree tree;
    uint32_t n_lanes;                   // = the tree's nodes: lane i takes brick first_brick + i, where there is one (the host does not know
                                        // where the bricks begin, and does not ask: every lane finds it by the same few loads)
    const uint32_t* glows; uint32_t n_materials;
    uint32_t* offsets;                  // n_lanes + 1: counts (0 for a lane without a brick), then (scanned in place) offsets; the last is the total
    uint32_t total;                     // write pass: the table's length (no record is written at or beyond it)
    blok_light* out;
};

__global__ __launch_bounds__(256) void model_lights_count_kernel(const ModelLightArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_lanes) return;
    const uint32_t node = L::first_brick(a.tree) + i;
    uint64_t open[6], glowing;
    uint32_t b[3];
    L::Node brick;
    a.offsets[i] = (node >= i && node < a.tree.n_nodes) ? L::brick_lights(a.tree, node, a.glows, a.n_materials, open, &glowing, b, &brick) : 0u;
}

__global__ __launch_bounds__(256) void model_lights_write_kernel(const ModelLightArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_lanes) return;
    const uint32_t at = a.offsets[i], end = a.offsets[i + 1u];
    if (end <= at || end > a.total) return;             // nothing of this brick (or offsets that are not the count pass's: nothing is written)
    const uint32_t node = L::first_brick(a.tree) + i;
    if (node < i || node >= a.tree.n_nodes) return;
    uint64_t open[6], glowing;
    uint32_t b[3];
    L::Node brick;
    if (L::brick_lights(a.tree, node, a.glows, a.n_materials, open, &glowing, b, &brick) != end - at) return;
    L::brick_write_lights(a.tree, brick, b, open, glowing, at, a.out);
}

// ---- the per-launch prefix ---------------------------------------------------------------------------------------------------------------
struct PrefixArgs {
    const blok_instance* instances; uint32_t n;
    const ModelDesc* models; const L::ModelLightTable* tables; uint32_t n_models;
    unsigned long long a_world; float vs;
    uint32_t* icum; blok_instance_lights_info* header;
};

__device__ __forceinline__ unsigned long long faces_of(const PrefixArgs& a, uint32_t i) {
    if (i >= a.n) return 0ull;
    const blok_instance I = a.instances[i];
    if (I.model >= a.n_models) return 0ull;
    const ModelDesc M = a.models[I.model];
    const L::ModelLightTable T = a.tables[I.model];
    const uint32_t e = L::scale_exponent(M.scale_log2);
    return L::instance_faces(instance_usable(I, M) && T.table != nullptr, T.n, e);
}

// Sum of v over the workgroup's 256 lanes in every lane (`part`: four words of LDS); v < 2^49, so 256 of them fit.
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* part) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// One workgroup loops over the table twice: the total first (it decides whether the launch carries instance lights at all), then the scan.
__global__ __launch_bounds__(256) void instance_lights_prefix_kernel(const PrefixArgs a) {
    __shared__ unsigned long long part[4];
    constexpr unsigned long long kCap = 1ull << 40;     // a running sum is capped here: far above 2^32, far below an overflow
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long total = 0ull;
    for (uint32_t base = 0u; base < a.n; base += 256u) {
        total += block_sum(faces_of(a, base + threadIdx.x), part);
        if (total > kCap) total = kCap;
        if (a.n - base <= 256u) break;                  // (base + 256 may wrap for n near 2^32)
    }
    const bool fit = L::instance_lights_fit(a.a_world, total);
    unsigned long long carry = 0ull, lit = 0ull;
    for (uint32_t base = 0u; base < a.n; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long mine = fit ? faces_of(a, i) : 0ull;
        unsigned long long upto = mine;                 // inclusive scan over the wave
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const unsigned long long t = __shfl_up(upto, off);
            if (lane >= off) upto += t;
        }
        __syncthreads();
        if (lane == 63u) part[wave] = upto;
        __syncthreads();
        unsigned long long before = carry;
        for (uint32_t w = 0u; w < wave; ++w) before += part[w];
        if (i < a.n) a.icum[i] = static_cast<uint32_t>(before + (upto - mine));
        carry += part[0] + part[1] + part[2] + part[3];
        lit += static_cast<unsigned long long>(__popcll(__ballot(mine != 0ull)));      // per wave; summed below
        if (a.n - base <= 256u) break;
    }
    const unsigned long long n_lit = block_sum(lane == 0u ? lit : 0ull, part);
    if (threadIdx.x == 0u) {
        a.icum[a.n] = static_cast<uint32_t>(carry);
        blok_instance_lights_info h{};
        h.a_inst = carry; h.a_total = a.a_world + carry; h.area_world = L::lights_area_world(a.a_world + carry, a.vs);
        h.n_lit = static_cast<uint32_t>(n_lit); h.disabled = fit ? 0u : 1u;
        *a.header = h;
    }
}

}  // namespace

GpuBuildStatus gpu_model_lights(const uint4* d_nodes, uint32_t n_nodes, const uint32_t* d_materials, uint32_t n_voxels, uint32_t levels, const int32_t origin[3],
                                const uint32_t* d_glows, uint32_t n_materials, GpuLights* out, std::string* why) {
    *out = GpuLights{};
    if (!d_nodes || !n_nodes || levels < 1u || levels > kMaxLevels) { *why = "model_lights: a model without a tree"; return GpuBuildStatus::Internal; }
    ModelLightArgs a{};
    a.tree = DeviceModelTree{LoadNode{d_nodes}, n_nodes, d_materials, n_voxels, levels, {origin[0], origin[1], origin[2]}};
    a.glows = d_glows; a.n_materials = n_materials;
    DeviceMem mem;
    a.n_lanes = n_nodes;
    const uint32_t blocks = blocks_for(a.n_lanes);
    BLOK_GPU_TRY(mem.alloc(&a.offsets, static_cast<uint64_t>(a.n_lanes) + 1u));
    BLOK_GPU_TRY(hipMemsetAsync(a.offsets + a.n_lanes, 0, sizeof(uint32_t), nullptr));
    hipLaunchKernelGGL(model_lights_count_kernel, dim3(blocks), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    // (a brick holds at most 384 records and a tree fewer than 2^24 bricks with any: the 32-bit sum cannot wrap for a tree the builders make;
    // the write pass checks every offset against the total all the same)
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.offsets, a.offsets, static_cast<int>(a.n_lanes + 1u)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, a.offsets, a.offsets, static_cast<int>(a.n_lanes + 1u)));
    BLOK_GPU_TRY(hipMemcpy(&a.total, a.offsets + a.n_lanes, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (a.total >= 0x80000000u) { *why = "model_lights: 2^31 or more faces"; return GpuBuildStatus::Unsupported; }
    if (a.total) {
        BLOK_GPU_TRY(mem.alloc(&a.out, a.total));
        hipLaunchKernelGGL(model_lights_write_kernel, dim3(blocks), dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
        BLOK_GPU_TRY(hipDeviceSynchronize());
        mem.release(a.out);
        out->d_lights = a.out;
    }
    out->n = a.total; out->n_faces = a.total;
    return GpuBuildStatus::Ok;
}

// ---- the light grid (lights_core.h: light_cells, listed_cell_index) ------------------------------------------------------------
// The route: (cell, light) pairs expanded in table order behind a scan, then sorted stably by cell (hipcub's radix sort, as the volume
// rebuild sorts its bricks).  No list is formed by atomics, so none depends on the order in which they land:
//   1. grid_measure_kernel: a lane per light, its cell range and the number of cells that list it; a reduction (hipcub) joins the ranges
//      and sums the numbers: {bounds, n_items}, the one thing the host reads before it allocates the result.
//   2. an exclusive scan of the per-light numbers: where each light's pairs begin.
//   3. grid_expand_kernel: a lane per pair; its light by a search of the offsets, its cell from its rank among the light's pairs.  Pair j
//      is written to slot j: table order.
//   4. the stable sort by cell index: within a cell the lights stay in ascending table index.
//   5. the segmented scan of du * dv: one exclusive scan G over the sorted pairs in wrapping 32-bit arithmetic, a segment's value the
//      difference to G at the segment's head (a list's sum is < 2^32, so the difference is exact): lcum = G[j] - G[start[g]],
//      faces[g] = G[start[g + 1]] - G[start[g]].  start[g] is the first sorted pair with a cell >= g, by a search per cell.
// The two figures of the lists' lengths (non-empty cells, the longest list) are an integer add and an integer max over the cells: atomics
// whose result no order changes.
namespace {

struct GridMeasure { int32_t lo[3], hi[3]; unsigned long long items; };
struct GridMeasureJoin {
    __host__ __device__ GridMeasure operator()(const GridMeasure& a, const GridMeasure& b) const {
        GridMeasure o;
        for (int k = 0; k < 3; ++k) { o.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k]; o.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k]; }
        o.items = a.items + b.items;
        return o;
    }
};

struct GridArgs {
    const blok_light* lights; uint32_t n;
    uint32_t c, reach;
    int32_t cell_lo[3]; uint32_t dim[3];
    uint32_t n_cells, n_items;
    GridMeasure* measures;              // n
    uint32_t* offsets;                  // n + 1: the lights' numbers of pairs (the last 0), then (scanned in place) where their pairs begin
    uint32_t *keys, *vals;              // n_items: the pairs in table order: cell index, light
    const uint32_t *keys_sorted, *vals_sorted;
    uint32_t* scan;                     // n_items + 1: du * dv of the sorted pairs' lights (the last 0), then (scanned in place) G
    uint32_t *start, *faces; blok_light_grid_item* items;      // the result
    uint32_t* stats;                    // [0] non-empty cells, [1] the longest list
};

__global__ __launch_bounds__(256) void grid_measure_kernel(const GridArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const L::CellRange r = L::light_cells(a.lights[i], a.c);
    GridMeasure m;
    for (int k = 0; k < 3; ++k) { m.lo[k] = r.lo[k]; m.hi[k] = r.hi[k]; }
    m.items = L::listed_cells(r, a.reach);
    a.measures[i] = m;
    a.offsets[i] = m.items < 0xFFFFFFFFull ? static_cast<uint32_t>(m.items) : 0xFFFFFFFFu;      // (used only once the sum has passed the limit)
}

__global__ __launch_bounds__(256) void grid_expand_kernel(const GridArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n_items) return;
    uint32_t lo = 0u, hi = a.n;                          // the last light whose pairs begin at or before j (offsets ascend strictly)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.offsets[mid] <= j) lo = mid; else hi = mid;
    }
    const L::CellRange r = L::light_cells(a.lights[lo], a.c);
    const uint32_t k = j - a.offsets[lo];
    a.keys[j] = L::listed_cell_index(r, a.reach, k, a.cell_lo, a.dim);
    a.vals[j] = lo;
}

__global__ __launch_bounds__(256) void grid_areas_kernel(const GridArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j > a.n_items) return;
    uint32_t area = 0u;
    if (j < a.n_items) { const blok_light& l = a.lights[a.vals_sorted[j]]; area = l.du * l.dv; }
    a.scan[j] = area;
}

__global__ __launch_bounds__(256) void grid_start_kernel(const GridArgs a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.n_cells) return;
    uint32_t lo = 0u, hi = a.n_items;                    // the first sorted pair whose cell is >= g (n_items: none)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.keys_sorted[mid] < g) lo = mid + 1u; else hi = mid;
    }
    a.start[g] = lo;
}

__global__ __launch_bounds__(256) void grid_cells_kernel(const GridArgs a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint32_t len = 0u;
    if (g < a.n_cells) {
        const uint32_t s0 = a.start[g], s1 = a.start[g + 1u];
        a.faces[g] = a.scan[s1] - a.scan[s0];
        len = s1 - s0;
    }
    const uint32_t nonempty = static_cast<uint32_t>(__popcll(__ballot(len != 0u)));
    uint32_t longest = len;
    for (int off = 32; off > 0; off >>= 1) { const uint32_t t = __shfl_down(longest, off); longest = t > longest ? t : longest; }
    if (lane_of() == 0u && nonempty) { atomicAdd(a.stats, nonempty); atomicMax(a.stats + 1, longest); }
}

__global__ __launch_bounds__(256) void grid_items_kernel(const GridArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n_items) return;
    const uint32_t g = a.keys_sorted[j];
    a.items[j] = blok_light_grid_item{a.vals_sorted[j], a.scan[j] - a.scan[a.start[g]]};
}

}  // namespace

GpuBuildStatus gpu_light_grid_build(const blok_light* d_lights, uint32_t n, uint32_t cell_log2, uint32_t reach, uint32_t share, GpuLightGrid* out,
                                    std::string* why) {
    *out = GpuLightGrid{};
    if (!d_lights || n == 0u || n >= 0x80000000u) { *why = "light_grid: no light table"; return GpuBuildStatus::Internal; }
    GridArgs a{};
    a.lights = d_lights; a.n = n; a.c = cell_log2; a.reach = reach;
    DeviceMem mem;
    GridMeasure* d_total;
    BLOK_GPU_TRY(mem.alloc(&a.measures, n));
    BLOK_GPU_TRY(mem.alloc(&a.offsets, static_cast<uint64_t>(n) + 1u));
    BLOK_GPU_TRY(mem.alloc(&d_total, 1u));
    BLOK_GPU_TRY(hipMemsetAsync(a.offsets + n, 0, sizeof(uint32_t), nullptr));
    hipLaunchKernelGGL(grid_measure_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    const L::GridBounds none = L::no_bounds();
    const GridMeasure nothing{{none.lo[0], none.lo[1], none.lo[2]}, {none.hi[0], none.hi[1], none.hi[2]}, 0ull};
    size_t temp_bytes = 0;
    uint8_t* d_temp;
    BLOK_GPU_TRY(hipcub::DeviceReduce::Reduce(nullptr, temp_bytes, a.measures, d_total, static_cast<int>(n), GridMeasureJoin{}, nothing));
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceReduce::Reduce(d_temp, temp_bytes, a.measures, d_total, static_cast<int>(n), GridMeasureJoin{}, nothing));
    GridMeasure total{};
    BLOK_GPU_TRY(hipMemcpy(&total, d_total, sizeof(total), hipMemcpyDeviceToHost));      // {bounds, n_items}: the one read before the result is allocated
    blok_light_grid_info& info = out->info;
    info.cell_log2 = cell_log2; info.reach = reach; info.share = share;
    L::grid_box(L::GridBounds{{total.lo[0], total.lo[1], total.lo[2]}, {total.hi[0], total.hi[1], total.hi[2]}}, reach, &info);
    info.n_items = total.items;
    if (info.n_cells > L::kGridMaxCells || info.n_items >= L::kGridMaxItems) {
        *why = "light_grid: " + std::to_string(info.n_cells) + " cells, " + std::to_string(info.n_items) + " items: more than 2^24 cells, or 2^28 or more items";
        return GpuBuildStatus::Unsupported;
    }
    info.bytes = L::grid_bytes(info.n_cells, info.n_items);
    a.n_cells = static_cast<uint32_t>(info.n_cells); a.n_items = static_cast<uint32_t>(info.n_items);
    for (int k = 0; k < 3; ++k) { a.cell_lo[k] = info.cell_lo[k]; a.dim[k] = info.dim[k]; }

    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.offsets, a.offsets, static_cast<int>(n + 1u)));
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, a.offsets, a.offsets, static_cast<int>(n + 1u)));
    uint32_t *keys_sorted, *vals_sorted;
    BLOK_GPU_TRY(mem.alloc(&a.keys, a.n_items));
    BLOK_GPU_TRY(mem.alloc(&a.vals, a.n_items));
    BLOK_GPU_TRY(mem.alloc(&keys_sorted, a.n_items));
    BLOK_GPU_TRY(mem.alloc(&vals_sorted, a.n_items));
    BLOK_GPU_TRY(mem.alloc(&a.scan, static_cast<uint64_t>(a.n_items) + 1u));
    BLOK_GPU_TRY(mem.alloc(&a.stats, 2u));
    BLOK_GPU_TRY(mem.alloc(&a.start, static_cast<uint64_t>(a.n_cells) + 1u));
    BLOK_GPU_TRY(mem.alloc(&a.faces, a.n_cells));
    BLOK_GPU_TRY(mem.alloc(&a.items, a.n_items));
    a.keys_sorted = keys_sorted; a.vals_sorted = vals_sorted;
    BLOK_GPU_TRY(hipMemsetAsync(a.stats, 0, 2u * sizeof(uint32_t), nullptr));
    hipLaunchKernelGGL(grid_expand_kernel, dim3(blocks_for(a.n_items)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    int key_bits = 1;
    while (key_bits < 32 && (1ull << key_bits) < info.n_cells) ++key_bits;
    BLOK_GPU_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, a.keys, keys_sorted, a.vals, vals_sorted, static_cast<int>(a.n_items), 0, key_bits));
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, a.keys, keys_sorted, a.vals, vals_sorted, static_cast<int>(a.n_items), 0, key_bits));
    hipLaunchKernelGGL(grid_areas_kernel, dim3(blocks_for(static_cast<uint64_t>(a.n_items) + 1u)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.scan, a.scan, static_cast<int>(a.n_items + 1u)));
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, a.scan, a.scan, static_cast<int>(a.n_items + 1u)));
    hipLaunchKernelGGL(grid_start_kernel, dim3(blocks_for(static_cast<uint64_t>(a.n_cells) + 1u)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    hipLaunchKernelGGL(grid_cells_kernel, dim3(blocks_for(a.n_cells)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    hipLaunchKernelGGL(grid_items_kernel, dim3(blocks_for(a.n_items)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    uint32_t stats[2] = {0u, 0u};
    BLOK_GPU_TRY(hipMemcpy(stats, a.stats, sizeof(stats), hipMemcpyDeviceToHost));      // behind every kernel above
    info.n_nonempty = stats[0]; info.max_items = stats[1];
    mem.release(a.start); mem.release(a.faces); mem.release(a.items);
    out->d_start = a.start; out->d_faces = a.faces; out->d_items = a.items;
    return GpuBuildStatus::Ok;
}

void launch_instance_lights_prefix(const blok_instance* instances, uint32_t n, const ModelDesc* models, const L::ModelLightTable* tables, uint32_t n_models,
                                   uint64_t a_world, float voxel_size, uint32_t* icum, blok_instance_lights_info* header, hipStream_t stream) {
    PrefixArgs a{};
    a.instances = instances; a.n = n; a.models = models; a.tables = tables; a.n_models = (models && tables) ? n_models : 0u;
    a.a_world = a_world; a.vs = voxel_size; a.icum = icum; a.header = header;
    hipLaunchKernelGGL(instance_lights_prefix_kernel, dim3(1), dim3(256), 0, stream, a);
}

}  // namespace blok
