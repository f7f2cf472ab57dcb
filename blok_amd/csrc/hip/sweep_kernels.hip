// Placed models swept against the resident volume (gpu_build.h: gpu_volume_sweep; include/blok_hip.h: blok_hip_volume_sweep_models).
//
// Both sides are read where they live: the model through its tree, the volume through its brick masks (which every edit keeps equal to
// density > 0).  One wave per 4^3 brick cell of a model's tree, as the stamp has it (stamp_kernels.hip), but for the whole table in one
// launch: a wave finds its placement by a wave-uniform search in the prefix sums of the placements' brick counts, reads that placement's
// record and walks root to brick through the scalar cache; lane b then owns voxel bit b.  The lane maps its voxel (../common/stamp_core.h),
// tests its own cell in the volume's mask, and — unless the model's brick holds a filled successor along the direction, see below —
// walks the volume's bricks along the axis, one 8-byte mask and its 4-bit column per brick (../common/sweep_core.h), to the first filled
// cell or the end of the box.  The wave's minimum goes into the placement's result with one atomicMin, the overlap ballot with one add.
//
// The in-brick skip (DESIGN.md §17 has the argument): a voxel whose successor u along the direction is filled in the same model brick
// does not scan.  If u's cell is filled, u overlaps and has a filled in-brick predecessor: that alone forces travel 0.  If it is empty,
// free(v) = min(free(u) + 1, max_distance) >= free(u), so v cannot lower the minimum.  Voxels on the brick's leading face always scan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/sweep_core.h"

namespace blok {

namespace {

namespace S = stamp;
namespace W = sweep;

struct SweepPlace {                 // one placement as the kernel reads it: six 16-byte words through the scalar cache
    const uint4* nodes;
    uint32_t levels, pad0;
    int32_t origin[3]; uint32_t pad1;      // the tree's corner, local coordinates
    uint32_t b0[3], pad2;                   // the bricks to visit: [b0, b0 + nb) in bricks from the tree's corner
    uint32_t nb[3], pad3;
    blok_instance place;
};
static_assert(sizeof(SweepPlace) == 96 && sizeof(blok_sweep_result) == 16, "records are whole 16-byte words");

struct SweepArgs {
    const SweepPlace* places;
    const uint64_t* prefix;         // n_places + 1: bricks of the placements before this one
    blok_sweep_result* results;     // travel starts at max_distance, n_overlap at 0
    uint32_t n_places;
    uint64_t wave_base, n_waves;    // this launch's first wave of the table's n_waves
    BrickMasks bricks;
    int32_t box_origin[3];
    uint32_t n[3];
    uint32_t direction, max_distance, flags;
};

__global__ __launch_bounds__(256) void sweep_kernel(const SweepArgs a) {
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint64_t t = a.wave_base + static_cast<uint64_t>(blockIdx.x) * 4u + wave_in_block;
    if (t >= a.n_waves) return;
    // the placement whose bricks hold wave t: the last one with prefix <= t (placements without bricks share their successor's prefix)
    uint32_t first = 0u, last = a.n_places;
    while (last - first > 1u) {
        const uint32_t mid = first + (last - first) / 2u;
        if (uniform_u64(a.prefix, mid) <= t) first = mid; else last = mid;
    }
    const SweepPlace P = uniform_record(a.places, first);
    const uint64_t r = t - uniform_u64(a.prefix, first);
    const uint64_t row = r / P.nb[0];
    const uint32_t bx = P.b0[0] + static_cast<uint32_t>(r - row * P.nb[0]);
    const uint32_t by = P.b0[1] + static_cast<uint32_t>(row % P.nb[1]), bz = P.b0[2] + static_cast<uint32_t>(row / P.nb[1]);
    uint4 node;
    if (!model_brick(P.nodes, P.levels, bx, by, bz, node)) return;      // an empty cell of the model: nothing below it
    const uint64_t mask = node_mask(node);
    blok_sweep_result* const result = a.results + first;
    const uint32_t axis = W::direction_axis(a.direction);
    const int sign = W::direction_sign(a.direction);
    const bool solid = W::outside_filled(a.flags);
    bool overlap = false;
    uint32_t travel = a.max_distance;
    if ((mask >> lane) & 1ull) {
        int64_t v[3];
        brick_lane_voxel(P.origin, bx, by, bz, lane, v);
        // box-local world coordinates, gathered by world axis with selects (the permutation is data: stamp::pick)
        int64_t wx = 0, wy = 0, wz = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            const uint32_t ax = P.place.axis[k];
            const int64_t w = S::to_world(P.place, k, v[k]) - S::pick(ax, a.box_origin[0], a.box_origin[1], a.box_origin[2]);
            wx = ax == 0u ? w : wx; wy = ax == 1u ? w : wy; wz = ax == 2u ? w : wz;
        }
        const bool in_x = wx >= 0 && wx < int64_t(a.n[0]), in_y = wy >= 0 && wy < int64_t(a.n[1]), in_z = wz >= 0 && wz < int64_t(a.n[2]);
        const bool in_column = (axis == 0u || in_x) && (axis == 1u || in_y) && (axis == 2u || in_z);      // inside in the two perpendicular axes
        const uint32_t ux = static_cast<uint32_t>(wx), uy = static_cast<uint32_t>(wy), uz = static_cast<uint32_t>(wz);      // used only where inside
        if (in_x && in_y && in_z) overlap = (a.bricks.at(ux >> 2, uy >> 2, uz >> 2) >> W::brick_bit(ux & 3u, uy & 3u, uz & 3u)) & 1ull;
        else overlap = solid;
        // the neighbours along the direction inside the model's own brick
        const uint32_t lk = W::local_axis(P.place, axis);
        const int ls = W::local_sign(P.place, lk, sign);
        const uint32_t c = (lane >> (2u * lk)) & 3u, stride = W::bit_stride(lk);
        const bool ahead = ls > 0 ? c < 3u : c > 0u, behind = ls > 0 ? c > 0u : c < 3u;
        const uint32_t up = ls > 0 ? lane + stride : lane - stride, down = ls > 0 ? lane - stride : lane + stride;
        const bool successor = ahead && ((mask >> (up & 63u)) & 1ull), predecessor = behind && ((mask >> (down & 63u)) & 1ull);
        if (overlap && predecessor) travel = 0u;                  // the predecessor did not scan: its first step lands here
        else if (!successor) {
            if (!in_column) travel = solid ? 0u : a.max_distance;
            else {
                const int64_t p = S::pick(axis, wx, wy, wz), n = S::pick(axis, a.n[0], a.n[1], a.n[2]);
                travel = W::free_travel(p, n, sign, a.max_distance, solid,
                    [&](int64_t b) {
                        const uint32_t ub = static_cast<uint32_t>(b);
                        const uint64_t m = a.bricks.at(axis == 0u ? ub : ux >> 2, axis == 1u ? ub : uy >> 2, axis == 2u ? ub : uz >> 2);
                        return W::column4(m, axis, ux & 3u, uy & 3u, uz & 3u);
                    },
                    // the placement's best so far, from the device's point of coherence; a stale value only costs work, never changes the minimum
                    [&]() { return __hip_atomic_load(&result->travel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) travel = min(travel, static_cast<uint32_t>(__shfl_xor(static_cast<int>(travel), off)));
    const uint64_t votes = __ballot(overlap);
    if (lane == 0u) {
        if (travel < a.max_distance) atomicMin(&result->travel, travel);
        if (votes) atomicAdd(reinterpret_cast<unsigned long long*>(&result->n_overlap), static_cast<unsigned long long>(__popcll(votes)));
    }
}

}  // namespace

GpuBuildStatus gpu_volume_sweep(const GpuVolume* v, const StampModel* models, const blok_instance* placements, uint32_t n_placements,
                                uint32_t direction, uint32_t max_distance, uint32_t flags, blok_sweep_result* out_results, std::string* why) {
    if (!cells_fit_32_bits(v, "sweep_models", why)) return GpuBuildStatus::Unsupported;
    if (n_placements == 0) return GpuBuildStatus::Ok;
    const uint32_t axis = W::direction_axis(direction);
    const int sign = W::direction_sign(direction);
    const bool solid = W::outside_filled(flags);
    const int64_t dims[3] = {v->nx, v->ny, v->nz};
    const int64_t far = int64_t(1) << 40;                         // beyond every mapped coordinate
    // one host block, one device block: the records, the results (travel = max_distance), the prefix
    const size_t places_bytes = size_t(n_placements) * sizeof(SweepPlace), results_bytes = size_t(n_placements) * sizeof(blok_sweep_result);
    const size_t prefix_bytes = (size_t(n_placements) + 1u) * sizeof(uint64_t);
    std::vector<unsigned char> block(places_bytes + results_bytes + prefix_bytes, 0);
    SweepPlace* places = reinterpret_cast<SweepPlace*>(block.data());
    blok_sweep_result* results = reinterpret_cast<blok_sweep_result*>(block.data() + places_bytes);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(block.data() + places_bytes + results_bytes);
    uint64_t n_waves = 0;
    for (uint32_t i = 0; i < n_placements; ++i) {
        const blok_instance& I = placements[i];
        const StampModel& M = models[i];
        // Without the flag only voxels whose column meets the box in the two perpendicular axes, and that do not start behind the box's far
        // end, can overlap or be stopped: the model's box is cut to those.  With the flag every voxel counts.
        int64_t clo[3], chi[3];
        bool empty = false;
        for (uint32_t k = 0; k < 3u; ++k) {
            clo[k] = M.lo[k]; chi[k] = M.hi[k];
            if (!solid) {
                const uint32_t ax = I.axis[k];
                const int64_t wlo = ax == axis && sign > 0 ? -far : v->origin[ax], whi = ax == axis && sign < 0 ? far : int64_t(v->origin[ax]) + dims[ax];
                int64_t lo, hi;
                S::local_span(I, k, wlo, whi, lo, hi);
                clo[k] = std::max<int64_t>(lo, M.lo[k]); chi[k] = std::min<int64_t>(hi, M.hi[k]);
            }
            if (clo[k] >= chi[k]) empty = true;
        }
        SweepPlace& p = places[i];
        p.nodes = M.nodes; p.levels = M.levels; p.place = I;
        for (int k = 0; k < 3; ++k) { p.origin[k] = M.origin[k]; p.b0[k] = 0u; p.nb[k] = 1u; }      // (empty: no brick, and a range that still divides)
        uint64_t bricks = 0u;
        if (!empty) {
            placed_brick_range(M, clo, chi, p.b0, p.nb);
            bricks = uint64_t(p.nb[0]) * p.nb[1] * p.nb[2];
        }
        prefix[i] = n_waves;
        n_waves += bricks;
        results[i].n_overlap = 0u; results[i].travel = max_distance; results[i].blocked = 0u;
    }
    prefix[n_placements] = n_waves;
    if (n_waves != 0u) {
        DeviceMem mem;
        unsigned char* d_block;
        BLOK_GPU_TRY(mem.alloc(&d_block, block.size()));
        BLOK_GPU_TRY(hipMemcpyAsync(d_block, block.data(), block.size(), hipMemcpyHostToDevice, nullptr));
        SweepArgs a{};
        a.places = reinterpret_cast<const SweepPlace*>(d_block);
        a.results = reinterpret_cast<blok_sweep_result*>(d_block + places_bytes);
        a.prefix = reinterpret_cast<const uint64_t*>(d_block + places_bytes + results_bytes);
        a.n_places = n_placements; a.n_waves = n_waves;
        a.bricks = brick_masks_of(*v);
        a.n[0] = v->nx; a.n[1] = v->ny; a.n[2] = v->nz;
        for (int k = 0; k < 3; ++k) a.box_origin[k] = v->origin[k];
        a.direction = direction; a.max_distance = max_distance; a.flags = flags;
        // the whole table in one launch (in several only above 2^32 bricks: the grid's limit, whatever the table's length)
        const uint64_t waves_per_launch = uint64_t(1) << 32;
        for (uint64_t base = 0; base < n_waves; base += waves_per_launch) {
            a.wave_base = base;
            const uint64_t waves = std::min<uint64_t>(waves_per_launch, n_waves - base);
            hipLaunchKernelGGL(sweep_kernel, dim3(static_cast<uint32_t>((waves + 3u) / 4u)), dim3(256), 0, nullptr, a);
            BLOK_GPU_TRY(hipGetLastError());
        }
        BLOK_GPU_TRY(hipMemcpy(results, a.results, results_bytes, hipMemcpyDeviceToHost));      // the call's one wait: behind every launch above
    }
    for (uint32_t i = 0; i < n_placements; ++i) {
        results[i].blocked = results[i].travel < max_distance ? 1u : 0u;
        out_results[i] = results[i];
    }
    return GpuBuildStatus::Ok;
}

}  // namespace blok
