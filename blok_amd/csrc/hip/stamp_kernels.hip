// Models stamped into the resident volume (gpu_build.h: gpu_volume_stamp; include/blok_hip.h: blok_hip_volume_stamp_models).
//
// The model is read where it lives: one wave per 4^3 brick cell of the model's tree that can land inside the volume's box (the box mapped
// into the model's lattice and cut with the model's own box first, so a model hanging mostly outside costs only its overlap).  The descent
// from the root is the same for all 64 lanes — wave-uniform 16-byte node records through the scalar cache — and lane b then owns voxel
// bit b of the brick: mask test, rank by popcount for the material id, the placement's mapping (../common/stamp_core.h), two 4-byte
// stores; KEEP adds one density load.  The mapping is a bijection, so no voxel is written twice within a placement; placements follow
// each other in stream order.  Written voxels are counted with one 64-bit add per wave after a ballot, spread over kCountSlots words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/stamp_core.h"

namespace blok {

namespace {

namespace S = stamp;

constexpr uint32_t kCountSlots = 32, kSlotWords = 8;      // one counter per 64 bytes: the waves' adds do not all meet at one address

struct StampArgs {
    const uint4* nodes; const uint32_t* materials;
    uint32_t levels;
    int32_t origin[3];              // the tree's corner, local coordinates
    uint32_t b0[3], nb[3];          // the bricks to visit: [b0, b0 + nb) in bricks from the tree's corner
    blok_instance place;
    int32_t box_origin[3];          // the volume's box
    uint32_t nx, ny, nz;
    float* density; uint32_t* ids;
    int mode; float value;
    unsigned long long* counts;     // kCountSlots * kSlotWords
};

__global__ __launch_bounds__(256) void stamp_kernel(const StampArgs a) {
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t ix = blockIdx.x * 4u + wave_in_block;
    if (ix >= a.nb[0]) return;
    const uint32_t bx = a.b0[0] + ix, by = a.b0[1] + blockIdx.y, bz = a.b0[2] + blockIdx.z;
    uint4 node;
    if (!model_brick(a.nodes, a.levels, bx, by, bz, node)) return;      // an empty cell of the model: nothing below it
    const uint64_t mask = node_mask(node);
    bool wrote = false;
    if ((mask >> lane) & 1ull) {
        int64_t v[3];
        brick_lane_voxel(a.origin, bx, by, bz, lane, v);
        // box-local world coordinates of the three LOCAL axes, and the cell's index through the strides of their world axes
        bool inside = true;
        uint64_t cell = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            const uint32_t ax = a.place.axis[k];
            const int64_t w = S::to_world(a.place, k, v[k]) - S::pick(ax, a.box_origin[0], a.box_origin[1], a.box_origin[2]);
            inside = inside && w >= 0 && w < S::pick(ax, a.nx, a.ny, a.nz);
            cell += static_cast<uint64_t>(w) * static_cast<uint64_t>(S::pick(ax, 1, a.nx, int64_t(a.nx) * a.ny));
        }
        if (inside) {                                             // clipped voxels are dropped silently
            const uint32_t material = a.mode == BLOK_STAMP_ERASE ? 0u : a.materials[node.z + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)))];
            const float present = a.mode == BLOK_STAMP_KEEP ? a.density[cell] : 0.0f;
            float d; uint32_t m;
            wrote = S::apply(a.mode, a.value, material, present, d, m);
            if (wrote) { a.density[cell] = d; a.ids[cell] = m; }
        }
    }
    const uint64_t votes = __ballot(wrote);
    if (lane == 0u && votes) {
        const uint32_t slot = (bx + 3u * by + 5u * bz) % kCountSlots;
        atomicAdd(a.counts + slot * kSlotWords, static_cast<unsigned long long>(__popcll(votes)));
    }
}

}  // namespace

GpuBuildStatus gpu_volume_stamp(GpuVolume* v, const StampModel* models, const blok_instance* placements, uint32_t n_placements, int mode,
                                float density, uint64_t* out_n_voxels, std::string* why) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!cells_fit_32_bits(v, "stamp_models", why)) return GpuBuildStatus::Unsupported;
    if (n_placements == 0) return GpuBuildStatus::Ok;
    DeviceMem mem;
    unsigned long long* d_counts;
    BLOK_GPU_TRY(mem.alloc(&d_counts, kCountSlots * kSlotWords));
    BLOK_GPU_TRY(hipMemsetAsync(d_counts, 0, kCountSlots * kSlotWords * sizeof(unsigned long long), nullptr));
    const int64_t dims[3] = {v->nx, v->ny, v->nz};
    for (uint32_t i = 0; i < n_placements; ++i) {
        const blok_instance& I = placements[i];
        const StampModel& M = models[i];
        // the volume's box in the model's lattice, cut with the model's box; and the world box that cut lands on
        int64_t clo[3], chi[3];
        uint32_t wlo[3], whi[3];
        bool empty = false;
        for (uint32_t k = 0; k < 3u; ++k) {
            const uint32_t ax = I.axis[k];
            int64_t lo, hi;
            S::local_span(I, k, v->origin[ax], int64_t(v->origin[ax]) + dims[ax], lo, hi);
            clo[k] = std::max<int64_t>(lo, M.lo[k]); chi[k] = std::min<int64_t>(hi, M.hi[k]);
            if (clo[k] >= chi[k]) { empty = true; break; }
            int64_t a0, a1;
            S::world_span(I, k, clo[k], chi[k], a0, a1);
            wlo[ax] = static_cast<uint32_t>(a0 - v->origin[ax]); whi[ax] = static_cast<uint32_t>(a1 - v->origin[ax]);
        }
        if (empty) continue;                                      // wholly outside: nothing written, not an error
        StampArgs a{};
        a.nodes = M.nodes; a.materials = M.materials; a.levels = M.levels;
        placed_brick_range(M, clo, chi, a.b0, a.nb);
        for (int k = 0; k < 3; ++k) { a.origin[k] = M.origin[k]; a.box_origin[k] = v->origin[k]; }
        a.place = I;
        a.nx = v->nx; a.ny = v->ny; a.nz = v->nz;
        a.density = v->d_density; a.ids = v->d_ids; a.mode = mode; a.value = density; a.counts = d_counts;
        hipLaunchKernelGGL(stamp_kernel, dim3((a.nb[0] + 3u) / 4u, a.nb[1], a.nb[2]), dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
        // this placement's box alone: two far-apart stamps must not refresh what lies between them
        const GpuBuildStatus st = gpu_volume_commit(v, wlo, whi, mode != BLOK_STAMP_ERASE ? Edit::MayFill : Edit::OnlyClears, why);
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
