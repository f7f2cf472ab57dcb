// The edit that thresholds a snapshot field over its region (gpu_build.h: gpu_volume_edit_by_distance, gpu_volume_edit_by_flood), once
// for both: a lane per region cell, 64 along x per wave; it reads the snapshot and the density, runs the per-cell step the host build runs
// (../common/field_edit_core.h), counts through a ballot and one atomic per wave; then the commit of every edit runs over the region.
// Included by distance_kernels.hip and flood_kernels.hip, local to each: each instantiates it with its own rule.
#ifndef BLOK_FIELD_EDIT_H
#define BLOK_FIELD_EDIT_H
#include <hip/hip_runtime.h>

#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/field_edit_core.h"

namespace blok {
namespace {

template <class Rule>
struct FieldEditArgs {
    float* density; uint32_t* ids;
    const uint16_t* field;
    uint32_t nx, ny;
    uint32_t lo[3], ext[3];
    uint32_t x_chunks;
    uint64_t n_waves;
    Rule rule;
    uint64_t* count;
};

template <class Rule>
__global__ __launch_bounds__(256) void field_edit_kernel(const FieldEditArgs<Rule> a) {
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t xc, y, z;
    row_segment(wave, a.x_chunks, a.ext[1], xc, y, z);
    const uint32_t x = 64u * xc + lane;
    bool writes = false;
    if (x < a.ext[0]) {
        const size_t cell = (a.lo[0] + x) + (a.lo[1] + y) * static_cast<size_t>(a.nx) + (a.lo[2] + z) * (static_cast<size_t>(a.nx) * a.ny);
        writes = field_edit::edit_cell(a.rule, a.field[x + static_cast<size_t>(a.ext[0]) * (y + static_cast<size_t>(a.ext[1]) * z)], a.density[cell], a.ids[cell]);
    }
    const uint32_t n = static_cast<uint32_t>(__popcll(__ballot(writes)));
    if (lane == 0u && n) atomicAdd(reinterpret_cast<unsigned long long*>(a.count), static_cast<unsigned long long>(n));
}

// The edit of the region [lo, lo + ext) (box-local, inside the box) by `rule` over its snapshot `field`; `entry` names the caller in the
// messages, may_fill says that the op may fill a voxel.  Writes the store, then commits the region as every edit does.  Blocking.
template <class Rule>
GpuBuildStatus edit_by_field(GpuVolume* v, const char* entry, const Rule& rule, const uint32_t lo[3], const uint32_t ext[3], const uint16_t* field,
                             bool may_fill, uint64_t* out_n_voxels, std::string* why) {
    *out_n_voxels = 0;
    if (!cells_fit_32_bits(v, entry, why)) return GpuBuildStatus::Unsupported;
    if (!ext[0] || !ext[1] || !ext[2]) return GpuBuildStatus::Ok;                          // an empty snapshot: nothing to write
    FieldEditArgs<Rule> a{};
    a.density = v->d_density; a.ids = v->d_ids; a.field = field; a.nx = v->nx; a.ny = v->ny;
    uint32_t hi[3];
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo[k]; a.ext[k] = ext[k]; hi[k] = lo[k] + ext[k]; }
    a.x_chunks = (a.ext[0] + 63u) / 64u;
    a.n_waves = static_cast<uint64_t>(a.x_chunks) * a.ext[1] * a.ext[2];
    a.rule = rule;
    DeviceMem mem;
    BLOK_GPU_TRY(mem.alloc(&a.count, 1u));
    BLOK_GPU_TRY(hipMemsetAsync(a.count, 0, sizeof(uint64_t), nullptr));
    hipLaunchKernelGGL(field_edit_kernel<Rule>, dim3(static_cast<uint32_t>((a.n_waves + 3u) / 4u)), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    const GpuBuildStatus st = gpu_volume_commit(v, a.lo, hi, may_fill ? Edit::MayFill : Edit::OnlyClears, why);      // (a PAINT changes no mask: the commit still marks its bricks dirty)
    BLOK_GPU_TRY(hipMemcpy(out_n_voxels, a.count, sizeof(uint64_t), hipMemcpyDeviceToHost));      // blocking, as gpu_volume_set_voxels is
    return st;
}

}  // namespace
}  // namespace blok
#endif
