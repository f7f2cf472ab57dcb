// The edit that thresholds a snapshot field over its region (include/blok_hip.h: blok_hip_volume_edit_by_distance,
// blok_hip_volume_edit_by_flood), once: the per-cell step the kernel (hip/field_edit.h) and the host build (edit_host below, for
// host/distance.cpp and host/flood.cpp) both run.  The rules stay in distance_core.h and flood_core.h; a rule object is {op, threshold}
// and what a written cell gets, over them.  No HIP types.
#ifndef BLOK_FIELD_EDIT_CORE_H
#define BLOK_FIELD_EDIT_CORE_H
#include <stddef.h>
#include <stdint.h>

#include "distance_core.h"
#include "flood_core.h"
#include "region_core.h"

#if defined(__HIPCC__)
#define BLOK_FIELD_EDIT_HD __host__ __device__ inline
#else
#define BLOK_FIELD_EDIT_HD inline
#endif

namespace blok {
namespace field_edit {

struct DistanceRule {
    int op; uint32_t threshold;
    float value; uint32_t material;                               // what a written cell gets
    BLOK_FIELD_EDIT_HD bool writes(uint32_t dist, float density) const { return distance::edit_writes(op, dist, threshold, distance::filled(density)); }
    BLOK_FIELD_EDIT_HD constexpr bool writes_density() const { return true; }
};
BLOK_FIELD_EDIT_HD DistanceRule distance_rule(int op, uint32_t d2, float density, uint32_t material) {
    const bool grow = op == BLOK_DISTANCE_GROW;
    return DistanceRule{op, d2, grow ? density : 0.0f, grow ? material : 0u};
}

struct FloodRule {
    int op; uint32_t threshold;
    float value; uint32_t material;                               // what a written cell gets (PAINT: the id alone)
    BLOK_FIELD_EDIT_HD bool writes(uint32_t dist, float density) const { return flood::edit_writes(op, dist, threshold, flood::filled(density)); }
    BLOK_FIELD_EDIT_HD bool writes_density() const { return flood::op_writes_density(op); }
};
BLOK_FIELD_EDIT_HD FloodRule flood_rule(int op, uint32_t d, float density, uint32_t material) {
    return FloodRule{op, d, flood::written_density(op, density), flood::written_material(op, material)};
}

// One cell whose snapshot value is `dist`: decides, writes, and says whether it wrote.
template <class Rule>
BLOK_FIELD_EDIT_HD bool edit_cell(const Rule& rule, uint32_t dist, float& density, uint32_t& id) {
    if (!rule.writes(dist, density)) return false;
    if (rule.writes_density()) density = rule.value;
    id = rule.material;
    return true;
}

// The host build's edit behind its argument check: the snapshot's region against the box, then every cell of it, x fastest.
template <class Info, class Rule>
inline int edit_host(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const uint16_t* field,
                     const Info& info, const Rule& rule, uint64_t* out_n_voxels) {
    const uint32_t dims[3] = {nx, ny, nz};
    int32_t region_hi[3];
    for (int a = 0; a < 3; ++a) {
        if (info.ext[a] > dims[a]) return BLOK_ERR_UNSUPPORTED;
        region_hi[a] = static_cast<int32_t>(int64_t(info.lo[a]) + info.ext[a]);
    }
    uint32_t lo[3], hi[3];
    const int rc = region::status(region::local(origin, dims, info.lo, region_hi, lo, hi));
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    const size_t ext[3] = {info.ext[0], info.ext[1], info.ext[2]};
    if (!ext[0] || !ext[1] || !ext[2]) return BLOK_OK;            // an empty snapshot: nothing to write
    if (!density || !material_ids || !field) return BLOK_ERR_INVALID_ARG;
    uint64_t n = 0;
    for (size_t z = 0; z < ext[2]; ++z)
        for (size_t y = 0; y < ext[1]; ++y)
            for (size_t x = 0; x < ext[0]; ++x) {
                const size_t cell = (lo[0] + x) + ((lo[2] + z) * ny + (lo[1] + y)) * nx;
                if (edit_cell(rule, field[x + ext[0] * (y + ext[1] * z)], density[cell], material_ids[cell])) ++n;
            }
    if (out_n_voxels) *out_n_voxels = n;
    return BLOK_OK;
}

}  // namespace field_edit
}  // namespace blok
#endif
