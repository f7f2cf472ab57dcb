// The column field and scatter on the host (include/blok_world.h: blok_column_field, blok_scatter): the contracts of
// blok_hip_volume_column_field and blok_hip_volume_scatter_models (blok_hip.h) over host arrays, through the rules the kernels use
// (../common/columns_core.h).  The field walks each column sixteen cells at a time over bits made from density > 0; scatter is a loop over the
// region's columns in index order.
#include "blok_world.h"
#include "../common/columns_core.h"
#include "../common/region_core.h"

#include <cstdint>

namespace K = blok::columns;

extern "C" {

int blok_column_field(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                      const int32_t region_lo[3], const int32_t region_hi[3], uint32_t axis, uint32_t flags, uint16_t* out_top,
                      uint32_t* out_material, blok_columns_info* out_info) {
    if (K::check_field_args(axis, flags) != 0) return BLOK_ERR_INVALID_ARG;
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t lo[3], hi[3];
    const int rc = blok::region::status(blok::region::local(origin, dims, region_lo, region_hi, lo, hi));
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    blok_columns_info info{};
    info.version = 1u; info.flags = flags; info.axis = axis; info.min_top = K::kNone; info.max_top = 0u;
    for (int a = 0; a < 3; ++a) { info.lo[a] = (origin ? origin[a] : 0) + static_cast<int32_t>(lo[a]); info.ext[a] = hi[a] - lo[a]; }
    const uint32_t p = K::axis_p(axis), q = K::axis_q(axis);
    if (info.ext[0] && info.ext[1] && info.ext[2]) {
        if (!density || !material_ids || !out_top || !out_material) return BLOK_ERR_INVALID_ARG;
        info.n_columns = uint64_t(info.ext[p]) * info.ext[q];
        const size_t stride[3] = {1u, nx, size_t(nx) * ny};
        const bool low = K::from_low(flags);
        for (uint32_t cq = 0; cq < info.ext[q]; ++cq)
            for (uint32_t cp = 0; cp < info.ext[p]; ++cp) {
                const size_t base = (lo[p] + cp) * stride[p] + (lo[q] + cq) * stride[q];
                // the column's sixteen cells of the bricks 4 g .. 4 g + 3 along the axis, cells past the box's end empty
                const auto bits_at = [&](uint32_t g) {
                    uint32_t bits = 0;
                    for (uint32_t k = 0; k < 16u; ++k)
                        if (16u * g + k < dims[axis] && density[base + (16u * g + k) * stride[axis]] > 0.0f) bits |= 1u << k;
                    return bits;
                };
                const uint32_t top = K::column_top(bits_at, lo[axis], hi[axis], low);
                const uint64_t column = cp + uint64_t(info.ext[p]) * cq;
                out_top[column] = static_cast<uint16_t>(top);
                out_material[column] = top == K::kNone ? 0u : material_ids[base + (lo[axis] + top) * stride[axis]];
                if (top != K::kNone) {
                    ++info.n_hit;
                    if (top < info.min_top) info.min_top = top;
                    if (top > info.max_top) info.max_top = top;
                }
            }
    }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

int blok_scatter(const uint16_t* top, const uint32_t* material, const blok_columns_info* columns_info, const blok_scatter_params* params,
                 const blok_scatter_entry* entries, uint32_t n_entries, blok_instance* out_instances, uint64_t capacity, blok_scatter_info* out_info) {
    if (K::check_scatter_args(columns_info, params, entries, n_entries) != 0) return BLOK_ERR_INVALID_ARG;
    const bool has_columns = columns_info->ext[0] && columns_info->ext[1] && columns_info->ext[2];
    if (has_columns && (!top || !material)) return BLOK_ERR_INVALID_ARG;
    const K::Field f = K::field_of(top, material, *columns_info);
    blok_scatter_info info{};
    info.version = 1u; info.flags = params->flags;
    const uint32_t w = K::weight_sum(entries, n_entries);
    // counted first, so that a table too small is refused before anything is written
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !out_instances) break;
        uint64_t n = 0;
        for (uint32_t z = 0; has_columns && z < f.ext[2]; ++z)
            for (uint32_t x = 0; x < f.ext[0]; ++x) {
                const int verdict = K::judge(f, *params, x, z);
                if (pass == 1) { if (verdict == K::kPlaced) out_instances[n++] = K::place(f, *params, entries, n_entries, w, x, z); continue; }
                if (verdict == K::kNotCandidate) continue;
                ++info.n_cells;
                if (verdict == K::kPlaced) ++info.n_placed; else ++info.n_rejected[verdict - K::kRejected];
            }
        if (pass == 0 && out_instances && capacity < info.n_placed) return BLOK_ERR_INVALID_ARG;
    }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

}  // extern "C"
