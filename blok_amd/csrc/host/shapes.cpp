// The shape table on the host (include/blok_world.h: blok_shapes_check, blok_shape_bounds, blok_shapes_voxels): the contract of
// blok_hip_volume_apply_shapes (blok_hip.h) over host arrays, through the rules the kernels use (../common/shapes_core.h).  The table is
// applied as the contract words it: shape by shape, in order, each over its own voxel box cut with the volume's.
#include "blok_world.h"
#include "../common/shapes_core.h"

#include <cstdint>
#include <cstdio>

namespace K = blok::shapes;

extern "C" {

int blok_shapes_check(const blok_shape* shapes, uint32_t n_shapes, uint32_t* out_index, char* err, size_t err_len) {
    if (out_index) *out_index = 0;
    if (err && err_len) err[0] = 0;
    const char* text = nullptr;
    uint32_t at = 0;
    if (n_shapes > BLOK_SHAPES_MAX) text = "more than BLOK_SHAPES_MAX shapes";
    else if (n_shapes && !shapes) text = "null table with a non-zero count";
    else
        for (uint32_t i = 0; i < n_shapes && !text; ++i)
            if (const int rule = K::check(shapes[i])) { text = K::rule_text(rule); at = i; }
    if (!text) return BLOK_OK;
    if (out_index) *out_index = at;
    if (err && err_len) std::snprintf(err, err_len, "shape %u: %s", at, text);
    return BLOK_ERR_INVALID_ARG;
}

int blok_shape_bounds(const blok_shape* shape, int32_t out_lo[3], int32_t out_hi[3]) {
    if (!shape || !out_lo || !out_hi || K::check(*shape)) return BLOK_ERR_INVALID_ARG;
    int64_t lo[3], hi[3];
    K::bounds(*shape, lo, hi);
    for (int k = 0; k < 3; ++k) { out_lo[k] = static_cast<int32_t>(lo[k]); out_hi[k] = static_cast<int32_t>(hi[k]); }
    return BLOK_OK;
}

int blok_shapes_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const blok_shape* shapes, uint32_t n_shapes, uint64_t* out_n_written) {
    if (out_n_written) *out_n_written = 0;
    if (!density || !material_ids || !nx || !ny || !nz) return BLOK_ERR_INVALID_ARG;
    const int rc = blok_shapes_check(shapes, n_shapes, nullptr, nullptr, 0);
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    const int64_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    const int64_t dims[3] = {nx, ny, nz};
    uint64_t written = 0;
    for (uint32_t i = 0; i < n_shapes; ++i) {
        const blok_shape& s = shapes[i];
        int64_t lo[3], hi[3];
        K::bounds(s, lo, hi);
        for (int k = 0; k < 3; ++k) {                              // box-local, cut with the box
            lo[k] = lo[k] - o[k] < 0 ? 0 : lo[k] - o[k];
            hi[k] = hi[k] - o[k] > dims[k] ? dims[k] : hi[k] - o[k];
        }
        for (int64_t z = lo[2]; z < hi[2]; ++z)
            for (int64_t y = lo[1]; y < hi[1]; ++y)
                for (int64_t x = lo[0]; x < hi[0]; ++x) {
                    if (!K::inside(s, 2 * (o[0] + x) + 1, 2 * (o[1] + y) + 1, 2 * (o[2] + z) + 1)) continue;
                    const size_t cell = size_t(x) + (size_t(z) * ny + size_t(y)) * nx;
                    written += K::apply(s, density[cell], material_ids[cell]);
                }
    }
    if (out_n_written) *out_n_written = written;
    return BLOK_OK;
}

}  // extern "C"
