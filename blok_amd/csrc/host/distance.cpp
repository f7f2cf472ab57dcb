// The distance field on the host (include/blok_world.h: blok_distance_field, blok_distance_edit): the contracts of
// blok_hip_volume_distance_field and blok_hip_volume_edit_by_distance (blok_hip.h) over host arrays, through the rules the kernels use
// (../common/distance_core.h).  Separable as the device's: nearest source along x by two scans of a row, then the capped min-plus step
// along y and along z, row against row so that the inner loop runs along x; input rows that hold no value are skipped.
#include "blok_world.h"
#include "../common/distance_core.h"
#include "../common/field_edit_core.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace D = blok::distance;

namespace {

// One min-plus pass along an axis whose rows are `ex` consecutive values: out row r (box coordinate out_lo + r) from the input rows within
// R of it; a row outside the box is `outside` throughout.  n_b independent slabs.
void axis_pass(const std::vector<uint16_t>& in, std::vector<uint16_t>& out, size_t ex, size_t in_stride_a, size_t in_stride_b, size_t out_stride_a,
               size_t out_stride_b, int64_t in_lo, int64_t in_rows, int64_t out_lo, int64_t out_rows, int64_t box_n, size_t n_b, int32_t R, uint32_t outside) {
    const uint32_t r2 = static_cast<uint32_t>(R * R);
    std::vector<uint8_t> any(static_cast<size_t>(in_rows));
    std::vector<uint32_t> best(ex);
    for (size_t b = 0; b < n_b; ++b) {
        for (int64_t r = 0; r < in_rows; ++r) {
            const uint16_t* row = in.data() + b * in_stride_b + static_cast<size_t>(r) * in_stride_a;
            any[static_cast<size_t>(r)] = std::any_of(row, row + ex, [](uint16_t g) { return g != D::kFar; });
        }
        for (int64_t r = 0; r < out_rows; ++r) {
            std::fill(best.begin(), best.end(), D::kFar);
            for (int32_t d = -R; d <= R; ++d) {
                const int64_t a = out_lo + r + d;
                if (a < 0 || a >= box_n) {
                    if (outside != D::kFar) for (size_t x = 0; x < ex; ++x) best[x] = D::min_plus_tap(best[x], outside, d);
                    continue;
                }
                if (!any[static_cast<size_t>(a - in_lo)]) continue;
                const uint16_t* row = in.data() + b * in_stride_b + static_cast<size_t>(a - in_lo) * in_stride_a;
                for (size_t x = 0; x < ex; ++x) best[x] = D::min_plus_tap(best[x], row[x], d);
            }
            uint16_t* o = out.data() + b * out_stride_b + static_cast<size_t>(r) * out_stride_a;
            for (size_t x = 0; x < ex; ++x) o[x] = static_cast<uint16_t>(D::min_plus_cap(best[x], r2));
        }
    }
}

}  // namespace

extern "C" {

int blok_distance_field(const float* density, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const int32_t region_lo[3],
                        const int32_t region_hi[3], uint32_t max_radius, uint32_t flags, uint16_t* out_field, blok_distance_info* out_info) {
    if (D::check_field_args(max_radius, flags) != D::kFine) return BLOK_ERR_INVALID_ARG;
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t lo[3], hi[3];
    const int rc = blok::region::status(blok::region::local(origin, dims, region_lo, region_hi, lo, hi));
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    blok_distance_info info{};
    info.version = 1u; info.flags = flags; info.max_radius = max_radius;
    size_t ext[3];
    for (int a = 0; a < 3; ++a) { ext[a] = hi[a] - lo[a]; info.lo[a] = (origin ? origin[a] : 0) + static_cast<int32_t>(lo[a]); info.ext[a] = hi[a] - lo[a]; }
    const size_t cells = ext[0] * ext[1] * ext[2];
    if (cells && (!density || !out_field)) return BLOK_ERR_INVALID_ARG;
    if (cells) {
        const uint32_t R = max_radius;
        const bool outside_source = D::outside_is_source(flags);
        // x, over the region widened by R along y and z and clipped to the box: the nearest source at or below each cell, then at or above
        const uint32_t y_lo = lo[1] > R ? lo[1] - R : 0u, y_hi = std::min(ny, hi[1] + R), z_lo = lo[2] > R ? lo[2] - R : 0u, z_hi = std::min(nz, hi[2] + R);
        const size_t wy = y_hi - y_lo, wz = z_hi - z_lo;
        std::vector<uint16_t> gx(ext[0] * wy * wz), gy(ext[0] * ext[1] * wz), field(cells);
        std::vector<uint32_t> below(ext[0]);
        for (uint32_t z = z_lo; z < z_hi; ++z)
            for (uint32_t y = y_lo; y < y_hi; ++y) {
                const float* row = density + (size_t(z) * ny + y) * nx;
                const auto source = [&](int64_t x) { return x < 0 || x >= int64_t(nx) ? outside_source : D::is_source(D::filled(row[x]), flags); };
                uint16_t* o = gx.data() + ((z - z_lo) * wy + (y - y_lo)) * ext[0];
                // a scan needs the sources up to R cells before the region's first cell: it starts there
                uint32_t run = D::kNone;                          // distance to the last source seen
                for (int64_t x = int64_t(lo[0]) - R; x < int64_t(hi[0]); ++x) {
                    run = source(x) ? 0u : run == D::kNone ? D::kNone : run + 1u;
                    if (x >= int64_t(lo[0])) below[static_cast<size_t>(x - lo[0])] = run;
                }
                run = D::kNone;
                for (int64_t x = int64_t(hi[0]) - 1 + R; x >= int64_t(lo[0]); --x) {
                    run = source(x) ? 0u : run == D::kNone ? D::kNone : run + 1u;
                    if (x < int64_t(hi[0])) o[x - lo[0]] = static_cast<uint16_t>(D::axis_value(below[static_cast<size_t>(x - lo[0])], run, R));
                }
            }
        const uint32_t outside = D::outside_value(flags);
        axis_pass(gx, gy, ext[0], ext[0], ext[0] * wy, ext[0], ext[0] * ext[1], y_lo, int64_t(wy), lo[1], int64_t(ext[1]), ny, wz, int32_t(R), outside);
        axis_pass(gy, field, ext[0], ext[0] * ext[1], ext[0], ext[0] * ext[1], ext[0], z_lo, int64_t(wz), lo[2], int64_t(ext[2]), nz, ext[1], int32_t(R), outside);
        for (size_t i = 0; i < cells; ++i) {
            out_field[i] = field[i];
            if (field[i] == 0u) ++info.n_zero;
            else if (field[i] == D::kFar) ++info.n_far;
            else ++info.n_near;
        }
    }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

int blok_distance_edit(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const uint16_t* field,
                       const blok_distance_info* info, int op, uint32_t d2, float density_value, uint32_t material, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!info || D::check_edit_args(*info, op, d2, density_value) != D::kFine) return BLOK_ERR_INVALID_ARG;
    return blok::field_edit::edit_host(density, material_ids, origin, nx, ny, nz, field, *info, blok::field_edit::distance_rule(op, d2, density_value, material), out_n_voxels);
}

}  // extern "C"
