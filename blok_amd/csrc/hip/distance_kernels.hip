// The capped squared distance field of the resident volume and the edits that threshold it (gpu_build.h: gpu_volume_distance_field /
// gpu_volume_edit_by_distance; include/blok_hip.h: blok_hip_volume_distance_field has the contract; the rules live in
// ../common/distance_core.h, shared with the host build).
//
// The field is three capped min-plus passes, one per axis (distance_core.h: why they compose exactly):
//   x. from the brick masks alone, in either layout (BrickMasks::at), never from the densities.  A workgroup takes the 16 cell rows of 64
//      bricks along x — 256 cells — with 64 bricks of halo on either side (255 cells reach no further): every lane loads one mask word,
//      turns it into source bits (cells past the box's end and whole bricks outside it take the outside state, TO_EMPTY inverts), the
//      nibbles are gathered into 16 bit strings of 768 bits in LDS, and a lane per cell finds the nearest source bit at or below and at or
//      above it with count-leading / count-trailing-zero steps over 64-bit words.  It runs over the region widened by R in y and z and
//      clipped to the box, and writes the squared distance along x, or FAR.
//   y, z. one kernel for both: a workgroup owns 64 consecutive x by 32 output rows along the pass's axis, and slides over the 32 + 2 R input
//      rows it needs in chunks of 64 rows staged in LDS (8 KiB); R <= 16 is one chunk.  A wave owns 8 of the output rows, a lane one x:
//      every global access is 128 contiguous bytes per wave instruction, every LDS read is conflict-free, and the window is a plain loop
//      over the rows of the chunk within R.  Rows outside the box enter as 0 or FAR (distance_core.h: outside_value).  The y pass runs
//      over the region widened by R in z; the z pass writes the snapshot and counts it: ballots, one atomic per wave and counter.
// The edit is field_edit.h's, with the distance rule.
// Everything is on the null stream, behind earlier edits.  The intermediates live for the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "field_edit.h"
#include "../common/distance_core.h"

namespace blok {

namespace {

namespace D = distance;

// ---- x pass ---------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRowBricks = 64u;                              // bricks along x whose cells a workgroup writes: 256 cells, a lane each
constexpr uint32_t kWindowBricks = 3u * kRowBricks;               // with a halo of 256 cells on either side
constexpr uint32_t kWindowWords = kWindowBricks * 4u / 64u;       // 12 words per bit string

struct AxisXArgs {
    BrickMasks masks;
    uint32_t nx, nbx;                                             // the box along x, in cells and bricks
    int32_t brick0;                                               // brick of the region's first cell: string bit 256 of chunk 0 is its cell 0
    uint32_t x_lo, x_hi, y_lo, y_hi, z_lo, z_hi;                  // cells written: the region along x, widened and clipped along y and z
    uint32_t by0, bz0, n_by;                                      // brick rows that hold them
    uint32_t x_chunks;
    uint32_t radius, to_empty, outside_filled;
    uint16_t* out;                                                // [x - x_lo + (x_hi - x_lo) * ((y - y_lo) + (y_hi - y_lo) * (z - z_lo))]
};

__global__ __launch_bounds__(256) void distance_x_kernel(const AxisXArgs a) {
    __shared__ uint64_t s_mask[kWindowBricks];                    // source bits of the window's bricks, bit x + 4 y + 16 z
    __shared__ uint64_t s_word[16][kWindowWords];                 // the 16 cell rows as bit strings along x
    const uint32_t t = threadIdx.x;
    const uint32_t xc = blockIdx.x % a.x_chunks, by = a.by0 + (blockIdx.x / a.x_chunks) % a.n_by, bz = a.bz0 + blockIdx.x / (a.x_chunks * a.n_by);
    if (t < kWindowBricks) {
        uint64_t m = 0ull;
        // only the bricks within R cells of the 256 written ones are looked at: the searches below stop at R
        if (4u * t + 3u + a.radius >= 4u * kRowBricks && 4u * t <= 8u * kRowBricks - 1u + a.radius) {
            const int32_t bx = a.brick0 + static_cast<int32_t>(kRowBricks * xc + t) - static_cast<int32_t>(kRowBricks);
            const uint64_t outside = a.outside_filled ? ~0ull : 0ull;
            if (bx < 0 || bx >= static_cast<int32_t>(a.nbx)) m = outside;
            else {
                m = a.masks.at(static_cast<uint32_t>(bx), by, bz);
                const uint32_t wx = a.nx - 4u * static_cast<uint32_t>(bx);      // cells of the brick inside the box along x, when below 4
                if (wx < 4u) {
                    const uint64_t inside = 0x1111111111111111ull * ((1ull << wx) - 1ull);
                    m = (m & inside) | (outside & ~inside);
                }
            }
            if (a.to_empty) m = ~m;
        }
        s_mask[t] = m;
    }
    __syncthreads();
    if (t < 16u * kWindowWords) {
        const uint32_t r = t / kWindowWords, w = t % kWindowWords;
        uint64_t word = 0ull;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) word |= ((s_mask[16u * w + k] >> (4u * r)) & 0xFull) << (4u * k);
        s_word[r][w] = word;
    }
    __syncthreads();
    const uint32_t x = static_cast<uint32_t>(a.brick0) * 4u + 4u * kRowBricks * xc + t;      // (the region lies in the box: brick0 >= 0)
    if (x < a.x_lo || x >= a.x_hi) return;
    const size_t ex = a.x_hi - a.x_lo, ey = a.y_hi - a.y_lo;
    for (uint32_t r = 0; r < 16u; ++r) {
        const uint32_t y = 4u * by + (r & 3u), z = 4u * bz + (r >> 2);
        if (y < a.y_lo || y >= a.y_hi || z < a.z_lo || z >= a.z_hi) continue;              // (wave-uniform)
        const auto word = [&](uint32_t i) { return s_word[r][i]; };
        const uint32_t p = 4u * kRowBricks + t;
        const uint32_t value = D::axis_value(D::nearest_below(word, p, a.radius), D::nearest_above(word, p, a.radius, kWindowWords), a.radius);
        a.out[(x - a.x_lo) + ex * ((y - a.y_lo) + ey * (z - a.z_lo))] = static_cast<uint16_t>(value);
    }
}

// ---- y and z passes -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kTileX = 64u;                                  // consecutive x per workgroup: a lane each
constexpr uint32_t kTileRows = 32u;                               // output rows along the axis per workgroup: 8 per wave
constexpr uint32_t kChunkRows = 64u;                              // input rows staged in LDS at a time: 64 x 64 x 2 bytes = 8 KiB
constexpr uint32_t kRowsPerWave = kTileRows / 4u;

struct AxisArgs {
    const uint16_t* in; uint16_t* out;
    uint32_t ex;                                                  // cells along x, of both arrays
    uint32_t x_chunks, a_tiles;
    uint64_t in_stride_a, in_stride_b, out_stride_a, out_stride_b;      // a: the pass's axis, b: the other one
    int32_t in_lo, out_lo, box_n;                                 // box coordinate of row 0 of either array along the axis; the box's extent along it
    uint32_t in_rows, out_rows;
    uint32_t radius, outside;                                     // outside: what a row outside the box enters as
    uint64_t* counts;                                             // the last pass: [0] cells with 0, [1] cells within R^2; else null
};

__global__ __launch_bounds__(256) void distance_axis_kernel(const AxisArgs a) {
    __shared__ uint16_t s_tile[kChunkRows][kTileX];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t xc = blockIdx.x % a.x_chunks, ta = (blockIdx.x / a.x_chunks) % a.a_tiles, b = blockIdx.x / (a.x_chunks * a.a_tiles);
    const uint32_t x = kTileX * xc + lane;
    const bool in_x = x < a.ex;
    const int32_t radius = static_cast<int32_t>(a.radius);
    const int32_t a0 = a.out_lo + static_cast<int32_t>(kTileRows * ta);                    // box coordinate of the tile's first output row
    const int32_t window_end = a0 + static_cast<int32_t>(kTileRows) + radius;             // one past the last input row any output row needs
    const uint16_t* in = a.in + b * a.in_stride_b + x;
    uint32_t best[kRowsPerWave];
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerWave; ++i) best[i] = D::kFar;
    for (int32_t c0 = a0 - radius; c0 < window_end; c0 += static_cast<int32_t>(kChunkRows)) {
        // stage rows c0 .. c0 + 63: rows outside the box are constant, rows inside it lie in the input (widened by R, clipped to the box)
#pragma unroll 4
        for (uint32_t j = wave; j < kChunkRows; j += 4u) {
            const int32_t row = c0 + static_cast<int32_t>(j);
            uint32_t g = D::kFar;
            if (row < window_end && in_x) {
                if (row < 0 || row >= a.box_n) g = a.outside;
                else if (static_cast<uint32_t>(row - a.in_lo) < a.in_rows) g = in[static_cast<uint64_t>(row - a.in_lo) * a.in_stride_a];
            }
            s_tile[j][lane] = static_cast<uint16_t>(g);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kRowsPerWave; ++i) {
            const int32_t row = a0 + static_cast<int32_t>(kRowsPerWave * wave + i);        // (wave-uniform, and so are the loop's ends)
            const int32_t j_lo = max(row - radius - c0, 0), j_hi = min(row + radius - c0, static_cast<int32_t>(kChunkRows) - 1);
            for (int32_t j = j_lo; j <= j_hi; ++j) best[i] = D::min_plus_tap(best[i], s_tile[j][lane], c0 + j - row);
        }
        __syncthreads();
    }
    uint32_t n_zero = 0u, n_near = 0u;
    uint16_t* out = a.out + b * a.out_stride_b + x;
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerWave; ++i) {
        const uint32_t row = kTileRows * ta + kRowsPerWave * wave + i;                     // counted from the output's first row
        const bool live = in_x && row < a.out_rows;
        const uint32_t value = D::min_plus_cap(best[i], a.radius * a.radius);
        if (live) out[static_cast<uint64_t>(row) * a.out_stride_a] = static_cast<uint16_t>(value);
        if (a.counts) {
            n_zero += static_cast<uint32_t>(__popcll(__ballot(live && value == 0u)));
            n_near += static_cast<uint32_t>(__popcll(__ballot(live && value != 0u && value != D::kFar)));
        }
    }
    if (a.counts && lane == 0u) {
        if (n_zero) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts), static_cast<unsigned long long>(n_zero));
        if (n_near) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + 1), static_cast<unsigned long long>(n_near));
    }
}

}  // namespace

GpuBuildStatus gpu_volume_distance_field(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t max_radius, uint32_t flags,
                                         GpuDistance* out, std::string* why) {
    uint32_t ext[3];
    GpuBuildStatus begun;
    const bool has_cells = gpu_field_begin(v, "distance_field", lo, hi, flags, out, ext, &begun, why);
    blok_distance_info& info = out->info;
    info.max_radius = max_radius;
    if (!has_cells) return begun;
    const uint64_t cells = static_cast<uint64_t>(ext[0]) * ext[1] * ext[2];
    // the region widened by R along y and z, clipped to the box: what the x pass (both) and the y pass (z) run over
    const uint32_t R = max_radius;
    const uint32_t y_lo = lo[1] > R ? lo[1] - R : 0u, y_hi = std::min(v->ny, hi[1] + R), z_lo = lo[2] > R ? lo[2] - R : 0u, z_hi = std::min(v->nz, hi[2] + R);
    const uint64_t wy = y_hi - y_lo, wz = z_hi - z_lo;
    // the y and z launches' block counts, before anything is allocated: a box a cell or two wide and billions long would pass the cell
    // check above and ask for more blocks than a grid's x extent holds (gpu_volume_create admits 4^7 cells per axis, so none exists today)
    const uint32_t xt = (ext[0] + kTileX - 1u) / kTileX, yt = (ext[1] + kTileRows - 1u) / kTileRows, zt = (ext[2] + kTileRows - 1u) / kTileRows;
    if (static_cast<uint64_t>(xt) * yt * wz > 0x7FFFFFFFull || static_cast<uint64_t>(xt) * zt * ext[1] > 0x7FFFFFFFull) {
        *why = "distance_field: region of more than 2^31 tiles"; return GpuBuildStatus::Unsupported;
    }
    DeviceMem mem;
    uint16_t *d_gx, *d_gy, *d_field;
    uint64_t* d_counts;
    BLOK_GPU_TRY(mem.alloc(&d_gx, ext[0] * wy * wz));
    BLOK_GPU_TRY(mem.alloc(&d_gy, ext[0] * static_cast<uint64_t>(ext[1]) * wz));
    BLOK_GPU_TRY(mem.alloc(&d_field, cells));
    BLOK_GPU_TRY(mem.alloc(&d_counts, 2u));
    BLOK_GPU_TRY(hipMemsetAsync(d_counts, 0, 2u * sizeof(uint64_t), nullptr));
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    AxisXArgs ax{};
    ax.masks = brick_masks_of(*v); ax.nx = v->nx; ax.nbx = v->nbx;
    ax.brick0 = static_cast<int32_t>(lo[0] / 4u);
    ax.x_lo = lo[0]; ax.x_hi = hi[0]; ax.y_lo = y_lo; ax.y_hi = y_hi; ax.z_lo = z_lo; ax.z_hi = z_hi;
    ax.by0 = y_lo / 4u; ax.bz0 = z_lo / 4u; ax.n_by = (y_hi - 1u) / 4u - ax.by0 + 1u;
    const uint32_t n_bz = (z_hi - 1u) / 4u - ax.bz0 + 1u;
    ax.x_chunks = (hi[0] - 4u * static_cast<uint32_t>(ax.brick0) + 4u * kRowBricks - 1u) / (4u * kRowBricks);
    ax.radius = R; ax.to_empty = D::to_empty(flags) ? 1u : 0u; ax.outside_filled = D::outside_filled(flags) ? 1u : 0u;
    ax.out = d_gx;
    const uint64_t x_blocks = static_cast<uint64_t>(ax.x_chunks) * ax.n_by * n_bz;      // at most the volume's bricks: below 2^31 (gpu_volume_create)
    hipLaunchKernelGGL(distance_x_kernel, dim3(static_cast<uint32_t>(x_blocks)), dim3(256), 0, nullptr, ax);
    BLOK_GPU_TRY(hipGetLastError());
    AxisArgs ay{};
    ay.in = d_gx; ay.out = d_gy; ay.ex = ext[0];
    ay.x_chunks = (ext[0] + kTileX - 1u) / kTileX; ay.a_tiles = (ext[1] + kTileRows - 1u) / kTileRows;
    ay.in_stride_a = ext[0]; ay.in_stride_b = ext[0] * wy; ay.out_stride_a = ext[0]; ay.out_stride_b = static_cast<uint64_t>(ext[0]) * ext[1];
    ay.in_lo = static_cast<int32_t>(y_lo); ay.in_rows = static_cast<uint32_t>(wy); ay.out_lo = static_cast<int32_t>(lo[1]); ay.out_rows = ext[1];
    ay.box_n = static_cast<int32_t>(v->ny); ay.radius = R; ay.outside = D::outside_value(flags); ay.counts = nullptr;
    hipLaunchKernelGGL(distance_axis_kernel, dim3(static_cast<uint32_t>(static_cast<uint64_t>(ay.x_chunks) * ay.a_tiles * wz)), dim3(256), 0, nullptr, ay);
    BLOK_GPU_TRY(hipGetLastError());
    AxisArgs az{};
    az.in = d_gy; az.out = d_field; az.ex = ext[0];
    az.x_chunks = ay.x_chunks; az.a_tiles = (ext[2] + kTileRows - 1u) / kTileRows;
    az.in_stride_a = static_cast<uint64_t>(ext[0]) * ext[1]; az.in_stride_b = ext[0]; az.out_stride_a = az.in_stride_a; az.out_stride_b = ext[0];
    az.in_lo = static_cast<int32_t>(z_lo); az.in_rows = static_cast<uint32_t>(wz); az.out_lo = static_cast<int32_t>(lo[2]); az.out_rows = ext[2];
    az.box_n = static_cast<int32_t>(v->nz); az.radius = R; az.outside = ay.outside; az.counts = d_counts;
    hipLaunchKernelGGL(distance_axis_kernel, dim3(static_cast<uint32_t>(static_cast<uint64_t>(az.x_chunks) * az.a_tiles * ext[1])), dim3(256), 0, nullptr, az);
    BLOK_GPU_TRY(hipGetLastError());
    uint64_t counts[2] = {0, 0};
    BLOK_GPU_TRY(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));      // (the call's wait)
    info.n_zero = counts[0]; info.n_near = counts[1]; info.n_far = cells - counts[0] - counts[1];
    mem.release(d_field);
    out->d_field = d_field;
    return GpuBuildStatus::Ok;
}

GpuBuildStatus gpu_volume_edit_by_distance(GpuVolume* v, const GpuDistance* field, int op, uint32_t d2, float density, uint32_t material,
                                           uint64_t* out_n_voxels, std::string* why) {
    return edit_by_field(v, "edit_by_distance", field_edit::distance_rule(op, d2, density, material), field->lo, field->info.ext, field->d_field,
                         op == BLOK_DISTANCE_GROW, out_n_voxels, why);
}

}  // namespace blok
