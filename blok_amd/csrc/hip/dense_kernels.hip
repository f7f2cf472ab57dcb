// Dense-grid path for BASELINE.json configs[1] ("256^3 dense grid, 1920x1080 primary-ray DDA, coalesced HBM, no SVO"): the
// uploaded id grid itself, kept in HBM in 8x8x8-cell tiles (2 KiB of ids each, so the 64 rays of a wave that meet neighbouring
// cells read the same few lines), plus one occupancy BIT per tile staged into LDS (256^3 -> 32^3 bits = 4 KiB) — the only
// acceleration structure.  One lane = one ray, walking the same T-sorted merge sequence of integer planes as the tree kernel
// (trace_kernels.h), two levels only: whole tiles whose bit is clear are stepped over, cells of occupied tiles one by one
// (Amanatides-Woo with every T evaluated from its integer plane, never accumulated), first filled cell whose clipped interval is
// non-empty wins.  Hence the records equal the tree kernel's and the reference's bit for bit.  No reference counterpart for
// the kernel (the reference has no DDA); the data it walks is Chunk::materialIds in bulk (reference
// blok/include/chunk.hpp:35-36).
#include "dense_kernels.h"
#include "dense_core.h"

namespace blok {

namespace {

// tiles the ids of an [nz][ny][nx] grid; cells beyond the grid inside the last tiles are 0
__global__ __launch_bounds__(256) void dense_tile_kernel(const uint32_t* ids, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t tx, uint32_t ty, uint32_t tz,
                                                          uint32_t* tiled, uint32_t* tile_bits) {
    const uint32_t tile = blockIdx.x;                    // one workgroup of 256 lanes per tile: 2 cells per lane
    if (tile >= tx * ty * tz) return;
    uint32_t any = 0;
    for (uint32_t c = threadIdx.x; c < 512u; c += 256u) {
        uint32_t x, y, z;
        dense_cell_of(tile, c, tx, ty, x, y, z);
        const uint32_t id = dense_source_id(ids, nx, ny, nz, x, y, z);
        tiled[static_cast<size_t>(tile) * 512u + c] = id;
        any |= id;
    }
    if (__syncthreads_or(any != 0u) && threadIdx.x == 0) atomicOr(tile_bits + (tile >> 5), 1u << (tile & 31u));
}

__global__ __launch_bounds__(64) void dense_kernel(const DenseArgs D) {
    extern __shared__ uint32_t lds_bits[];
    const TraceArgs& A = D.trace;
    const uint32_t lane = threadIdx.x;
    const bool bits_in_lds = D.bit_words <= kDenseLdsWords;
    if (bits_in_lds) {
        for (uint32_t i = lane; i < D.bit_words; i += 64u) lds_bits[i] = D.tile_bits[i];
        __syncthreads();
    }
    const uint32_t bx_count = (A.w + kWaveW - 1u) / kWaveW;
    const uint32_t bx = blockIdx.x % bx_count, by = blockIdx.x / bx_count;
    const uint32_t rx = bx * kWaveW + lane % kWaveW, ry = by * kWaveH + lane / kWaveW;
    if (rx >= A.w || ry >= A.h) return;
    const size_t out_index = static_cast<size_t>(ry) * A.w + rx;
    const Sink sink{A.out ? A.out + out_index : nullptr, A.out_rgba ? A.out_rgba + out_index : nullptr};
    const RayIn r = primary_ray(A, A.x0 + rx, A.y0 + ry);

    const DenseGrid G{{A.origin[0], A.origin[1], A.origin[2]}, D.tx, D.ty, D.tz, D.tiled};
    uint4 rec;
    if (!dense_walk(r, G, [&](uint32_t w) { return bits_in_lds ? lds_bits[w] : D.tile_bits[w]; }, rec)) { write_miss(sink); return; }
    if (sink.hit) *reinterpret_cast<uint4*>(sink.hit) = rec;
    if (sink.rgba) *sink.rgba = shade_rgba(A.mat_table, A.n_materials, rec.y, (rec.w >> 16) & 0xFFu);
}

}  // namespace

void launch_dense_tile(const uint32_t* ids, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t* tiled,
                       uint32_t* tile_bits, hipStream_t stream) {
    hipLaunchKernelGGL(dense_tile_kernel, dim3(tx * ty * tz), dim3(256), 0, stream, ids, nx, ny, nz, tx, ty, tz, tiled, tile_bits);
}

void launch_dense(const DenseArgs& args, hipStream_t stream) {
    const uint32_t blocks = ((args.trace.w + kWaveW - 1u) / kWaveW) * ((args.trace.h + kWaveH - 1u) / kWaveH);
    if (!blocks) return;
    const size_t lds = (args.bit_words <= kDenseLdsWords ? args.bit_words : 0u) * sizeof(uint32_t);
    hipLaunchKernelGGL(dense_kernel, dim3(blocks), dim3(64), lds, stream, args);
}

}  // namespace blok
