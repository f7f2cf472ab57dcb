// The scroll of the resident volume (gpu_build.h: gpu_volume_scroll; include/blok_hip.h: blok_hip_volume_scroll has the contract; the rules
// live in ../common/scroll_core.h, shared with the host build).
//
// The dense arrays: out of place into a second pair, which the volume then adopts.  A wave owns 64 consecutive lanes of a destination row
//   (row_segment), so y and z are wave-uniform and a row whose source row lies outside the old box is stores of zeros with no loads.
//   delta[0] is a multiple of 4: where nx is one too, a lane moves four cells with one 16-byte load and one 16-byte store per array (1 KiB
//   per wave instruction, source and destination both 16-byte aligned); a ragged nx takes the same kernel with one cell per lane.  All
//   indices are 64-bit.  Each array is read once and written once: the masks are not derived from the densities again.
// The masks: moved, not recomputed.  A lane per destination brick reads its source brick's word through BrickMasks::at in either layout,
//   cuts it by the box's ragged end (scroll::cut_mask) and writes it into a second mask array — a permutation in place would race — which
//   the volume adopts as well; in the row-major layout the lane writes the brick's non-empty flag beside it.  What lies above the masks
//   is gpu_volume_masks_replaced's (gpu_build.hip).
// The counts: the same lane adds the popcounts of its brick's old word and of its new word; two shuffle reductions per wave, a row per
//   workgroup through LDS, folded by a second small launch (as columns_kernels.hip does; no atomic per wave).
// Everything is on the null stream, behind earlier edits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/scroll_core.h"

namespace blok {

namespace {

namespace K = scroll;

struct MoveArgs {
    const uint32_t* src_density; const uint32_t* src_ids;      // bit patterns: a density is moved, never computed with
    uint32_t* dst_density; uint32_t* dst_ids;
    uint32_t nx, ny, nz;
    uint32_t row_items;                               // a lane's items per row: nx / 4 (16-byte path) or nx
    uint32_t x_chunks;                                // segments of 64 items per row
    int32_t delta[3];
    uint64_t n_waves;                                 // x_chunks * ny * nz
};

template <bool kWide>
__global__ __launch_bounds__(256) void scroll_move_kernel(const MoveArgs a) {
    using Item = std::conditional_t<kWide, uint4, uint32_t>;
    constexpr uint32_t kCells = kWide ? 4u : 1u;
    const uint64_t wave = uniform64(blockIdx.x * 4ull + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    uint32_t xc, y, z;
    row_segment(wave, a.x_chunks, a.ny, xc, y, z);
    const uint32_t item = xc * 64u + (threadIdx.x & 63u);
    if (item >= a.row_items) return;
    const uint32_t x = item * kCells;
    Item density{}, id{};                             // (+0.0f, 0)
    uint32_t sx, sy, sz;
    if (K::source(y, a.delta[1], a.ny, &sy) && K::source(z, a.delta[2], a.nz, &sz)) {      // wave-uniform: an exposed row loads nothing
        // (16-byte path: delta[0] and nx are multiples of 4, so the four cells of an item have a source together or not at all)
        if (K::source(x, a.delta[0], a.nx, &sx)) {
            const uint64_t src = (static_cast<uint64_t>(sz) * a.ny + sy) * a.nx + sx;
            density = *reinterpret_cast<const Item*>(a.src_density + src);
            id = *reinterpret_cast<const Item*>(a.src_ids + src);
        }
    }
    const uint64_t dst = (static_cast<uint64_t>(z) * a.ny + y) * a.nx + x;
    *reinterpret_cast<Item*>(a.dst_density + dst) = density;
    *reinterpret_cast<Item*>(a.dst_ids + dst) = id;
}

struct MaskArgs {
    BrickMasks old_masks;
    uint64_t* new_masks;                              // null: count only (BLOK_SCROLL_PLAN_ONLY, a zero delta)
    uint32_t* new_flag;                               // row-major layout: mask != 0; null in the keyed layout
    uint32_t nx, ny, nz, nbz;
    int32_t delta_bricks[3];
    uint64_t n_bricks;
    uint32_t* rows;                                   // per workgroup: [0] filled voxels of the old words, [1] of the new words
};

__global__ __launch_bounds__(256) void scroll_mask_kernel(const MaskArgs a) {
    const uint64_t brick = blockIdx.x * 256ull + threadIdx.x;
    uint32_t before = 0u, kept = 0u;
    if (brick < a.n_bricks) {
        const BrickMasks& M = a.old_masks;
        const uint32_t bx = static_cast<uint32_t>(brick % M.nbx), by = static_cast<uint32_t>((brick / M.nbx) % M.nby),
                       bz = static_cast<uint32_t>(brick / (static_cast<uint64_t>(M.nbx) * M.nby));
        before = static_cast<uint32_t>(__popcll(M.at(bx, by, bz)));
        uint64_t mask = 0ull;
        uint32_t sx, sy, sz;
        if (K::source(bx, a.delta_bricks[0], M.nbx, &sx) && K::source(by, a.delta_bricks[1], M.nby, &sy) && K::source(bz, a.delta_bricks[2], a.nbz, &sz))
            mask = K::cut_mask(M.at(sx, sy, sz), bx, by, bz, a.nx, a.ny, a.nz);
        kept = static_cast<uint32_t>(__popcll(mask));
        if (a.new_masks) {
            const uint64_t at = M.key_digits == 0u ? brick : cell_key(bx, by, bz, M.key_digits);
            a.new_masks[at] = mask;
            if (a.new_flag) a.new_flag[at] = mask != 0ull;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        before += static_cast<uint32_t>(__shfl_xor(static_cast<int>(before), d));
        kept += static_cast<uint32_t>(__shfl_xor(static_cast<int>(kept), d));
    }
    __shared__ uint32_t s_values[4][2];
    if ((threadIdx.x & 63u) == 0u) { s_values[threadIdx.x >> 6][0] = before; s_values[threadIdx.x >> 6][1] = kept; }
    __syncthreads();
    if (threadIdx.x < 2u)
        a.rows[static_cast<size_t>(blockIdx.x) * 2u + threadIdx.x] = s_values[0][threadIdx.x] + s_values[1][threadIdx.x] + s_values[2][threadIdx.x] + s_values[3][threadIdx.x];
}

// out[c] (zero before the launch) takes the sum of column c of all rows: at most gridDim.x atomics per column.
__global__ __launch_bounds__(256) void scroll_fold_kernel(const uint32_t* rows, uint32_t n_rows, unsigned long long* out) {
    __shared__ unsigned long long s_acc[256];
    const uint32_t c = threadIdx.x & 1u;
    unsigned long long acc = 0ull;
    for (uint64_t row = blockIdx.x * 128ull + (threadIdx.x >> 1); row < n_rows; row += gridDim.x * 128ull) acc += rows[row * 2u + c];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 2u) {
        for (uint32_t k = 1; k < 128u; ++k) acc += s_acc[threadIdx.x + 2u * k];
        atomicAdd(out + c, acc);
    }
}

}  // namespace

GpuBuildStatus gpu_volume_scroll(GpuVolume* v, const int32_t delta[3], bool write, uint64_t* out_n_filled_before, uint64_t* out_n_filled_kept,
                                 std::string* why) {
    DeviceMem mem;
    const uint64_t n_bricks = v->bricks(), n_mask_words = v->keyed ? v->n_keys : n_bricks;
    const uint32_t mask_blocks = blocks_for(n_bricks);
    // every allocation before the first write: a failed one leaves the volume as it was
    uint32_t *d_density = nullptr, *d_ids = nullptr, *d_flag = nullptr, *d_rows = nullptr;
    uint64_t* d_masks = nullptr;
    unsigned long long* d_totals = nullptr;
    BLOK_GPU_TRY(mem.alloc(&d_rows, static_cast<uint64_t>(mask_blocks) * 2u));
    BLOK_GPU_TRY(mem.alloc(&d_totals, 2u));
    MoveArgs m{};
    const bool wide = v->nx % 4u == 0u;
    if (write) {
        m.nx = v->nx; m.ny = v->ny; m.nz = v->nz;
        m.row_items = wide ? v->nx / 4u : v->nx;
        m.x_chunks = (m.row_items + 63u) / 64u;
        m.n_waves = static_cast<uint64_t>(m.x_chunks) * v->ny * v->nz;
        if ((m.n_waves + 3u) / 4u > 0x7FFFFFFFull) { *why = "scroll: more than 2^31 workgroups of rows"; return GpuBuildStatus::Unsupported; }
        BLOK_GPU_TRY(mem.alloc(&d_density, v->cells()));
        BLOK_GPU_TRY(mem.alloc(&d_ids, v->cells()));
        BLOK_GPU_TRY(mem.alloc(&d_masks, n_mask_words));
        if (v->keyed) BLOK_GPU_TRY(hipMemsetAsync(d_masks, 0, n_mask_words * sizeof(uint64_t), nullptr));      // (the keys outside the box stay empty)
        else {
            BLOK_GPU_TRY(mem.alloc(&d_flag, n_bricks + 1u));
            BLOK_GPU_TRY(hipMemsetAsync(d_flag + n_bricks, 0, sizeof(uint32_t), nullptr));                      // (the scan's sentinel)
        }
        m.src_density = reinterpret_cast<const uint32_t*>(v->d_density); m.src_ids = v->d_ids;
        m.dst_density = d_density; m.dst_ids = d_ids;
        for (int a = 0; a < 3; ++a) m.delta[a] = delta[a];
        const uint32_t move_blocks = static_cast<uint32_t>((m.n_waves + 3u) / 4u);
        if (wide) hipLaunchKernelGGL(scroll_move_kernel<true>, dim3(move_blocks), dim3(256), 0, nullptr, m);
        else hipLaunchKernelGGL(scroll_move_kernel<false>, dim3(move_blocks), dim3(256), 0, nullptr, m);
        BLOK_GPU_TRY(hipGetLastError());
    }
    MaskArgs k{};
    k.old_masks = brick_masks_of(*v); k.new_masks = d_masks; k.new_flag = d_flag;
    k.nx = v->nx; k.ny = v->ny; k.nz = v->nz; k.nbz = v->nbz;
    for (int a = 0; a < 3; ++a) k.delta_bricks[a] = delta[a] / 4;
    k.n_bricks = n_bricks; k.rows = d_rows;
    BLOK_GPU_TRY(hipMemsetAsync(d_totals, 0, 2u * sizeof(unsigned long long), nullptr));
    hipLaunchKernelGGL(scroll_mask_kernel, dim3(mask_blocks), dim3(256), 0, nullptr, k);
    BLOK_GPU_TRY(hipGetLastError());
    hipLaunchKernelGGL(scroll_fold_kernel, dim3(std::min<uint32_t>((mask_blocks + 127u) / 128u, 64u)), dim3(256), 0, nullptr, d_rows, mask_blocks, d_totals);
    BLOK_GPU_TRY(hipGetLastError());
    unsigned long long totals[2] = {0ull, 0ull};
    BLOK_GPU_TRY(hipMemcpy(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost));      // the call's wait
    if (out_n_filled_before) *out_n_filled_before = totals[0];
    if (out_n_filled_kept) *out_n_filled_kept = totals[1];
    if (!write) return GpuBuildStatus::Ok;
    // the volume adopts the new arrays; the old ones go with `mem` once the device has finished (frames of other streams read trees, never
    // these arrays, but the wait costs nothing behind the one above)
    BLOK_GPU_TRY(hipDeviceSynchronize());
    for (void* p : {static_cast<void*>(d_density), static_cast<void*>(d_ids), static_cast<void*>(d_masks), static_cast<void*>(d_flag)}) mem.release(p);
    mem.ptrs.insert(mem.ptrs.end(), {static_cast<void*>(v->d_density), static_cast<void*>(v->d_ids), static_cast<void*>(v->d_masks)});
    v->d_density = reinterpret_cast<float*>(d_density); v->d_ids = d_ids; v->d_masks = d_masks;
    if (!v->keyed) { mem.ptrs.push_back(v->d_flag); v->d_flag = d_flag; }
    return gpu_volume_masks_replaced(v, why);
}

}  // namespace blok
