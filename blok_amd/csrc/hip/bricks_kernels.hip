// The resident volume as a sparse brick stream (gpu_build.h: gpu_volume_encode_bricks / gpu_volume_decode_bricks; include/blok_hip.h:
// blok_hip_volume_encode_bricks has the contract; the rules live in ../common/bricks_core.h, shared with the host build).
//
// Encode is the first volume kernel that reads the WHOLE dense store, so its shape is set by bytes:
//   1. classify: one lane per brick, 64 consecutive bricks along x per wave.  Each of the 16 (y, z) rows of such a brick row is one
//      16-byte load per lane — 1 KiB contiguous per wave instruction — when the volume's nx and the region's x origin are multiples of 4;
//      every other region takes dword loads in the same lane mapping.  The density plane goes first, then the ids, so sixteen vectors are
//      live, not thirty-two.  A plane comes to three words per lane — the mask of its cells that count, and the OR and the AND of their
//      values: all equal iff OR == AND — so mask and uniformity are plain per-lane integer work with no cross-lane traffic.  Per brick it
//      writes a 16-byte draft (mask, the two uniform values) and two count words for the scans.
//   2. two exclusive scans (hipcub), in place: (stored << 32 | density entries) and (stored cells << 32 | material entries); their last
//      entries are the four totals.
//   3. emit: one lane per brick again; a stored brick writes its record at its rank and, for a plane that is not uniform, re-reads its
//      cells for the payload.  Drafts keep emit from reading the arrays a second time for the bricks that need no payload.
// With FILLED_ONLY on a region whose corner lies on the brick grid a lane whose d_masks word is 0 loads nothing (the masks equal
// density > 0 after every edit).
// Decode: default mode clears the destination, then one lane per stored brick scatters its cells, then the refresh of every edit runs
// over the destination box.  Everything is on the null stream, behind earlier edits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/bricks_core.h"

namespace blok {

namespace {

namespace B = bricks;

struct ClassifyArgs {
    const uint32_t* density;        // the store's densities as bit patterns
    const uint32_t* ids;
    uint32_t nx, ny;
    uint32_t lo[3], ext[3], nb[3];  // the region, box-local, and its bricks
    uint32_t x_chunks;              // waves per brick row: ceil(nb[0] / 64)
    uint32_t n_waves;               // x_chunks * nb[1] * nb[2]
    uint32_t filled_only;
    uint32_t use_masks;             // FILLED_ONLY and the region's corner on the brick grid: a zero mask word skips the brick
    BrickMasks masks;
    uint4* drafts;                  // per brick: mask lo, mask hi, density value, material value (the values of uniform planes)
    uint64_t* count_a;              // per brick: stored << 32 | density payload entries
    uint64_t* count_b;              // per brick: stored cells << 32 | material payload entries
};

// The 16 rows of the lane's brick from one plane.  kVector: one 16-byte load per row (nx % 4 == 0 and lo[0] % 4 == 0: the address is
// 16-byte aligned and the row's four cells lie inside the box's x extent even where the region cuts the brick); else a dword per cell.
// No load is conditional: where the region cuts the brick, a row or a cell beyond the cut reads the last one inside it again (wx, wy, wz
// are at least 1), and the caller's `inside` mask drops what it holds.
template <bool kVector>
__device__ __forceinline__ void load_rows(const uint32_t* plane, size_t cell0, size_t stride_y, size_t stride_z, uint32_t wx, uint32_t wy, uint32_t wz,
                                          uint4 rows[16]) {
#pragma unroll
    for (uint32_t r = 0; r < 16u; ++r) {
        const uint32_t* p = plane + cell0 + min(r & 3u, wy - 1u) * stride_y + min(r >> 2, wz - 1u) * stride_z;
        if constexpr (kVector) rows[r] = *reinterpret_cast<const uint4*>(p);
        else rows[r] = make_uint4(p[0], p[min(1u, wx - 1u)], p[min(2u, wx - 1u)], p[min(3u, wx - 1u)]);
    }
}

template <bool kVector, bool kFilledOnly>
__global__ __launch_bounds__(256) void brick_classify_kernel(const ClassifyArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (wave >= a.n_waves) return;
    const uint32_t xc = wave % a.x_chunks, by = (wave / a.x_chunks) % a.nb[1], bz = wave / (a.x_chunks * a.nb[1]);
    const uint32_t bx = xc * 64u + lane;
    if (bx >= a.nb[0]) return;
    uint64_t by_density = 0ull, mask = 0ull;
    uint32_t or_d = 0u, and_d = 0xFFFFFFFFu, or_m = 0u, and_m = 0xFFFFFFFFu;
    // (with FILLED_ONLY on the brick grid a zero mask word says nothing is filled: nothing is loaded)
    if (!(kFilledOnly && a.use_masks) || a.masks.at(a.lo[0] / 4u + bx, a.lo[1] / 4u + by, a.lo[2] / 4u + bz) != 0ull) {
        // the part of the brick inside the region: wx * wy * wz cells, each at least 1 (wy and wz are wave-uniform)
        const uint32_t wx = min(4u, a.ext[0] - 4u * bx), wy = min(4u, a.ext[1] - 4u * by), wz = min(4u, a.ext[2] - 4u * bz);
        const uint64_t inside = B::region_mask(a.ext, bx, by, bz);
        const size_t stride_y = a.nx, stride_z = static_cast<size_t>(a.nx) * a.ny;
        const size_t cell0 = (a.lo[0] + 4u * bx) + (a.lo[1] + 4u * by) * stride_y + (a.lo[2] + 4u * bz) * stride_z;
        uint4 rows[16];
        // density: the cells the density alone makes stored, and the OR / AND of their patterns
        load_rows<kVector>(a.density, cell0, stride_y, stride_z, wx, wy, wz, rows);
#pragma unroll
        for (uint32_t r = 0; r < 16u; ++r) {
            const uint32_t c[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
#pragma unroll
            for (uint32_t x = 0; x < 4u; ++x) {
                const uint32_t bit = 4u * r + x;                      // = cell_bit(x, r & 3, r >> 2)
                const bool s = (((inside >> bit) & 1ull) != 0ull) & B::stored(c[x], 0u, kFilledOnly);
                by_density |= static_cast<uint64_t>(s) << bit;
                or_d |= s ? c[x] : 0u; and_d &= s ? c[x] : 0xFFFFFFFFu;
            }
        }
        // (left to itself the scheduler lifts the second plane's loads above the first plane's arithmetic: thirty-two vectors live)
        __builtin_amdgcn_sched_barrier(0);
        // ids: the stored cells are those plus, by default, the cells with a non-zero id
        load_rows<kVector>(a.ids, cell0, stride_y, stride_z, wx, wy, wz, rows);
#pragma unroll
        for (uint32_t r = 0; r < 16u; ++r) {
            const uint32_t c[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
#pragma unroll
            for (uint32_t x = 0; x < 4u; ++x) {
                const uint32_t bit = 4u * r + x;
                const bool s = (((by_density >> bit) & 1ull) != 0ull) | (!kFilledOnly & (((inside >> bit) & 1ull) != 0ull) & (c[x] != 0u));
                mask |= static_cast<uint64_t>(s) << bit;
                or_m |= s ? c[x] : 0u; and_m &= s ? c[x] : 0xFFFFFFFFu;
            }
        }
    }
    // a cell stored by its id alone has the density pattern 0: the densities are uniform iff no cell is stored by its density (all are
    // 0 then, and or_d is 0), or the cells stored by it agree and there is no other stored cell
    const bool uniform_d = by_density == 0ull || (or_d == and_d && mask == by_density);
    const bool uniform_m = or_m == and_m;
    const uint32_t cells = B::popcount64(mask);
    const size_t brick = bx + static_cast<size_t>(a.nb[0]) * (by + static_cast<size_t>(a.nb[1]) * bz);
    a.drafts[brick] = make_uint4(static_cast<uint32_t>(mask), static_cast<uint32_t>(mask >> 32), or_d, or_m);
    a.count_a[brick] = (static_cast<uint64_t>(mask != 0ull) << 32) | (uniform_d ? 0u : cells);
    a.count_b[brick] = (static_cast<uint64_t>(cells) << 32) | (uniform_m ? 0u : cells);
}

struct EmitArgs {
    const uint32_t* density; const uint32_t* ids;
    uint32_t nx, ny;
    uint32_t lo[3], nb[3];
    uint32_t n_bricks;              // of the region
    const uint4* drafts;
    const uint64_t* scan_a; const uint64_t* scan_b;      // the exclusive scans, n_bricks + 1 entries
    blok_brick_record* records;
    uint32_t* density_payload; uint32_t* material_payload;
};

__global__ __launch_bounds__(256) void brick_emit_kernel(const EmitArgs a) {
    const uint32_t brick = blockIdx.x * 256u + threadIdx.x;
    if (brick >= a.n_bricks) return;
    const uint64_t a0 = a.scan_a[brick], a1 = a.scan_a[brick + 1u];
    if ((a1 >> 32) == (a0 >> 32)) return;                         // not stored
    const uint64_t b0 = a.scan_b[brick], b1 = a.scan_b[brick + 1u];
    const uint4 draft = a.drafts[brick];
    const uint64_t mask = static_cast<uint64_t>(draft.x) | (static_cast<uint64_t>(draft.y) << 32);
    const uint32_t n_density = static_cast<uint32_t>(a1) - static_cast<uint32_t>(a0), n_material = static_cast<uint32_t>(b1) - static_cast<uint32_t>(b0);
    const uint32_t kind = (n_density == 0u ? B::kUniformDensity : 0u) | (n_material == 0u ? B::kUniformMaterial : 0u);
    const uint32_t density_base = static_cast<uint32_t>(a0), material_base = static_cast<uint32_t>(b0);
    a.records[a0 >> 32] = B::make_record(brick, mask, kind, draft.z, draft.w, density_base, material_base);
    if (kind == (B::kUniformDensity | B::kUniformMaterial)) return;
    const uint32_t bx = brick % a.nb[0], by = (brick / a.nb[0]) % a.nb[1], bz = brick / (a.nb[0] * a.nb[1]);
    const size_t stride_y = a.nx, stride_z = static_cast<size_t>(a.nx) * a.ny;
    const size_t cell0 = (a.lo[0] + 4u * bx) + (a.lo[1] + 4u * by) * stride_y + (a.lo[2] + 4u * bz) * stride_z;
    uint32_t rank = 0u;
    for (uint64_t m = mask; m; m &= m - 1ull, ++rank) {           // the payload, in ascending bit order
        const uint32_t bit = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(m))) - 1u;
        const size_t cell = cell0 + (bit & 3u) + ((bit >> 2) & 3u) * stride_y + (bit >> 4) * stride_z;
        if (!(kind & B::kUniformDensity)) a.density_payload[density_base + rank] = a.density[cell];
        if (!(kind & B::kUniformMaterial)) a.material_payload[material_base + rank] = a.ids[cell];
    }
}

struct DecodeArgs {
    uint32_t* density; uint32_t* ids;
    uint32_t nx, ny;
    uint32_t lo[3], ext[3], nb[3];  // the destination, box-local, and its bricks
    const blok_brick_record* records; uint32_t n_records;
    const uint32_t* density_payload; const uint32_t* material_payload;
};

// Default mode: every cell of the destination gets (+0.0f, 0) before the stored ones are written.
__global__ __launch_bounds__(256) void brick_clear_kernel(const DecodeArgs a, uint32_t n_cells) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cells) return;
    const uint32_t x = i % a.ext[0], y = (i / a.ext[0]) % a.ext[1], z = i / (a.ext[0] * a.ext[1]);
    const size_t cell = (a.lo[0] + x) + (a.lo[1] + y) * static_cast<size_t>(a.nx) + (a.lo[2] + z) * (static_cast<size_t>(a.nx) * a.ny);
    a.density[cell] = 0u; a.ids[cell] = 0u;
}

// One lane per stored brick.  Bricks are distinct and their cells disjoint: no cell is written twice.
__global__ __launch_bounds__(256) void brick_scatter_kernel(const DecodeArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_records) return;
    const blok_brick_record r = a.records[i];
    const uint32_t bx = r.brick % a.nb[0], by = (r.brick / a.nb[0]) % a.nb[1], bz = r.brick / (a.nb[0] * a.nb[1]);
    const size_t stride_y = a.nx, stride_z = static_cast<size_t>(a.nx) * a.ny;
    const size_t cell0 = (a.lo[0] + 4u * bx) + (a.lo[1] + 4u * by) * stride_y + (a.lo[2] + 4u * bz) * stride_z;
    uint32_t rank = 0u;
    for (uint64_t m = r.mask; m; m &= m - 1ull, ++rank) {
        const uint32_t bit = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(m))) - 1u;
        const size_t cell = cell0 + (bit & 3u) + ((bit >> 2) & 3u) * stride_y + (bit >> 4) * stride_z;
        a.density[cell] = (r.kind & B::kUniformDensity) ? r.density : a.density_payload[r.density + rank];
        a.ids[cell] = (r.kind & B::kUniformMaterial) ? r.material : a.material_payload[r.material + rank];
    }
}

GpuBuildStatus exclusive_sum(DeviceMem& mem, uint64_t* d_words, uint64_t n, std::string* why) {
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, d_words, d_words, static_cast<int>(n)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_words, d_words, static_cast<int>(n)));
    return GpuBuildStatus::Ok;
}

}  // namespace

void gpu_bricks_free(GpuBricks* b) {
    if (b->d_records) (void)hipFree(b->d_records);
    if (b->d_density) (void)hipFree(b->d_density);
    if (b->d_material) (void)hipFree(b->d_material);
    *b = GpuBricks{};
}

GpuBuildStatus gpu_volume_encode_bricks(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t flags, GpuBricks* out, std::string* why) {
    *out = GpuBricks{};
    if (!cells_fit_32_bits(v, "encode_bricks", why)) return GpuBuildStatus::Unsupported;
    blok_bricks_info& info = out->info;
    info.version = 1u; info.flags = flags;
    ClassifyArgs c{};
    for (int k = 0; k < 3; ++k) {
        c.lo[k] = lo[k]; c.ext[k] = hi[k] > lo[k] ? hi[k] - lo[k] : 0u;
        info.lo[k] = v->origin[k] + static_cast<int32_t>(lo[k]); info.ext[k] = c.ext[k];
    }
    if (!c.ext[0] || !c.ext[1] || !c.ext[2]) return GpuBuildStatus::Ok;
    B::brick_counts(c.ext, c.nb);
    const uint64_t n = static_cast<uint64_t>(c.nb[0]) * c.nb[1] * c.nb[2];
    if (n >= 0x7FFFFFFFull) { *why = "encode_bricks: region of more than 2^31 bricks"; return GpuBuildStatus::Unsupported; }      // (the scans count in int; gpu_volume_create admits no such box)
    c.density = reinterpret_cast<const uint32_t*>(v->d_density); c.ids = v->d_ids; c.nx = v->nx; c.ny = v->ny;
    c.x_chunks = (c.nb[0] + 63u) / 64u;
    c.n_waves = c.x_chunks * c.nb[1] * c.nb[2];
    c.filled_only = (flags & BLOK_BRICKS_FILLED_ONLY) ? 1u : 0u;
    c.use_masks = c.filled_only && lo[0] % 4u == 0u && lo[1] % 4u == 0u && lo[2] % 4u == 0u;
    c.masks = brick_masks_of(*v);
    DeviceMem mem;
    BLOK_GPU_TRY(mem.alloc(&c.drafts, n));
    BLOK_GPU_TRY(mem.alloc(&c.count_a, n + 1u));
    BLOK_GPU_TRY(mem.alloc(&c.count_b, n + 1u));
    BLOK_GPU_TRY(hipMemsetAsync(c.count_a + n, 0, sizeof(uint64_t), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(c.count_b + n, 0, sizeof(uint64_t), nullptr));
    // (edits are enqueued on the null stream, and so is this: it reads what they leave)
    const dim3 grid((c.n_waves + 3u) / 4u);
    const bool vector = v->nx % 4u == 0u && lo[0] % 4u == 0u;
    if (vector && c.filled_only) hipLaunchKernelGGL((brick_classify_kernel<true, true>), grid, dim3(256), 0, nullptr, c);
    else if (vector) hipLaunchKernelGGL((brick_classify_kernel<true, false>), grid, dim3(256), 0, nullptr, c);
    else if (c.filled_only) hipLaunchKernelGGL((brick_classify_kernel<false, true>), grid, dim3(256), 0, nullptr, c);
    else hipLaunchKernelGGL((brick_classify_kernel<false, false>), grid, dim3(256), 0, nullptr, c);
    BLOK_GPU_TRY(hipGetLastError());
    GpuBuildStatus st = exclusive_sum(mem, c.count_a, n + 1u, why);
    if (st != GpuBuildStatus::Ok) return st;
    st = exclusive_sum(mem, c.count_b, n + 1u, why);
    if (st != GpuBuildStatus::Ok) return st;
    uint64_t total_a = 0, total_b = 0;
    BLOK_GPU_TRY(hipMemcpy(&total_a, c.count_a + n, sizeof(total_a), hipMemcpyDeviceToHost));
    BLOK_GPU_TRY(hipMemcpy(&total_b, c.count_b + n, sizeof(total_b), hipMemcpyDeviceToHost));
    info.n_bricks = total_a >> 32; info.n_density = total_a & 0xFFFFFFFFull;
    info.n_voxels = total_b >> 32; info.n_material = total_b & 0xFFFFFFFFull;
    if (!info.n_bricks) return GpuBuildStatus::Ok;
    EmitArgs e{};
    e.density = c.density; e.ids = c.ids; e.nx = c.nx; e.ny = c.ny;
    for (int k = 0; k < 3; ++k) { e.lo[k] = c.lo[k]; e.nb[k] = c.nb[k]; }
    e.n_bricks = static_cast<uint32_t>(n);
    e.drafts = c.drafts; e.scan_a = c.count_a; e.scan_b = c.count_b;
    BLOK_GPU_TRY(mem.alloc(&e.records, info.n_bricks));
    if (info.n_density) BLOK_GPU_TRY(mem.alloc(&e.density_payload, info.n_density));
    if (info.n_material) BLOK_GPU_TRY(mem.alloc(&e.material_payload, info.n_material));
    hipLaunchKernelGGL(brick_emit_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, e);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(hipDeviceSynchronize());
    mem.release(e.records); mem.release(e.density_payload); mem.release(e.material_payload);
    out->d_records = e.records; out->d_density = e.density_payload; out->d_material = e.material_payload;
    return GpuBuildStatus::Ok;
}

GpuBuildStatus gpu_volume_decode_bricks(GpuVolume* v, const GpuBricks* stream, const uint32_t dst_lo[3], uint32_t flags, std::string* why) {
    if (!cells_fit_32_bits(v, "decode_bricks", why)) return GpuBuildStatus::Unsupported;
    const blok_bricks_info& info = stream->info;
    if (!info.ext[0] || !info.ext[1] || !info.ext[2]) return GpuBuildStatus::Ok;
    DecodeArgs a{};
    a.density = reinterpret_cast<uint32_t*>(v->d_density); a.ids = v->d_ids; a.nx = v->nx; a.ny = v->ny;
    uint32_t hi[3];
    for (int k = 0; k < 3; ++k) { a.lo[k] = dst_lo[k]; a.ext[k] = info.ext[k]; hi[k] = dst_lo[k] + info.ext[k]; }
    B::brick_counts(a.ext, a.nb);
    a.records = stream->d_records; a.n_records = static_cast<uint32_t>(info.n_bricks);
    a.density_payload = stream->d_density; a.material_payload = stream->d_material;
    const uint64_t n_cells = static_cast<uint64_t>(a.ext[0]) * a.ext[1] * a.ext[2];      // inside the box: below 2^32
    if (!(flags & BLOK_BRICKS_KEEP_OTHERS)) {
        hipLaunchKernelGGL(brick_clear_kernel, dim3(blocks_for(n_cells)), dim3(256), 0, nullptr, a, static_cast<uint32_t>(n_cells));
        BLOK_GPU_TRY(hipGetLastError());
    } else if (!a.n_records) return GpuBuildStatus::Ok;           // a paste of nothing writes nothing
    if (a.n_records) {
        hipLaunchKernelGGL(brick_scatter_kernel, dim3(blocks_for(a.n_records)), dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
    }
    const GpuBuildStatus st = gpu_volume_commit(v, a.lo, hi, Edit::MayFill, why);      // (a written density may be positive)
    BLOK_GPU_TRY(hipDeviceSynchronize());                         // blocking, as gpu_volume_set_voxels is
    return st;
}

}  // namespace blok
