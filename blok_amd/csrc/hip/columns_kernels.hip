// The column field of the resident volume and scatter onto it (gpu_build.h: gpu_volume_column_field / gpu_columns_scatter;
// include/blok_hip.h: blok_hip_volume_column_field and blok_hip_volume_scatter_models have the contracts; the rules live in
// ../common/columns_core.h, shared with the host build).
//
// The field: a lane per column, 64 consecutive column indices to a wave, so the tops leave as 128 contiguous bytes per wave instruction.
//   A lane walks its column from the entry face through columns::column_top, sixteen cells at a time: the aligned group of four bricks
//   along the axis, whose mask words — in either layout (BrickMasks::part), never the densities — are four independent loads off one
//   base, in flight together; the four lanes that share a brick load the same word, and along y in the keyed layout a wave's four loads
//   fill four whole 128-byte lines.  The lane's sixteen cells become one 16-bit string, cut by the region, and one count-leading /
//   trailing-zero step finds the hit.  A lane stops at its first hit and then loads the one material id of its top cell.  Counts: a ballot and two shuffle reductions per wave, a row per workgroup, folded by a second small launch.
// Scatter: a lane per column of the snapshot, in index order, so that the table comes out sorted with no sort.  A column that is not its
//   cell's candidate drops out after one hash; the footprint's up to 17 x 17 tops sit behind the four cheaper tests.  Pass 1 judges, counts
//   per verdict (ballots, a row per workgroup, folded by a second small launch) and keeps each wave's ballot of placed lanes and its popcount; one exclusive
//   scan (hipcub) of the popcounts; pass 2 writes each placed lane's 32-byte record at its wave's base + its rank in the ballot.
// Everything is on the null stream, behind earlier edits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/columns_core.h"

namespace blok {

namespace {

namespace K = columns;

// ---- counts without contended atomics ----------------------------------------------------------------------------------------------------
// A wave's counts go through LDS into one row of kCols words per workgroup; a second small launch folds the rows, column by column (sum, min
// or max: two bits per column in `ops`), and ends in at most 64 atomics per column.  (One atomic per wave on one address costs some 10 ns
// each: 49 k of them were half of the first version's millisecond per field of a 1024^3 box.)
constexpr uint32_t kCols = 8u;
constexpr uint32_t kSum = 0u, kMin = 1u, kMax = 2u;
__device__ __forceinline__ unsigned long long fold(uint32_t op, unsigned long long a, unsigned long long b) { return op == kSum ? a + b : op == kMin ? (a < b ? a : b) : (a > b ? a : b); }
__device__ __forceinline__ unsigned long long fold_identity(uint32_t op) { return op == kMin ? ~0ull : 0ull; }

// Called by every thread of a workgroup of 256: lane 0 of each wave holds the wave's values.
__device__ __forceinline__ void store_block_row(const uint32_t (&wave_values)[kCols], uint32_t ops, uint32_t* rows) {
    __shared__ uint32_t s_values[4][kCols];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (uint32_t c = 0; c < kCols; ++c) s_values[threadIdx.x >> 6][c] = wave_values[c];
    __syncthreads();
    if (threadIdx.x < kCols) {
        const uint32_t op = (ops >> (2u * threadIdx.x)) & 3u;
        unsigned long long r = s_values[0][threadIdx.x];
        for (uint32_t w = 1; w < 4u; ++w) r = fold(op, r, s_values[w][threadIdx.x]);
        rows[static_cast<size_t>(blockIdx.x) * kCols + threadIdx.x] = static_cast<uint32_t>(r);
    }
}

// out[c] (holding the identity of its fold before the launch) takes column c of all rows.
__global__ __launch_bounds__(256) void fold_rows_kernel(const uint32_t* rows, uint32_t n_rows, uint32_t ops, unsigned long long* out) {
    __shared__ unsigned long long s_acc[256];
    const uint32_t c = threadIdx.x & (kCols - 1u), op = (ops >> (2u * c)) & 3u;
    unsigned long long acc = fold_identity(op);
    for (uint64_t row = blockIdx.x * 32ull + (threadIdx.x >> 3); row < n_rows; row += gridDim.x * 32ull) acc = fold(op, acc, rows[row * kCols + c]);
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < kCols) {
        for (uint32_t k = 1; k < 32u; ++k) acc = fold(op, acc, s_acc[threadIdx.x + kCols * k]);
        if (op == kSum) atomicAdd(out + c, acc); else if (op == kMin) atomicMin(out + c, acc); else atomicMax(out + c, acc);
    }
}

struct FieldArgs {
    BrickMasks masks;
    const uint32_t* ids;
    uint32_t nx, ny;
    uint32_t axis, low;
    uint32_t p_lo, q_lo, a_lo, a_hi;                  // box-local: the region's corner on the two other axes, its cells along the axis
    uint32_t ext_p;
    uint64_t n_columns;
    uint16_t* top;
    uint32_t* material;
    uint32_t* rows;                                   // per workgroup: [0] columns that hit, [1] least top, [2] greatest top
};

constexpr uint32_t kFieldOps = kSum | (kMin << 2) | (kMax << 4);

__global__ __launch_bounds__(256) void column_field_kernel(const FieldArgs a) {
    const uint64_t column = blockIdx.x * 256ull + threadIdx.x;
    const bool live = column < a.n_columns;
    uint32_t top = K::kNone;
    if (live) {
        const uint32_t gp = a.p_lo + static_cast<uint32_t>(column % a.ext_p), gq = a.q_lo + static_cast<uint32_t>(column / a.ext_p);
        const uint32_t p = K::axis_p(a.axis), q = K::axis_q(a.axis);
        const uint32_t b_first = a.a_lo >> 2, b_last = (a.a_hi - 1u) >> 2;
        // a brick's index is the sum of its three coordinates' parts: the column's two once, the walk's one per group of four bricks
        const uint64_t fixed = a.masks.part(gp >> 2, p) + a.masks.part(gq >> 2, q), step = a.masks.part(1u, a.axis);
        const auto bits_at = [&](uint32_t g) {
            const uint64_t* group = a.masks.masks + fixed + a.masks.part(4u * g, a.axis);
            uint64_t m[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) m[k] = (4u * g + k >= b_first && 4u * g + k <= b_last) ? group[k * step] : 0ull;      // four loads in flight
            return K::group_bits(K::mask_column(m[0], a.axis, gp & 3u, gq & 3u), K::mask_column(m[1], a.axis, gp & 3u, gq & 3u),
                                 K::mask_column(m[2], a.axis, gp & 3u, gq & 3u), K::mask_column(m[3], a.axis, gp & 3u, gq & 3u));
        };
        top = K::column_top(bits_at, a.a_lo, a.a_hi, a.low != 0u);
        uint32_t id = 0u;
        if (top != K::kNone) {
            const uint32_t along = a.a_lo + top;
            const uint32_t x = a.axis == 0u ? along : gp, y = a.axis == 1u ? along : a.axis == 0u ? gp : gq, z = a.axis == 2u ? along : gq;
            id = a.ids[x + (static_cast<size_t>(z) * a.ny + y) * a.nx];
        }
        a.top[column] = static_cast<uint16_t>(top);
        a.material[column] = id;
    }
    const bool hit = top != K::kNone;
    const uint32_t n_hit = static_cast<uint32_t>(__popcll(__ballot(hit)));
    uint32_t least = hit ? top : 0xFFFFFFFFu, most = hit ? top : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        least = min(least, static_cast<uint32_t>(__shfl_xor(static_cast<int>(least), d)));
        most = max(most, static_cast<uint32_t>(__shfl_xor(static_cast<int>(most), d)));
    }
    const uint32_t values[kCols] = {n_hit, least, most, 0u, 0u, 0u, 0u, 0u};
    store_block_row(values, kFieldOps, a.rows);
}

struct ScatterArgs {
    K::Field field;
    blok_scatter_params params;
    const blok_scatter_entry* entries;
    uint32_t n_entries, weight_sum;
    uint64_t n_columns, n_waves;
    uint64_t* ballots;                                // per wave: its placed lanes
    uint32_t* counts;                                 // per wave: how many; scanned in place into the wave's base
    uint32_t* rows;                                   // per workgroup: the columns of every verdict
    blok_instance* table;
};

__global__ __launch_bounds__(256) void scatter_judge_kernel(const ScatterArgs a) {
    const uint64_t column = blockIdx.x * 256ull + threadIdx.x;
    int verdict = K::kNotCandidate;
    if (column < a.n_columns) verdict = K::judge(a.field, a.params, static_cast<uint32_t>(column % a.field.ext[0]), static_cast<uint32_t>(column / a.field.ext[0]));
    const bool first = (threadIdx.x & 63u) == 0u;
    const uint64_t placed = __ballot(verdict == K::kPlaced);
    uint32_t values[kCols] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int v = K::kPlaced; v < K::kVerdicts; ++v) values[v] = static_cast<uint32_t>(__popcll(__ballot(verdict == v)));
    store_block_row(values, 0u, a.rows);
    const uint64_t wave = column >> 6;
    if (first && wave < a.n_waves) { a.ballots[wave] = placed; a.counts[wave] = static_cast<uint32_t>(__popcll(placed)); }
}

__global__ __launch_bounds__(256) void scatter_emit_kernel(const ScatterArgs a) {
    const uint64_t column = blockIdx.x * 256ull + threadIdx.x;
    const uint64_t wave = column >> 6;
    if (wave >= a.n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t placed = a.ballots[wave];
    if (!((placed >> lane) & 1ull)) return;
    const uint32_t rank = static_cast<uint32_t>(__popcll(placed & ((1ull << lane) - 1ull)));
    a.table[static_cast<uint64_t>(a.counts[wave]) + rank] =
        K::place(a.field, a.params, a.entries, a.n_entries, a.weight_sum, static_cast<uint32_t>(column % a.field.ext[0]), static_cast<uint32_t>(column / a.field.ext[0]));
}

static_assert(K::kVerdicts <= static_cast<int>(kCols), "a column per verdict");

// The folds of the n_rows rows the launch before left in d_rows, into totals[kCols] (host memory): the call's wait.
GpuBuildStatus fold_rows(DeviceMem& mem, const uint32_t* d_rows, uint32_t n_rows, uint32_t ops, unsigned long long totals[kCols], std::string* why) {
    unsigned long long* d_totals;
    BLOK_GPU_TRY(mem.alloc(&d_totals, static_cast<uint64_t>(kCols)));
    for (uint32_t c = 0; c < kCols; ++c) totals[c] = ((ops >> (2u * c)) & 3u) == kMin ? ~0ull : 0ull;
    BLOK_GPU_TRY(hipMemcpy(d_totals, totals, kCols * sizeof(unsigned long long), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(fold_rows_kernel, dim3(std::min<uint32_t>((n_rows + 31u) / 32u, 64u)), dim3(256), 0, nullptr, d_rows, n_rows, ops, d_totals);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(hipMemcpy(totals, d_totals, kCols * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return GpuBuildStatus::Ok;
}

}  // namespace

void gpu_columns_free(GpuColumns* c) {
    if (c->d_top) (void)hipFree(c->d_top);
    if (c->d_material) (void)hipFree(c->d_material);
    *c = GpuColumns{};
}

void gpu_scatter_free(GpuScatter* s) {
    if (s->d_table) (void)hipFree(s->d_table);
    *s = GpuScatter{};
}

GpuBuildStatus gpu_volume_column_field(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t axis, uint32_t flags, GpuColumns* out,
                                       std::string* why) {
    uint32_t ext[3];
    GpuBuildStatus begun;
    const bool has_cells = gpu_field_begin(v, "column_field", lo, hi, flags, out, ext, &begun, why);
    blok_columns_info& info = out->info;
    info.axis = axis; info.min_top = K::kNone; info.max_top = 0u;
    if (!has_cells) return begun;
    const uint32_t p = K::axis_p(axis), q = K::axis_q(axis);
    info.n_columns = static_cast<uint64_t>(ext[p]) * ext[q];      // at most 2^28 (gpu_volume_create admits 4^7 cells per axis): 2^20 blocks
    DeviceMem mem;
    uint16_t* d_top;
    uint32_t* d_material;
    uint32_t* d_rows;
    const uint32_t n_blocks = blocks_for(info.n_columns);
    BLOK_GPU_TRY(mem.alloc(&d_top, info.n_columns));
    BLOK_GPU_TRY(mem.alloc(&d_material, info.n_columns));
    BLOK_GPU_TRY(mem.alloc(&d_rows, static_cast<uint64_t>(n_blocks) * kCols));
    FieldArgs a{};
    a.masks = brick_masks_of(*v); a.ids = v->d_ids; a.nx = v->nx; a.ny = v->ny;
    a.axis = axis; a.low = K::from_low(flags) ? 1u : 0u;
    a.p_lo = lo[p]; a.q_lo = lo[q]; a.a_lo = lo[axis]; a.a_hi = hi[axis];
    a.ext_p = ext[p]; a.n_columns = info.n_columns;
    a.top = d_top; a.material = d_material; a.rows = d_rows;
    // (edits are enqueued on the null stream, and so is this: it reads the masks and the ids they leave)
    hipLaunchKernelGGL(column_field_kernel, dim3(n_blocks), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    unsigned long long counts[kCols];
    const GpuBuildStatus folded = fold_rows(mem, d_rows, n_blocks, kFieldOps, counts, why);
    if (folded != GpuBuildStatus::Ok) return folded;
    info.n_hit = counts[0];
    if (counts[0]) { info.min_top = static_cast<uint32_t>(counts[1]); info.max_top = static_cast<uint32_t>(counts[2]); }
    mem.release(d_top); mem.release(d_material);
    out->d_top = d_top; out->d_material = d_material;
    return GpuBuildStatus::Ok;
}

GpuBuildStatus gpu_columns_scatter(const GpuColumns* columns, const blok_scatter_params& params, const blok_scatter_entry* entries, uint32_t n_entries,
                                   GpuScatter* out, std::string* why) {
    *out = GpuScatter{};
    out->info.version = 1u; out->info.flags = params.flags;
    const blok_columns_info& ci = columns->info;
    if (!ci.n_columns) return GpuBuildStatus::Ok;
    ScatterArgs a{};
    a.field = K::field_of(columns->d_top, columns->d_material, ci);
    a.params = params;
    a.n_entries = n_entries; a.weight_sum = K::weight_sum(entries, n_entries);
    a.n_columns = ci.n_columns; a.n_waves = (ci.n_columns + 63u) / 64u;
    DeviceMem mem;
    blok_scatter_entry* d_entries;
    const uint32_t n_blocks = blocks_for(a.n_columns);
    BLOK_GPU_TRY(mem.alloc(&d_entries, n_entries));
    BLOK_GPU_TRY(mem.alloc(&a.ballots, a.n_waves));
    BLOK_GPU_TRY(mem.alloc(&a.counts, a.n_waves));
    BLOK_GPU_TRY(mem.alloc(&a.rows, static_cast<uint64_t>(n_blocks) * kCols));
    BLOK_GPU_TRY(hipMemcpy(d_entries, entries, n_entries * sizeof(blok_scatter_entry), hipMemcpyHostToDevice));
    a.entries = d_entries;
    hipLaunchKernelGGL(scatter_judge_kernel, dim3(n_blocks), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    unsigned long long totals[kCols];
    const GpuBuildStatus folded = fold_rows(mem, a.rows, n_blocks, 0u, totals, why);
    if (folded != GpuBuildStatus::Ok) return folded;
    blok_scatter_info& info = out->info;
    info.n_placed = totals[K::kPlaced];
    info.n_cells = info.n_placed;
    for (int r = 0; r < 5; ++r) { info.n_rejected[r] = totals[K::kRejected + r]; info.n_cells += totals[K::kRejected + r]; }
    if (!info.n_placed) return GpuBuildStatus::Ok;
    BLOK_GPU_TRY(mem.alloc(&a.table, info.n_placed));
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.counts, a.counts, static_cast<int>(a.n_waves)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, a.counts, a.counts, static_cast<int>(a.n_waves)));
    hipLaunchKernelGGL(scatter_emit_kernel, dim3(n_blocks), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    BLOK_GPU_TRY(hipStreamSynchronize(nullptr));            // (the scratch arrays outlive the kernels)
    mem.release(a.table);
    out->d_table = a.table;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
