// Neighbour-count rules stepped over the resident volume (gpu_build.h: gpu_volume_automaton; include/blok_hip.h:
// blok_hip_volume_automaton has the contract; the rule lives in ../common/automaton_core.h, shared with the host build).
//
// A step is three launches and the commit of every edit:
//   decide. from the brick masks alone, in either layout (BrickMasks::part), never a density or an id.  A lane per brick of the region, 64
//     bricks along x per wave (bricks_kernels.hip's arrangement).  The lane loads its brick's word and its 26 neighbours' — a brick beyond
//     the grid is 0 or all ones by BOX_IS_SOLID, the cells of a ragged last brick past the box's end likewise (lod_core.h: solid) — and
//     decides its 64 cells at once (automaton_core.h: brick_step): shifted words, carry-save adders into five bit planes, the rule's two
//     truth tables (wave-uniform) evaluated on the planes, the result cut to the region's cells of the brick.  It writes the brick's born
//     and died words to the call's scratch (16 bytes per region brick) and counts: per wave three shuffle sums and one atomic instruction
//     of three lanes.
//   births. a wave per region brick, gone at once when the brick's born word is 0; a lane per cell.  Lanes 0 .. 26 hold the words of the 27
//     bricks around (the masks are still those of before the step), every lane finds its filled neighbours in them through shuffles, a
//     born lane reads those neighbours' ids into its column of a 26 KiB LDS array (26 ids a lane do not stay in registers: the unrolled
//     form spilled), votes over the column (automaton_core.h: vote) and writes (density, id).
//   deaths. the same shape over the died words: (0.0f, 0).
// Everything is on the null stream, behind earlier edits; the host reads the step's three counters behind the decide launch, which is how
// it knows that a step changes nothing.
#include <hip/hip_runtime.h>

#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/automaton_core.h"

namespace blok {

namespace {

namespace K = automaton;

constexpr uint32_t kCounters = 3u;                         // per step: cells born, cells that died, region cells filled before the step

struct RegionBricks {
    uint32_t dims[3], nb[3];                               // the box, in cells and in bricks
    uint32_t lo[3], hi[3];                                 // the region, box-local
    uint32_t b0[3], n[3];                                  // the bricks that hold it: [b0, b0 + n)
};

struct DecideArgs {
    BrickMasks masks;
    RegionBricks r;
    uint32_t x_chunks;
    uint64_t n_waves;
    uint32_t neighbourhood, survive, birth, solid;
    uint64_t* words;                                       // per region brick, x fastest: born, died
    unsigned long long* counts;                            // kCounters of this step
};

__global__ __launch_bounds__(256) void automaton_decide_kernel(const DecideArgs a) {
    const uint64_t wave = blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;                          // (a whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t xc, ry, rz;
    row_segment(wave, a.x_chunks, a.r.n[1], xc, ry, rz);
    xc = __builtin_amdgcn_readfirstlane(xc); ry = __builtin_amdgcn_readfirstlane(ry); rz = __builtin_amdgcn_readfirstlane(rz);
    const uint32_t rx = 64u * xc + lane;
    const bool live = rx < a.r.n[0];
    const uint32_t bx = a.r.b0[0] + rx, by = a.r.b0[1] + ry, bz = a.r.b0[2] + rz;
    uint64_t born = 0ull, died = 0ull, filled = 0ull;
    if (live) {
        // a brick's index is the sum of its coordinates' parts: the lane's three along x, the wave's along y and z (scalar)
        uint64_t px[3], py[3], pz[3];
        for (uint32_t j = 0; j < 3u; ++j) { px[j] = a.masks.part(bx + j - 1u, 0u); py[j] = a.masks.part(by + j - 1u, 1u); pz[j] = a.masks.part(bz + j - 1u, 2u); }
        uint64_t seen27[27];
#pragma unroll
        for (uint32_t j = 0; j < 27u; ++j) {
            const uint32_t jx = j % 3u, jy = (j / 3u) % 3u, jz = j / 9u;
            const uint32_t qx = bx + jx - 1u, qy = by + jy - 1u, qz = bz + jz - 1u;      // (a coordinate below 0 wraps and fails the test)
            const bool in_grid = qx < a.r.nb[0] && qy < a.r.nb[1] && qz < a.r.nb[2];
            const uint64_t m = in_grid ? a.masks.masks[px[jx] + py[jy] + pz[jz]] : 0ull;
            seen27[j] = K::seen(m, in_grid, qx, qy, qz, a.r.dims, a.solid != 0u);
        }
        const uint64_t mask = a.masks.masks[px[1] + py[1] + pz[1]];
        const uint64_t cells = K::region_cells(bx, by, bz, a.r.lo, a.r.hi);
        K::brick_step(seen27, mask, cells, a.neighbourhood, a.survive, a.birth, &born, &died);
        filled = mask & cells;
        const size_t i = rx + static_cast<size_t>(a.r.n[0]) * (ry + static_cast<size_t>(a.r.n[1]) * rz);
        *reinterpret_cast<ulonglong2*>(a.words + 2u * i) = make_ulonglong2(born, died);
    }
    uint32_t sum[kCounters] = {static_cast<uint32_t>(__popcll(born)), static_cast<uint32_t>(__popcll(died)), static_cast<uint32_t>(__popcll(filled))};
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        for (uint32_t k = 0; k < kCounters; ++k) sum[k] += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum[k]), d));
    if (lane < kCounters) {
        const uint32_t value = lane == 0u ? sum[0] : lane == 1u ? sum[1] : sum[2];
        if (value) atomicAdd(a.counts + lane, static_cast<unsigned long long>(value));
    }
}

struct WriteArgs {
    BrickMasks masks;
    RegionBricks r;
    const uint64_t* words;
    uint64_t n_bricks;                                     // of the region
    float* density; uint32_t* ids;
    uint32_t neighbourhood, fixed, material;
    float value;
};

// The wave's region brick and its word (born: which 0, died: which 1); false = nothing to write, the whole wave leaves.
__device__ __forceinline__ bool brick_of_wave(const WriteArgs& a, uint32_t which, uint32_t& bx, uint32_t& by, uint32_t& bz, uint64_t& word) {
    const uint64_t wave = blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (wave >= a.n_bricks) return false;
    const uint32_t i = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave));      // (at most 2^26 bricks: the volume's cells fit 32 bits)
    word = uniform_u64(a.words, 2u * i + which);
    if (!word) return false;
    bx = a.r.b0[0] + i % a.r.n[0];
    const uint32_t row = i / a.r.n[0];
    by = a.r.b0[1] + row % a.r.n[1]; bz = a.r.b0[2] + row / a.r.n[1];
    return true;
}

__global__ __launch_bounds__(256) void automaton_births_kernel(const WriteArgs a) {
    uint32_t bx, by, bz;
    uint64_t born;
    if (!brick_of_wave(a, 0u, bx, by, bz, born)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = 4u * bx + (lane & 3u), y = 4u * by + ((lane >> 2) & 3u), z = 4u * bz + (lane >> 4);
    const bool is_born = (born >> lane) & 1ull;             // (a born cell lies in the region, and so in the box)
    uint32_t id = a.material;
    __shared__ uint32_t s_ids[26][256];
    if (!a.fixed) {                                         // (wave-uniform)
        // lane j < 27 holds the word of brick j of the 3^3 bricks around: 0 beyond the grid, where nobody votes
        uint32_t word_lo = 0u, word_hi = 0u;
        if (lane < 27u) {
            const uint32_t qx = bx + lane % 3u - 1u, qy = by + (lane / 3u) % 3u - 1u, qz = bz + lane / 9u - 1u;
            if (qx < a.r.nb[0] && qy < a.r.nb[1] && qz < a.r.nb[2]) {
                const uint64_t m = a.masks.at(qx, qy, qz);
                word_lo = static_cast<uint32_t>(m); word_hi = static_cast<uint32_t>(m >> 32);
            }
        }
        // the voters' ids go through LDS, a column per lane (no lane reads another's: no barrier): 26 ids a lane would not stay in registers
        uint32_t voters = 0u;
#pragma unroll 1
        for (uint32_t i = 0; i < a.neighbourhood; ++i) {    // (wave-uniform: the offset is scalar)
            int32_t d[3];
            K::offset(i, d);
            // the neighbour, in cells of the 12^3 block of the 27 bricks: 3 .. 8 per axis
            const uint32_t cx = 4u + (lane & 3u) + d[0], cy = 4u + ((lane >> 2) & 3u) + d[1], cz = 4u + (lane >> 4) + d[2];
            const uint32_t from = (cx >> 2) + 3u * (cy >> 2) + 9u * (cz >> 2), bit = (cx & 3u) | ((cy & 3u) << 2) | ((cz & 3u) << 4);
            // (every lane takes part in the shuffles: the wave is whole here; both halves, since the half wanted is the reader's to choose)
            const uint32_t lo = static_cast<uint32_t>(__shfl(static_cast<int>(word_lo), static_cast<int>(from)));
            const uint32_t hi = static_cast<uint32_t>(__shfl(static_cast<int>(word_hi), static_cast<int>(from)));
            const uint32_t qx = x + d[0], qy = y + d[1], qz = z + d[2];      // (below 0 wraps and fails the test)
            const bool in_box = qx < a.r.dims[0] && qy < a.r.dims[1] && qz < a.r.dims[2];
            const bool filled = (((bit < 32u ? lo : hi) >> (bit & 31u)) & 1u) != 0u;
            if (is_born && in_box && filled) {
                voters |= 1u << i;
                s_ids[i][threadIdx.x] = a.ids[(static_cast<size_t>(qz) * a.r.dims[1] + qy) * a.r.dims[0] + qx];
            }
        }
        if (is_born) id = K::vote([&](uint32_t i) { return s_ids[i][threadIdx.x]; }, a.neighbourhood, voters, a.material);
    }
    if (is_born) {
        const size_t cell = (static_cast<size_t>(z) * a.r.dims[1] + y) * a.r.dims[0] + x;
        a.density[cell] = a.value; a.ids[cell] = id;
    }
}

__global__ __launch_bounds__(256) void automaton_deaths_kernel(const WriteArgs a) {
    uint32_t bx, by, bz;
    uint64_t died;
    if (!brick_of_wave(a, 1u, bx, by, bz, died)) return;
    const uint32_t lane = threadIdx.x & 63u;
    if (!((died >> lane) & 1ull)) return;
    const uint32_t x = 4u * bx + (lane & 3u), y = 4u * by + ((lane >> 2) & 3u), z = 4u * bz + (lane >> 4);
    const size_t cell = (static_cast<size_t>(z) * a.r.dims[1] + y) * a.r.dims[0] + x;
    a.density[cell] = 0.0f; a.ids[cell] = 0u;
}

}  // namespace

GpuBuildStatus gpu_volume_automaton(GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], const blok_automaton_rule& rule, uint64_t* out_step_counts,
                                    blok_automaton_info* out_info, std::string* why) {
    if (!cells_fit_32_bits(v, "volume_automaton", why)) return GpuBuildStatus::Unsupported;
    blok_automaton_info info;
    K::plan(v->origin, lo, hi, rule.flags, &info);
    if (out_step_counts)
        for (uint32_t k = 0; k < 2u * rule.steps; ++k) out_step_counts[k] = 0u;
    *out_info = info;
    if (!info.ext[0] || !info.ext[1] || !info.ext[2]) return GpuBuildStatus::Ok;
    RegionBricks r{};
    r.dims[0] = v->nx; r.dims[1] = v->ny; r.dims[2] = v->nz; r.nb[0] = v->nbx; r.nb[1] = v->nby; r.nb[2] = v->nbz;
    uint64_t n_bricks = 1u;
    for (int k = 0; k < 3; ++k) {
        r.lo[k] = lo[k]; r.hi[k] = hi[k];
        r.b0[k] = lo[k] / 4u; r.n[k] = (hi[k] - 1u) / 4u - r.b0[k] + 1u;
        n_bricks *= r.n[k];
    }
    // everything the call allocates, before anything is written: a failed allocation leaves the volume untouched
    DeviceMem mem;
    uint64_t* d_words;
    unsigned long long* d_counts;
    BLOK_GPU_TRY(mem.alloc(&d_words, 2u * n_bricks));
    BLOK_GPU_TRY(mem.alloc(&d_counts, static_cast<uint64_t>(kCounters) * rule.steps));
    BLOK_GPU_TRY(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * kCounters * rule.steps, nullptr));
    DecideArgs da{};
    da.r = r;
    da.x_chunks = (r.n[0] + 63u) / 64u;
    da.n_waves = static_cast<uint64_t>(da.x_chunks) * r.n[1] * r.n[2];      // at most the volume's bricks: 2^26
    da.neighbourhood = rule.neighbourhood; da.survive = rule.survive; da.birth = rule.birth;
    da.solid = (rule.flags & BLOK_AUTOMATON_BOX_IS_SOLID) ? 1u : 0u;
    da.words = d_words;
    WriteArgs wa{};
    wa.r = r; wa.words = d_words; wa.n_bricks = n_bricks;
    wa.density = v->d_density; wa.ids = v->d_ids;
    wa.neighbourhood = rule.neighbourhood; wa.fixed = (rule.flags & BLOK_AUTOMATON_FIXED_MATERIAL) ? 1u : 0u; wa.material = rule.material; wa.value = rule.density;
    const uint32_t write_blocks = static_cast<uint32_t>((n_bricks + 3u) / 4u);
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    for (uint32_t step = 0; step < rule.steps; ++step) {
        da.masks = brick_masks_of(*v); da.counts = d_counts + static_cast<size_t>(kCounters) * step;
        hipLaunchKernelGGL(automaton_decide_kernel, dim3(static_cast<uint32_t>((da.n_waves + 3u) / 4u)), dim3(256), 0, nullptr, da);
        BLOK_GPU_TRY(hipGetLastError());
        unsigned long long counts[kCounters] = {0, 0, 0};
        BLOK_GPU_TRY(hipMemcpy(counts, da.counts, sizeof(counts), hipMemcpyDeviceToHost));      // (the step's wait)
        info.steps_run = step + 1u;
        info.n_filled = counts[2];
        if (!counts[0] && !counts[1]) break;                // a fixed point: this step counts, nothing is written, no later one runs
        // Births before deaths, each in a launch of its own.  The voters of a born cell are the cells filled BEFORE the step, those that
        // die in it included: the births launch reads their ids and the old masks (the commit below is what changes the masks) and writes
        // only cells that were empty, whose ids never vote — so no lane reads an id another lane of the launch writes.  A death zeroes
        // the id of a cell that may be a voter, so the deaths run in the launch behind.
        wa.masks = da.masks;
        if (counts[0]) {
            hipLaunchKernelGGL(automaton_births_kernel, dim3(write_blocks), dim3(256), 0, nullptr, wa);
            BLOK_GPU_TRY(hipGetLastError());
        }
        if (counts[1]) {
            hipLaunchKernelGGL(automaton_deaths_kernel, dim3(write_blocks), dim3(256), 0, nullptr, wa);
            BLOK_GPU_TRY(hipGetLastError());
        }
        const GpuBuildStatus st = gpu_volume_commit(v, lo, hi, rule.birth ? Edit::MayFill : Edit::OnlyClears, why);
        if (st != GpuBuildStatus::Ok) return st;
        info.n_born += counts[0]; info.n_died += counts[1];
        info.n_filled = counts[2] + counts[0] - counts[1];
        if (out_step_counts) { out_step_counts[2u * step] = counts[0]; out_step_counts[2u * step + 1u] = counts[1]; }
    }
    BLOK_GPU_TRY(hipStreamSynchronize(nullptr));             // blocking, as every edit is: the scratch goes with the call
    *out_info = info;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
