// The light table from the quads snapshot (gpu_build.h: gpu_lights_from_quads; include/blok_hip.h: blok_hip_lights_from_quads).  The
// predicates are ../common/lights_core.h; DESIGN.md §32 has the contract.
//
// A lane per quad, two passes and one scan between them; no sort, no atomics, integer arithmetic only:
//   1. lights_count_kernel: a quad is kept iff its key's material index is in the emissive set.  One ballot gives the wave's number of
//      kept quads, one reduction their unit faces: a pair per wave.
//   2. an exclusive scan of the pairs (hipcub); its last entry is the totals, the one thing the host reads before it allocates the result.
//   3. lights_write_kernel: the same test; a kept quad's slot is its wave's offset plus its rank in the ballot, its cum the wave's face
//      offset plus the faces of the kept lanes before it (a scan over the wave by shuffles).  The order is the quads' order by construction.
// The owned set: every kept quad stores 1 to the byte of its material index (all writers of a byte write the same value), and
// lights_pack_kernel packs the 65536 bytes into the 2048 words the path loop tests.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <string>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/lights_core.h"

namespace blok {

namespace {

namespace L = lights;

struct WaveSum { unsigned long long n, faces; };
struct WaveSumAdd {
    __host__ __device__ WaveSum operator()(const WaveSum& a, const WaveSum& b) const { return WaveSum{a.n + b.n, a.faces + b.faces}; }
};

struct LightArgs {
    const blok_quad* quads; uint32_t n_quads;
    const uint32_t* glows; uint32_t n_materials;
    WaveSum* sums;                      // per wave of the grid, + 1: counts, then (scanned in place) offsets; the last is the totals
    blok_light* out;
    uint8_t* owned_bytes;               // [kSetBits]
};

__device__ __forceinline__ uint32_t lane_of() { return threadIdx.x & 63u; }

// the quad of this lane (zeros beyond the end) and whether it becomes a light
__device__ __forceinline__ bool kept_quad(const LightArgs& a, uint32_t i, uint4& head, uint4& tail) {
    head = make_uint4(0u, 0u, 0u, 0u); tail = head;
    if (i >= a.n_quads) return false;
    const uint4* rec = reinterpret_cast<const uint4*>(a.quads + i);      // 32-byte records in a hipMalloc'ed array: 16-byte aligned
    head = rec[0]; tail = rec[1];                                         // lo[3], du | dv, material, face, reserved
    return L::keeps(tail.y, a.glows, a.n_materials);
}

__global__ __launch_bounds__(256) void lights_count_kernel(const LightArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint4 head, tail;
    const bool keep = kept_quad(a, i, head, tail);
    unsigned long long faces = keep ? static_cast<unsigned long long>(head.w) * tail.x : 0ull;
    for (int off = 32; off > 0; off >>= 1) faces += __shfl_down(faces, off);
    const unsigned long long kept = __ballot(keep);
    if (lane_of() == 0u) a.sums[blockIdx.x * 4u + (threadIdx.x >> 6)] = WaveSum{static_cast<unsigned long long>(__popcll(kept)), faces};
}

__global__ __launch_bounds__(256) void lights_write_kernel(const LightArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint4 head, tail;
    const bool keep = kept_quad(a, i, head, tail);
    const unsigned long long mine = keep ? static_cast<unsigned long long>(head.w) * tail.x : 0ull;
    unsigned long long upto = mine;                                       // inclusive scan over the wave
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const unsigned long long t = __shfl_up(upto, off);
        if (lane_of() >= off) upto += t;
    }
    const unsigned long long kept = __ballot(keep);
    if (!keep) return;
    const WaveSum base = a.sums[blockIdx.x * 4u + (threadIdx.x >> 6)];
    const unsigned long long at = base.n + static_cast<unsigned long long>(__popcll(kept & ((1ull << lane_of()) - 1ull)));
    tail.w = static_cast<uint32_t>(base.faces + (upto - mine));           // (the host has checked the total: it fits)
    uint4* rec = reinterpret_cast<uint4*>(a.out + at);
    rec[0] = head; rec[1] = tail;
    a.owned_bytes[L::material_index(tail.y, a.n_materials)] = 1u;
}

__global__ __launch_bounds__(256) void lights_pack_kernel(const uint8_t* bytes, uint32_t* words) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= L::kSetWords) return;
    uint32_t bits = 0u;
    for (uint32_t b = 0; b < 32u; ++b) bits |= (bytes[w * 32u + b] ? 1u : 0u) << b;
    words[w] = bits;
}

}  // namespace

GpuBuildStatus gpu_lights_from_quads(const blok_quad* d_quads, uint64_t n_quads, const uint32_t* d_glows, uint32_t n_materials, uint32_t* d_owned,
                                     GpuLights* out, std::string* why) {
    *out = GpuLights{};
    if (n_quads >= 0xFFFFFF00ull) { *why = "lights_from_quads: 2^32 or more quads in the snapshot"; return GpuBuildStatus::Unsupported; }
    BLOK_GPU_TRY(hipMemsetAsync(d_owned, 0, L::kSetWords * sizeof(uint32_t), nullptr));
    if (n_quads == 0) { BLOK_GPU_TRY(hipDeviceSynchronize()); return GpuBuildStatus::Ok; }
    LightArgs a{};
    a.quads = d_quads; a.n_quads = static_cast<uint32_t>(n_quads); a.glows = d_glows; a.n_materials = n_materials;
    const uint32_t blocks = blocks_for(n_quads), waves = blocks * 4u;
    DeviceMem mem;
    BLOK_GPU_TRY(mem.alloc(&a.sums, waves + 1u));
    BLOK_GPU_TRY(mem.alloc(&a.owned_bytes, L::kSetBits));
    BLOK_GPU_TRY(hipMemsetAsync(a.sums + waves, 0, sizeof(WaveSum), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(a.owned_bytes, 0, L::kSetBits, nullptr));
    hipLaunchKernelGGL(lights_count_kernel, dim3(blocks), dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, temp_bytes, a.sums, a.sums, WaveSumAdd{}, WaveSum{0ull, 0ull}, static_cast<int>(waves + 1u)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveScan(d_temp, temp_bytes, a.sums, a.sums, WaveSumAdd{}, WaveSum{0ull, 0ull}, static_cast<int>(waves + 1u)));
    WaveSum total{};
    BLOK_GPU_TRY(hipMemcpy(&total, a.sums + waves, sizeof(total), hipMemcpyDeviceToHost));
    if (total.n >= 0x80000000ull || total.faces > 0xFFFFFFFFull) {
        *why = "lights_from_quads: 2^31 or more lights, or 2^32 or more unit faces";
        return GpuBuildStatus::Unsupported;
    }
    if (total.n) {
        BLOK_GPU_TRY(mem.alloc(&a.out, total.n));
        hipLaunchKernelGGL(lights_write_kernel, dim3(blocks), dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
        hipLaunchKernelGGL(lights_pack_kernel, dim3(L::kSetWords / 256u), dim3(256), 0, nullptr, a.owned_bytes, d_owned);
        BLOK_GPU_TRY(hipGetLastError());
        BLOK_GPU_TRY(hipDeviceSynchronize());
        mem.release(a.out);
        out->d_lights = a.out;
    }
    out->n = static_cast<uint32_t>(total.n); out->n_faces = total.faces;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
