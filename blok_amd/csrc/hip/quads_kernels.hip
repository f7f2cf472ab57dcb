// The resident volume's surface as merged quads (gpu_build.h: gpu_volume_extract_quads; include/blok_hip.h:
// blok_hip_volume_extract_quads).  The predicates are ../common/quads_core.h; DESIGN.md §14 has the contract and the measured cost.
//
// Three passes, no sort and no float anywhere:
//   1. quad_face_kernel<face>: a wave owns 64 cells along u of one plane and walks kRows rows up v.  A cell's exposure comes from the
//      brick masks alone (its own brick's word and the neighbouring brick's: no density read); the material id is read only where the
//      face is exposed.  Three ballots per row give the row's bit words S (run starts), T (run ends) and D (same as the cell below),
//      written only where the row has an exposed cell (the words are cleared beforehand).  The cell below rolls through the walk in
//      registers; the cells left of lane 0 and right of lane 63 are evaluated, by those two lanes, only when they matter.
//   2. quad_row_kernel<false>: a lane per row (face, plane, v) walks the row's words (quads::row_walk_word) and counts the runs that are
//      not linked to the row below: the quads that start in this row.  An exclusive scan over the rows in canonical order (hipcub) turns
//      the counts into offsets; its last entry is the total, the one number the host reads before it allocates the result.
//   3. quad_row_kernel<true>: the same walk; every origin grows upwards while the next row holds a linked identical run
//      (quads::row_has_linked_run) and is written at its row's offset, in u order.  The result is sorted by construction.
// Exposed unit faces are counted from the ballots: one 64-bit integer atomic per wave into one of kSpread words.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "gpu_build.h"
#include "device_mem.h"
#include "../common/quads_core.h"
#include "../common/sweep_core.h"      // brick_bit

namespace blok {

namespace {

namespace Q = quads;

constexpr uint32_t kRows = 16;          // rows of v per wave of the face pass
constexpr uint32_t kSpread = 64;        // copies of the exposed-face count

struct FaceDims {
    uint32_t ns, nv, nu, wu;            // planes, rows per plane, cells per row, 64-bit words per row
    uint64_t word_base;                 // of the face's words within S, T and D: word (s, w, v) at word_base + (s * wu + w) * nv + v
};

struct QuadArgs {
    BrickMasks bricks; const uint32_t* ids;
    uint32_t nx, ny, nz;
    int32_t origin[3];
    uint32_t lo[3], hi[3];              // region, box-local, half-open
    uint32_t ignore_material;
    FaceDims face[6];
    uint32_t row_base[7];               // canonical row index of each face's first row; [6] = rows in all
    uint64_t *S, *T, *D;
    unsigned long long* counts;         // per row, rows + 1 entries: origins, then (scanned in place) offsets; the last is the total
    unsigned long long* n_faces;        // [kSpread]
    blok_quad* out;
};

// Face kFace of the voxel (x, y, z), box-local; `inside`: the voxel lies in the region (otherwise nothing is read).
template <uint32_t kFace>
__device__ __forceinline__ Q::Cell face_cell(const QuadArgs& a, uint32_t x, uint32_t y, uint32_t z, bool inside) {
    Q::Cell none; none.exposed = 0u; none.key = 0u;
    if (!inside) return none;
    const uint64_t m = a.bricks.at(x >> 2, y >> 2, z >> 2);
    if (!((m >> sweep::brick_bit(x & 3u, y & 3u, z & 3u)) & 1ull)) return none;
    constexpr int A = static_cast<int>(kFace >> 1);
    constexpr uint32_t step = (kFace & 1u) ? 0xFFFFFFFFu : 1u;      // (-1 wraps: a coordinate below 0 fails the box test as one above does)
    const uint32_t qx = x + (A == 0 ? step : 0u), qy = y + (A == 1 ? step : 0u), qz = z + (A == 2 ? step : 0u);
    bool neighbour = false;
    if (qx < a.nx && qy < a.ny && qz < a.nz) {
        const bool same_brick = (qx >> 2) == (x >> 2) && (qy >> 2) == (y >> 2) && (qz >> 2) == (z >> 2);
        const uint64_t mq = same_brick ? m : a.bricks.at(qx >> 2, qy >> 2, qz >> 2);
        neighbour = (mq >> sweep::brick_bit(qx & 3u, qy & 3u, qz & 3u)) & 1ull;
    }
    if (neighbour) return none;
    const uint32_t material = a.ignore_material ? 0u : a.ids[(static_cast<size_t>(z) * a.ny + y) * a.nx + x];
    return Q::cell(true, false, material, a.ignore_material != 0u);
}

template <uint32_t kFace>
__global__ __launch_bounds__(256) void quad_face_kernel(const QuadArgs a) {
    constexpr int A = static_cast<int>(kFace >> 1);
    const FaceDims d = a.face[kFace];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nvb = (d.nv + kRows - 1u) / kRows;
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);      // wave-uniform
    if (item >= static_cast<uint64_t>(d.ns) * d.wu * nvb) return;
    // consecutive waves: consecutive planes for the x faces (their lanes run along y, so neighbouring planes share cache lines), else
    // consecutive words of a row
    uint32_t s, w, vb;
    if (A == 0) { s = static_cast<uint32_t>(item % d.ns); w = static_cast<uint32_t>((item / d.ns) % d.wu); vb = static_cast<uint32_t>(item / (static_cast<uint64_t>(d.ns) * d.wu)); }
    else { w = static_cast<uint32_t>(item % d.wu); vb = static_cast<uint32_t>((item / d.wu) % nvb); s = static_cast<uint32_t>(item / (static_cast<uint64_t>(d.wu) * nvb)); }
    const uint32_t u = w * 64u + lane;
    const bool in_u = u < d.nu;
    const uint32_t v0 = vb * kRows, v1 = min(d.nv, v0 + kRows);
    // box-local coordinates from (s, u, v): x faces (y, z), y faces (x, z), z faces (x, y)
    const uint32_t cs = a.lo[A] + s, cu = a.lo[Q::u_axis(A)] + u, cv0 = a.lo[Q::v_axis(A)];
    Q::Cell below; below.exposed = 0u; below.key = 0u;
    uint32_t exposed_faces = 0;
    uint64_t* const words_s = a.S + d.word_base + (static_cast<uint64_t>(s) * d.wu + w) * d.nv;
    uint64_t* const words_t = a.T + d.word_base + (static_cast<uint64_t>(s) * d.wu + w) * d.nv;
    uint64_t* const words_d = a.D + d.word_base + (static_cast<uint64_t>(s) * d.wu + w) * d.nv;
#pragma unroll 1
    for (uint32_t v = v0 ? v0 - 1u : 0u; v < v1; ++v) {      // (one row early: the first trip of a later block only fills `below`)
        const uint32_t cv = cv0 + v;
        const uint32_t x = A == 0 ? cs : cu, y = A == 0 ? cu : A == 1 ? cs : cv, z = A == 2 ? cs : cv;
        const Q::Cell c = face_cell<kFace>(a, x, y, z, in_u);
        if (v < v0) { below = c; continue; }
        const uint64_t E = __ballot(c.exposed != 0u);
        if (E) {
            Q::Cell left, right;
            left.exposed = __shfl_up(c.exposed, 1); left.key = __shfl_up(c.key, 1);
            right.exposed = __shfl_down(c.exposed, 1); right.key = __shfl_down(c.key, 1);
            const bool edge_lane = lane == 0u || lane == 63u;
            if (__ballot(edge_lane && c.exposed)) {
                // the cells outside the wave's 64: u - 1 for lane 0, u + 1 for lane 63 (outside the region: not exposed)
                const uint32_t ue = lane == 0u ? u - 1u : u + 1u;
                const bool wanted = edge_lane && (lane == 0u ? w > 0u : ue < d.nu);
                const uint32_t ce = a.lo[Q::u_axis(A)] + ue;
                const uint32_t ex = A == 0 ? cs : ce, ey = A == 0 ? ce : A == 1 ? cs : cv;
                const Q::Cell e = face_cell<kFace>(a, ex, ey, z, wanted);
                if (lane == 0u) left = e;
                if (lane == 63u) right = e;
            } else {
                if (lane == 0u) { left.exposed = 0u; left.key = 0u; }
                if (lane == 63u) { right.exposed = 0u; right.key = 0u; }
            }
            const uint64_t S = __ballot(Q::starts_run(c, left)), T = __ballot(Q::ends_run(c, right)), D = __ballot(Q::same(c, below));
            if (lane == 0u) { words_s[v] = S; words_t[v] = T; words_d[v] = D; }
            exposed_faces += static_cast<uint32_t>(__popcll(E));
        }
        below = c;
    }
    if (lane == 0u && exposed_faces) atomicAdd(a.n_faces + (blockIdx.x % kSpread), static_cast<unsigned long long>(exposed_faces));
}

// A lane per row, rows in canonical order (face, plane, v).  kWrite = false: counts[row] = quads that start in the row.  kWrite = true:
// counts[row] is the row's offset; each of its quads is measured upwards and written.
template <bool kWrite>
__global__ __launch_bounds__(256) void quad_row_kernel(const QuadArgs a) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= a.row_base[6]) return;
    uint32_t f = 0;
    while (row >= a.row_base[f + 1u]) ++f;
    const FaceDims d = a.face[f];
    const uint32_t r = row - a.row_base[f], s = r / d.nv, v = r % d.nv;
    const uint64_t base = d.word_base + static_cast<uint64_t>(s) * d.wu * d.nv;
    const uint64_t *S = a.S + base, *T = a.T + base, *D = a.D + base;
    unsigned long long at = kWrite ? a.counts[row] : 0ull;
    if (kWrite && a.counts[row + 1u] == at) return;          // no quad starts in this row
    uint32_t n = 0;
    Q::RowWalk walk;
    Q::row_walk_reset(walk);
    const int A = static_cast<int>(f >> 1);
    for (uint32_t w = 0; w < d.wu; ++w) {
        const uint64_t i = static_cast<uint64_t>(w) * d.nv + v;
        const uint64_t sw = S[i], tw = T[i];
        if (!(sw | tw) && !walk.open) continue;
        const uint64_t dw = D[i], sb = v ? S[i - 1u] : 0ull, tb = v ? T[i - 1u] : 0ull;
        Q::row_walk_word(walk, w, sw, tw, dw, sb, tb, [&](uint32_t u0, uint32_t u1, bool linked) {
            if (linked) return;
            ++n;
            if constexpr (kWrite) {
                uint32_t dv = 1;
                for (uint32_t vv = v + 1u; vv < d.nv; ++vv, ++dv)
                    if (!Q::row_has_linked_run(u0, u1, [&](uint32_t ww, uint64_t& s_, uint64_t& t_, uint64_t& d_) {
                            const uint64_t j = static_cast<uint64_t>(ww) * d.nv + vv;
                            s_ = S[j]; t_ = T[j]; d_ = D[j];
                        })) break;
                // lo: the plane (+1 for the positive faces), the first cell along u, the row
                const int32_t ps = a.origin[A] + static_cast<int32_t>(a.lo[A] + s) + ((f & 1u) ? 0 : 1);
                const int32_t pu = a.origin[Q::u_axis(A)] + static_cast<int32_t>(a.lo[Q::u_axis(A)] + u0);
                const int32_t pv = a.origin[Q::v_axis(A)] + static_cast<int32_t>(a.lo[Q::v_axis(A)] + v);
                uint4 head, tail;
                head.x = static_cast<uint32_t>(A == 0 ? ps : pu); head.y = static_cast<uint32_t>(A == 0 ? pu : A == 1 ? ps : pv);
                head.z = static_cast<uint32_t>(A == 2 ? ps : pv); head.w = u1 - u0 + 1u;
                // the key: the material id of the run's first cell
                uint32_t material = 0;
                if (!a.ignore_material) {
                    const uint32_t cs = a.lo[A] + s, cu = a.lo[Q::u_axis(A)] + u0, cv = a.lo[Q::v_axis(A)] + v;
                    const uint32_t x = A == 0 ? cs : cu, y = A == 0 ? cu : A == 1 ? cs : cv, z = A == 2 ? cs : cv;
                    material = a.ids[(static_cast<size_t>(z) * a.ny + y) * a.nx + x];
                }
                tail.x = dv; tail.y = material; tail.z = f; tail.w = 0u;
                uint4* rec = reinterpret_cast<uint4*>(a.out + at);      // 32-byte records in a hipMalloc'ed array: 16-byte aligned
                rec[0] = head; rec[1] = tail;
                ++at;
            }
        });
    }
    if (!kWrite) a.counts[row] = n;
}

template <uint32_t kFace>
void launch_face(const QuadArgs& a) {
    const FaceDims& d = a.face[kFace];
    const uint64_t waves = static_cast<uint64_t>(d.ns) * d.wu * ((d.nv + kRows - 1u) / kRows);
    hipLaunchKernelGGL((quad_face_kernel<kFace>), dim3(static_cast<uint32_t>((waves + 3u) / 4u)), dim3(256), 0, nullptr, a);
}

}  // namespace

void gpu_quads_free(GpuQuads* q) {
    if (q->d_quads) (void)hipFree(q->d_quads);
    *q = GpuQuads{};
}

GpuBuildStatus gpu_volume_extract_quads(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t flags, GpuQuads* out,
                                        uint64_t* out_n_faces, std::string* why) {
    *out = GpuQuads{}; *out_n_faces = 0;
    if (!cells_fit_32_bits(v, "extract_quads", why)) return GpuBuildStatus::Unsupported;
    if (lo[0] >= hi[0] || lo[1] >= hi[1] || lo[2] >= hi[2]) return GpuBuildStatus::Ok;
    QuadArgs a{};
    a.bricks = brick_masks_of(*v); a.ids = v->d_ids;
    a.nx = v->nx; a.ny = v->ny; a.nz = v->nz;
    a.ignore_material = (flags & BLOK_QUADS_IGNORE_MATERIAL) ? 1u : 0u;
    const uint32_t ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    for (int c = 0; c < 3; ++c) { a.origin[c] = v->origin[c]; a.lo[c] = lo[c]; a.hi[c] = hi[c]; }
    uint64_t words = 0, rows = 0;
    for (uint32_t f = 0; f < 6u; ++f) {
        const int A = Q::normal_axis(f);
        FaceDims& d = a.face[f];
        d.ns = ext[A]; d.nu = ext[Q::u_axis(A)]; d.nv = ext[Q::v_axis(A)]; d.wu = (d.nu + 63u) / 64u;
        d.word_base = words;
        words += static_cast<uint64_t>(d.ns) * d.wu * d.nv;
        a.row_base[f] = static_cast<uint32_t>(rows);
        rows += static_cast<uint64_t>(d.ns) * d.nv;
        if (rows >= 0x7FFFFFFFull) { *why = "extract_quads: 2^31 or more rows in the region"; return GpuBuildStatus::Unsupported; }
    }
    a.row_base[6] = static_cast<uint32_t>(rows);
    DeviceMem mem;
    uint64_t* d_words;
    BLOK_GPU_TRY(mem.alloc(&d_words, 3u * words));
    a.S = d_words; a.T = d_words + words; a.D = d_words + 2u * words;
    BLOK_GPU_TRY(mem.alloc(&a.counts, rows + 1u));
    BLOK_GPU_TRY(mem.alloc(&a.n_faces, kSpread));
    BLOK_GPU_TRY(hipMemsetAsync(d_words, 0, 3u * words * sizeof(uint64_t), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(a.counts + rows, 0, sizeof(unsigned long long), nullptr));
    BLOK_GPU_TRY(hipMemsetAsync(a.n_faces, 0, kSpread * sizeof(unsigned long long), nullptr));
    launch_face<0>(a); launch_face<1>(a); launch_face<2>(a); launch_face<3>(a); launch_face<4>(a); launch_face<5>(a);
    BLOK_GPU_TRY(hipGetLastError());
    const dim3 row_grid(static_cast<uint32_t>((rows + 255u) / 256u));
    hipLaunchKernelGGL((quad_row_kernel<false>), row_grid, dim3(256), 0, nullptr, a);
    BLOK_GPU_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.counts, a.counts, static_cast<int>(rows + 1u)));
    uint8_t* d_temp;
    BLOK_GPU_TRY(mem.alloc(&d_temp, temp_bytes));
    BLOK_GPU_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, a.counts, a.counts, static_cast<int>(rows + 1u)));
    unsigned long long total = 0;
    std::vector<unsigned long long> faces(kSpread);
    BLOK_GPU_TRY(hipMemcpy(&total, a.counts + rows, sizeof(total), hipMemcpyDeviceToHost));
    BLOK_GPU_TRY(hipMemcpy(faces.data(), a.n_faces, kSpread * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t n_faces = 0;
    for (const unsigned long long n : faces) n_faces += n;
    if (!(flags & BLOK_QUADS_COUNT_ONLY) && total) {
        BLOK_GPU_TRY(mem.alloc(&a.out, total));
        hipLaunchKernelGGL((quad_row_kernel<true>), row_grid, dim3(256), 0, nullptr, a);
        BLOK_GPU_TRY(hipGetLastError());
        BLOK_GPU_TRY(hipDeviceSynchronize());
        mem.release(a.out);
        out->d_quads = a.out;
    }
    out->n_quads = total; *out_n_faces = n_faces;
    return GpuBuildStatus::Ok;
}

}  // namespace blok
