// gfx950 kernels of the posed primary frame and rays (posed_core.h has the semantics, the per-ray math and the bins' margin).  They run
// after the instance pass (instance_kernels.hip) on its stream and compose its records with the poses' in place.
#include "posed_core.h"
#include "volume_device.h"      // uniform_record, uniform_word

namespace blok {

namespace {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// The loop every lane of a wave runs over its candidate poses (uniform across the wave): list[0 .. n) or, list == null, every pose.
// The 64-byte pose and the 64-byte descriptor come through the scalar cache, one load each: the nine matrix elements, the pivot and the
// local point are scalar operands of the lane's ray transform.  `active`: the lane has a ray.  Leaves the composed record in rec, the face
// to shade it by in shade (if won != kInstanceNone) and the winning pose's index in won.
__device__ __forceinline__ void compose_poses(const PosedArgs& Q, const uint32_t* list, uint32_t n, bool active, const RayIn& r, float best,
                                              uint4* stk, uint4& rec, uint32_t& shade, uint32_t& won) {
    const InstanceArgs& P = Q.frame;
    const float vs = P.world.voxel_size, inv_vs = P.world.inv_voxel_size;
    won = kInstanceNone;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t idx = list ? uniform_word(list, j) : j;
        const blok_pose S = uniform_record(Q.poses, idx);
        if (S.model >= P.n_models) continue;
        const ModelDesc M = uniform_record(P.models, S.model);
        if (!pose_usable(S, M)) continue;
        RayIn l;
        const bool finite = pose_ray(S, r, l);
        l.tmax = best;
        const bool enters = active && finite && instance_box_entered(M, vs, l);
        if (__ballot(enters) == 0ull) continue;        // no lane of the wave enters the model's box
        if (enters) {
            const HitInfo h = walk(model_args(M, vs, inv_vs), l, stk);
            if (h.found) { rec = pose_record(h); shade = pose_shade_face(S, h.face); best = h.t; won = idx; }
        }
    }
}

__device__ __forceinline__ float best_of(const uint4& w, float tmax) {
    return ((w.w >> 24) & 1u) ? __uint_as_float(w.x) : tmax;
}

}  // namespace

// One wave per bin: the poses whose widened preimage box may cover the bin, in ascending index order (ballot + mbcnt ranks, no atomics).
__global__ __launch_bounds__(64) void posed_bins_kernel(const PosedArgs Q) {
    const InstanceArgs& P = Q.frame;
    const TraceArgs& A = P.world;
    const uint32_t lane = threadIdx.x, bin = blockIdx.x;
    const uint32_t bxi = bin % P.bins_x, byi = bin / P.bins_x;
    // the bin's pixels, frame coordinates, inclusive
    const float px0 = static_cast<float>(A.x0 + bxi * kBinPixels), py0 = static_cast<float>(A.y0 + byi * kBinPixels);
    const float px1 = static_cast<float>(A.x0 + min((bxi + 1u) * kBinPixels, A.w) - 1u), py1 = static_cast<float>(A.y0 + min((byi + 1u) * kBinPixels, A.h) - 1u);
    uint32_t* list = P.bins + static_cast<size_t>(bin) * kBinWords;
    uint32_t count = 0;
    for (uint32_t base = 0; base < Q.n_poses; base += 64u) {
        const uint32_t idx = base + lane;
        bool cover = false;
        if (idx < Q.n_poses) {
            const blok_pose S = Q.poses[idx];
            if (S.model < P.n_models) {
                const ModelDesc M = P.models[S.model];
                if (pose_usable(S, M)) {
                    float flo[3], fhi[3];
                    float x0, y0, x1, y1;
                    cover = !P.view.usable || !pose_world_box(S, M, A.voxel_size, P.view.pos, flo, fhi) || !project_box(P.view, flo, fhi, x0, y0, x1, y1) ||
                            (x0 <= px1 && x1 >= px0 && y0 <= py1 && y1 >= py0);
                }
            }
        }
        const unsigned long long mask = __ballot(cover);
        const uint32_t slot = count + lanes_below(mask);
        if (cover && slot < kBinCapacity) list[1u + slot] = idx;
        count += static_cast<uint32_t>(__popcll(mask));
    }
    if (lane == 0) list[0] = count > kBinCapacity ? kBinOverflow : count;
}

// One wave per 8x8 pixel tile of the rectangle: the pixel's composed record so far, then the bin's poses.  A tile whose bin lists no pose
// touches nothing; ids are written only where a pose wins.
__global__ __launch_bounds__(64) void posed_pass_kernel(const PosedArgs Q) {
    extern __shared__ uint4 lds_stack[];       // [stack_levels][64], as the world walk's
    const InstanceArgs& P = Q.frame;
    const TraceArgs& A = P.world;
    const uint32_t lane = threadIdx.x;
    const uint32_t tiles_x = (A.w + kWaveW - 1u) / kWaveW;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t* bin = P.bins + static_cast<size_t>((ty * kWaveH / kBinPixels) * P.bins_x + tx * kWaveW / kBinPixels) * kBinWords;
    const uint32_t head = uniform_word(bin, 0u);
    if (head == 0u) return;
    const uint32_t lx = tx * kWaveW + lane % kWaveW, ly = ty * kWaveH + lane / kWaveW;
    const bool inside = lx < A.w && ly < A.h;
    const size_t i = static_cast<size_t>(ly) * A.w + lx;
    RayIn r{};
    float best = A.tmax;
    if (inside) {
        best = best_of(*reinterpret_cast<const uint4*>(P.hits + i), A.tmax);
        r = primary_ray(A, A.x0 + lx, A.y0 + ly);
    }
    uint4 rec{};
    uint32_t won, shade = 0u;
    if (head == kBinOverflow) compose_poses(Q, nullptr, Q.n_poses, inside, r, best, lds_stack + lane, rec, shade, won);
    else compose_poses(Q, bin + 1, head, inside, r, best, lds_stack + lane, rec, shade, won);
    if (!inside || won == kInstanceNone) return;
    *reinterpret_cast<uint4*>(P.hits + i) = rec;
    if (P.rgba) P.rgba[i] = shade_rgba(A.mat_table, A.n_materials, rec.y, shade);
    if (P.ids) P.ids[i] = BLOK_POSE_ID | won;
}

// One lane per explicit ray: the whole pose table, no bins.
__global__ __launch_bounds__(64) void posed_rays_kernel(const PosedArgs Q) {
    extern __shared__ uint4 lds_stack[];
    const InstanceArgs& P = Q.frame;
    const TraceArgs& A = P.world;
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + lane;
    const bool active = i < A.n_rays;
    RayIn r{};
    float best = 0.0f;
    if (active) {
        const blok_ray ray = A.rays[i];
        r = RayIn{ray.org[0], ray.org[1], ray.org[2], ray.dir[0], ray.dir[1], ray.dir[2], ray.tmin, ray.tmax};
        best = best_of(*reinterpret_cast<const uint4*>(P.hits + i), ray.tmax);
    }
    uint4 rec{};
    uint32_t won, shade = 0u;
    compose_poses(Q, nullptr, Q.n_poses, active, r, best, lds_stack + lane, rec, shade, won);
    if (!active || won == kInstanceNone) return;
    *reinterpret_cast<uint4*>(P.hits + i) = rec;
    if (P.ids) P.ids[i] = BLOK_POSE_ID | won;
}

void launch_posed_bins(const PosedArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(posed_bins_kernel, dim3(args.frame.bins_x * args.frame.bins_y), dim3(64), 0, stream, args);
}

void launch_posed_pass(const PosedArgs& args, hipStream_t stream) {
    const uint32_t tiles = ((args.frame.world.w + kWaveW - 1u) / kWaveW) * ((args.frame.world.h + kWaveH - 1u) / kWaveH);
    hipLaunchKernelGGL(posed_pass_kernel, dim3(tiles), dim3(64), static_cast<size_t>(args.frame.stack_levels) * 64u * sizeof(uint4), stream, args);
}

void launch_posed_rays(const PosedArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(posed_rays_kernel, dim3((args.frame.world.n_rays + 63u) / 64u), dim3(64),
                       static_cast<size_t>(args.frame.stack_levels) * 64u * sizeof(uint4), stream, args);
}

}  // namespace blok
