// gfx950 kernels of the instanced primary frame and rays (instance_core.h has the semantics and the per-ray math).  They run after the
// world pass on its stream and compose its records with the instances' in place.
#include "instance_core.h"
#include "volume_device.h"      // uniform_record, uniform_word

namespace blok {

namespace {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// The loop every lane of a wave runs over its candidate instances (uniform across the wave): list[0 .. n) or, list == null, every
// instance.  `active`: the lane has a ray.  Leaves the composed record in rec (if won != kInstanceNone) and the winner in won.
__device__ __forceinline__ void compose_instances(const InstanceArgs& P, const uint32_t* list, uint32_t n, bool active, const RayIn& r,
                                                  float best, uint4* stk, uint4& rec, uint32_t& won) {
    const float vs = P.world.voxel_size, inv_vs = P.world.inv_voxel_size;
    won = kInstanceNone;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t idx = list ? uniform_word(list, j) : j;
        const blok_instance I = uniform_record(P.instances, idx);
        if (I.model >= P.n_models) continue;
        const ModelDesc M = uniform_record(P.models, I.model);
        if (!instance_usable(I, M)) continue;
        RayIn l = instance_ray(I, vs, r);
        l.tmax = best;
        const bool enters = active && instance_box_entered(M, vs, l);
        if (__ballot(enters) == 0ull) continue;        // no lane of the wave enters the model's box
        if (enters) {
            const HitInfo h = walk(model_args(M, vs, inv_vs), l, stk);
            if (h.found) { rec = instance_record(I, h, M.scale_log2); best = h.t; won = idx; }
        }
    }
}

__device__ __forceinline__ float best_of(const uint4& w, float tmax) {
    return ((w.w >> 24) & 1u) ? __uint_as_float(w.x) : tmax;
}

}  // namespace

// One wave per bin: the instances whose world box may cover the bin, in ascending index order (ballot + mbcnt ranks, no atomics).
__global__ __launch_bounds__(64) void instance_bins_kernel(const InstanceArgs P) {
    const TraceArgs& A = P.world;
    const uint32_t lane = threadIdx.x, bin = blockIdx.x;
    const uint32_t bxi = bin % P.bins_x, byi = bin / P.bins_x;
    // the bin's pixels, frame coordinates, inclusive
    const float px0 = static_cast<float>(A.x0 + bxi * kBinPixels), py0 = static_cast<float>(A.y0 + byi * kBinPixels);
    const float px1 = static_cast<float>(A.x0 + min((bxi + 1u) * kBinPixels, A.w) - 1u), py1 = static_cast<float>(A.y0 + min((byi + 1u) * kBinPixels, A.h) - 1u);
    const float vs = A.voxel_size;
    uint32_t* list = P.bins + static_cast<size_t>(bin) * kBinWords;
    uint32_t count = 0;
    for (uint32_t base = 0; base < P.n_instances; base += 64u) {
        const uint32_t idx = base + lane;
        bool cover = false;
        if (idx < P.n_instances) {
            const blok_instance I = P.instances[idx];
            if (I.model < P.n_models) {
                const ModelDesc M = P.models[I.model];
                if (instance_usable(I, M)) {
                    float flo[3], fhi[3];
                    for (uint32_t a = 0; a < 3u; ++a) {
                        int64_t lo, hi;
                        instance_world_span(I, M, a, lo, hi);
                        flo[a] = static_cast<float>(lo) * vs; fhi[a] = static_cast<float>(hi) * vs;
                    }
                    float x0, y0, x1, y1;
                    cover = !P.view.usable || !project_box(P.view, flo, fhi, x0, y0, x1, y1) ||
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

// One wave per 8x8 pixel tile of the rectangle (the walk's footprint): the pixel's world record, then the bin's instances.
__global__ __launch_bounds__(64) void instance_pass_kernel(const InstanceArgs P) {
    extern __shared__ uint4 lds_stack[];       // [stack_levels][64], as the world walk's
    const TraceArgs& A = P.world;
    const uint32_t lane = threadIdx.x;
    const uint32_t tiles_x = (A.w + kWaveW - 1u) / kWaveW;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t lx = tx * kWaveW + lane % kWaveW, ly = ty * kWaveH + lane / kWaveW;
    const bool inside = lx < A.w && ly < A.h;
    const size_t i = static_cast<size_t>(ly) * A.w + lx;
    const uint32_t* bin = P.bins + static_cast<size_t>((ty * kWaveH / kBinPixels) * P.bins_x + tx * kWaveW / kBinPixels) * kBinWords;
    const uint32_t head = uniform_word(bin, 0u);
    if (head == 0u) {
        if (P.ids && inside) P.ids[i] = kInstanceNone;
        return;
    }
    RayIn r{};
    float best = A.tmax;
    if (inside) {
        best = best_of(*reinterpret_cast<const uint4*>(P.hits + i), A.tmax);
        r = primary_ray(A, A.x0 + lx, A.y0 + ly);
    }
    uint4 rec{};
    uint32_t won;
    if (head == kBinOverflow) compose_instances(P, nullptr, P.n_instances, inside, r, best, lds_stack + lane, rec, won);
    else compose_instances(P, bin + 1, head, inside, r, best, lds_stack + lane, rec, won);
    if (!inside) return;
    if (won != kInstanceNone) {
        *reinterpret_cast<uint4*>(P.hits + i) = rec;
        if (P.rgba) P.rgba[i] = shade_rgba(A.mat_table, A.n_materials, rec.y, (rec.w >> 16) & 0xFFu);
    }
    if (P.ids) P.ids[i] = won;
}

// One lane per explicit ray: the whole instance table, no bins.
__global__ __launch_bounds__(64) void instance_rays_kernel(const InstanceArgs P) {
    extern __shared__ uint4 lds_stack[];
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
    uint32_t won;
    compose_instances(P, nullptr, P.n_instances, active, r, best, lds_stack + lane, rec, won);
    if (!active) return;
    if (won != kInstanceNone) *reinterpret_cast<uint4*>(P.hits + i) = rec;
    if (P.ids) P.ids[i] = won;
}

void launch_instance_bins(const InstanceArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(instance_bins_kernel, dim3(args.bins_x * args.bins_y), dim3(64), 0, stream, args);
}

void launch_instance_pass(const InstanceArgs& args, hipStream_t stream) {
    const uint32_t tiles = ((args.world.w + kWaveW - 1u) / kWaveW) * ((args.world.h + kWaveH - 1u) / kWaveH);
    hipLaunchKernelGGL(instance_pass_kernel, dim3(tiles), dim3(64), static_cast<size_t>(args.stack_levels) * 64u * sizeof(uint4), stream, args);
}

void launch_instance_rays(const InstanceArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(instance_rays_kernel, dim3((args.world.n_rays + 63u) / 64u), dim3(64), static_cast<size_t>(args.stack_levels) * 64u * sizeof(uint4),
                       stream, args);
}

}  // namespace blok
