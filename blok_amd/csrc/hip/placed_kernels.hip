// gfx950 kernels of placed models on the primary frame and on explicit rays: the lattice instances, then the poses, each a bins, a pass and
// a rays kernel over one body (instance_core.h: what a kind is; it and posed_core.h have the kinds, the semantics and the per-ray math).
// They run after the world pass on its stream and compose its records with theirs in place.
#include "posed_core.h"
#include "volume_device.h"      // uniform_record, uniform_word

namespace blok {

namespace {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

__device__ __forceinline__ float best_of(const uint4& w, float tmax) {
    return ((w.w >> 24) & 1u) ? __uint_as_float(w.x) : tmax;
}

// The loop every lane of a wave runs over its candidate records (uniform across the wave): list[0 .. n) or, list == null, every record.
// The record and the 64-byte descriptor come through the scalar cache, one load each: they are scalar operands of the lane's ray
// transform.  `active`: the lane has a ray.  Leaves the composed record and the face to shade it by in hit (if won != kInstanceNone)
// and the winner's index in won.
template <class K>
__device__ __forceinline__ void compose(const typename K::Args& Q, const uint32_t* list, uint32_t n, bool active, const RayIn& r, float best,
                                        uint4* stk, typename K::Hit& hit, uint32_t& won) {
    const InstanceArgs& P = K::frame(Q);
    const float vs = P.world.voxel_size, inv_vs = P.world.inv_voxel_size;
    won = kInstanceNone;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t idx = list ? uniform_word(list, j) : j;
        const typename K::Record S = uniform_record(K::table(Q), idx);
        if (S.model >= P.n_models) continue;
        const ModelDesc M = uniform_record(P.models, S.model);
        if (!K::usable(S, M)) continue;
        RayIn l;
        const bool finite = K::local_ray(S, vs, r, l);
        l.tmax = best;
        const bool enters = active && finite && instance_box_entered(M, vs, l);
        if (__ballot(enters) == 0ull) continue;        // no lane of the wave enters the model's box
        if (enters) {
            const HitInfo h = walk(model_args(M, vs, inv_vs), l, stk);
            if (h.found) { hit = K::record(S, M, h); best = h.t; won = idx; }
        }
    }
}

// One wave per bin: the records whose world box may cover the bin, in ascending index order (ballot + mbcnt ranks, no atomics).
template <class K>
__device__ __forceinline__ void bins(const typename K::Args& Q) {
    const InstanceArgs& P = K::frame(Q);
    const TraceArgs& A = P.world;
    const uint32_t lane = threadIdx.x, bin = blockIdx.x;
    const uint32_t bxi = bin % P.bins_x, byi = bin / P.bins_x;
    // the bin's pixels, frame coordinates, inclusive
    const float px0 = static_cast<float>(A.x0 + bxi * kBinPixels), py0 = static_cast<float>(A.y0 + byi * kBinPixels);
    const float px1 = static_cast<float>(A.x0 + min((bxi + 1u) * kBinPixels, A.w) - 1u), py1 = static_cast<float>(A.y0 + min((byi + 1u) * kBinPixels, A.h) - 1u);
    uint32_t* list = P.bins + static_cast<size_t>(bin) * kBinWords;
    uint32_t count = 0;
    for (uint32_t base = 0; base < K::count(Q); base += 64u) {
        const uint32_t idx = base + lane;
        bool cover = false;
        if (idx < K::count(Q)) {
            const typename K::Record S = K::table(Q)[idx];
            if (S.model < P.n_models) {
                const ModelDesc M = P.models[S.model];
                if (K::usable(S, M)) {
                    float flo[3], fhi[3];
                    float x0, y0, x1, y1;
                    cover = !P.view.usable || !K::world_box(S, M, A.voxel_size, P.view.pos, flo, fhi) || !project_box(P.view, flo, fhi, x0, y0, x1, y1) ||
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

// One wave per 8x8 pixel tile of the rectangle (the walk's footprint): the pixel's composed record so far, then the bin's records.
template <class K>
__device__ __forceinline__ void pass(const typename K::Args& Q, uint4* lds_stack) {
    const InstanceArgs& P = K::frame(Q);
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
        if (K::owns_ids && P.ids && inside) P.ids[i] = kInstanceNone;
        return;
    }
    RayIn r{};
    float best = A.tmax;
    if (inside) {
        best = best_of(*reinterpret_cast<const uint4*>(P.hits + i), A.tmax);
        r = primary_ray(A, A.x0 + lx, A.y0 + ly);
    }
    typename K::Hit hit;
    uint32_t won;
    if (head == kBinOverflow) compose<K>(Q, nullptr, K::count(Q), inside, r, best, lds_stack + lane, hit, won);
    else compose<K>(Q, bin + 1, head, inside, r, best, lds_stack + lane, hit, won);
    if (!inside || (!K::owns_ids && won == kInstanceNone)) return;
    if (won != kInstanceNone) {
        *reinterpret_cast<uint4*>(P.hits + i) = hit.rec;
        if (P.rgba) P.rgba[i] = shade_rgba(A.mat_table, A.n_materials, hit.rec.y, hit.shade_face());
    }
    if (P.ids) P.ids[i] = K::id_tag | won;
}

// One lane per explicit ray: the whole table, no bins.
template <class K>
__device__ __forceinline__ void rays(const typename K::Args& Q, uint4* lds_stack) {
    const InstanceArgs& P = K::frame(Q);
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
    typename K::Hit hit;
    uint32_t won;
    compose<K>(Q, nullptr, K::count(Q), active, r, best, lds_stack + lane, hit, won);
    if (!active || (!K::owns_ids && won == kInstanceNone)) return;
    if (won != kInstanceNone) *reinterpret_cast<uint4*>(P.hits + i) = hit.rec;
    if (P.ids) P.ids[i] = K::id_tag | won;
}

// The launch geometry: a wave per bin; a wave per 8x8 tile or per 64 rays with the walk's LDS stack, [stack_levels][64].
dim3 bins_grid(const InstanceArgs& f) { return dim3(f.bins_x * f.bins_y); }
dim3 pass_grid(const InstanceArgs& f) { return dim3(((f.world.w + kWaveW - 1u) / kWaveW) * ((f.world.h + kWaveH - 1u) / kWaveH)); }
dim3 rays_grid(const InstanceArgs& f) { return dim3((f.world.n_rays + 63u) / 64u); }
size_t stack_bytes(const InstanceArgs& f) { return static_cast<size_t>(f.stack_levels) * 64u * sizeof(uint4); }

}  // namespace

__global__ __launch_bounds__(64) void instance_bins_kernel(const InstanceArgs P) { bins<LatticeKind>(P); }
__global__ __launch_bounds__(64) void instance_pass_kernel(const InstanceArgs P) {
    extern __shared__ uint4 lds_stack[];
    pass<LatticeKind>(P, lds_stack);
}
__global__ __launch_bounds__(64) void instance_rays_kernel(const InstanceArgs P) {
    extern __shared__ uint4 lds_stack[];
    rays<LatticeKind>(P, lds_stack);
}
__global__ __launch_bounds__(64) void posed_bins_kernel(const PosedArgs Q) { bins<PoseKind>(Q); }
__global__ __launch_bounds__(64) void posed_pass_kernel(const PosedArgs Q) {
    extern __shared__ uint4 lds_stack[];
    pass<PoseKind>(Q, lds_stack);
}
__global__ __launch_bounds__(64) void posed_rays_kernel(const PosedArgs Q) {
    extern __shared__ uint4 lds_stack[];
    rays<PoseKind>(Q, lds_stack);
}

void launch_instance_bins(const InstanceArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(instance_bins_kernel, bins_grid(args), dim3(64), 0, stream, args);
}
void launch_instance_pass(const InstanceArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(instance_pass_kernel, pass_grid(args), dim3(64), stack_bytes(args), stream, args);
}
void launch_instance_rays(const InstanceArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(instance_rays_kernel, rays_grid(args), dim3(64), stack_bytes(args), stream, args);
}
void launch_posed_bins(const PosedArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(posed_bins_kernel, bins_grid(args.frame), dim3(64), 0, stream, args);
}
void launch_posed_pass(const PosedArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(posed_pass_kernel, pass_grid(args.frame), dim3(64), stack_bytes(args.frame), stream, args);
}
void launch_posed_rays(const PosedArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(posed_rays_kernel, rays_grid(args.frame), dim3(64), stack_bytes(args.frame), stream, args);
}

}  // namespace blok
