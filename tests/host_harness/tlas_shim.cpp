// TEST INFRASTRUCTURE: the instance BVH of the instanced path frame (blok_amd/csrc/hip/tlas_core.h) compiled for the CPU: the serial build
// and the stackless queries, next to the linear composition of instance_shim.cpp.  Never linked into the shipped libraries.
#include "instance_shim.cpp"
#include "tlas_core.h"

namespace {
// The model store as the kernels see it; a null handle is a destroyed model.
std::vector<ModelDesc> descs(void* const* models, size_t n_models) {
    std::vector<ModelDesc> d(n_models);
    for (size_t i = 0; i < n_models; ++i) d[i] = models[i] ? static_cast<const Tree*>(models[i])->desc : ModelDesc{};
    return d;
}
RayIn ray_in(const blok_ray& r) { return RayIn{r.org[0], r.org[1], r.org[2], r.dir[0], r.dir[1], r.dir[2], r.tmin, r.tmax}; }
}  // namespace

extern "C" {

uint32_t ts_max() { return kTlasMax; }
uint32_t ts_node_count(uint32_t n) { return tlas_nodes(n); }

// tlas_build_host into out (ts_node_count(n) nodes).
void ts_build(void* const* models, size_t n_models, const blok_instance* inst, uint32_t n, TlasNode* out) {
    const std::vector<ModelDesc> d = descs(models, n_models);
    tlas_build_host(inst, n, d.data(), static_cast<uint32_t>(n_models), out);
}

// World walk, then the instances through the tree (linear = 1: the loop in index order, skipping destroyed models, as tlas_closest does
// above kTlasMax).  any[i]: tlas_any over the instances alone on the ray's own interval; alone[i]: tlas_closest over the instances alone found one.
void ts_compose(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_ray* rays,
                size_t n, int linear, blok_hit* out, uint32_t* ids, uint8_t* any, uint8_t* alone) {
    const Tree* W = static_cast<const Tree*>(world);
    const TraceArgs wa = model_args(W->desc, 1.0f, 1.0f);
    const std::vector<ModelDesc> d = descs(models, n_models);
    std::vector<TlasNode> nodes;
    if (!linear && n_inst <= kTlasMax) {
        nodes.resize(tlas_nodes(n_inst));
        tlas_build_host(inst, n_inst, d.data(), static_cast<uint32_t>(n_models), nodes.data());
    }
    const TlasScene S{inst, d.data(), nodes.empty() ? nullptr : nodes.data(), nullptr, n_inst, static_cast<uint32_t>(n_models)};
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r = ray_in(rays[i]);
        trace_one(wa, r, stack.data(), Sink{out + i, nullptr});
        uint4 rec;
        ids[i] = tlas_closest(S, 1.0f, 1.0f, r, out[i].hit ? out[i].t : r.tmax, stack.data(), rec);
        if (ids[i] != kInstanceNone) std::memcpy(out + i, &rec, sizeof(rec));
        any[i] = tlas_any(S, 1.0f, 1.0f, r, stack.data()) ? 1 : 0;
        alone[i] = tlas_closest(S, 1.0f, 1.0f, r, r.tmax, stack.data(), rec) != kInstanceNone ? 1 : 0;
    }
}

}  // extern "C"
