// TEST INFRASTRUCTURE: the instance math of the gfx950 kernels (blok_amd/csrc/hip/instance_core.h) with the walk of trace_core.h,
// compiled for the CPU: one ray at a time, world first, then every instance in order through the kernels' candidate (placed_candidate).  Never linked into the shipped libraries.
#define BLOK_TRACE_HOST_HARNESS 1
#include "instance_core.h"
#include "reference_world.h"

#include <cstring>
#include <vector>

using namespace blok;

namespace {
struct Tree {
    HostTree tree;
    std::vector<uint4> nodes;
    ModelDesc desc{};
};

Tree* finish(std::vector<VoxelRec>& voxels, const char** why) {
    auto* t = new Tree();
    if (!build_tree(voxels, t->tree, why)) { delete t; return nullptr; }
    t->nodes.resize(t->tree.nodes.size());
    std::memcpy(t->nodes.data(), t->tree.nodes.data(), t->nodes.size() * sizeof(uint4));
    t->desc.nodes = t->nodes.data();
    t->desc.materials = t->tree.materials.data();
    t->desc.levels = t->tree.levels;
    for (int a = 0; a < 3; ++a) { t->desc.origin[a] = t->tree.origin[a]; t->desc.lo[a] = INT32_MAX; t->desc.hi[a] = INT32_MIN; }
    for (const VoxelRec& v : voxels) {
        const int32_t c[3] = {v.x, v.y, v.z};
        for (int a = 0; a < 3; ++a) { t->desc.lo[a] = std::min(t->desc.lo[a], c[a]); t->desc.hi[a] = std::max(t->desc.hi[a], c[a] + 1); }
    }
    return t;
}
}  // namespace

extern "C" {

void* is_world(const blok_svo_node* nodes, size_t n_nodes, const blok_sub_chunk* subs, size_t n_subs, const char** why) {
    std::vector<VoxelRec> voxels;
    if (!extract_voxels(nodes, n_nodes, subs, n_subs, voxels, why)) return nullptr;
    return finish(voxels, why);
}

void* is_model(const int32_t* xyz, const uint32_t* mats, size_t n, const char** why) {
    std::vector<VoxelRec> voxels(n);
    for (size_t i = 0; i < n; ++i) voxels[i] = VoxelRec{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], mats[i]};
    return finish(voxels, why);
}

void is_free(void* t) { delete static_cast<Tree*>(t); }

// instance_ray for n rays
void is_transform(const blok_instance* inst, float vs, const blok_ray* rays, size_t n, blok_ray* out) {
    for (size_t i = 0; i < n; ++i) {
        const RayIn r{rays[i].org[0], rays[i].org[1], rays[i].org[2], rays[i].dir[0], rays[i].dir[1], rays[i].dir[2], rays[i].tmin, rays[i].tmax};
        const RayIn l = instance_ray(*inst, vs, r);
        out[i] = blok_ray{{l.ox, l.oy, l.oz}, l.tmin, {l.dx, l.dy, l.dz}, l.tmax};
    }
}

// instance_record of local hits (t, material, voxel, face of each record; all are hits)
void is_map_back(const blok_instance* inst, const blok_hit* local, size_t n, blok_hit* out) {
    for (size_t i = 0; i < n; ++i) {
        HitInfo h{};
        h.found = true; h.t = local[i].t; h.material = local[i].material_id; h.face = local[i].face;
        h.vx = local[i].voxel[0]; h.vy = local[i].voxel[1]; h.vz = local[i].voxel[2];
        const uint4 rec = instance_record(*inst, h);
        std::memcpy(out + i, &rec, sizeof(rec));
    }
}

int is_usable(const blok_instance* inst, const void* model) {
    return instance_usable(*inst, static_cast<const Tree*>(model)->desc) ? 1 : 0;
}

// World walk, then every instance with tmax = the best t so far (the kernels' composition).  models[i]: the tree of model id i.
void is_compose(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_ray* rays,
                size_t n, blok_hit* out, uint32_t* ids) {
    const Tree* W = static_cast<const Tree*>(world);
    const TraceArgs wa = model_args(W->desc, 1.0f, 1.0f);
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r{rays[i].org[0], rays[i].org[1], rays[i].org[2], rays[i].dir[0], rays[i].dir[1], rays[i].dir[2], rays[i].tmin, rays[i].tmax};
        trace_one(wa, r, stack.data(), Sink{out + i, nullptr});
        float best = out[i].hit ? out[i].t : r.tmax;
        ids[i] = kInstanceNone;
        for (uint32_t j = 0; j < n_inst; ++j) {
            if (inst[j].model >= n_models) continue;
            const ModelDesc& M = static_cast<const Tree*>(models[inst[j].model])->desc;
            if (!instance_usable(inst[j], M)) continue;
            LatticeKind::Hit hit;
            if (placed_candidate<LatticeKind>(inst[j], M, 1.0f, 1.0f, r, best, stack.data(), hit)) {
                std::memcpy(out + i, &hit.rec, sizeof(hit.rec));
                ids[i] = j;
            }
        }
    }
}

}  // extern "C"
