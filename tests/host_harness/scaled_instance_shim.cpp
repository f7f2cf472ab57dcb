// TEST INFRASTRUCTURE: scaled models (include/blok_hip.h, "Scaled models") through the instance math and the instance BVH of the gfx950
// kernels (blok_amd/csrc/hip/instance_core.h, tlas_core.h), compiled for the CPU with the exponent settable and the world's voxel size an
// argument.  The linear loop is the primary frame's (placed_kernels.hip: compose, through instance_core.h: placed_candidate); the tree queries are the path kernel's.
// Never linked into the shipped libraries.  -DSCALED_INSTANCE_SHIM_MAIN: a stand-alone program over the same entries, for the sanitizers.
#include "tlas_shim.cpp"

namespace {
// The model store's device copy of the descriptors for a world of voxel size vs (api_instances.hip: upload_models): a model whose voxel
// size vs * 2^e is above the limit is, to the kernels, a destroyed one.
std::vector<ModelDesc> store_descs(void* const* models, size_t n_models, float vs) {
    std::vector<ModelDesc> d = descs(models, n_models);
    for (ModelDesc& m : d)
        if (!model_size_usable(m, vs)) m.nodes = nullptr;
    return d;
}
}  // namespace

extern "C" {

// What blok_hip_model_set_scale checks and does: 0 on success, -1 for an exponent above the limit (nothing changed).  The descriptor's
// box is the model's own times 2^e (the bounds at the old scale are multiples of its cell, so the division is exact).
int ss_set_scale(void* model, uint32_t scale_log2) {
    if (scale_log2 > kMaxScaleLog2) return -1;
    ModelDesc& d = static_cast<Tree*>(model)->desc;
    for (int a = 0; a < 3; ++a) {
        d.lo[a] = d.lo[a] / (1 << d.scale_log2) * (1 << scale_log2);
        d.hi[a] = d.hi[a] / (1 << d.scale_log2) * (1 << scale_log2);
    }
    d.scale_log2 = scale_log2;
    return 0;
}
uint32_t ss_scale(const void* model) { return static_cast<const Tree*>(model)->desc.scale_log2; }

// What the kernels make of an instance in a world of voxel size vs: instance_usable with the store's copy of the descriptor (the lattice
// limit on the scaled span; vs * 2^e <= 256 through the store).
int ss_usable(const blok_instance* inst, void* model, float vs) {
    void* const one[1] = {model};
    return instance_usable(*inst, store_descs(one, 1, vs)[0]) ? 1 : 0;
}

// instance_world_span on the three world axes: lo[3], hi[3].
void ss_span(const blok_instance* inst, const void* model, int64_t* lo, int64_t* hi) {
    for (uint32_t a = 0; a < 3u; ++a) instance_world_span(*inst, static_cast<const Tree*>(model)->desc, a, lo[a], hi[a]);
}

// World walk at voxel size vs (world == null: no world, every ray starts as a miss), then every instance in index order with tmax = the
// best t so far.
void ss_compose(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, float vs, const blok_ray* rays,
                size_t n, blok_hit* out, uint32_t* ids) {
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r = ray_in(rays[i]);
        if (world) trace_one(model_args(static_cast<const Tree*>(world)->desc, vs, inv_vs), r, stack.data(), Sink{out + i, nullptr});
        else std::memset(out + i, 0, sizeof(blok_hit));
        float best = out[i].hit ? out[i].t : r.tmax;
        ids[i] = kInstanceNone;
        for (uint32_t j = 0; j < n_inst; ++j) {
            if (inst[j].model >= n_models) continue;
            const ModelDesc& M = d[inst[j].model];
            if (!instance_usable(inst[j], M)) continue;
            LatticeKind::Hit hit;
            if (placed_candidate<LatticeKind>(inst[j], M, vs, inv_vs, r, best, stack.data(), hit)) {
                std::memcpy(out + i, &hit.rec, sizeof(hit.rec));
                ids[i] = j;
            }
        }
    }
}

// tlas_build_host at voxel size vs into out (ts_node_count(n) nodes).
void ss_build(void* const* models, size_t n_models, const blok_instance* inst, uint32_t n, float vs, TlasNode* out) {
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    tlas_build_host(inst, n, d.data(), static_cast<uint32_t>(n_models), out);
}

// The instances alone through the tree (tlas_closest from a miss; any[i]: tlas_any on the ray's own interval).
void ss_closest(void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, float vs, const blok_ray* rays, size_t n,
                blok_hit* out, uint32_t* ids, uint8_t* any) {
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    std::vector<TlasNode> nodes(tlas_nodes(n_inst));
    tlas_build_host(inst, n_inst, d.data(), static_cast<uint32_t>(n_models), nodes.data());
    const TlasScene S{inst, d.data(), nodes.data(), nullptr, n_inst, static_cast<uint32_t>(n_models)};
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r = ray_in(rays[i]);
        std::memset(out + i, 0, sizeof(blok_hit));
        uint4 rec;
        ids[i] = tlas_closest(S, vs, inv_vs, r, r.tmax, stack.data(), rec);
        if (ids[i] != kInstanceNone) std::memcpy(out + i, &rec, sizeof(rec));
        any[i] = tlas_any(S, vs, inv_vs, r, stack.data()) ? 1 : 0;
    }
}

}  // extern "C"

#ifdef SCALED_INSTANCE_SHIM_MAIN
#include <cstdio>
#include <cstdlib>

// Mixed exponents and all 48 orientations over seeded models, rays aimed at the instances' boxes: the linear loop and the tree must agree
// on every record and id, the spans must hold every reported voxel, and the limits must refuse what they refuse.
namespace {
uint32_t g_state = 12345u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
float unit() { return static_cast<float>(rnd() & 0xFFFFu) / 65536.0f; }
#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "scaled_instance_shim: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)
}  // namespace

int main() {
    const char* why = "";
    std::vector<void*> models;
    for (uint32_t m = 0; m < 4u; ++m) {
        std::vector<int32_t> xyz;
        std::vector<uint32_t> mats;
        for (int i = 0; i < 40 + 30 * int(m); ++i) {
            xyz.push_back(int32_t(rnd() % 9u) - 3); xyz.push_back(int32_t(rnd() % 7u) - 2); xyz.push_back(int32_t(rnd() % 5u));
            mats.push_back(1u + rnd() % 50u);
        }
        void* h = is_model(xyz.data(), mats.data(), mats.size(), &why);
        REQUIRE(h != nullptr);
        REQUIRE(ss_set_scale(h, m) == 0 && ss_scale(h) == m);
        models.push_back(h);
    }
    REQUIRE(ss_set_scale(models[0], 9u) == -1 && ss_scale(models[0]) == 0u);
    static const uint8_t perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (const float vs : {1.0f, 0.5f}) {
        std::vector<blok_instance> table;
        for (uint32_t p = 0; p < 6u; ++p)
            for (uint32_t f = 0; f < 8u; ++f) {
                blok_instance I{};
                I.model = (p * 8u + f) % 4u;
                for (int a = 0; a < 3; ++a) { I.offset[a] = int32_t(rnd() % 160u) - 80; I.axis[a] = perms[p][a]; }
                I.flip = static_cast<uint8_t>(f);
                table.push_back(I);
            }
        const uint32_t n_inst = static_cast<uint32_t>(table.size());
        std::vector<blok_ray> rays;
        for (uint32_t i = 0; i < 1500u; ++i) {
            const blok_instance& I = table[i % n_inst];
            int64_t lo[3], hi[3];
            ss_span(&I, models[I.model], lo, hi);
            blok_ray r{};
            float target[3];
            for (int a = 0; a < 3; ++a) {
                r.org[a] = (unit() * 400.0f - 200.0f) * vs;
                target[a] = (static_cast<float>(lo[a]) + unit() * static_cast<float>(hi[a] - lo[a])) * vs;
                r.dir[a] = target[a] - r.org[a];
            }
            r.tmin = 0.001f; r.tmax = 1.0e4f;
            rays.push_back(r);
        }
        std::vector<blok_hit> lin(rays.size()), tree(rays.size());
        std::vector<uint32_t> lin_ids(rays.size()), tree_ids(rays.size());
        std::vector<uint8_t> any(rays.size());
        ss_compose(nullptr, models.data(), models.size(), table.data(), n_inst, vs, rays.data(), rays.size(), lin.data(), lin_ids.data());
        ss_closest(models.data(), models.size(), table.data(), n_inst, vs, rays.data(), rays.size(), tree.data(), tree_ids.data(), any.data());
        size_t won = 0;
        for (size_t i = 0; i < rays.size(); ++i) {
            REQUIRE(lin_ids[i] == tree_ids[i] && std::memcmp(&lin[i], &tree[i], sizeof(blok_hit)) == 0);
            REQUIRE((any[i] != 0) == (lin_ids[i] != kInstanceNone));
            if (lin_ids[i] == kInstanceNone) continue;
            ++won;
            const blok_instance& I = table[lin_ids[i]];
            int64_t lo[3], hi[3];
            ss_span(&I, models[I.model], lo, hi);
            const uint32_t e = ss_scale(models[I.model]);
            for (int a = 0; a < 3; ++a) {
                const int64_t v = lin[i].voxel[a];
                REQUIRE(v >= lo[a] && v + (int64_t(1) << e) <= hi[a]);       // the cell's lowest world voxel, the whole cell inside the span
            }
        }
        REQUIRE(won > 300);
        std::vector<TlasNode> nodes(ts_node_count(n_inst));
        ss_build(models.data(), models.size(), table.data(), n_inst, vs, nodes.data());
        REQUIRE(nodes[0].escape == n_inst);                                  // every instance usable
    }
    // the limits: a span ending exactly at the lattice's end, one cell further; vs * 2^e = 256 and 512
    {
        const int32_t one[3] = {0, 0, 0};
        const uint32_t mat = 1u;
        void* h = is_model(one, &mat, 1, &why);
        REQUIRE(h != nullptr && ss_set_scale(h, 3u) == 0);
        blok_instance I{};
        I.axis[0] = 0; I.axis[1] = 1; I.axis[2] = 2;
        I.offset[0] = 32760;
        REQUIRE(ss_usable(&I, h, 1.0f) == 1);
        I.offset[0] = 32761;
        REQUIRE(ss_usable(&I, h, 1.0f) == 0);
        I.offset[0] = -32760; I.flip = 1;
        REQUIRE(ss_usable(&I, h, 1.0f) == 1);
        I.offset[0] = -32761;
        REQUIRE(ss_usable(&I, h, 1.0f) == 0);
        I.offset[0] = 0; I.flip = 0;
        REQUIRE(ss_usable(&I, h, 32.0f) == 1 && ss_usable(&I, h, 64.0f) == 0);
        is_free(h);
    }
    for (void* h : models) is_free(h);
    std::puts("scaled_instance_shim: ok");
    return 0;
}
#endif
