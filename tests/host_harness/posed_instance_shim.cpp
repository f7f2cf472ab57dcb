// TEST INFRASTRUCTURE: posed models (include/blok_hip.h, "Posed models") through the pose math of the gfx950 kernels
// (blok_amd/csrc/hip/posed_core.h) with the walk of trace_core.h, compiled for the CPU.  The loop is the posed kernels'
// (placed_kernels.hip: compose, through instance_core.h: placed_candidate) on top of the instance loop of scaled_instance_shim.cpp.  Never linked into the shipped libraries.
// -DPOSED_INSTANCE_SHIM_MAIN: a stand-alone program that replays case files written by tests/test_posed_instances_cpu.py, for the sanitizers.
#include "scaled_instance_shim.cpp"
#include "posed_core.h"

extern "C" {

// What the kernels make of a pose in a world of voxel size vs (pose_usable with the store's copy of the descriptor), and the rule that
// names what is wrong with its floats (pose_core.h: 0 = fine).
int ps_usable(const blok_pose* pose, void* model, float vs) {
    void* const one[1] = {model};
    return pose_usable(*pose, store_descs(one, 1, vs)[0]) ? 1 : 0;
}
// ... of a model whose descriptor holds the box [lo, hi) * 2^e (a tree the host build refuses to make: the device captures can reach it).
int ps_box_usable(const blok_pose* pose, const int32_t* lo, const int32_t* hi, uint32_t scale_log2) {
    static const uint4 node{};
    ModelDesc M{};
    M.nodes = &node;
    M.scale_log2 = scale_log2;
    for (int a = 0; a < 3; ++a) { M.lo[a] = lo[a] * (1 << scale_log2); M.hi[a] = hi[a] * (1 << scale_log2); }
    return pose_usable(*pose, M) ? 1 : 0;
}
int ps_floats_rule(const blok_pose* pose) { return pose::floats_rule(*pose); }

// pose_ray for n rays; ok[i] = 0 where the ray does not enter the pose.
void ps_transform(const blok_pose* pose, const blok_ray* rays, size_t n, blok_ray* out, uint8_t* ok) {
    for (size_t i = 0; i < n; ++i) {
        RayIn l{};
        ok[i] = pose_ray(*pose, ray_in(rays[i]), l) ? 1 : 0;
        out[i] = blok_ray{{l.ox, l.oy, l.oz}, l.tmin, {l.dx, l.dy, l.dz}, l.tmax};
    }
}

uint32_t ps_shade_face(const blok_pose* pose, uint32_t face) { return pose_shade_face(*pose, face); }

// pose_world_box for a camera at cam: 1 and the box, or 0 ("covers everything").
int ps_world_box(const blok_pose* pose, const void* model, float vs, const float* cam, float* lo, float* hi) {
    return pose_world_box(*pose, static_cast<const Tree*>(model)->desc, vs, cam, lo, hi) ? 1 : 0;
}

// ss_compose, then every pose in index order with tmax = the best t so far; a pose's id is BLOK_POSE_ID | index.
void ps_compose(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses,
                uint32_t n_poses, float vs, const blok_ray* rays, size_t n, blok_hit* out, uint32_t* ids) {
    ss_compose(world, models, n_models, inst, n_inst, vs, rays, n, out, ids);
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r = ray_in(rays[i]);
        float best = out[i].hit ? out[i].t : r.tmax;
        for (uint32_t j = 0; j < n_poses; ++j) {
            if (poses[j].model >= n_models) continue;
            const ModelDesc& M = d[poses[j].model];
            if (!pose_usable(poses[j], M)) continue;
            PoseKind::Hit hit;
            if (placed_candidate<PoseKind>(poses[j], M, vs, inv_vs, r, best, stack.data(), hit)) {
                std::memcpy(out + i, &hit.rec, sizeof(hit.rec));
                ids[i] = PoseKind::id_tag | j;
            }
        }
    }
}

}  // extern "C"

#ifdef POSED_INSTANCE_SHIM_MAIN
#include <cstdio>
#include <cstdlib>

// Each argument is a case file (little endian, written by the test):
//   u32 n_models, per model {u32 n_voxels, u32 exponent, i32 xyz[3 n], u32 materials[n]},
//   f32 vs, u32 n_world_voxels, i32 xyz[3 n], u32 materials[n] (0: no world; the world's tree is built from its voxel list),
//   u32 n_instances, blok_instance[], u32 n_poses, blok_pose[], u32 n_rays, blok_ray[], blok_hit[n_rays], u32 ids[n_rays]
// The composition is replayed and must reproduce the recorded records and ids; every pose goes through pose_usable, pose_world_box and
// pose_shade_face on the way.
namespace {
#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "posed_instance_shim: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)

struct Reader {
    std::vector<unsigned char> bytes;
    size_t at = 0;
    bool ok = true;
    template <class T> T one() { T v{}; read(&v, 1); return v; }
    template <class T> void read(T* out, size_t n) {
        if (n > (bytes.size() - at) / sizeof(T)) { ok = false; return; }
        if (n) std::memcpy(out, bytes.data() + at, n * sizeof(T));
        at += n * sizeof(T);
    }
};

int replay(const char* path) {
    Reader R;
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    unsigned char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) R.bytes.insert(R.bytes.end(), buf, buf + got);
    std::fclose(f);
    const char* why = "";
    std::vector<void*> models;
    const uint32_t n_models = R.one<uint32_t>();
    REQUIRE(R.ok && n_models <= 64u);
    for (uint32_t m = 0; m < n_models; ++m) {
        const uint32_t n = R.one<uint32_t>(), e = R.one<uint32_t>();
        REQUIRE(R.ok && n >= 1u && n <= (1u << 20));
        std::vector<int32_t> xyz(size_t(n) * 3u);
        std::vector<uint32_t> mats(n);
        R.read(xyz.data(), xyz.size()); R.read(mats.data(), mats.size());
        REQUIRE(R.ok);
        void* h = is_model(xyz.data(), mats.data(), n, &why);
        REQUIRE(h != nullptr && ss_set_scale(h, e) == 0);
        models.push_back(h);
    }
    const float vs = R.one<float>();
    const uint32_t n_world = R.one<uint32_t>();
    REQUIRE(R.ok && n_world <= (1u << 22));
    std::vector<int32_t> world_xyz(size_t(n_world) * 3u);
    std::vector<uint32_t> world_mats(n_world);
    R.read(world_xyz.data(), world_xyz.size()); R.read(world_mats.data(), world_mats.size());
    void* world = n_world ? is_model(world_xyz.data(), world_mats.data(), n_world, &why) : nullptr;
    REQUIRE(R.ok && (world != nullptr) == (n_world != 0u));
    const uint32_t n_inst = R.one<uint32_t>();
    REQUIRE(R.ok && n_inst <= (1u << 20));
    std::vector<blok_instance> inst(n_inst);
    R.read(inst.data(), inst.size());
    const uint32_t n_poses = R.one<uint32_t>();
    REQUIRE(R.ok && n_poses <= (1u << 20));
    std::vector<blok_pose> poses(n_poses);
    R.read(poses.data(), poses.size());
    const uint32_t n_rays = R.one<uint32_t>();
    REQUIRE(R.ok && n_rays <= (1u << 24));
    std::vector<blok_ray> rays(n_rays);
    std::vector<blok_hit> want(n_rays), got(n_rays);
    std::vector<uint32_t> want_ids(n_rays), ids(n_rays);
    R.read(rays.data(), rays.size()); R.read(want.data(), want.size()); R.read(want_ids.data(), want_ids.size());
    REQUIRE(R.ok && R.at == R.bytes.size());
    ps_compose(world, models.data(), models.size(), inst.data(), n_inst, poses.data(), n_poses, vs, rays.data(), rays.size(), got.data(), ids.data());
    size_t won = 0;
    for (uint32_t i = 0; i < n_rays; ++i) {
        REQUIRE(ids[i] == want_ids[i] && std::memcmp(&got[i], &want[i], sizeof(blok_hit)) == 0);
        if (ids[i] != kInstanceNone && (ids[i] & BLOK_POSE_ID)) {
            ++won;
            const blok_pose& S = poses[ids[i] & 0x7FFFFFFFu];
            const ModelDesc& M = static_cast<const Tree*>(models[S.model])->desc;
            for (int a = 0; a < 3; ++a) {                          // the record's voxel is the model's own
                const int64_t v = got[i].voxel[a];
                REQUIRE(v >= (M.lo[a] >> M.scale_log2) && v < (M.hi[a] >> M.scale_log2));
            }
            REQUIRE(got[i].face < 6u && pose_shade_face(S, got[i].face) < 6u);
        }
    }
    const float cam[3] = {rays.empty() ? 0.0f : rays[0].org[0], rays.empty() ? 0.0f : rays[0].org[1], rays.empty() ? 0.0f : rays[0].org[2]};
    for (const blok_pose& S : poses) {
        if (S.model >= models.size() || !ps_usable(&S, models[S.model], vs)) continue;
        float lo[3], hi[3];
        if (ps_world_box(&S, models[S.model], vs, cam, lo, hi)) REQUIRE(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]);
    }
    std::printf("posed_instance_shim: %s: %u rays, %zu won by poses\n", path, n_rays, won);
    if (world) is_free(world);
    for (void* h : models) is_free(h);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (const int rc = replay(argv[i])) return rc;
    // the limits: each float non-finite, each magnitude bound
    blok_pose S{};
    S.m[0][0] = S.m[1][1] = S.m[2][2] = 1.0f;
    REQUIRE(ps_floats_rule(&S) == 0);
    float* words = &S.m[0][0];
    for (int w = 0; w < 15; ++w) {
        const float keep = words[w];
        words[w] = __builtin_nanf(""); REQUIRE(ps_floats_rule(&S) == pose::kNotFinite);
        words[w] = __builtin_inff(); REQUIRE(ps_floats_rule(&S) == pose::kNotFinite);
        const float bound = w < 9 ? 1024.0f : 1048576.0f;
        words[w] = bound; REQUIRE(ps_floats_rule(&S) == 0);
        words[w] = -__builtin_nextafterf(bound, 2.0f * bound); REQUIRE(ps_floats_rule(&S) == (w < 9 ? pose::kMatrix : (w < 12 ? pose::kPivot : pose::kLocal)));
        words[w] = keep;
    }
    std::puts("posed_instance_shim: ok");
    return 0;
}
#endif
