// TEST INFRASTRUCTURE: what the posed path kernel adds to the instanced one (blok_amd/csrc/hip/posed_paths_core.h, path_core.h), compiled for
// the CPU on top of posed_instance_shim.cpp: the normal of a posed hit, the sampling frame of any unit normal, and the path loop's pose
// queries (closest with tmax = the best t so far, any hit) with the per-lane candidate.  Never linked into the shipped libraries.
// -DPOSED_PATHS_SHIM_MAIN: a stand-alone program that replays the case files of tests/test_posed_paths_cpu.py, for the sanitizers.
#include "posed_instance_shim.cpp"
#include "path_core.h"

extern "C" {

// pose_world_normal for the six local faces: out[face][3].
void pp_normals(const blok_pose* pose, float* out) {
    for (uint32_t f = 0; f < 6u; ++f) pose_world_normal(*pose, f, out[3 * f], out[3 * f + 1], out[3 * f + 2]);
}

// The sampling frame of normal n: general != 0: tangent_frame_of_normal (the posed kernel's), else tangent_frame_of_face.  out: tangent, bitangent.
void pp_tangent_frame(const float* n, int general, float* out) {
    V3 t, b;
    if (general) tangent_frame_of_normal(v3(n[0], n[1], n[2]), t, b);
    else tangent_frame_of_face(v3(n[0], n[1], n[2]), t, b);
    out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = b.x; out[4] = b.y; out[5] = b.z;
}

// The path loop's composition of n rays: ss_compose (world, then instances), then poses_closest with tmax = the composed t so far (out, ids as
// ps_compose's), and for any[i] the shadow rule: 1 iff the world or an instance reports a voxel in [tmin, tmax), else poses_any's answer.
void pp_compose(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses,
                uint32_t n_poses, float vs, const blok_ray* rays, size_t n, blok_hit* out, uint32_t* ids, uint8_t* any) {
    ss_compose(world, models, n_models, inst, n_inst, vs, rays, n, out, ids);
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    const PoseScene S{poses, n_poses};
    for (size_t i = 0; i < n; ++i) {
        const RayIn r = ray_in(rays[i]);
        any[i] = out[i].hit ? 1 : (poses_any(S, d.data(), static_cast<uint32_t>(n_models), vs, inv_vs, r, stack.data()) ? 1 : 0);
        uint4 rec{};
        const uint32_t won = poses_closest(S, d.data(), static_cast<uint32_t>(n_models), vs, inv_vs, r, out[i].hit ? out[i].t : r.tmax, stack.data(), rec);
        if (won != kInstanceNone) { std::memcpy(out + i, &rec, sizeof(rec)); ids[i] = BLOK_POSE_ID | won; }
    }
}

}  // extern "C"

#ifdef POSED_PATHS_SHIM_MAIN
// Each argument is a case file of posed_instance_shim.cpp's layout.  The path loop's composition is replayed and must reproduce the recorded
// records and ids (those of the primary frame's composition: the same rule); every pose's six normals must be unit vectors or axis normals, and
// the general sampling frame must equal the face frame on the six axis normals.
#include <cstdio>
#include <cstdlib>

namespace {
#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "posed_paths_shim: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)

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
}  // namespace

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        Reader R;
        FILE* f = std::fopen(argv[a], "rb");
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
        std::vector<uint8_t> any(n_rays);
        R.read(rays.data(), rays.size()); R.read(want.data(), want.size()); R.read(want_ids.data(), want_ids.size());
        REQUIRE(R.ok && R.at == R.bytes.size());
        pp_compose(world, models.data(), models.size(), inst.data(), n_inst, poses.data(), n_poses, vs, rays.data(), rays.size(), got.data(), ids.data(),
                   any.data());
        for (uint32_t i = 0; i < n_rays; ++i) REQUIRE(ids[i] == want_ids[i] && std::memcmp(&got[i], &want[i], sizeof(blok_hit)) == 0 && any[i] == want[i].hit);
        for (const blok_pose& S : poses) {
            float n[18];
            pp_normals(&S, n);
            for (int k = 0; k < 6; ++k) {
                const float q = n[3 * k] * n[3 * k] + n[3 * k + 1] * n[3 * k + 1] + n[3 * k + 2] * n[3 * k + 2];
                REQUIRE(q > 0.999f && q < 1.001f);
            }
        }
        std::printf("posed_paths_shim: %s: %u rays\n", argv[a], n_rays);
        if (world) is_free(world);
        for (void* h : models) is_free(h);
    }
    for (uint32_t f = 0; f < 6u; ++f) {
        float n[3], a[6], b[6];
        axis_normal(f, n[0], n[1], n[2]);
        pp_tangent_frame(n, 1, a); pp_tangent_frame(n, 0, b);
        REQUIRE(std::memcmp(a, b, sizeof(a)) == 0);
    }
    std::puts("posed_paths_shim: ok");
    return 0;
}
#endif
