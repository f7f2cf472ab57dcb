// TEST INFRASTRUCTURE: the pose BVH of the posed path frame (blok_amd/csrc/hip/pose_tlas_core.h, posed_paths_core.h) compiled for the CPU on
// top of posed_paths_shim.cpp: the serial build, the leaf boxes, and the path loop's pose queries through the tree next to the linear loop.
// Never linked into the shipped libraries.
// -DPOSE_TLAS_SHIM_MAIN: a stand-alone program that replays the case files of tests/test_posed_paths_cpu.py through tree and loop, for the sanitizers.
#include "posed_paths_shim.cpp"

extern "C" {

uint32_t pt_max() { return kTlasMax; }
uint32_t pt_node_count(uint32_t n) { return tlas_nodes(n); }

// pose_tlas_build_host into out (pt_node_count(n) nodes).
void pt_build(void* const* models, size_t n_models, const blok_pose* poses, uint32_t n, float vs, const float* cam, TlasNode* out) {
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    pose_tlas_build_host(poses, n, d.data(), static_cast<uint32_t>(n_models), vs, cam, out);
}

// The origin box of a launch (6 doubles: lo, hi) and every pose's leaf box before the int rounding (kind[i]: PoseLeafKind; box[6 i ..]: flo, fhi).
void pt_boxes(void* const* models, size_t n_models, const blok_pose* poses, uint32_t n, float vs, const float* cam, double* origin, uint32_t* kind, double* box) {
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    PoseBoxD U = pose_box_empty();
    for (uint32_t i = 0; i < n; ++i) {
        PoseBoxD b;
        if (poses[i].model < n_models && pose_usable(poses[i], d[poses[i].model]) && pose_preimage_box(poses[i], d[poses[i].model], vs, b)) pose_box_join(U, b);
    }
    const PoseOrigins O = pose_origin_box(U, cam, vs);
    for (int a = 0; a < 3; ++a) { origin[a] = O.box.lo[a]; origin[3 + a] = O.box.hi[a]; }
    for (uint32_t i = 0; i < n; ++i) {
        kind[i] = kPoseLeafSkipped;
        if (poses[i].model >= n_models || !pose_usable(poses[i], d[poses[i].model])) continue;
        kind[i] = pose_world_box_from(poses[i], d[poses[i].model], vs, O, box + 6 * i, box + 6 * i + 3) ? kPoseLeafBoxed : kPoseLeafUnbounded;
    }
}

// pp_compose with the pose queries through the tree built for a camera at cam (tree = 0: the linear loop; more than kTlasMax poses: the loop).
void pt_compose(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses,
                uint32_t n_poses, float vs, const float* cam, int tree, const blok_ray* rays, size_t n, blok_hit* out, uint32_t* ids, uint8_t* any) {
    ss_compose(world, models, n_models, inst, n_inst, vs, rays, n, out, ids);
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    std::vector<TlasNode> nodes;
    if (tree && n_poses >= 1u && n_poses <= kTlasMax) {
        nodes.resize(tlas_nodes(n_poses));
        pose_tlas_build_host(poses, n_poses, d.data(), static_cast<uint32_t>(n_models), vs, cam, nodes.data());
    }
    std::vector<uint4> stack(size_t(kMaxLevels) * kBlock);
    const PoseScene S{poses, n_poses, nodes.empty() ? nullptr : nodes.data()};
    for (size_t i = 0; i < n; ++i) {
        const RayIn r = ray_in(rays[i]);
        any[i] = out[i].hit ? 1 : (poses_any(S, d.data(), static_cast<uint32_t>(n_models), vs, inv_vs, r, stack.data()) ? 1 : 0);
        uint4 rec{};
        const uint32_t won = poses_closest(S, d.data(), static_cast<uint32_t>(n_models), vs, inv_vs, r, out[i].hit ? out[i].t : r.tmax, stack.data(), rec);
        if (won != kInstanceNone) { std::memcpy(out + i, &rec, sizeof(rec)); ids[i] = BLOK_POSE_ID | won; }
    }
}

}  // extern "C"

#ifdef POSE_TLAS_SHIM_MAIN
#include <cstdio>
#include <cstdlib>

// Each argument is a case file of posed_instance_shim.cpp's layout.  The path loop's composition is replayed through the tree (built for a camera
// at the first ray's origin) and through the loop; both must reproduce the recorded records and ids, and the tree must keep its invariants.
namespace {
#define PT_REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "pose_tlas_shim: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)
struct PtReader {
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
        PtReader R;
        FILE* f = std::fopen(argv[a], "rb");
        PT_REQUIRE(f != nullptr);
        unsigned char buf[65536];
        for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) R.bytes.insert(R.bytes.end(), buf, buf + got);
        std::fclose(f);
        const char* why = "";
        std::vector<void*> models;
        const uint32_t n_models = R.one<uint32_t>();
        PT_REQUIRE(R.ok && n_models <= 64u);
        for (uint32_t m = 0; m < n_models; ++m) {
            const uint32_t n = R.one<uint32_t>(), e = R.one<uint32_t>();
            PT_REQUIRE(R.ok && n >= 1u && n <= (1u << 20));
            std::vector<int32_t> xyz(size_t(n) * 3u);
            std::vector<uint32_t> mats(n);
            R.read(xyz.data(), xyz.size()); R.read(mats.data(), mats.size());
            PT_REQUIRE(R.ok);
            void* h = is_model(xyz.data(), mats.data(), n, &why);
            PT_REQUIRE(h != nullptr && ss_set_scale(h, e) == 0);
            models.push_back(h);
        }
        const float vs = R.one<float>();
        const uint32_t n_world = R.one<uint32_t>();
        PT_REQUIRE(R.ok && n_world <= (1u << 22));
        std::vector<int32_t> world_xyz(size_t(n_world) * 3u);
        std::vector<uint32_t> world_mats(n_world);
        R.read(world_xyz.data(), world_xyz.size()); R.read(world_mats.data(), world_mats.size());
        void* world = n_world ? is_model(world_xyz.data(), world_mats.data(), n_world, &why) : nullptr;
        PT_REQUIRE(R.ok && (world != nullptr) == (n_world != 0u));
        const uint32_t n_inst = R.one<uint32_t>();
        PT_REQUIRE(R.ok && n_inst <= (1u << 20));
        std::vector<blok_instance> inst(n_inst);
        R.read(inst.data(), inst.size());
        const uint32_t n_poses = R.one<uint32_t>();
        PT_REQUIRE(R.ok && n_poses <= (1u << 20));
        std::vector<blok_pose> poses(n_poses);
        R.read(poses.data(), poses.size());
        const uint32_t n_rays = R.one<uint32_t>();
        PT_REQUIRE(R.ok && n_rays <= (1u << 24));
        std::vector<blok_ray> rays(n_rays);
        std::vector<blok_hit> want(n_rays), got(n_rays);
        std::vector<uint32_t> want_ids(n_rays), ids(n_rays);
        std::vector<uint8_t> any(n_rays);
        R.read(rays.data(), rays.size()); R.read(want.data(), want.size()); R.read(want_ids.data(), want_ids.size());
        PT_REQUIRE(R.ok && R.at == R.bytes.size());
        const float cam[3] = {n_rays ? rays[0].org[0] : 0.0f, n_rays ? rays[0].org[1] : 0.0f, n_rays ? rays[0].org[2] : 0.0f};
        for (int tree = 0; tree < 2; ++tree) {
            pt_compose(world, models.data(), models.size(), inst.data(), n_inst, poses.data(), n_poses, vs, cam, tree, rays.data(), rays.size(), got.data(),
                       ids.data(), any.data());
            for (uint32_t i = 0; i < n_rays; ++i) PT_REQUIRE(ids[i] == want_ids[i] && std::memcmp(&got[i], &want[i], sizeof(blok_hit)) == 0 && any[i] == want[i].hit);
        }
        if (n_poses >= 1u && n_poses <= kTlasMax) {
            std::vector<TlasNode> nodes(tlas_nodes(n_poses));
            pt_build(models.data(), models.size(), poses.data(), n_poses, vs, cam, nodes.data());
            const uint32_t P = nodes[0].child;
            PT_REQUIRE(P == tlas_slots(n_poses) && nodes[0].escape <= n_poses);
            for (uint32_t k = 1; k < 2u * P; ++k) PT_REQUIRE(nodes[k].escape == tlas_escape(k));
        }
        std::printf("pose_tlas_shim: %s: %u rays\n", argv[a], n_rays);
        if (world) is_free(world);
        for (void* h : models) is_free(h);
    }
    std::puts("pose_tlas_shim: ok");
    return 0;
}
#endif
