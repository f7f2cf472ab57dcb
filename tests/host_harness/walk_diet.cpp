// TEST INFRASTRUCTURE: the walk of trace_core.h on the CPU, one ray at a time, through its plain loop and through its CAPPED loop — a walk
// cut off after `cap` trips is walked again from the root with tmin = the tCur it returned, as the path kernel's tail pool does (path_core.h).
// A shared library for tests/test_walk_loop_diet_cpu.py, and with -DWALK_DIET_MAIN a program of its own for the sanitizer run (it reads one
// case file: world, rays, expected records).  Never linked into the shipped libraries.
#define BLOK_TRACE_HOST_HARNESS 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "trace_core.h"
#include "reference_world.h"

using namespace blok;

namespace {
struct World {
    HostTree tree;
    std::vector<uint4> nodes;
};

TraceArgs args_of(const World& w) {
    TraceArgs a{};
    a.voxel_size = 1.0f; a.inv_voxel_size = 1.0f;
    a.nodes = w.nodes.data();
    a.materials = w.tree.materials.data();
    for (int i = 0; i < 3; ++i) a.origin[i] = w.tree.origin[i];
    a.levels = w.tree.levels;
    a.tmin = BLOK_RAY_TMIN; a.tmax = BLOK_RAY_TMAX;
    return a;
}

World* build_world(const blok_svo_node* nodes, size_t n_nodes, const blok_sub_chunk* subs, size_t n_subs, const char** why) {
    std::vector<VoxelRec> voxels;
    if (!extract_voxels(nodes, n_nodes, subs, n_subs, voxels, why)) return nullptr;
    World* w = new World();
    if (!build_tree(voxels, w->tree, why)) { delete w; return nullptr; }
    w->nodes.resize(w->tree.nodes.size());
    std::memcpy(w->nodes.data(), w->tree.nodes.data(), w->nodes.size() * sizeof(uint4));
    return w;
}

// One ray through the capped loop.  A cut walk starts again from the root at the parameter it returned; a restart that did not get past the
// parameter it started from (the cap is smaller than the way down from the root) is followed by one without a cap, through the same
// instantiation (the kernel's rounds without a cap pass 2^32 - 1 too).  Returns how often the walk was cut; `backwards` counts returned
// parameters below the one the walk started from (never: tCur does not decrease).
uint32_t trace_capped(const TraceArgs& a, const RayIn& r, uint32_t cap, uint4* stk, blok_hit* out, uint32_t* backwards) {
    const WalkRay R = walk_ray(a, r.ox, r.oy, r.oz, safe_inv(r.dx), safe_inv(r.dy), safe_inv(r.dz));
    float tmin = r.tmin;
    uint32_t cuts = 0u, this_cap = cap;
    for (;;) {
        WalkState s;
        walk_enter(a, R, tmin, r.tmax, s);
        walk_loop<true>(a, R, r.tmax, s, stk, this_cap);
        if (!s.walking) {
            if (s.found) {
                const HitInfo h = walk_hit(a, r, R, s);
                uint4 rec;                                       // trace_one's record
                rec.x = __float_as_uint(h.t);
                rec.y = h.material;
                rec.z = (static_cast<uint32_t>(h.vx) & 0xFFFFu) | (static_cast<uint32_t>(h.vy) << 16);
                rec.w = (static_cast<uint32_t>(h.vz) & 0xFFFFu) | (h.face << 16) | (1u << 24);
                std::memcpy(out, &rec, sizeof(rec));
            } else {
                write_miss(Sink{out, nullptr});
            }
            return cuts;
        }
        ++cuts;
        if (s.tCur < tmin) ++*backwards;
        if (!(s.tCur > tmin)) this_cap = 0xFFFFFFFFu;
        tmin = s.tCur;
    }
}

void trace_all(const World& w, const blok_ray* rays, size_t n, uint32_t cap, blok_hit* out, uint64_t* cuts, uint32_t* backwards) {
    const TraceArgs a = args_of(w);
    std::vector<uint4> stack(size_t(kMaxLevels) * 2 * kBlock);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r{rays[i].org[0], rays[i].org[1], rays[i].org[2], rays[i].dir[0], rays[i].dir[1], rays[i].dir[2], rays[i].tmin, rays[i].tmax};
        if (cap == 0u) trace_one(a, r, stack.data(), Sink{out + i, nullptr});
        else *cuts += trace_capped(a, r, cap, stack.data(), out + i, backwards);
    }
}
}  // namespace

#ifndef WALK_DIET_MAIN
extern "C" {
void* wd_build(const blok_svo_node* nodes, size_t n_nodes, const blok_sub_chunk* subs, size_t n_subs, const char** why) {
    static const char* none = "";
    *why = none;
    return build_world(nodes, n_nodes, subs, n_subs, why);
}
void wd_free(void* h) { delete static_cast<World*>(h); }
uint32_t wd_levels(const void* h) { return static_cast<const World*>(h)->tree.levels; }
void wd_origin(const void* h, int32_t* origin) { for (int i = 0; i < 3; ++i) origin[i] = static_cast<const World*>(h)->tree.origin[i]; }
// cap 0: the plain loop (trace_one); otherwise the capped loop with restarts.  cuts, backwards: see trace_capped.
void wd_trace(const void* h, const blok_ray* rays, size_t n, uint32_t cap, blok_hit* out, uint64_t* cuts, uint32_t* backwards) {
    *cuts = 0u; *backwards = 0u;
    trace_all(*static_cast<const World*>(h), rays, n, cap, out, cuts, backwards);
}
}
#else
// walk_diet_main FILE: uint64 n_nodes, n_subs, n_rays, n_caps; the nodes; the sub-chunks; the rays; the expected 16-byte records; the caps
// (uint32 each, 0 = the plain loop).  Prints one line per cap and exits 0 when every record of every cap equals the expected one.
namespace {
template <class T> bool read_n(std::FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
}
int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: walk_diet_main FILE\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t head[4];
    std::vector<blok_svo_node> nodes; std::vector<blok_sub_chunk> subs; std::vector<blok_ray> rays; std::vector<blok_hit> want; std::vector<uint32_t> caps;
    const bool ok = std::fread(head, sizeof(uint64_t), 4, f) == 4 && read_n(f, nodes, head[0]) && read_n(f, subs, head[1]) && read_n(f, rays, head[2]) &&
                    read_n(f, want, head[2]) && read_n(f, caps, head[3]);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short file\n"); return 2; }
    const char* why = "";
    World* w = build_world(nodes.data(), nodes.size(), subs.data(), subs.size(), &why);
    if (!w) { std::fprintf(stderr, "world refused: %s\n", why); return 2; }
    int rc = 0;
    std::vector<blok_hit> got(rays.size());
    for (uint32_t cap : caps) {
        uint64_t cuts = 0u; uint32_t backwards = 0u;
        std::memset(got.data(), 0, got.size() * sizeof(blok_hit));
        trace_all(*w, rays.data(), rays.size(), cap, got.data(), &cuts, &backwards);
        size_t differ = 0;
        for (size_t i = 0; i < rays.size(); ++i) differ += std::memcmp(&got[i], &want[i], sizeof(blok_hit)) != 0;
        std::printf("cap %u rays %zu differ %zu cuts %llu backwards %u\n", cap, rays.size(), differ, static_cast<unsigned long long>(cuts), backwards);
        if (differ != 0 || backwards != 0) rc = 1;
    }
    delete w;
    return rc;
}
#endif
