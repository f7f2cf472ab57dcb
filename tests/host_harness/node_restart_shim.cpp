// TEST INFRASTRUCTURE: the one-trip entry of a listed ray at the node its restarted walk ends in (blok_amd/csrc/hip/trace_core.h:
// restart_node_word, walk_enter_node — the text packed_frame_node_kernel and trace_count_own_kernel compile), on the CPU, for
// tests/test_brick_restart_host.py.  Per ray: the counted walk (walk_loop<false, true, true>) leaves its own start and restarted trips, the
// count launch's side turns them into the node word, and the frame's side — the node loaded the way the kernel loads it — either settles the
// ray with a record or says "not settled"; beside it the walk from the root over the same interval.  Built with -DNODE_RESTART_SHIM_MAIN it
// is a stand-alone program over a generated world instead (for a sanitizer build).  Never linked into the shipped libraries.
#define BLOK_TRACE_HOST_HARNESS 1
#include "trace_core.h"
#include "reference_world.h"

#include <cstring>
#include <vector>

using namespace blok;

namespace {
struct World {
    HostTree tree;
    std::vector<uint4> nodes;
};

TraceArgs make_args(const World& w, const blok_camera& cam, uint32_t width, uint32_t height) {
    TraceArgs a{};
    a.voxel_size = 1.0f; a.inv_voxel_size = 1.0f;
    a.nodes = w.nodes.data();
    a.materials = w.tree.materials.data();
    for (int i = 0; i < 3; ++i) a.origin[i] = w.tree.origin[i];
    a.levels = w.tree.levels;
    a.tmin = BLOK_RAY_TMIN; a.tmax = BLOK_RAY_TMAX;
    a.cam = cam; a.frame_w = width; a.frame_h = height;
    return a;
}

World* adopt(std::vector<VoxelRec>& voxels, const char** why) {
    auto* w = new World();
    if (!build_tree(voxels, w->tree, why)) { delete w; return nullptr; }
    w->nodes.resize(w->tree.nodes.size());
    std::memcpy(w->nodes.data(), w->tree.nodes.data(), w->nodes.size() * sizeof(uint4));
    return w;
}

// The record trace_one writes for a hit (trace_core.h), as packed_frame_node_kernel writes it.
void write_hit(blok_hit* dst, const HitInfo& h) {
    uint4 rec;
    rec.x = __float_as_uint(h.t);
    rec.y = h.material;
    rec.z = (static_cast<uint32_t>(h.vx) & 0xFFFFu) | (static_cast<uint32_t>(h.vy) << 16);
    rec.w = (static_cast<uint32_t>(h.vz) & 0xFFFFu) | (h.face << 16) | (1u << 24);
    *reinterpret_cast<uint4*>(dst) = rec;
}
}

extern "C" {

void* nr_build(const blok_svo_node* nodes, size_t n_nodes, const blok_sub_chunk* subs, size_t n_subs, const char** why) {
    static const char* none = "";
    *why = none;
    std::vector<VoxelRec> voxels;
    if (!extract_voxels(nodes, n_nodes, subs, n_subs, voxels, why)) return nullptr;
    return adopt(voxels, why);
}
// A tree as blok_hip_download_tree returns it (the device's own node order), with its origin and levels (blok_world_stats).
void* nr_adopt(const void* nodes, size_t n_nodes, const uint32_t* materials, size_t n_materials, const int32_t* origin, uint32_t levels) {
    auto* w = new World();
    w->nodes.resize(n_nodes);
    std::memcpy(w->nodes.data(), nodes, n_nodes * sizeof(uint4));
    w->tree.materials.assign(materials, materials + n_materials);
    for (int i = 0; i < 3; ++i) w->tree.origin[i] = origin[i];
    w->tree.levels = levels;
    return w;
}
void nr_free(void* w) { delete static_cast<World*>(w); }
uint32_t nr_levels(const void* w) { return static_cast<const World*>(w)->tree.levels; }
const void* nr_tree_nodes(const void* w, size_t* count, int32_t* origin) {
    const World* W = static_cast<const World*>(w);
    *count = W->nodes.size();
    for (int i = 0; i < 3; ++i) origin[i] = W->tree.origin[i];
    return W->nodes.data();
}

// Every ray of the rectangle, row-major.  tstart (optional): a per-pixel lower bound the counted walk starts from, as the wave tiles' bounds.
// spoil: 0 the word as counted; 1 its level replaced by one the tree has not (levels, levels + 1, .. 7 in turn, the index kept);
// 2 the word replaced by 0xFFFFFFFF.
// jitter_clip: TraceArgs::jitter_clip of the launch (two floats).
// -> through the pointers: the counted word, the ray's own start, its restarted trips; the verified start voxel of the restarted interval in
// tree coordinates (x, y, z; -1 where there is none); settled (1 / 0); the record of the entry (for a settled ray), and the record of the
// walk from the root over [max(tmin, own start), tmax).  Returns the node loads that were out of range
// (always 0: the entry reads nodes[0] for a ray without a word).
uint32_t nr_run(const void* wp, const blok_camera* cam, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* tstart, const float* jitter_clip,
                int spoil, uint32_t* words, float* own_starts, uint8_t* restarts, int32_t* cells, uint8_t* settled, blok_hit* entry_records, blok_hit* root_records) {
    const World* W = static_cast<const World*>(wp);
    TraceArgs a = make_args(*W, *cam, width, height);
    if (jitter_clip) { a.jitter_clip[0] = jitter_clip[0]; a.jitter_clip[1] = jitter_clip[1]; }
    const int side = 1 << (2 * a.levels);
    std::vector<uint4> stack(size_t(kMaxLevels) * 2 * kBlock);
    uint32_t out_of_range = 0u, turn = 0u;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t at = size_t(y) * w + x;
            RayIn r = primary_ray(a, x0 + x, y0 + y);
            if (tstart) r.tmin = fmaxf(r.tmin, tstart[at]);
            const WalkRay R = walk_ray(a, r.ox, r.oy, r.oz, safe_inv(r.dx), safe_inv(r.dy), safe_inv(r.dz));
            // the count launch: walk_wave<true, true> on the host
            WalkState s;
            walk_enter(a, R, r.tmin, r.tmax, s);
            uint32_t n_trips = 0u, own_trips = 0u;
            float own_start = r.tmin;
            walk_loop<false, true, true>(a, R, r.tmax, s, stack.data(), 0u, &n_trips, &own_start, &own_trips);
            RayIn from = r;
            from.tmin = fmaxf(a.tmin, own_start);
            uint32_t word = own_trips != 0u && own_trips <= a.levels ? restart_node_word(a, from, R, a.levels - own_trips) : kNodeWordNone;
            words[at] = word; own_starts[at] = own_start; restarts[at] = static_cast<uint8_t>(own_trips);
            {
                float fx, fy, fz, tFx, tFy, tFz;
                const bool have = start_voxel(a, from, R, fx, fy, fz, tFx, tFy, tFz);
                const int q[3] = {static_cast<int>(__float_as_uint(fx) & 0x7FFFFFu), static_cast<int>(__float_as_uint(fy) & 0x7FFFFFu), static_cast<int>(__float_as_uint(fz) & 0x7FFFFFu)};
                const bool neg[3] = {!(R.ax.inv > 0.0f), !(R.ay.inv > 0.0f), !(R.az.inv > 0.0f)};
                for (int k = 0; k < 3; ++k) cells[3 * at + k] = have ? (neg[k] ? side - 1 - q[k] : q[k]) : -1;
            }
            if (spoil == 1 && word != kNodeWordNone) {
                const uint32_t span = 8u - a.levels;                   // levels the tree has not: levels .. 7
                const uint32_t wrong = a.levels + (turn++ % span);
                word = (word & kNodeWordIndexMask) | (wrong << kNodeWordLevelShift);
                if (word == kNodeWordNone) word &= ~1u;
            }
            if (spoil == 2) word = kNodeWordNone;
            // the frame: the node in front of the set-up, the last trip alone
            const size_t index = word == kNodeWordNone ? 0u : (word & kNodeWordIndexMask);
            if (index >= W->nodes.size()) { ++out_of_range; settled[at] = 0; continue; }
            const uint4 rec = a.nodes[index];
            WalkState e;
            const bool ok = walk_enter_node(a, from, R, word, rec, e);
            settled[at] = ok ? 1 : 0;
            std::memset(&entry_records[at], 0, sizeof(blok_hit));
            if (ok) {
                if (e.found) write_hit(&entry_records[at], walk_hit(a, from, R, e));
                else write_miss(Sink{&entry_records[at], nullptr});
            }
            trace_one(a, from, stack.data(), Sink{&root_records[at], nullptr});
        }
    return out_of_range;
}

}

#ifdef NODE_RESTART_SHIM_MAIN
#include <stdio.h>
// A generated world (a hollow ball over a floor with holes, 64^3, and a 4^3 one of one level) seen from outside, from inside and grazing:
// every settled ray's record must be the walk's from the root, and no spoilt word may settle or read out of range.
static blok_camera look(float px, float py, float pz, float tx, float ty, float tz, float fov_deg, uint32_t w, uint32_t h) {
    blok_camera c{};
    float f[3] = {tx - px, ty - py, tz - pz};
    const float fl = __builtin_sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (float& v : f) v /= fl;
    float rt[3] = {f[1] * 0.0f - f[2] * 1.0f, f[2] * 0.0f - f[0] * 0.0f, f[0] * 1.0f - f[1] * 0.0f};      // f x (0, 1, 0)
    const float rl = __builtin_sqrtf(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2]);
    for (float& v : rt) v /= rl;
    const float up[3] = {rt[1] * f[2] - rt[2] * f[1], rt[2] * f[0] - rt[0] * f[2], rt[0] * f[1] - rt[1] * f[0]};
    c.pos[0] = px; c.pos[1] = py; c.pos[2] = pz;
    for (int i = 0; i < 3; ++i) { c.fwd[i] = f[i]; c.right[i] = rt[i]; c.up[i] = up[i]; }
    c.tan_half_fov = __builtin_tanf(fov_deg * 0.5f * 3.14159265f / 180.0f);
    c.aspect = static_cast<float>(w) / static_cast<float>(h);
    return c;
}

int main() {
    unsigned long long bad = 0, settled_total = 0, rays = 0;
    for (int n : {64, 4}) {
        std::vector<VoxelRec> voxels;
        for (int z = 0; z < n; ++z)
            for (int y = 0; y < n; ++y)
                for (int x = 0; x < n; ++x) {
                    const float dx = x - n * 0.5f, dy = y - n * 0.55f, dz = z - n * 0.5f, d = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
                    const bool ball = d < n * 0.3f && d > n * 0.22f, floor = y < n / 8 && ((x / 3 + z / 3) % 5) != 0;
                    if (ball || floor) voxels.push_back(VoxelRec{x, y, z, 1u + static_cast<uint32_t>((x + 2 * y + 3 * z) % 7)});
                }
        const char* why = "";
        World* W = adopt(voxels, &why);
        if (!W) { printf("node restart: no tree (%s)\n", why); return 2; }
        const uint32_t w = 96, h = 64;
        const float m = static_cast<float>(n);
        const blok_camera cams[3] = {look(m * 1.9f, m * 0.8f, m * 1.4f, m * 0.5f, m * 0.3f, m * 0.5f, 60.0f, w, h),
                                     look(m * 0.47f, m * 0.82f, m * 0.52f, m * 0.14f, m * 0.17f, m * 0.22f, 70.0f, w, h),
                                     look(-m * 0.33f, m * 0.49f, m * 0.45f, m * 1.9f, m * 0.45f, m * 0.64f, 50.0f, w, h)};
        std::vector<uint32_t> words(w * h);
        std::vector<float> starts(w * h);
        std::vector<uint8_t> restarts(w * h), settled(w * h);
        std::vector<blok_hit> entry(w * h), root(w * h);
        std::vector<int32_t> cells(3 * w * h);
        for (const blok_camera& cam : cams)
            for (int spoil = 0; spoil < 3; ++spoil) {
                bad += nr_run(W, &cam, w, h, 0, 0, w, h, nullptr, nullptr, spoil, words.data(), starts.data(), restarts.data(), cells.data(), settled.data(), entry.data(), root.data());
                for (uint32_t i = 0; i < w * h; ++i) {
                    rays += spoil == 0;
                    if (spoil == 0) {
                        settled_total += settled[i];
                        bad += settled[i] && std::memcmp(&entry[i], &root[i], sizeof(blok_hit)) != 0;
                        bad += !settled[i] && words[i] != kNodeWordNone;      // a ray with a word is settled by its last trip
                    } else bad += settled[i] != 0;
                }
            }
        nr_free(W);
    }
    printf("node restart: %llu rays, %llu settled, %llu mismatches\n", rays, settled_total, bad);
    return bad != 0;
}
#endif
