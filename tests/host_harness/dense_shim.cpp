// TEST INFRASTRUCTURE: the dense-grid kernel's per-ray body (blok_amd/csrc/hip/dense_core.h) on the CPU, one "lane" at a time, over a
// grid tiled on the host with the helpers the tiling kernel uses.  No HIP is involved; never linked into the shipped libraries.
#define BLOK_TRACE_HOST_HARNESS 1
#include <cstddef>
#include <cstdint>
static thread_local size_t g_tiles = 0;                  // tiles of the grid being walked
static thread_local uint64_t g_out_of_grid = 0;          // walks that addressed a tile outside it (ended there as a miss; 0 in a working walk)
static thread_local unsigned char* g_steps = nullptr;    // optional log of the axis of every step
static thread_local uint32_t g_steps_len = 0, g_steps_cap = 0;
#define BLOK_DENSE_TILE(tile) do { if ((tile) >= g_tiles) { ++g_out_of_grid; return false; } } while (0)
#define BLOK_DENSE_STEP(axis) do { if (g_steps) { if (g_steps_len < g_steps_cap) g_steps[g_steps_len] = (unsigned char)(axis); ++g_steps_len; } } while (0)
#include "dense_core.h"

#include <vector>

using namespace blok;

namespace {
struct HostDense {
    DenseGrid grid;
    std::vector<uint32_t> tiled;       // exactly tiles * 512 words
    std::vector<uint32_t> bits;        // exactly bit_words words: the "global array"
    std::vector<uint32_t> staged;      // the kernel's LDS copy of them
};

void trace(const HostDense& H, const RayIn& r, int global_bits, blok_hit* out) {
    const Sink sink{out, nullptr};
    g_tiles = H.bits.empty() ? 0 : H.tiled.size() / 512u;
    const uint32_t* words = global_bits ? H.bits.data() : H.staged.data();
    uint4 rec;
    if (!dense_walk(r, H.grid, [&](uint32_t w) { return words[w]; }, rec)) { write_miss(sink); return; }
    *reinterpret_cast<uint4*>(sink.hit) = rec;
}
}  // namespace

extern "C" {

void* ds_new(const uint32_t* ids, uint32_t nx, uint32_t ny, uint32_t nz, const int32_t* origin) {
    auto* H = new HostDense();
    const uint32_t tx = (nx + 7u) / 8u, ty = (ny + 7u) / 8u, tz = (nz + 7u) / 8u;      // as keep_dense_grid (api.hip)
    const size_t tiles = size_t(tx) * ty * tz;
    H->tiled.assign(tiles * 512u, 0u);
    H->bits.assign((tiles + 31u) / 32u, 0u);
    for (uint32_t tile = 0; tile < tiles; ++tile) {
        uint32_t any = 0;
        for (uint32_t c = 0; c < 512u; ++c) {
            uint32_t x, y, z;
            dense_cell_of(tile, c, tx, ty, x, y, z);
            const uint32_t id = dense_source_id(ids, nx, ny, nz, x, y, z);
            H->tiled[size_t(tile) * 512u + c] = id;
            any |= id;
        }
        if (any) H->bits[tile >> 5] |= 1u << (tile & 31u);
    }
    H->staged = H->bits;
    H->grid = DenseGrid{{origin[0], origin[1], origin[2]}, tx, ty, tz, H->tiled.data()};
    return H;
}
void ds_free(void* h) { delete static_cast<HostDense*>(h); }

uint64_t ds_out_of_grid() { const uint64_t n = g_out_of_grid; g_out_of_grid = 0; return n; }      // since the last call

// one ray with the axis of every step logged (cap bytes); returns the number of steps
uint32_t ds_trace_steps(const void* h, const blok_ray* ray, int global_bits, unsigned char* steps, uint32_t cap, blok_hit* out) {
    g_steps = steps; g_steps_len = 0; g_steps_cap = cap;
    const RayIn r{ray->org[0], ray->org[1], ray->org[2], ray->dir[0], ray->dir[1], ray->dir[2], ray->tmin, ray->tmax};
    trace(*static_cast<const HostDense*>(h), r, global_bits, out);
    g_steps = nullptr;
    return g_steps_len;
}

void ds_trace_rays(const void* h, const blok_ray* rays, size_t n, int global_bits, blok_hit* out) {
    const HostDense& H = *static_cast<const HostDense*>(h);
    for (size_t i = 0; i < n; ++i) {
        const RayIn r{rays[i].org[0], rays[i].org[1], rays[i].org[2], rays[i].dir[0], rays[i].dir[1], rays[i].dir[2], rays[i].tmin, rays[i].tmax};
        trace(H, r, global_bits, out + i);
    }
}

// the kernel's pixel -> ray mapping (primary_ray) over the whole frame; jitter_clip may be null
void ds_trace_primary(const void* h, const blok_camera* cam, uint32_t width, uint32_t height, const float* jitter_clip, int global_bits, blok_hit* out) {
    const HostDense& H = *static_cast<const HostDense*>(h);
    TraceArgs a{};
    a.cam = *cam; a.frame_w = width; a.frame_h = height;
    if (jitter_clip) { a.jitter_clip[0] = jitter_clip[0]; a.jitter_clip[1] = jitter_clip[1]; }
    a.tmin = BLOK_RAY_TMIN; a.tmax = BLOK_RAY_TMAX;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) trace(H, primary_ray(a, x, y), global_bits, out + size_t(y) * width + x);
}

}
