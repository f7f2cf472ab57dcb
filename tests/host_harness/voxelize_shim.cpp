// TEST INFRASTRUCTURE: the exact tests of the gfx950 voxelizer (blok_amd/csrc/hip/voxelize_core.h) compiled for the CPU, driven one
// triangle and one voxel at a time: the dense arrays blok_hip_volume_voxelize_mesh must leave.  Never linked into the shipped libraries.
#define BLOK_VOX_HOST_HARNESS 1
#include "voxelize_core.h"

#include <cstddef>
#include <vector>

using namespace blok;

extern "C" {

// density / ids: [z][y][x] over the box, updated in place.  Returns 0, or -1 when the call must be refused (nothing written).
int vs_voxelize(const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz, float* density, uint32_t* ids, const float* pos, size_t n_vertices,
                const uint32_t* tris, size_t n_tris, const uint32_t* tri_mats, uint32_t material, float value, int mode, uint64_t* out_n) {
    *out_n = 0;
    if (!(value > 0.0f) || !std::isfinite(value) || (mode != 0 && mode != 1)) return -1;
    std::vector<vox::Tri> T(n_tris);
    for (size_t i = 0; i < n_tris; ++i) {
        int64_t q[3][3];
        for (int k = 0; k < 3; ++k) {
            const uint32_t vi = tris[3 * i + k];
            if (vi >= n_vertices) return -1;
            for (int c = 0; c < 3; ++c) {
                if (!vox::coord_ok(pos[3 * vi + c])) return -1;
                q[k][c] = vox::snap(pos[3 * vi + c]);
            }
        }
        for (int c = 0; c < 3; ++c) {
            T[i].v0[c] = q[0][c]; T[i].w1[c] = q[1][c] - q[0][c]; T[i].w2[c] = q[2][c] - q[0][c];
            if (vox::max64(q[0][c], vox::max64(q[1][c], q[2][c])) - vox::min64(q[0][c], vox::min64(q[1][c], q[2][c])) > vox::kMaxExtent) return -1;
        }
    }
    const size_t cells = size_t(nx) * ny * nz;
    const int32_t dims[3] = {nx, ny, nz};
    const int64_t O[3] = {int64_t(origin[0]) * 256, int64_t(origin[1]) * 256, int64_t(origin[2]) * 256};
    std::vector<uint32_t> owner(cells, 0xFFFFFFFFu);          // lowest triangle over each surface voxel
    for (size_t i = 0; i < n_tris; ++i) {
        const vox::Tri& t = T[i];
        int64_t lo[3], hi[3];
        bool empty = false;
        for (int c = 0; c < 3; ++c) {
            const int64_t a = vox::min64(0, vox::min64(t.w1[c], t.w2[c])) + t.v0[c], b = vox::max64(0, vox::max64(t.w1[c], t.w2[c])) + t.v0[c];
            lo[c] = vox::max64(vox::voxel_lo(a) - origin[c], 0); hi[c] = vox::min64(vox::voxel_hi(b) - origin[c], dims[c] - 1);
            empty |= lo[c] > hi[c];
        }
        if (empty) continue;
        for (int64_t z = lo[2]; z <= hi[2]; ++z)
            for (int64_t y = lo[1]; y <= hi[1]; ++y)
                for (int64_t x = lo[0]; x <= hi[0]; ++x) {
                    const size_t at = (size_t(z) * ny + size_t(y)) * nx + size_t(x);
                    if (owner[at] != 0xFFFFFFFFu) continue;
                    const int64_t b[3] = {O[0] + 256 * x - t.v0[0], O[1] + 256 * y - t.v0[1], O[2] + 256 * z - t.v0[2]};
                    if (vox::box_overlaps(t, b, 256)) owner[at] = uint32_t(i);
                }
    }
    std::vector<uint8_t> inside(mode == 1 ? cells : 0, 0);
    if (mode == 1) {
        for (size_t i = 0; i < n_tris; ++i) {
            const vox::Tri& t = T[i];
            const int64_t ylo = vox::min64(0, vox::min64(t.w1[1], t.w2[1])), yhi = vox::max64(0, vox::max64(t.w1[1], t.w2[1]));
            const int64_t zlo = vox::min64(0, vox::min64(t.w1[2], t.w2[2])), zhi = vox::max64(0, vox::max64(t.w1[2], t.w2[2]));
            // columns whose centre lies in the triangle's yz range
            const int64_t j0 = vox::max64(vox::ceil_div(ylo + t.v0[1] - O[1] - 128, 256), 0), j1 = vox::min64(vox::floor_div(yhi + t.v0[1] - O[1] - 128, 256), ny - 1);
            const int64_t k0 = vox::max64(vox::ceil_div(zlo + t.v0[2] - O[2] - 128, 256), 0), k1 = vox::min64(vox::floor_div(zhi + t.v0[2] - O[2] - 128, 256), nz - 1);
            for (int64_t k = k0; k <= k1; ++k)
                for (int64_t j = j0; j <= j1; ++j) {
                    const int64_t Y = O[1] + 256 * j + 128 - t.v0[1], Z = O[2] + 256 * k + 128 - t.v0[2];
                    if (!vox::column_inside(t, Y, Z)) continue;
                    int64_t x = vox::crossing_voxel(t, Y, Z, O[0] + 128 - t.v0[0]);
                    if (x >= nx) continue;
                    if (x < 0) x = 0;
                    inside[(size_t(k) * ny + size_t(j)) * nx + size_t(x)] ^= 1u;
                }
        }
        for (size_t row = 0; row < size_t(ny) * nz; ++row) {
            uint8_t p = 0;
            for (int32_t x = 0; x < nx; ++x) { p ^= inside[row * nx + x]; inside[row * nx + x] = p; }
        }
    }
    uint64_t n = 0;
    for (size_t at = 0; at < cells; ++at) {
        if (owner[at] != 0xFFFFFFFFu) { density[at] = value; ids[at] = tri_mats ? tri_mats[owner[at]] : material; ++n; }
        else if (mode == 1 && inside[at]) { density[at] = value; ids[at] = material; ++n; }
    }
    *out_n = n;
    return 0;
}

}  // extern "C"
