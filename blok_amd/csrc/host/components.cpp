// Connected components of a voxel volume on the host (include/blok_world.h: blok_components_label): the contract of
// blok_hip_volume_label_components (blok_hip.h) over host arrays, through the index arithmetic and the union-find the kernels use
// (../common/components_core.h), run serially.  The result does not depend on the order of the unions.
#include "blok_world.h"
#include "../common/components_core.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace K = blok::components;

namespace {
struct SerialCells {
    uint32_t* parent;
    uint32_t load(uint32_t i) const { return parent[i]; }
    uint32_t fetch_min(uint32_t i, uint32_t v) const { const uint32_t old = parent[i]; parent[i] = std::min(old, v); return old; }
};
}  // namespace

extern "C" {

int blok_components_label(const float* density, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                          const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                          uint32_t* labels_out, uint64_t label_capacity, blok_component* components_out, uint64_t component_capacity,
                          uint64_t* out_n_components, uint64_t* out_n_voxels) {
    if (out_n_components) *out_n_components = 0;
    if (out_n_voxels) *out_n_voxels = 0;
    if (flags) return BLOK_ERR_INVALID_ARG;
    if ((region_lo == nullptr) != (region_hi == nullptr)) return BLOK_ERR_INVALID_ARG;
    const int64_t dims[3] = {nx, ny, nz};
    const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = region_lo ? int64_t(region_lo[a]) - org[a] : 0;
        hi[a] = region_hi ? int64_t(region_hi[a]) - org[a] : dims[a];
        if (lo[a] > hi[a]) return BLOK_ERR_INVALID_ARG;
    }
    for (int a = 0; a < 3; ++a) if (lo[a] < 0 || hi[a] > dims[a]) return BLOK_ERR_UNSUPPORTED;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    K::Region g{};
    for (int a = 0; a < 3; ++a) { g.lo[a] = uint32_t(lo[a]); g.ext[a] = uint32_t(hi[a] - lo[a]); }
    const uint64_t n = K::cells(g);
    if (n > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;          // 2^32 cells: the sentinel would be an index
    if (n == 0) return BLOK_OK;
    if (!density) return BLOK_ERR_INVALID_ARG;

    std::vector<uint32_t> parent(n);
    const SerialCells cells{parent.data()};
    uint64_t n_voxels = 0;
    for (uint32_t r = 0; r < n; ++r) {
        uint32_t x, y, z;
        K::cell_of(g, r, x, y, z);
        const size_t cell = (static_cast<size_t>(g.lo[2] + z) * ny + (g.lo[1] + y)) * nx + g.lo[0] + x;
        const bool f = K::filled(density[cell]);
        parent[r] = f ? r : BLOK_LABEL_EMPTY;
        n_voxels += f;
    }
    for (uint32_t r = 0; r < n; ++r) {
        if (parent[r] == BLOK_LABEL_EMPTY) continue;
        uint32_t c[3];
        K::cell_of(g, r, c[0], c[1], c[2]);
        for (uint32_t a = 0; a < 3u; ++a)
            if (c[a] + 1u < g.ext[a] && parent[r + K::stride(g, a)] != BLOK_LABEL_EMPTY) K::unite(cells, r, r + K::stride(g, a));
    }
    // flatten in index order (a root comes before everything below it), and the records in label order
    struct Acc { uint32_t mn[3], mx[3]; uint64_t count; };
    std::vector<uint32_t> roots;
    std::vector<Acc> acc;
    std::vector<uint32_t> rank(n);                                // of a root's cell: its record
    for (uint32_t r = 0; r < n; ++r) {
        if (parent[r] == BLOK_LABEL_EMPTY) continue;
        const uint32_t root = parent[r] == r ? r : parent[parent[r]];      // parent[r] < r is flattened already
        parent[r] = root;
        if (root == r) { rank[r] = uint32_t(roots.size()); roots.push_back(r); acc.push_back(Acc{{~0u, ~0u, ~0u}, {0u, 0u, 0u}, 0u}); }
        Acc& A = acc[rank[root]];
        uint32_t c[3];
        K::cell_of(g, r, c[0], c[1], c[2]);
        for (int a = 0; a < 3; ++a) { A.mn[a] = std::min(A.mn[a], c[a]); A.mx[a] = std::max(A.mx[a], c[a]); }
        ++A.count;
    }
    if (labels_out) std::copy(parent.begin(), parent.begin() + std::min<uint64_t>(n, label_capacity), labels_out);
    if (components_out)
        for (uint64_t i = 0; i < std::min<uint64_t>(roots.size(), component_capacity); ++i) {
            blok_component& c = components_out[i];
            c.label = roots[i]; c.touches = K::touches(g, acc[i].mn, acc[i].mx); c.n_voxels = acc[i].count;
            for (int a = 0; a < 3; ++a) {
                c.lo[a] = int32_t(org[a] + lo[a] + acc[i].mn[a]);
                c.hi[a] = int32_t(org[a] + lo[a] + acc[i].mx[a] + 1);
            }
        }
    if (out_n_components) *out_n_components = roots.size();
    if (out_n_voxels) *out_n_voxels = n_voxels;
    return BLOK_OK;
}

}  // extern "C"
