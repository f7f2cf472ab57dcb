// A model resampled into a voxel volume through an affine map, on the host (include/blok_world.h: blok_affine_from_instance,
// blok_affine_from_matrix, blok_affine_stamp_voxels): the contract of blok_hip_volume_stamp_affine (blok_hip.h) over host arrays, through
// the arithmetic the kernel uses (../common/affine_core.h).  The model is a voxel list looked up by coordinate — a dense array of its box,
// or a hash when the box is large — never a tree: the build shares the sampling with the kernel and nothing of its descent.
#include "blok_world.h"
#include "../common/affine_core.h"
#include "../common/region_core.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace A = blok::affine;
namespace S = blok::stamp;

namespace {

struct Key {
    int32_t x, y, z;
    bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct KeyHash {
    size_t operator()(const Key& k) const {
        uint64_t h = uint64_t(uint32_t(k.x)) * 0x9E3779B97F4A7C15ull;
        h = (h ^ (h >> 29)) + uint64_t(uint32_t(k.y)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 31)) + uint64_t(uint32_t(k.z)) * 0x94D049BB133111EBull;
        return size_t(h ^ (h >> 32));
    }
};

// The list by coordinate: list index + 1 of the LAST entry that names a voxel, 0 = no voxel there.
struct Lookup {
    int64_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};      // the list's box, half open
    std::vector<uint32_t> dense;
    std::unordered_map<Key, uint32_t, KeyHash> hash;
    bool is_dense = false;

    static constexpr uint64_t kDenseCells = uint64_t(1) << 24;

    Lookup(const int32_t* xyz, size_t n) {
        for (int a = 0; a < 3; ++a) { lo[a] = INT64_MAX; hi[a] = INT64_MIN; }
        for (size_t i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) { lo[a] = std::min<int64_t>(lo[a], xyz[3 * i + a]); hi[a] = std::max<int64_t>(hi[a], int64_t(xyz[3 * i + a]) + 1); }
        const uint64_t ex = uint64_t(hi[0] - lo[0]), ey = uint64_t(hi[1] - lo[1]), ez = uint64_t(hi[2] - lo[2]);
        is_dense = ex <= kDenseCells && ey <= kDenseCells && ez <= kDenseCells && ex * ey <= kDenseCells && ex * ey * ez <= kDenseCells;
        if (is_dense) dense.assign(size_t(ex * ey * ez), 0u);
        else hash.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            const int32_t* p = xyz + 3 * i;
            if (is_dense) dense[cell(p[0], p[1], p[2])] = uint32_t(i) + 1u;
            else hash[Key{p[0], p[1], p[2]}] = uint32_t(i) + 1u;
        }
    }
    size_t cell(int64_t x, int64_t y, int64_t z) const { return size_t((x - lo[0]) + ((y - lo[1]) + (z - lo[2]) * (hi[1] - lo[1])) * (hi[0] - lo[0])); }
    uint32_t at(const int64_t v[3]) const {
        for (int a = 0; a < 3; ++a) if (v[a] < lo[a] || v[a] >= hi[a]) return 0u;
        if (is_dense) return dense[cell(v[0], v[1], v[2])];
        const auto it = hash.find(Key{int32_t(v[0]), int32_t(v[1]), int32_t(v[2])});
        return it == hash.end() ? 0u : it->second;
    }
};

}  // namespace

extern "C" {

int blok_affine_from_instance(const blok_instance* placement, uint32_t scale_log2, blok_affine* out) {
    if (!placement || !out) return BLOK_ERR_INVALID_ARG;
    blok_affine a;
    if (!A::from_instance(*placement, scale_log2, a)) return BLOK_ERR_INVALID_ARG;
    *out = a;
    return BLOK_OK;
}

int blok_affine_from_matrix(const double forward[12], blok_affine* out) {
    if (!forward || !out) return BLOK_ERR_INVALID_ARG;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(forward[i])) return BLOK_ERR_INVALID_ARG;
    const double* F = forward;
    const double f[3][3] = {{F[0], F[1], F[2]}, {F[4], F[5], F[6]}, {F[8], F[9], F[10]}}, T[3] = {F[3], F[7], F[11]};
    // the inverse as adjugate / determinant
    double c[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[j][i] = f[i1][j1] * f[i2][j2] - f[i1][j2] * f[i2][j1];
        }
    const double det = f[0][0] * c[0][0] + f[0][1] * c[1][0] + f[0][2] * c[2][0];
    double scale = 1.0;
    for (int i = 0; i < 3; ++i) scale *= std::sqrt(f[i][0] * f[i][0] + f[i][1] * f[i][1] + f[i][2] * f[i][2]);
    if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * scale)) return BLOK_ERR_INVALID_ARG;      // singular (a zero row: 0 > 0 is false)
    blok_affine a{};
    double off[3];
    for (int j = 0; j < 3; ++j) {
        const double fl = std::floor(T[j]);
        if (!(fl >= -2147483648.0 && fl <= 2147483647.0)) return BLOK_ERR_INVALID_ARG;
        a.anchor[j] = int32_t(fl);
        off[j] = (fl + 0.5) - T[j];
    }
    for (int k = 0; k < 3; ++k) {
        double tk = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double inv = c[k][j] / det;
            const double mk = std::rint(inv * 65536.0);
            if (!(std::fabs(mk) <= double(A::kMaxM))) return BLOK_ERR_INVALID_ARG;
            a.m[k][j] = int32_t(mk);
            tk += inv * off[j];
        }
        tk = std::rint(tk * 65536.0);
        if (!(std::fabs(tk) <= double(A::kMaxT))) return BLOK_ERR_INVALID_ARG;
        a.t[k] = int64_t(tk);
    }
    *out = a;
    return BLOK_OK;
}

int blok_affine_stamp_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                             const int32_t* model_xyz, const uint32_t* model_materials, size_t n, const blok_affine* record,
                             const int32_t region_lo[3], const int32_t region_hi[3], int mode, float value, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    const int32_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    const uint32_t dims[3] = {nx, ny, nz};
    if (!record || A::well_formed(*record, org, dims) != A::kFine || !S::mode_known(mode)) return BLOK_ERR_INVALID_ARG;
    if (mode != BLOK_STAMP_ERASE && (!std::isfinite(value) || !(value > 0.0f))) return BLOK_ERR_INVALID_ARG;
    if (n && (!model_xyz || (mode != BLOK_STAMP_ERASE && !model_materials))) return BLOK_ERR_INVALID_ARG;
    if (n > 0xFFFFFFFEull) return BLOK_ERR_UNSUPPORTED;
    uint32_t lo[3], hi[3];
    if (const int rule = blok::region::local(org, dims, region_lo, region_hi, lo, hi)) return blok::region::status(rule);
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    if (n == 0 || lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) return BLOK_OK;
    if (!density || !material_ids) return BLOK_ERR_INVALID_ARG;
    const Lookup model(model_xyz, n);
    const int32_t zero[3] = {0, 0, 0};
    const A::Frame F = A::frame(*record, org, zero);
    uint64_t written = 0;
    for (uint32_t z = lo[2]; z < hi[2]; ++z)
        for (uint32_t y = lo[1]; y < hi[1]; ++y)
            for (uint32_t x = lo[0]; x < hi[0]; ++x) {
                const int64_t v[3] = {A::voxel(A::value(F, 0, x, y, z)), A::voxel(A::value(F, 1, x, y, z)), A::voxel(A::value(F, 2, x, y, z))};
                const uint32_t at = model.at(v);
                if (!at) continue;
                const size_t cell = size_t(x) + (size_t(z) * ny + y) * nx;
                float d; uint32_t m;
                if (!S::apply(mode, value, model_materials ? model_materials[at - 1u] : 0u, density[cell], d, m)) continue;
                density[cell] = d; material_ids[cell] = m;
                ++written;
            }
    if (out_n_voxels) *out_n_voxels = written;
    return BLOK_OK;
}

}  // extern "C"
