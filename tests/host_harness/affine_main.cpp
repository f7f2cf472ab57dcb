// The affine stamp's core header and host build (blok_amd/csrc/common/affine_core.h, blok_amd/csrc/host/affine.cpp) at their limits, in a
// program of its own that tests/test_affine_cpu.py builds with ASan + UBSan (-fno-sanitize-recover=all: a signed overflow, a shift out of
// range or a read past an array ends the run).  Records at |m| = 2^22, |t| = 2^40 and an anchor 2^20 - 1 from the box, on boxes at either
// end of the int16 lattice: sample, frame / value, tile_interval and the host build against 128-bit integers.  Prints "affine ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blok_world.h"
#include "../../blok_amd/csrc/common/affine_core.h"

namespace A = blok::affine;

namespace {

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

__int128 exact(const blok_affine& r, int k, const int64_t w[3]) {
    __int128 P = r.t[k];
    for (int j = 0; j < 3; ++j) P += static_cast<__int128>(r.m[k][j]) * (static_cast<__int128>(w[j]) - r.anchor[j]);
    return P;
}
int64_t floor16(__int128 P) { return static_cast<int64_t>(P >= 0 ? P / 65536 : -((-P + 65535) / 65536)); }

int run_case(const blok_affine& r, const int32_t origin[3], const uint32_t dims[3]) {
    CHECK(A::well_formed(r, origin, dims) == A::kFine);
    const int32_t model_origin[3] = {-(1 << 23), 1 << 23, 16};
    const A::Frame F = A::frame(r, origin, model_origin);
    // every cell: the record's rule, the frame's regrouping of it, both against 128 bits
    int64_t lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    for (uint32_t z = 0; z < dims[2]; ++z)
        for (uint32_t y = 0; y < dims[1]; ++y)
            for (uint32_t x = 0; x < dims[0]; ++x) {
                const int64_t w[3] = {int64_t(origin[0]) + x, int64_t(origin[1]) + y, int64_t(origin[2]) + z};
                int64_t v[3];
                A::sample(r, w, v);
                for (int k = 0; k < 3; ++k) {
                    const __int128 P = exact(r, k, w);
                    CHECK(P < (static_cast<__int128>(1) << 44) && P > -(static_cast<__int128>(1) << 44));
                    CHECK(v[k] == floor16(P));
                    const int64_t Pf = A::value(F, k, x, y, z);
                    CHECK(Pf == static_cast<int64_t>(P - static_cast<__int128>(model_origin[k]) * 65536));
                    CHECK(A::voxel(Pf) == v[k] - model_origin[k]);
                    lo[k] = Pf < lo[k] ? Pf : lo[k]; hi[k] = Pf > hi[k] ? Pf : hi[k];
                }
            }
    // the interval of the whole box is exact, and so is that of a ragged tile inside it
    const uint32_t zero[3] = {0, 0, 0};
    int64_t Plo[3], Phi[3];
    A::tile_interval(F, zero, dims, Plo, Phi);
    for (int k = 0; k < 3; ++k) CHECK(Plo[k] == lo[k] && Phi[k] == hi[k]);
    const uint32_t tl[3] = {dims[0] / 3, dims[1] / 2, dims[2] - 1}, ext[3] = {dims[0] - tl[0], 1, 1};
    A::tile_interval(F, tl, ext, Plo, Phi);
    for (int k = 0; k < 3; ++k) {
        const int64_t a = A::value(F, k, tl[0], tl[1], tl[2]), b = A::value(F, k, dims[0] - 1, tl[1], tl[2]);
        CHECK(Plo[k] == (a < b ? a : b) && Phi[k] == (a < b ? b : a));
    }
    // the host build: a model of one voxel where the box's last cell samples is found by that cell
    const int64_t w[3] = {int64_t(origin[0]) + dims[0] - 1, int64_t(origin[1]) + dims[1] - 1, int64_t(origin[2]) + dims[2] - 1};
    int64_t v[3];
    A::sample(r, w, v);
    const int32_t xyz[6] = {int32_t(v[0]), int32_t(v[1]), int32_t(v[2]), int32_t(v[0]), int32_t(v[1]), int32_t(v[2])};
    const uint32_t mats[2] = {5, 9};                              // the last duplicate wins
    std::vector<float> density(size_t(dims[0]) * dims[1] * dims[2], 0.0f);
    std::vector<uint32_t> ids(density.size(), 0u);
    uint64_t n = 0;
    CHECK(blok_affine_stamp_voxels(density.data(), ids.data(), origin, dims[0], dims[1], dims[2], xyz, mats, 2, &r, nullptr, nullptr, BLOK_STAMP_SET, 2.0f, &n) == BLOK_OK);
    CHECK(n >= 1 && ids.back() == 9u && density.back() == 2.0f);
    uint64_t kept = 0;
    CHECK(blok_affine_stamp_voxels(density.data(), ids.data(), origin, dims[0], dims[1], dims[2], xyz, mats, 2, &r, nullptr, nullptr, BLOK_STAMP_KEEP, 1.0f, &kept) == BLOK_OK);
    CHECK(kept == 0);
    CHECK(blok_affine_stamp_voxels(density.data(), ids.data(), origin, dims[0], dims[1], dims[2], xyz, mats, 2, &r, nullptr, nullptr, BLOK_STAMP_ERASE, 0.0f, &kept) == BLOK_OK);
    CHECK(kept == n && ids.back() == 0u);
    return 1;
}

}  // namespace

int main() {
    const uint32_t dims[3] = {70, 9, 6};
    const int32_t origins[2][3] = {{-32768, -32768, -32768}, {32768 - 70, 32768 - 9, 32768 - 6}};
    const int32_t reach = (1 << 20) - 1, M = 1 << 22;
    const int64_t T = int64_t(1) << 40;
    int cases = 0;
    for (const auto& origin : origins)
        for (int below = 0; below < 2; ++below)
            for (int sm = 0; sm < 2; ++sm)
                for (int st = 0; st < 2; ++st)
                    for (int mixed = 0; mixed < 2; ++mixed)
                        for (int zero_row = 0; zero_row < 2; ++zero_row) {
                            blok_affine r{};
                            for (int j = 0; j < 3; ++j)
                                r.anchor[j] = below ? origin[j] + int32_t(dims[j]) - 1 - reach : origin[j] + reach;
                            for (int k = 0; k < 3; ++k) {
                                for (int j = 0; j < 3; ++j) r.m[k][j] = (sm ? -M : M) * ((mixed && ((k + j) & 1)) ? -1 : 1);
                                r.t[k] = (st ? -T : T) * ((mixed && (k & 1)) ? -1 : 1);
                            }
                            if (zero_row) for (int j = 0; j < 3; ++j) r.m[1][j] = 0;      // rank below 3
                            cases += run_case(r, origin, dims);
                        }
    // one past each limit is refused; from_instance at its largest exponent; from_matrix at |m| = 2^22
    blok_affine r{};
    r.m[0][0] = M + 1;
    CHECK(A::well_formed(r, origins[0], dims) == A::kMatrix);
    r.m[0][0] = M; r.t[2] = -T - 1;
    CHECK(A::well_formed(r, origins[0], dims) == A::kTranslation);
    r.t[2] = -T; r.anchor[0] = origins[0][0] + (1 << 20);
    CHECK(A::well_formed(r, origins[0], dims) == A::kAnchor);
    r.anchor[0] = origins[0][0] + reach; r.reserved[4] = 1;
    CHECK(A::well_formed(r, origins[0], dims) == A::kReserved);
    blok_instance I{};
    I.offset[0] = 2147483647; I.offset[1] = -2147483647 - 1; I.axis[0] = 2; I.axis[1] = 0; I.axis[2] = 1; I.flip = 5;
    CHECK(blok_affine_from_instance(&I, 8, &r) == BLOK_OK && r.m[0][2] == -256 && r.t[0] == -128 && r.m[1][0] == 256 && r.t[2] == -128);
    CHECK(blok_affine_from_instance(&I, 9, &r) == BLOK_ERR_INVALID_ARG);
    const double f[12] = {1.0 / 64, 0, 0, -2147483648.0, 0, -1.0 / 64, 0, 2147483647.5, 0, 0, 1.0 / 64, 0.999};
    CHECK(blok_affine_from_matrix(f, &r) == BLOK_OK && r.m[0][0] == M && r.m[1][1] == -M && r.anchor[0] == -2147483647 - 1 && r.anchor[1] == 2147483647);
    const double g[12] = {1e-300, 0, 0, 0, 0, 1e-300, 0, 0, 0, 0, 1e-300, 0};
    CHECK(blok_affine_from_matrix(g, &r) == BLOK_ERR_INVALID_ARG);
    std::printf("affine ok %d\n", cases);
    return 0;
}
