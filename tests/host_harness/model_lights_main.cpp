// TEST INFRASTRUCTURE: a stand-alone program over the host build of a model's light table and the record map
// (blok_amd/csrc/host/model_lights.cpp, csrc/common/lights_core.h) for the sanitizers (tests/test_model_lights_cpu.py).  Each argument is
// a case file: u64 n_voxels, u64 n_materials, u64 n_faces, the voxels (3 x i32 each), their ids (u32), the materials, the expected table.
// The build is replayed (count call, exact capacity, short capacity); then every orientation x exponent x face of the record map is checked
// against the rule restated over the cell's corners.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blok_world.h"
#include "../../blok_amd/csrc/common/lights_core.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "model_lights_main: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)

static int one_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    uint64_t head[3];
    REQUIRE(std::fread(head, sizeof(head), 1, f) == 1);
    REQUIRE(head[0] >= 1 && head[0] <= (1u << 20) && head[1] >= 1 && head[1] <= (1u << 17) && head[2] <= 6 * head[0]);
    std::vector<int32_t> xyz(3 * head[0]);
    std::vector<uint32_t> ids(head[0]);
    std::vector<blok_material> mats(head[1]);
    std::vector<blok_light> want(head[2]);
    REQUIRE(std::fread(xyz.data(), sizeof(int32_t), xyz.size(), f) == xyz.size());
    REQUIRE(std::fread(ids.data(), sizeof(uint32_t), ids.size(), f) == ids.size());
    REQUIRE(std::fread(mats.data(), sizeof(blok_material), mats.size(), f) == mats.size());
    REQUIRE(want.empty() || std::fread(want.data(), sizeof(blok_light), want.size(), f) == want.size());
    std::fclose(f);

    uint64_t n = ~0ull;
    REQUIRE(blok_model_lights(xyz.data(), ids.data(), ids.size(), mats.data(), mats.size(), nullptr, 0, &n) == BLOK_OK && n == want.size());
    std::vector<blok_light> got(n);
    REQUIRE(blok_model_lights(xyz.data(), ids.data(), ids.size(), mats.data(), mats.size(), got.data(), got.size(), &n) == BLOK_OK && n == want.size());
    REQUIRE(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(blok_light)) == 0);
    if (got.size() > 1) {      // a short capacity writes a prefix and nothing behind it
        std::vector<blok_light> part(got.size(), blok_light{{7, 7, 7}, 7, 7, 7, 7, 7});
        REQUIRE(blok_model_lights(xyz.data(), ids.data(), ids.size(), mats.data(), mats.size(), part.data(), got.size() / 2, &n) == BLOK_OK && n == want.size());
        REQUIRE(std::memcmp(part.data(), want.data(), (got.size() / 2) * sizeof(blok_light)) == 0 && part[got.size() / 2].face == 7u);
    }
    REQUIRE(blok_model_lights(nullptr, ids.data(), ids.size(), mats.data(), mats.size(), nullptr, 0, &n) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_model_lights(xyz.data(), ids.data(), ids.size(), mats.data(), 0, nullptr, 0, &n) == BLOK_ERR_INVALID_ARG);
    std::printf("model_lights_main: %s: %llu faces\n", path, static_cast<unsigned long long>(want.size()));
    return 0;
}

static int record_map() {
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const uint32_t exps[] = {0u, 1u, 3u, 8u};
    const int32_t cell[3] = {-3, 5, 2};
    for (const auto& p : perms) for (uint32_t flip = 0; flip < 8u; ++flip) for (const uint32_t e : exps) for (uint32_t face = 0; face < 6u; ++face) {
        blok_instance I{};
        I.model = 4u; I.offset[0] = 100; I.offset[1] = -200; I.offset[2] = 32000;
        for (int k = 0; k < 3; ++k) I.axis[k] = static_cast<uint8_t>(p[k]);
        I.flip = static_cast<uint8_t>(flip);
        blok_light m{};
        for (int k = 0; k < 3; ++k) m.lo[k] = cell[k];
        if (!(face & 1u)) m.lo[face >> 1] += 1;
        m.du = m.dv = 1u; m.material = 77u; m.face = face; m.cum = 9u;
        blok_light w{};
        blok_instance_light_record(&I, e, &m, &w);
        const int64_t s = int64_t(1) << e;
        REQUIRE(w.du == s && w.dv == s && w.material == 77u && w.cum == 0u && w.face < 6u);
        for (int k = 0; k < 3; ++k) {
            const int a = p[k];
            const bool f = (flip >> k) & 1u;
            const int64_t low = f ? I.offset[a] - (int64_t(cell[k]) + 1) * s : I.offset[a] + int64_t(cell[k]) * s;
            if (static_cast<uint32_t>(k) == (face >> 1)) {
                const uint32_t n = (face & 1u) ^ (f ? 1u : 0u);
                REQUIRE(w.face == 2u * static_cast<uint32_t>(a) + n && w.lo[a] == low + (n ? 0 : s));
            } else {
                REQUIRE(w.lo[a] == low);
            }
        }
    }
    blok_light untouched{{1, 2, 3}, 4, 5, 6, 7, 8};
    blok_instance_light_record(nullptr, 0u, nullptr, &untouched);
    REQUIRE(untouched.cum == 8u);
    return 0;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) if (one_file(argv[a])) return 1;
    if (record_map()) return 1;
    std::puts("model_lights_main: ok");
    return 0;
}
