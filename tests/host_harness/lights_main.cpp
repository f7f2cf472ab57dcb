// TEST INFRASTRUCTURE: a stand-alone program over the host light-table build (blok_amd/csrc/host/lights.cpp, csrc/common/lights_core.h) for
// the sanitizers (tests/test_lights_cpu.py).  Each argument is a case file: u64 n_quads, u64 n_materials, u64 n_lights, f32 voxel size,
// u32 pad, the quads, the materials, the expected lights.  The build is replayed (count call, exact capacity, short capacity), the table
// must pass blok_lights_check, and every pick in [0, A) of a table with A <= 65536 must land in the light and cell that owns it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blok_world.h"
#include "../../blok_amd/csrc/common/lights_core.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "lights_main: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)

namespace L = blok::lights;

static int one_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    uint64_t head[3]; float vs; uint32_t pad;
    REQUIRE(std::fread(head, sizeof(head), 1, f) == 1 && std::fread(&vs, 4, 1, f) == 1 && std::fread(&pad, 4, 1, f) == 1);
    REQUIRE(head[0] <= (1u << 22) && head[1] >= 1 && head[1] <= (1u << 17) && head[2] <= head[0]);
    std::vector<blok_quad> quads(head[0]);
    std::vector<blok_material> mats(head[1]);
    std::vector<blok_light> want(head[2]);
    REQUIRE(quads.empty() || std::fread(quads.data(), sizeof(blok_quad), quads.size(), f) == quads.size());
    REQUIRE(std::fread(mats.data(), sizeof(blok_material), mats.size(), f) == mats.size());
    REQUIRE(want.empty() || std::fread(want.data(), sizeof(blok_light), want.size(), f) == want.size());
    std::fclose(f);

    blok_lights_info info{};
    REQUIRE(blok_lights_from_quads(quads.data(), quads.size(), mats.data(), mats.size(), nullptr, 0, vs, &info) == BLOK_OK);
    REQUIRE(info.n == want.size());
    std::vector<blok_light> got(info.n);
    blok_lights_info again{};
    REQUIRE(blok_lights_from_quads(quads.data(), quads.size(), mats.data(), mats.size(), got.data(), got.size(), vs, &again) == BLOK_OK);
    REQUIRE(std::memcmp(&info, &again, sizeof(info)) == 0);
    REQUIRE(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(blok_light)) == 0);
    if (got.size() > 1) {      // a short capacity writes a prefix and nothing behind it
        std::vector<blok_light> part(got.size(), blok_light{{7, 7, 7}, 7, 7, 7, 7, 7});
        REQUIRE(blok_lights_from_quads(quads.data(), quads.size(), mats.data(), mats.size(), part.data(), got.size() / 2, vs, nullptr) == BLOK_OK);
        REQUIRE(std::memcmp(part.data(), want.data(), (got.size() / 2) * sizeof(blok_light)) == 0 && part[got.size() / 2].face == 7u);
    }
    char err[128];
    blok_lights_info checked{};
    REQUIRE(blok_lights_check(got.data(), got.size(), &checked, err, sizeof(err)) == BLOK_OK && checked.n_faces == info.n_faces);
    if (info.n && info.n_faces <= 65536u) {
        uint32_t light = 0;
        for (uint32_t pick = 0; pick < info.n_faces; ++pick) {
            while (light + 1u < info.n && got[light + 1u].cum <= pick) ++light;
            REQUIRE(L::find_light(got.data(), info.n, pick) == light);
            const uint32_t off = pick - got[light].cum;
            REQUIRE(off < got[light].du * got[light].dv);
            float q[3], nl[3];
            L::sample_point(got[light], off, 0.5f, 0.5f, vs, q, nl);
            const uint32_t a = got[light].face >> 1;
            REQUIRE(q[a] == float(got[light].lo[a]) * vs && nl[a] == ((got[light].face & 1u) ? -1.0f : 1.0f));
        }
    }
    std::printf("lights_main: %s: %u lights, %llu faces\n", path, info.n, static_cast<unsigned long long>(info.n_faces));
    return 0;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) if (one_file(argv[a])) return 1;
    // the ends of the pick: never A itself
    const uint32_t rs[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu}, faces[] = {1u, 2u, 6u, 4096u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (const uint32_t r : rs) for (const uint32_t n : faces) REQUIRE(L::pick_of(r, n) < n);
    // the rules, one broken at a time
    const blok_light good[2] = {{{0, 0, 0}, 2, 3, 1, 0, 0}, {{5, 5, 5}, 1, 1, 1, 5, 6}};
    char err[128];
    REQUIRE(blok_lights_check(good, 2, nullptr, err, sizeof(err)) == BLOK_OK);
    blok_light bad[2];
    std::memcpy(bad, good, sizeof(good)); bad[1].face = 6;
    REQUIRE(blok_lights_check(bad, 2, nullptr, err, sizeof(err)) == BLOK_ERR_INVALID_ARG && std::strstr(err, "light 1"));
    std::memcpy(bad, good, sizeof(good)); bad[0].dv = 0;
    REQUIRE(blok_lights_check(bad, 2, nullptr, err, sizeof(err)) == BLOK_ERR_INVALID_ARG);
    std::memcpy(bad, good, sizeof(good)); bad[1].cum = 5;
    REQUIRE(blok_lights_check(bad, 2, nullptr, err, sizeof(err)) == BLOK_ERR_INVALID_ARG);
    std::memcpy(bad, good, sizeof(good)); bad[1].lo[2] = 32769;
    REQUIRE(blok_lights_check(bad, 2, nullptr, err, sizeof(err)) == BLOK_ERR_INVALID_ARG);
    const blok_light forged[1] = {{{-32768, -32768, -32768}, 65536, 65536, 1, 4, 0}};
    REQUIRE(blok_lights_check(forged, 1, nullptr, err, sizeof(err)) == BLOK_ERR_UNSUPPORTED);
    std::puts("lights_main: ok");
    return 0;
}
