// TEST INFRASTRUCTURE: a stand-alone program over the host light-grid build (blok_amd/csrc/host/light_grid.cpp, csrc/common/lights_core.h)
// for the sanitizers (tests/test_light_grid_cpu.py).  Each argument is a case file: u64 n_lights, u64 n_cells, u64 n_items, u32 cell_log2,
// u32 reach, the lights, then the expected start (n_cells + 1 words), faces (n_cells words) and items.  The build is replayed (count call,
// exact capacities, capacities one short), the arrays compared, and for grids of at most 2^20 cell-light pairs every list is checked
// against in_cell over every light.  Behind the files: the parameter ranges and the two limits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blok_world.h"
#include "../../blok_amd/csrc/common/lights_core.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "light_grid_main: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)

namespace L = blok::lights;

static int one_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    uint64_t head[3]; uint32_t par[2];
    REQUIRE(std::fread(head, sizeof(head), 1, f) == 1 && std::fread(par, sizeof(par), 1, f) == 1);
    REQUIRE(head[0] >= 1 && head[0] <= (1u << 20) && head[1] <= (1u << 24) && head[2] < (1u << 28));
    std::vector<blok_light> lights(head[0]);
    std::vector<uint32_t> want_start(head[1] + 1), want_faces(head[1]);
    std::vector<blok_light_grid_item> want_items(head[2]);
    REQUIRE(std::fread(lights.data(), sizeof(blok_light), lights.size(), f) == lights.size());
    REQUIRE(std::fread(want_start.data(), 4, want_start.size(), f) == want_start.size());
    REQUIRE(std::fread(want_faces.data(), 4, want_faces.size(), f) == want_faces.size());
    REQUIRE(want_items.empty() || std::fread(want_items.data(), sizeof(blok_light_grid_item), want_items.size(), f) == want_items.size());
    std::fclose(f);
    const uint32_t c = par[0], R = par[1], share = 192u;

    blok_light_grid_info info{};
    REQUIRE(blok_light_grid_build(lights.data(), lights.size(), c, R, share, nullptr, nullptr, nullptr, 0, 0, &info) == BLOK_OK);
    REQUIRE(info.n_cells == head[1] && info.n_items == head[2] && info.cell_log2 == c && info.reach == R && info.share == share && info.reserved == 0u);
    REQUIRE(info.n_cells == uint64_t(info.dim[0]) * info.dim[1] * info.dim[2] && info.bytes == (2 * info.n_cells + 1) * 4 + info.n_items * 8);
    // exactly as large as needed: the sanitizer sees a write one past any of them
    std::vector<uint32_t> start(info.n_cells + 1), faces(info.n_cells);
    std::vector<blok_light_grid_item> items(info.n_items);
    blok_light_grid_info again{};
    REQUIRE(blok_light_grid_build(lights.data(), lights.size(), c, R, share, start.data(), faces.data(), items.data(), info.n_cells, info.n_items, &again) == BLOK_OK);
    REQUIRE(std::memcmp(&info, &again, sizeof(info)) == 0);
    REQUIRE(std::memcmp(start.data(), want_start.data(), start.size() * 4) == 0);
    REQUIRE(std::memcmp(faces.data(), want_faces.data(), faces.size() * 4) == 0);
    REQUIRE(items.empty() || std::memcmp(items.data(), want_items.data(), items.size() * sizeof(blok_light_grid_item)) == 0);
    // a capacity one short, or one array missing: refused, nothing written
    std::vector<uint32_t> untouched(start.size(), 0xABABABABu);
    REQUIRE(blok_light_grid_build(lights.data(), lights.size(), c, R, share, untouched.data(), faces.data(), items.data(), info.n_cells - 1, info.n_items, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(lights.data(), lights.size(), c, R, share, untouched.data(), faces.data(), items.data(), info.n_cells, info.n_items - 1, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(lights.data(), lights.size(), c, R, share, untouched.data(), nullptr, items.data(), info.n_cells, info.n_items, nullptr) == BLOK_ERR_INVALID_ARG);
    for (const uint32_t w : untouched) REQUIRE(w == 0xABABABABu);
    // the lists against the predicate, the figures against the lists
    uint32_t nonempty = 0, longest = 0;
    for (uint64_t g = 0; g < info.n_cells; ++g) {
        const uint32_t len = start[g + 1] - start[g];
        nonempty += len ? 1u : 0u;
        longest = len > longest ? len : longest;
    }
    REQUIRE(nonempty == info.n_nonempty && longest == info.max_items && start[0] == 0u && start[info.n_cells] == info.n_items);
    if (info.n_cells * lights.size() <= (1u << 20)) {
        for (uint32_t z = 0; z < info.dim[2]; ++z) for (uint32_t y = 0; y < info.dim[1]; ++y) for (uint32_t x = 0; x < info.dim[0]; ++x) {
            const uint64_t g = (uint64_t(z) * info.dim[1] + y) * info.dim[0] + x;
            uint32_t at = start[g], sum = 0;
            for (uint32_t i = 0; i < lights.size(); ++i) {
                const L::CellRange r = L::light_cells(lights[i], c);
                if (!L::in_cell(r, R, info.cell_lo[0] + int32_t(x), info.cell_lo[1] + int32_t(y), info.cell_lo[2] + int32_t(z))) continue;
                REQUIRE(at < start[g + 1] && items[at].light == i && items[at].lcum == sum);
                at += 1; sum += lights[i].du * lights[i].dv;
            }
            REQUIRE(at == start[g + 1] && faces[g] == sum);
        }
    }
    std::printf("light_grid_main: %s: %llu cells, %llu items\n", path, static_cast<unsigned long long>(info.n_cells), static_cast<unsigned long long>(info.n_items));
    return 0;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) if (one_file(argv[a])) return 1;
    const blok_light one[1] = {{{5, -3, 9}, 1, 1, 3, 2, 0}};
    blok_light_grid_info info{};
    // the parameter ranges
    REQUIRE(blok_light_grid_build(one, 1, 2, 0, 1, nullptr, nullptr, nullptr, 0, 0, &info) == BLOK_OK && info.n_cells == 1 && info.n_items == 1);
    REQUIRE(blok_light_grid_build(one, 1, 12, 3, 255, nullptr, nullptr, nullptr, 0, 0, &info) == BLOK_OK && info.n_cells == 343 && info.n_items == 343 && info.max_items == 1);
    REQUIRE(blok_light_grid_build(one, 1, 1, 0, 1, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(one, 1, 13, 0, 1, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(one, 1, 4, 4, 1, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(one, 1, 4, 1, 0, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(one, 1, 4, 1, 256, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(one, 0, 4, 1, 128, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    REQUIRE(blok_light_grid_build(nullptr, 1, 4, 1, 128, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    const blok_light bad[1] = {{{5, -3, 9}, 1, 1, 3, 2, 7}};      // cum is not the running sum
    REQUIRE(blok_light_grid_build(bad, 1, 4, 1, 128, nullptr, nullptr, nullptr, 0, 0, nullptr) == BLOK_ERR_INVALID_ARG);
    // the limits: nothing is allocated for a grid beyond them, so the count call answers at once
    const blok_light corners[2] = {{{-32768, -32768, -32768}, 1, 1, 3, 1, 0}, {{32767, 32767, 32767}, 1, 1, 3, 1, 1}};
    REQUIRE(blok_light_grid_build(corners, 2, 2, 3, 128, nullptr, nullptr, nullptr, 0, 0, &info) == BLOK_ERR_UNSUPPORTED && info.n_cells > (1ull << 24) && info.n_items == 2 * 343);
    std::vector<blok_light> plates(37, blok_light{{0, 0, 0}, 4096, 4096, 3, 4, 0});
    for (uint32_t i = 0; i < plates.size(); ++i) plates[i].cum = i << 24;
    REQUIRE(blok_light_grid_build(plates.data(), plates.size(), 2, 3, 128, nullptr, nullptr, nullptr, 0, 0, &info) == BLOK_ERR_UNSUPPORTED);
    REQUIRE(info.n_cells == 1030ull * 1030 * 7 && info.n_items == 37ull * 1030 * 1030 * 7 && info.n_items >= (1ull << 28));
    std::puts("light_grid_main: ok");
    return 0;
}
