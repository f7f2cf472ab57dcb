// Built with -fsanitize=address,undefined by tests/test_terrain_lod_cpu.py: the tile arithmetic of csrc/common/terrain_lod_core.h — a
// column of voxels as bits along y — beside a loop that looks at one voxel at a time, over seeded tiles of random words; then the walks
// (column_solid, column_ore) beside terrain::solid and terrain::material voxel by voxel, and blok_terrain_reduce into arrays of exactly the
// planned size.  Prints "ok <tiles>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "blok_world.h"
#include "../../blok_amd/csrc/common/terrain_lod_core.h"

namespace T = blok::terrain;
namespace TL = blok::terrain_lod;

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t next() {                                       // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// words of several densities, the all-ones and all-zeros among them
uint64_t word() {
    switch (next() % 6u) {
        case 0: return 0ull;
        case 1: return ~0ull;
        case 2: return next() & next();
        case 3: return next() | next();
        default: return next();
    }
}

constexpr int kN = 4, kH = kN + 2;                      // a tile of 4 x 4 columns, 6 x 6 with its halo

// the vote, written again: the weights of equal ids add, the largest sum wins, a tie goes to the smallest id
uint32_t plain_vote(const std::vector<std::pair<uint32_t, uint32_t>>& weighted) {
    std::map<uint32_t, uint32_t> sums;
    for (const auto& [w, id] : weighted) if (w) sums[id] += w;
    uint32_t best = 0, best_sum = 0;
    for (const auto& [id, sum] : sums) if (sum > best_sum) { best = id; best_sum = sum; }      // (ascending ids: the first of a tie stays)
    return best;
}

bool tile(uint32_t t) {
    TL::Column col[kH][kH];                             // [z][x]
    int32_t height[kH][kH];
    bool in_region[kH][kH];
    const int32_t y0 = 2 * static_cast<int32_t>(next() % 200u) - 200;
    const int32_t row_lo = y0 - 3 + static_cast<int32_t>(next() % 40u), row_hi = row_lo + static_cast<int32_t>(next() % 70u);
    const uint32_t flags = static_cast<uint32_t>(next() % 2u) * BLOK_LOD_VOTE_EXPOSED;
    blok_terrain_params p{};
    p.soil_depth = static_cast<uint32_t>(next() % 5u) == 0u ? 0xFFFFFFFFu : static_cast<uint32_t>(next() % 6u);
    p.surface_material = 1u + static_cast<uint32_t>(next() % 3u); p.soil_material = 1u + static_cast<uint32_t>(next() % 3u);
    p.rock_material = static_cast<uint32_t>(next() % 3u); p.ore_material = 0xFFFFFFF0u + static_cast<uint32_t>(next() % 3u);
    for (int z = 0; z < kH; ++z)
        for (int x = 0; x < kH; ++x) {
            col[z][x] = TL::Column{word(), static_cast<uint32_t>(next() % 4u)};
            height[z][x] = y0 - 8 + static_cast<int32_t>(next() % 80u);
            in_region[z][x] = next() % 8u != 0u;
        }
    const uint64_t rows = TL::rows_in(y0, row_lo, row_hi);
    TL::Words words[kN][kN];
    uint64_t ore_source[kN][kN];
    for (int z = 0; z < kN; ++z)
        for (int x = 0; x < kN; ++x) {
            const TL::Column& c = col[z + 1][x + 1];
            TL::Words& w = words[z][x];
            w.filled = in_region[z + 1][x + 1] ? c.solid & rows : 0ull;
            w.exposed = TL::exposed(w.filled, c, col[z + 1][x].solid, col[z + 1][x + 2].solid, col[z][x + 1].solid, col[z + 2][x + 1].solid);
            TL::depth_words(height[z + 1][x + 1], y0, p.soil_depth, &w.soil, &w.deep);
            ore_source[z][x] = word();
        }
    for (int z = 0; z < kN; ++z)
        for (int x = 0; x < kN; ++x) {
            const uint64_t cell_exposed = words[z][x].exposed | words[z][x ^ 1].exposed | words[z ^ 1][x].exposed | words[z ^ 1][x ^ 1].exposed;
            const uint64_t votes = TL::voters(words[z][x].filled, words[z][x].exposed, cell_exposed, flags);
            words[z][x].ore = ore_source[z][x] & votes & words[z][x].deep;      // (the kernel asks the noise for these voxels alone)
        }
    // one voxel at a time
    const auto solid_at = [&](int x, int y, int z) -> bool {      // halo'd column (x, z), row y0 + y, -1 <= y <= 64
        const TL::Column& c = col[z][x];
        return y < 0 ? (c.halo & 1u) != 0u : y >= 64 ? (c.halo & 2u) != 0u : ((c.solid >> y) & 1ull) != 0ull;
    };
    const auto filled_at = [&](int x, int y, int z) { return in_region[z][x] && y0 + y >= row_lo && y0 + y < row_hi && solid_at(x, y, z); };
    const auto exposed_at = [&](int x, int y, int z) {
        return filled_at(x, y, z) && !(solid_at(x - 1, y, z) && solid_at(x + 1, y, z) && solid_at(x, y - 1, z) && solid_at(x, y + 1, z) && solid_at(x, y, z - 1) && solid_at(x, y, z + 1));
    };
    for (int cz = 0; cz < kN / 2; ++cz)
        for (int cx = 0; cx < kN / 2; ++cx)
            for (uint32_t pair = 0; pair < 32u; ++pair) {
                uint32_t want_n = 0, want_e = 0;
                std::vector<std::pair<uint32_t, uint32_t>> by_n, by_e;
                for (int dz = 0; dz < 2; ++dz)
                    for (int dy = 0; dy < 2; ++dy)
                        for (int dx = 0; dx < 2; ++dx) {
                            const int x = 2 * cx + dx + 1, z = 2 * cz + dz + 1, y = 2 * static_cast<int>(pair) + dy;
                            const bool f = filled_at(x, y, z), e = exposed_at(x, y, z);
                            want_n += f; want_e += e;
                            const int64_t d = int64_t(height[z][x]) - (int64_t(y0) + y);
                            // (a filled voxel above its column's height does not occur in the terrain: the words call it surface)
                            const uint32_t id = d <= 0 ? p.surface_material : d <= int64_t(p.soil_depth) ? p.soil_material
                                              : ((ore_source[z - 1][x - 1] >> y) & 1ull) ? p.ore_material : p.rock_material;
                            by_n.push_back({f ? 1u : 0u, id}); by_e.push_back({e ? 1u : 0u, id});
                        }
                const uint32_t want_id = !want_n ? 0u : plain_vote(((flags & BLOK_LOD_VOTE_EXPOSED) && want_e) ? by_e : by_n);
                const TL::Words four[4] = {words[2 * cz][2 * cx], words[2 * cz][2 * cx + 1], words[2 * cz + 1][2 * cx], words[2 * cz + 1][2 * cx + 1]};
                uint32_t n, e, id;
                TL::cell(four, pair, p, flags, &n, &e, &id);
                if (n != want_n || e != want_e || id != want_id) {
                    std::printf("tile %u cell (%d, %u, %d): n %u e %u id %u, per voxel n %u e %u id %u\n", t, cx, pair, cz, n, e, id, want_n, want_e, want_id);
                    return false;
                }
            }
    return true;
}

// the walks beside the function, and the host build into arrays of exactly the planned size
bool walks() {
    blok_terrain_params p{};
    p.seed = 0xB10C0001u; p.base_height = -20; p.amplitude = 48u; p.height_cell_log2 = 5u; p.height_octaves = 4u; p.cave_cell_log2 = 4u; p.cave_octaves = 2u;
    p.cave_threshold = 24000u; p.cave_roof = 3u; p.soil_depth = 3u; p.ore_cell_log2 = 3u; p.ore_threshold = 52000u;
    p.surface_material = 1u; p.soil_material = 2u; p.rock_material = 3u; p.ore_material = 4u; p.density = 1.5f;
    T::Walker w, v;
    for (uint32_t k = 0; k < 64u; ++k) {
        const int32_t X = static_cast<int32_t>(next() % 400u) - 200, Z = static_cast<int32_t>(next() % 400u) - 200;
        const int32_t y0 = 2 * (static_cast<int32_t>(next() % 60u) - 45), glo = y0 - 2 + static_cast<int32_t>(next() % 30u), ghi = glo + static_cast<int32_t>(next() % 80u);
        const int32_t H = T::height(p, X, Z);
        T::walker_reset(w); T::walker_reset(v);
        const TL::Column c = TL::column_solid(p, w, X, Z, H, y0, glo, ghi);
        for (int32_t y = -1; y <= 64; ++y) {
            const int32_t Y = y0 + y;
            const bool want = (Y < glo || Y >= ghi) ? true : T::solid(p, v, X, Y, Z, H);
            const bool got = y < 0 ? (c.halo & 1u) != 0u : y >= 64 ? (c.halo & 2u) != 0u : ((c.solid >> y) & 1ull) != 0ull;
            if (got != want) { std::printf("column (%d, %d) row %d: solid %d, the function %d\n", X, Z, Y, int(got), int(want)); return false; }
        }
        uint64_t soil, deep;
        TL::depth_words(H, y0, p.soil_depth, &soil, &deep);
        const uint64_t want_rows = c.solid & TL::rows_in(y0, glo, ghi) & deep & next();
        T::walker_reset(w);
        const uint64_t ore = TL::column_ore(p, w, X, Z, H, y0, want_rows);
        for (uint32_t y = 0; y < 64u; ++y) {
            if (!((want_rows >> y) & 1ull)) { if ((ore >> y) & 1ull) { std::printf("ore outside the rows asked for\n"); return false; } continue; }
            if ((((ore >> y) & 1ull) != 0ull) != (T::material(p, v, X, y0 + static_cast<int32_t>(y), Z, H) == p.ore_material)) { std::printf("column (%d, %d) row %u: ore differs\n", X, Z, y); return false; }
        }
    }
    for (uint32_t flags = 0; flags < 4u; ++flags) {
        const int32_t lo[3] = {-33, -27, 5}, hi[3] = {36, 21, 24};
        blok_lod_info info;
        if (blok_terrain_reduce(&p, lo, hi, 3u, flags, nullptr, 0u, &info) != BLOK_OK) { std::printf("plan refused\n"); return false; }
        uint64_t bytes = 0;
        for (uint32_t j = 0; j < 3u; ++j) bytes += 8u * info.level[j].n_cells;
        std::vector<uint8_t> planes(bytes);
        if (blok_terrain_reduce(&p, lo, hi, 3u, flags, planes.data(), bytes, &info) != BLOK_OK) { std::printf("reduce refused\n"); return false; }
        if (blok_terrain_reduce(&p, lo, hi, 3u, flags, planes.data(), bytes - 1u, &info) != BLOK_ERR_INVALID_ARG) { std::printf("a short array accepted\n"); return false; }
        uint64_t filled = 0;
        T::walker_reset(v);
        for (int32_t Z = lo[2]; Z < hi[2]; ++Z)
            for (int32_t X = lo[0]; X < hi[0]; ++X) {
                const int32_t H = T::height(p, X, Z);
                for (int32_t Y = lo[1]; Y < hi[1]; ++Y) filled += T::solid(p, v, X, Y, Z, H);
            }
        for (uint32_t j = 0; j < 3u; ++j)
            if (info.level[j].sum_n != filled) { std::printf("flags %u level %u: sum_n %llu, the function %llu\n", flags, j + 1u, (unsigned long long)info.level[j].sum_n, (unsigned long long)filled); return false; }
    }
    return true;
}

}  // namespace

int main() {
    const uint32_t tiles = 400u;
    for (uint32_t t = 0; t < tiles; ++t)
        if (!tile(t)) return 1;
    if (!walks()) return 1;
    std::printf("ok %u\n", tiles);
    return 0;
}
