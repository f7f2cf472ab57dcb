// A program of its own (tests/test_automaton_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/automaton.cpp, which
// carries csrc/common/automaton_core.h): for every case file named on the command line — 13 int32 (nx ny nz, origin, whether a region is
// passed, its lo and hi), a blok_automaton_rule, then the densities and the ids — it runs
//   1. blok_automaton_voxels, the host build's loop per cell, on arrays of exactly the box's size, and
//   2. the same call on the whole-brick arithmetic of automaton_core.h, exactly what the decide kernel runs on the device: brick masks from
//      density > 0, seen() of the 27 bricks around every brick of the region, brick_step, then the births (with the vote) and the deaths
//      from the born and died words,
// and prints one line: the return code, steps_run, the three counts, checksums of the two arrays and of the step counts, and whether the
// brick run equals the cell loop bit for bit (arrays, step counts, info).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "blok_world.h"
#include "../../blok_amd/csrc/common/automaton_core.h"

namespace K = blok::automaton;

static unsigned long long checksum(const void* p, size_t n_words) {
    unsigned long long s = 0;
    for (size_t i = 0; i < n_words; ++i) { uint32_t w = 0; std::memcpy(&w, static_cast<const char*>(p) + 4u * i, sizeof(uint32_t)); s += static_cast<unsigned long long>(w) * (i + 1u); }
    return s;
}

// The call on whole bricks; the arguments have passed the cell loop's checks, the region [lo, hi) is box-local and not empty.
static void run_on_bricks(std::vector<float>& density, std::vector<uint32_t>& ids, const int32_t origin[3], const uint32_t dims[3], const uint32_t lo[3],
                          const uint32_t hi[3], const blok_automaton_rule& rule, std::vector<uint64_t>& step_counts, blok_automaton_info* info) {
    K::plan(origin, lo, hi, rule.flags, info);
    const uint32_t nb[3] = {(dims[0] + 3u) / 4u, (dims[1] + 3u) / 4u, (dims[2] + 3u) / 4u};
    const bool solid = (rule.flags & BLOK_AUTOMATON_BOX_IS_SOLID) != 0u, fixed = (rule.flags & BLOK_AUTOMATON_FIXED_MATERIAL) != 0u;
    const auto cell = [&](uint32_t x, uint32_t y, uint32_t z) { return (size_t(z) * dims[1] + y) * dims[0] + x; };
    const auto brick = [&](uint32_t bx, uint32_t by, uint32_t bz) { return bx + (size_t(bz) * nb[1] + by) * nb[0]; };
    std::vector<uint64_t> masks(size_t(nb[0]) * nb[1] * nb[2]), born(masks.size()), died(masks.size());
    for (uint32_t step = 0; step < rule.steps; ++step) {
        std::fill(masks.begin(), masks.end(), 0ull);
        for (uint32_t z = 0; z < dims[2]; ++z)
            for (uint32_t y = 0; y < dims[1]; ++y)
                for (uint32_t x = 0; x < dims[0]; ++x)
                    if (density[cell(x, y, z)] > 0.0f) masks[brick(x >> 2, y >> 2, z >> 2)] |= 1ull << ((x & 3u) | ((y & 3u) << 2) | ((z & 3u) << 4));
        uint64_t n_born = 0, n_died = 0, n_filled = 0;
        for (uint32_t bz = lo[2] / 4u; bz <= (hi[2] - 1u) / 4u; ++bz)
            for (uint32_t by = lo[1] / 4u; by <= (hi[1] - 1u) / 4u; ++by)
                for (uint32_t bx = lo[0] / 4u; bx <= (hi[0] - 1u) / 4u; ++bx) {
                    uint64_t seen27[27];
                    for (uint32_t j = 0; j < 27u; ++j) {
                        const uint32_t qx = bx + j % 3u - 1u, qy = by + (j / 3u) % 3u - 1u, qz = bz + j / 9u - 1u;
                        const bool in_grid = qx < nb[0] && qy < nb[1] && qz < nb[2];
                        seen27[j] = K::seen(in_grid ? masks[brick(qx, qy, qz)] : 0ull, in_grid, qx, qy, qz, dims, solid);
                    }
                    const size_t b = brick(bx, by, bz);
                    const uint64_t cells = K::region_cells(bx, by, bz, lo, hi);
                    K::brick_step(seen27, masks[b], cells, rule.neighbourhood, rule.survive, rule.birth, &born[b], &died[b]);
                    n_born += uint64_t(__builtin_popcountll(born[b])); n_died += uint64_t(__builtin_popcountll(died[b]));
                    n_filled += uint64_t(__builtin_popcountll(masks[b] & cells));
                }
        info->steps_run = step + 1u;
        info->n_filled = n_filled;
        if (!n_born && !n_died) break;
        for (int pass = 0; pass < 2; ++pass)                  // the births, then the deaths
            for (uint32_t bz = lo[2] / 4u; bz <= (hi[2] - 1u) / 4u; ++bz)
                for (uint32_t by = lo[1] / 4u; by <= (hi[1] - 1u) / 4u; ++by)
                    for (uint32_t bx = lo[0] / 4u; bx <= (hi[0] - 1u) / 4u; ++bx) {
                        const uint64_t word = pass == 0 ? born[brick(bx, by, bz)] : died[brick(bx, by, bz)];
                        for (uint32_t c = 0; c < 64u; ++c) {
                            if (!((word >> c) & 1ull)) continue;
                            const uint32_t x = 4u * bx + (c & 3u), y = 4u * by + ((c >> 2) & 3u), z = 4u * bz + (c >> 4);
                            if (pass == 1) { density[cell(x, y, z)] = 0.0f; ids[cell(x, y, z)] = 0u; continue; }
                            uint32_t cast[26], voters = 0u;
                            for (uint32_t i = 0; i < 26u; ++i) {
                                cast[i] = 0u;
                                if (i >= rule.neighbourhood) continue;
                                int32_t d[3];
                                K::offset(i, d);
                                const uint32_t qx = x + uint32_t(d[0]), qy = y + uint32_t(d[1]), qz = z + uint32_t(d[2]);
                                if (qx >= dims[0] || qy >= dims[1] || qz >= dims[2]) continue;
                                if (!((masks[brick(qx >> 2, qy >> 2, qz >> 2)] >> ((qx & 3u) | ((qy & 3u) << 2) | ((qz & 3u) << 4))) & 1ull)) continue;
                                voters |= 1u << i; cast[i] = ids[cell(qx, qy, qz)];
                            }
                            density[cell(x, y, z)] = rule.density;
                            ids[cell(x, y, z)] = fixed ? rule.material : K::vote([&](uint32_t i) { return cast[i]; }, rule.neighbourhood, voters, rule.material);
                        }
                    }
        info->n_born += n_born; info->n_died += n_died;
        info->n_filled = n_filled + n_born - n_died;
        step_counts[2u * step] = n_born; step_counts[2u * step + 1u] = n_died;
    }
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        int32_t h[13];
        blok_automaton_rule rule;
        if (!f || std::fread(h, sizeof(int32_t), 13, f) != 13 || std::fread(&rule, sizeof rule, 1, f) != 1) { std::printf("unreadable\n"); return 1; }
        const size_t cells = size_t(h[0]) * size_t(h[1]) * size_t(h[2]);
        std::vector<float> density(cells);
        std::vector<uint32_t> ids(cells);
        if (std::fread(density.data(), 4, cells, f) != cells || std::fread(ids.data(), 4, cells, f) != cells) { std::printf("short\n"); return 1; }
        std::fclose(f);
        const int32_t* lo = h[6] ? h + 7 : nullptr;
        const int32_t* hi = h[6] ? h + 10 : nullptr;
        const uint32_t n_counts = rule.steps >= 1u && rule.steps <= 255u ? 2u * rule.steps : 0u;
        std::vector<float> d2 = density;
        std::vector<uint32_t> m2 = ids;
        std::vector<uint64_t> counts(n_counts, 0u), counts2(n_counts, 0u);      // exactly 2 * steps: a write past it is the sanitizer's to find
        blok_automaton_info info, info2;
        std::memset(&info, 0, sizeof info);
        std::memset(&info2, 0, sizeof info2);
        const int rc = blok_automaton_voxels(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), lo, hi, &rule,
                                             n_counts ? counts.data() : nullptr, &info);
        int same = -1;                                          // -1: nothing to compare (a refusal, or an empty region)
        if (rc == BLOK_OK && info.ext[0] && info.ext[1] && info.ext[2]) {
            const uint32_t dims[3] = {uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2])};
            uint32_t l[3], u[3];
            for (int a = 0; a < 3; ++a) { l[a] = lo ? uint32_t(lo[a] - h[3 + a]) : 0u; u[a] = hi ? uint32_t(hi[a] - h[3 + a]) : dims[a]; }
            run_on_bricks(d2, m2, h + 3, dims, l, u, rule, counts2, &info2);
            same = std::memcmp(d2.data(), density.data(), 4u * cells) == 0 && std::memcmp(m2.data(), ids.data(), 4u * cells) == 0 && counts2 == counts &&
                   std::memcmp(&info, &info2, sizeof info) == 0;
        }
        std::printf("%d %u %llu %llu %llu %llu %llu %llu %d\n", rc, info.steps_run, static_cast<unsigned long long>(info.n_born), static_cast<unsigned long long>(info.n_died),
                    static_cast<unsigned long long>(info.n_filled), checksum(density.data(), cells), checksum(ids.data(), cells), checksum(counts.data(), 2u * counts.size()), same);
    }
    return 0;
}
