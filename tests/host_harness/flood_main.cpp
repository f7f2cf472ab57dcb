// A program of its own (tests/test_flood_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/flood.cpp): for every case
// file named on the command line — 19 int32 (nx ny nz, origin, whole, lo, hi, n_seeds, K, flags, material, op, d), then the densities, the
// ids and the seeds — it takes blok_flood_field into an array of exactly the region's size, applies blok_flood_edit, and prints one line:
// the two return codes, the info's counts, the cells written and a checksum of the field and of both arrays.
#include <cstdio>
#include <cstring>
#include <vector>

#include "blok_world.h"

template <class T>
static unsigned long long checksum(const std::vector<T>& v) {
    unsigned long long s = 0;
    for (size_t i = 0; i < v.size(); ++i) { uint32_t w = 0; std::memcpy(&w, &v[i], sizeof(T)); s += static_cast<unsigned long long>(w) * (i + 1u); }
    return s;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        int32_t h[19];
        if (!f || std::fread(h, sizeof(int32_t), 19, f) != 19) { std::printf("unreadable\n"); return 1; }
        const size_t cells = size_t(h[0]) * size_t(h[1]) * size_t(h[2]);
        std::vector<float> density(cells);
        std::vector<uint32_t> ids(cells);
        std::vector<int32_t> seeds(3u * size_t(h[13]));
        if (std::fread(density.data(), 4, cells, f) != cells || std::fread(ids.data(), 4, cells, f) != cells ||
            std::fread(seeds.data(), 4, seeds.size(), f) != seeds.size()) { std::printf("short\n"); return 1; }
        std::fclose(f);
        const int32_t* lo = h[6] ? nullptr : h + 7;
        const int32_t* hi = h[6] ? nullptr : h + 10;
        size_t region = cells;
        if (!h[6]) { region = 1; for (int a = 0; a < 3; ++a) region *= h[10 + a] > h[7 + a] ? size_t(h[10 + a] - h[7 + a]) : 0u; }
        std::vector<uint16_t> field(region);                      // exactly the region: a write past it is the sanitizer's to find
        blok_flood_info info;
        std::memset(&info, 0, sizeof info);
        const int rc = blok_flood_field(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), lo, hi, seeds.empty() ? nullptr : seeds.data(),
                                        seeds.size() / 3u, uint32_t(h[14]), uint32_t(h[15]), uint32_t(h[16]), field.data(), &info);
        unsigned long long written = 0;
        int rc_edit = -99;
        if (rc == BLOK_OK) rc_edit = blok_flood_edit(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), field.data(), &info, h[17], uint32_t(h[18]), 0.75f, 6u,
                                                     reinterpret_cast<uint64_t*>(&written));
        std::printf("%d %d %u %llu %llu %llu %llu %llu %llu %llu\n", rc, rc_edit, info.farthest, (unsigned long long)info.n_seed, (unsigned long long)info.n_reached,
                    (unsigned long long)info.n_unreached, written, checksum(field), checksum(density), checksum(ids));
    }
    return 0;
}
