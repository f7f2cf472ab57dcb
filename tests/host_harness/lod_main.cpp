// A program of its own (tests/test_lod_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/lod.cpp, which carries
// csrc/common/lod_core.h): for every case file named on the command line — 15 int32 (nx ny nz, origin, whether a region is passed, its lo and
// hi, levels, flags), then the densities and the ids — it takes blok_lod_reduce's plan, then the reduction into an array of exactly the
// planned size, and prints one line: the two return codes, the planned bytes, and a checksum of the planes and of the info.
#include <cstdio>
#include <cstring>
#include <vector>

#include "blok_world.h"

static_assert(sizeof(blok_lod_level) == 64 && sizeof(blok_lod_info) == 360, "the sizes the header states");

static unsigned long long checksum(const void* p, size_t n_words) {
    unsigned long long s = 0;
    for (size_t i = 0; i < n_words; ++i) { uint32_t w = 0; std::memcpy(&w, static_cast<const char*>(p) + 4u * i, sizeof(uint32_t)); s += static_cast<unsigned long long>(w) * (i + 1u); }
    return s;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        int32_t h[15];
        if (!f || std::fread(h, sizeof(int32_t), 15, f) != 15) { std::printf("unreadable\n"); return 1; }
        const size_t cells = size_t(h[0]) * size_t(h[1]) * size_t(h[2]);
        std::vector<float> density(cells);
        std::vector<uint32_t> ids(cells);
        if (std::fread(density.data(), 4, cells, f) != cells || std::fread(ids.data(), 4, cells, f) != cells) { std::printf("short\n"); return 1; }
        std::fclose(f);
        const int32_t* lo = h[6] ? h + 7 : nullptr;
        const int32_t* hi = h[6] ? h + 10 : nullptr;
        blok_lod_info planned, info;
        std::memset(&planned, 0, sizeof planned);
        std::memset(&info, 0, sizeof info);
        const int rc_plan = blok_lod_reduce(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), lo, hi, uint32_t(h[13]), uint32_t(h[14]),
                                            nullptr, 0, &planned);
        uint64_t bytes = 0;
        for (uint32_t j = 0; j < 5u; ++j) bytes += 8u * planned.level[j].n_cells;
        std::vector<unsigned char> planes(bytes);                  // exactly the planned size: a write past it is the sanitizer's to find
        const int rc = blok_lod_reduce(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), lo, hi, uint32_t(h[13]), uint32_t(h[14]),
                                       bytes ? planes.data() : nullptr, bytes, &info);
        std::printf("%d %d %llu %llu %llu\n", rc_plan, rc, static_cast<unsigned long long>(bytes), checksum(planes.data(), bytes / 4u), checksum(&info, sizeof info / 4u));
    }
    return 0;
}
