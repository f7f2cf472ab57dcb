// A program of its own (tests/test_scroll_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/scroll.cpp): for every case
// file named on the command line — 10 int32 (nx ny nz, origin, delta, whether delta is passed or null), then the densities and the ids — it
// takes blok_scroll_plan, then blok_scroll_voxels into arrays of exactly the contracted size, and prints one line: the two return codes, a
// checksum of each output array and of each info record.
#include <cstdio>
#include <cstring>
#include <vector>

#include "blok_world.h"

static_assert(sizeof(blok_scroll_box) == 24 && sizeof(blok_scroll_info) == 200, "the sizes the header states");

template <class T>
static unsigned long long checksum(const T* v, size_t n) {
    unsigned long long s = 0;
    for (size_t i = 0; i < n; ++i) { uint32_t w = 0; std::memcpy(&w, &v[i], sizeof(uint32_t)); s += static_cast<unsigned long long>(w) * (i + 1u); }
    return s;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        int32_t h[10];
        if (!f || std::fread(h, sizeof(int32_t), 10, f) != 10) { std::printf("unreadable\n"); return 1; }
        const size_t cells = size_t(h[0]) * size_t(h[1]) * size_t(h[2]);
        std::vector<float> density(cells);
        std::vector<uint32_t> ids(cells);
        if (std::fread(density.data(), 4, cells, f) != cells || std::fread(ids.data(), 4, cells, f) != cells) { std::printf("short\n"); return 1; }
        std::fclose(f);
        const int32_t* delta = h[9] ? h + 6 : nullptr;
        blok_scroll_info planned, moved;
        std::memset(&planned, 0, sizeof planned);
        std::memset(&moved, 0, sizeof moved);
        const int rc_plan = blok_scroll_plan(h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), delta, &planned);
        std::vector<float> out_density(cells);                    // exactly the contracted sizes: a write past them is the sanitizer's to find
        std::vector<uint32_t> out_ids(cells);
        const int rc = blok_scroll_voxels(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), delta, out_density.data(),
                                          out_ids.data(), &moved);
        std::printf("%d %d %llu %llu %llu %llu\n", rc_plan, rc, checksum(out_density.data(), cells), checksum(out_ids.data(), cells),
                    checksum(reinterpret_cast<const uint32_t*>(&planned), sizeof planned / 4u), checksum(reinterpret_cast<const uint32_t*>(&moved), sizeof moved / 4u));
    }
    return 0;
}
