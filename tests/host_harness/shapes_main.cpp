// A program of its own (tests/test_shapes_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/shapes.cpp): for every case
// file named on the command line — 7 int32 (nx ny nz, origin, the number of shapes), the shape records, then the densities and the ids — it
// takes blok_shapes_check, blok_shape_bounds of every shape, and blok_shapes_voxels over arrays of exactly the contracted size, and prints
// one line: the two return codes, the written count and a checksum of each array.
#include <cstdio>
#include <cstring>
#include <vector>

#include "blok_world.h"

static_assert(sizeof(blok_shape) == 64, "the size the header states");

template <class T>
static unsigned long long checksum(const T* v, size_t n) {
    unsigned long long s = 0;
    for (size_t i = 0; i < n; ++i) { uint32_t w = 0; std::memcpy(&w, &v[i], sizeof(uint32_t)); s += static_cast<unsigned long long>(w) * (i + 1u); }
    return s;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        int32_t h[7];
        if (!f || std::fread(h, sizeof(int32_t), 7, f) != 7) { std::printf("unreadable\n"); return 1; }
        const size_t cells = size_t(h[0]) * size_t(h[1]) * size_t(h[2]), n = size_t(h[6]);
        std::vector<blok_shape> shapes(n);                         // exactly the contracted sizes: an access past them is the sanitizer's to find
        std::vector<float> density(cells);
        std::vector<uint32_t> ids(cells);
        if (std::fread(shapes.data(), sizeof(blok_shape), n, f) != n || std::fread(density.data(), 4, cells, f) != cells || std::fread(ids.data(), 4, cells, f) != cells) {
            std::printf("short\n");
            return 1;
        }
        std::fclose(f);
        uint32_t bad = 0;
        char err[128];
        const int rc_check = blok_shapes_check(shapes.data(), uint32_t(n), &bad, err, sizeof err);
        for (size_t k = 0; k < n; ++k) {
            int32_t lo[3], hi[3];
            (void)blok_shape_bounds(&shapes[k], lo, hi);
        }
        uint64_t written = 0;
        const int rc = blok_shapes_voxels(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), shapes.data(), uint32_t(n), &written);
        std::printf("%d %d %llu %llu %llu\n", rc_check, rc, static_cast<unsigned long long>(written), checksum(density.data(), cells), checksum(ids.data(), cells));
    }
    return 0;
}
