// A program of its own (tests/test_columns_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/columns.cpp): for every case
// file named on the command line — 16 int32 (nx ny nz, origin, whole, lo, hi, axis, flags, n_entries), then the densities and the ids, then
// with n_entries > 0 one blok_scatter_params and the entries — it takes blok_column_field into planes of exactly the contracted size, then
// blok_scatter, counting first and then into a table of exactly n_placed records, and prints one line: the field's return code, its info's
// counts and a checksum of each plane; the scatter's return code (-99: not run), its info's counts and a checksum of the table.
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
        int32_t h[16];
        if (!f || std::fread(h, sizeof(int32_t), 16, f) != 16) { std::printf("unreadable\n"); return 1; }
        const size_t cells = size_t(h[0]) * size_t(h[1]) * size_t(h[2]);
        std::vector<float> density(cells);
        std::vector<uint32_t> ids(cells);
        blok_scatter_params params;
        std::memset(&params, 0, sizeof params);
        std::vector<blok_scatter_entry> entries(static_cast<size_t>(h[15]));
        if (std::fread(density.data(), 4, cells, f) != cells || std::fread(ids.data(), 4, cells, f) != cells) { std::printf("short\n"); return 1; }
        if (h[15] && (std::fread(&params, sizeof params, 1, f) != 1 || std::fread(entries.data(), sizeof(blok_scatter_entry), entries.size(), f) != entries.size())) {
            std::printf("short\n"); return 1;
        }
        std::fclose(f);
        const int32_t* lo = h[6] ? nullptr : h + 7;
        const int32_t* hi = h[6] ? nullptr : h + 10;
        size_t ext[3] = {size_t(h[0]), size_t(h[1]), size_t(h[2])};
        if (!h[6]) for (int a = 0; a < 3; ++a) ext[a] = h[10 + a] > h[7 + a] ? size_t(h[10 + a] - h[7 + a]) : 0u;
        const uint32_t axis = uint32_t(h[13]);
        size_t columns = 0;
        if (axis <= 2u && ext[0] && ext[1] && ext[2]) columns = ext[axis == 0u ? 1 : 0] * ext[axis == 2u ? 1 : 2];
        std::vector<uint16_t> top(columns);                       // exactly the contracted sizes: a write past them is the sanitizer's to find
        std::vector<uint32_t> material(columns);
        blok_columns_info info;
        std::memset(&info, 0, sizeof info);
        const int rc = blok_column_field(density.data(), ids.data(), h + 3, uint32_t(h[0]), uint32_t(h[1]), uint32_t(h[2]), lo, hi, axis, uint32_t(h[14]), top.data(),
                                         material.data(), &info);
        int rc_scatter = -99;
        blok_scatter_info counted, placed;
        std::memset(&counted, 0, sizeof counted);
        std::memset(&placed, 0, sizeof placed);
        std::vector<uint32_t> words;
        if (rc == BLOK_OK && h[15]) {
            rc_scatter = blok_scatter(top.data(), material.data(), &info, &params, entries.data(), uint32_t(entries.size()), nullptr, 0, &counted);
            if (rc_scatter == BLOK_OK) {
                std::vector<blok_instance> table(size_t(counted.n_placed));
                rc_scatter = blok_scatter(top.data(), material.data(), &info, &params, entries.data(), uint32_t(entries.size()), table.data(), table.size(), &placed);
                if (std::memcmp(&counted, &placed, sizeof counted) != 0) { std::printf("the counting call and the writing call disagree\n"); return 1; }
                words.resize(table.size() * (sizeof(blok_instance) / 4u));
                if (!words.empty()) std::memcpy(words.data(), table.data(), words.size() * 4u);
            }
        }
        std::printf("%d %llu %llu %u %u %llu %llu %d %llu %llu %llu %llu %llu %llu %llu %llu\n", rc, (unsigned long long)info.n_columns, (unsigned long long)info.n_hit, info.min_top,
                    info.max_top, checksum(top), checksum(material), rc_scatter, (unsigned long long)placed.n_cells, (unsigned long long)placed.n_placed,
                    (unsigned long long)placed.n_rejected[0], (unsigned long long)placed.n_rejected[1], (unsigned long long)placed.n_rejected[2],
                    (unsigned long long)placed.n_rejected[3], (unsigned long long)placed.n_rejected[4], checksum(words));
    }
    return 0;
}
