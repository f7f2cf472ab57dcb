// TEST INFRASTRUCTURE: the keyed brick index (blok_amd/csrc/hip/volume_device.h: cell_key / key_cell) compiled for the host, as a program
// of its own so that it runs under -fsanitize=address,undefined (tests/test_cell_key_cpu.py).  For every d = 1..3 and every cell with
// x, y, z < 4^d: the key is below 64^d, no two cells share one, each digit is x | y << 2 | z << 4 of its level, least significant level
// first, and key_cell gives the cell back.  Prints the number of cells checked; a failed check prints the cell and exits with 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "volume_device.h"

int main() {
    uint64_t checked = 0;
    for (uint32_t d = 1; d <= 3u; ++d) {
        const uint32_t n = 1u << (2u * d);
        std::vector<uint8_t> seen(static_cast<size_t>(1) << (6u * d), 0);
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t y = 0; y < n; ++y)
                for (uint32_t x = 0; x < n; ++x) {
                    const uint64_t key = blok::cell_key(x, y, z, d);
                    bool ok = key < seen.size() && !seen[key];
                    for (uint32_t j = 0; ok && j < d; ++j)
                        ok = ((key >> (6u * j)) & 63u) == (((x >> (2u * j)) & 3u) | (((y >> (2u * j)) & 3u) << 2) | (((z >> (2u * j)) & 3u) << 4));
                    uint32_t bx = ~0u, by = ~0u, bz = ~0u;
                    blok::key_cell(key, d, bx, by, bz);
                    if (!ok || bx != x || by != y || bz != z) {
                        std::printf("digits %u cell (%u, %u, %u): key %llu -> (%u, %u, %u)\n", d, x, y, z, static_cast<unsigned long long>(key), bx, by, bz);
                        return 1;
                    }
                    seen[key] = 1;
                    ++checked;
                }
    }
    std::printf("%llu\n", static_cast<unsigned long long>(checked));
    return 0;
}
