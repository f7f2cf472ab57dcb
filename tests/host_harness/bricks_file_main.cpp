// A program of its own (tests/test_bricks_cpu.py builds it with ASan + UBSan together with blok_amd/csrc/host/bricks.cpp): reads every
// .bvol file named on the command line with blok_bricks_read_file — the sizes first, then arrays of exactly those sizes — and validates
// what it got once more, and once with each record's fields disturbed.  One line per file: "ok <bricks> <voxels>" or "refused <text>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "blok_world.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        char err[256] = "";
        blok_bricks_info info;
        if (blok_bricks_read_file(argv[i], &info, nullptr, nullptr, nullptr, err, sizeof err) != BLOK_OK) { std::printf("refused %s\n", err); continue; }
        std::vector<blok_brick_record> records(info.n_bricks);
        std::vector<uint32_t> density(info.n_density), material(info.n_material);
        if (blok_bricks_read_file(argv[i], &info, records.data(), density.data(), material.data(), err, sizeof err) != BLOK_OK) { std::printf("refused %s\n", err); continue; }
        if (blok_bricks_validate(&info, records.data(), density.data(), material.data(), err, sizeof err) != BLOK_OK) { std::printf("refused %s\n", err); continue; }
        // every field of every record disturbed in turn: the validation reads no more than the arrays hold, whatever the record says
        unsigned refused = 0, tried = 0;
        for (size_t r = 0; r < records.size(); ++r) {
            const blok_brick_record keep = records[r];
            for (int field = 0; field < 5; ++field) {
                blok_brick_record& rec = records[r];
                if (field == 0) rec.mask = ~rec.mask;
                if (field == 1) rec.brick = 0xFFFFFFFFu;
                if (field == 2) rec.kind ^= 7u;
                if (field == 3) rec.density += 0x80000000u;
                if (field == 4) rec.material += 0x80000000u;
                ++tried;
                if (blok_bricks_validate(&info, records.data(), density.data(), material.data(), err, sizeof err) != BLOK_OK) ++refused;
                rec = keep;
            }
        }
        std::printf("ok %llu %llu disturbed %u refused %u\n", static_cast<unsigned long long>(info.n_bricks), static_cast<unsigned long long>(info.n_voxels), tried, refused);
    }
    return 0;
}
