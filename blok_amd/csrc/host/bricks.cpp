// The sparse brick stream on the host (include/blok_world.h: blok_bricks_*): the contract of blok_hip_volume_encode_bricks /
// blok_hip_volume_decode_bricks (blok_hip.h) over host arrays, through the rules the kernels use (../common/bricks_core.h), brick by brick
// and cell by cell; and the .bvol file that holds a stream.
#include "blok_world.h"
#include "../common/bricks_core.h"
#include "../common/region_core.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace B = blok::bricks;

namespace {

const char kMagic[8] = {'B', 'L', 'O', 'K', 'B', 'V', 'L', '1'};

int fail(char* err, size_t err_len, int code, const std::string& msg) {
    if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
    return code;
}

uint32_t float_bits(float f) { uint32_t u; std::memcpy(&u, &f, sizeof u); return u; }

std::string validation_text(int rule, uint64_t bad, const blok_bricks_info& info) {
    std::string s = std::string("brick stream: ") + B::rule_text(rule);
    if (bad < info.n_bricks) s += " (record " + std::to_string(bad) + ")";
    return s;
}

}  // namespace

extern "C" {

int blok_bricks_encode(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags, blok_bricks_info* out_info,
                       blok_brick_record* records, uint64_t record_capacity, uint32_t* density_payload, uint64_t density_capacity,
                       uint32_t* material_payload, uint64_t material_capacity) {
    if (!out_info || (flags & ~B::kEncodeFlags)) return BLOK_ERR_INVALID_ARG;
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t lo[3], hi[3];
    const int rc = blok::region::status(blok::region::local(origin, dims, region_lo, region_hi, lo, hi));      // (the codes of the device entry)
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    blok_bricks_info info{};
    info.version = 1u; info.flags = flags;
    for (int a = 0; a < 3; ++a) { info.lo[a] = (origin ? origin[a] : 0) + static_cast<int32_t>(lo[a]); info.ext[a] = hi[a] - lo[a]; }
    const bool empty = !info.ext[0] || !info.ext[1] || !info.ext[2];
    if (!empty && (!density || !material_ids)) return BLOK_ERR_INVALID_ARG;
    const bool filled_only = (flags & BLOK_BRICKS_FILLED_ONLY) != 0u;
    const bool write = records != nullptr;
    uint32_t nb[3];
    B::brick_counts(info.ext, nb);
    if (!empty)
        for (uint32_t bz = 0; bz < nb[2]; ++bz) for (uint32_t by = 0; by < nb[1]; ++by) for (uint32_t bx = 0; bx < nb[0]; ++bx) {
            B::BrickDraft d;
            uint32_t dv[64], mv[64], n = 0;
            for (uint32_t z = 0; z < 4u && 4u * bz + z < info.ext[2]; ++z) for (uint32_t y = 0; y < 4u && 4u * by + y < info.ext[1]; ++y)
                for (uint32_t x = 0; x < 4u && 4u * bx + x < info.ext[0]; ++x) {
                    const size_t cell = (lo[0] + 4u * bx + x) + ((lo[1] + 4u * by + y) + static_cast<size_t>(lo[2] + 4u * bz + z) * ny) * nx;
                    const uint32_t bits = float_bits(density[cell]), id = material_ids[cell];
                    const uint64_t before = d.mask;
                    d.add(B::cell_bit(x, y, z), bits, id, filled_only);
                    if (d.mask != before) { dv[n] = bits; mv[n] = id; ++n; }
                }
            if (!d.mask) continue;
            const uint32_t kind = d.kind();
            if (write) {
                if (info.n_bricks >= record_capacity) return BLOK_ERR_INVALID_ARG;
                records[info.n_bricks] = B::make_record(bx + nb[0] * (by + nb[1] * bz), d.mask, kind, d.density.first, d.material.first,
                                                        static_cast<uint32_t>(info.n_density), static_cast<uint32_t>(info.n_material));
                if (!(kind & B::kUniformDensity)) {
                    if (!density_payload || info.n_density + n > density_capacity) return BLOK_ERR_INVALID_ARG;
                    std::memcpy(density_payload + info.n_density, dv, n * sizeof(uint32_t));
                }
                if (!(kind & B::kUniformMaterial)) {
                    if (!material_payload || info.n_material + n > material_capacity) return BLOK_ERR_INVALID_ARG;
                    std::memcpy(material_payload + info.n_material, mv, n * sizeof(uint32_t));
                }
            }
            ++info.n_bricks; info.n_voxels += n;
            if (!(kind & B::kUniformDensity)) info.n_density += n;
            if (!(kind & B::kUniformMaterial)) info.n_material += n;
        }
    *out_info = info;
    return BLOK_OK;
}

int blok_bricks_validate(const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                         const uint32_t* material_payload, char* err, size_t err_len) {
    if (!info) return fail(err, err_len, BLOK_ERR_INVALID_ARG, "brick stream: null info");
    uint64_t bad = 0;
    const int rule = B::validate(*info, records, density_payload, material_payload, &bad);
    if (rule) return fail(err, err_len, BLOK_ERR_INVALID_ARG, validation_text(rule, bad, *info));
    return BLOK_OK;
}

int blok_bricks_decode(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                       const uint32_t* material_payload, const int32_t dst_lo[3], uint32_t flags, char* err, size_t err_len) {
    if (flags & ~B::kDecodeFlags) return fail(err, err_len, BLOK_ERR_INVALID_ARG, "bricks_decode: unknown flag bits");
    const int rc = blok_bricks_validate(info, records, density_payload, material_payload, err, err_len);
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return fail(err, err_len, BLOK_ERR_UNSUPPORTED, "bricks_decode: box above 2^32 cells");
    const int64_t dims[3] = {nx, ny, nz};
    int64_t lo[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = int64_t(dst_lo ? dst_lo[a] : info->lo[a]) - (origin ? origin[a] : 0);
        if (lo[a] < 0 || lo[a] + int64_t(info->ext[a]) > dims[a]) return fail(err, err_len, BLOK_ERR_UNSUPPORTED, "bricks_decode: destination leaves the box");
    }
    const bool empty = !info->ext[0] || !info->ext[1] || !info->ext[2];
    if (empty) return BLOK_OK;
    if (!density || !material_ids) return fail(err, err_len, BLOK_ERR_INVALID_ARG, "bricks_decode: null volume array");
    const auto cell_of = [&](int64_t x, int64_t y, int64_t z) { return static_cast<size_t>((lo[0] + x) + ((lo[1] + y) + (lo[2] + z) * dims[1]) * dims[0]); };
    if (!(flags & BLOK_BRICKS_KEEP_OTHERS))
        for (uint32_t z = 0; z < info->ext[2]; ++z) for (uint32_t y = 0; y < info->ext[1]; ++y) for (uint32_t x = 0; x < info->ext[0]; ++x) {
            density[cell_of(x, y, z)] = 0.0f; material_ids[cell_of(x, y, z)] = 0u;
        }
    uint32_t nb[3];
    B::brick_counts(info->ext, nb);
    for (uint64_t i = 0; i < info->n_bricks; ++i) {
        const blok_brick_record& r = records[i];
        const uint32_t bx = r.brick % nb[0], by = (r.brick / nb[0]) % nb[1], bz = r.brick / (nb[0] * nb[1]);
        uint32_t rank = 0;
        for (uint32_t bit = 0; bit < 64u; ++bit) {
            if (!((r.mask >> bit) & 1ull)) continue;
            const size_t cell = cell_of(4u * bx + (bit & 3u), 4u * by + ((bit >> 2) & 3u), 4u * bz + (bit >> 4));
            density[cell] = B::bits_float((r.kind & B::kUniformDensity) ? r.density : density_payload[r.density + rank]);
            material_ids[cell] = (r.kind & B::kUniformMaterial) ? r.material : material_payload[r.material + rank];
            ++rank;
        }
    }
    return BLOK_OK;
}

int blok_bricks_write_file(const char* path, const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                           const uint32_t* material_payload, char* err, size_t err_len) {
    if (!path) return fail(err, err_len, BLOK_ERR_INVALID_ARG, "bricks_write_file: null path");
    const int rc = blok_bricks_validate(info, records, density_payload, material_payload, err, err_len);
    if (rc != BLOK_OK) return rc;
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return fail(err, err_len, BLOK_ERR_INVALID_ARG, std::string("cannot open '") + path + "' for writing");
    bool ok = std::fwrite(kMagic, 1, sizeof kMagic, f) == sizeof kMagic && std::fwrite(info, sizeof *info, 1, f) == 1;
    ok = ok && (!info->n_bricks || std::fwrite(records, sizeof *records, info->n_bricks, f) == info->n_bricks);
    ok = ok && (!info->n_density || std::fwrite(density_payload, sizeof(uint32_t), info->n_density, f) == info->n_density);
    ok = ok && (!info->n_material || std::fwrite(material_payload, sizeof(uint32_t), info->n_material, f) == info->n_material);
    if (std::fclose(f) != 0 || !ok) return fail(err, err_len, BLOK_ERR_INVALID_ARG, std::string("write to '") + path + "' failed");
    return BLOK_OK;
}

int blok_bricks_read_file(const char* path, blok_bricks_info* out_info, blok_brick_record* records, uint32_t* density_payload,
                          uint32_t* material_payload, char* err, size_t err_len) {
    if (!path || !out_info) return fail(err, err_len, BLOK_ERR_INVALID_ARG, "bricks_read_file: null argument");
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return fail(err, err_len, BLOK_ERR_INVALID_ARG, std::string("cannot open '") + path + "'");
    const auto close_fail = [&](const std::string& msg) { std::fclose(f); return fail(err, err_len, BLOK_ERR_INVALID_ARG, std::string("'") + path + "': " + msg); };
    if (std::fseek(f, 0, SEEK_END) != 0) return close_fail("cannot seek");
    const long end = std::ftell(f);
    if (end < 0 || std::fseek(f, 0, SEEK_SET) != 0) return close_fail("cannot seek");
    const uint64_t length = static_cast<uint64_t>(end);
    char magic[8];
    blok_bricks_info info;
    if (length < sizeof magic + sizeof info) return close_fail("truncated header");
    if (std::fread(magic, 1, sizeof magic, f) != sizeof magic || std::memcmp(magic, kMagic, sizeof magic) != 0) return close_fail("not a .bvol file");
    if (std::fread(&info, sizeof info, 1, f) != 1) return close_fail("truncated header");
    if (info.version != 1u) return close_fail("version is not 1");
    // every size against the file's length, before anything is allocated by the caller or read here; none of the sums can wrap: each
    // count is bounded by what is left of the length first
    uint64_t left = length - (sizeof magic + sizeof info);
    if (info.n_bricks > left / sizeof(blok_brick_record)) return close_fail("header promises more records than the file holds");
    left -= info.n_bricks * sizeof(blok_brick_record);
    if (info.n_density > left / sizeof(uint32_t)) return close_fail("header promises more density payload than the file holds");
    left -= info.n_density * sizeof(uint32_t);
    if (info.n_material > left / sizeof(uint32_t)) return close_fail("header promises more material payload than the file holds");
    left -= info.n_material * sizeof(uint32_t);
    if (left != 0u) return close_fail("bytes after the material payload");
    *out_info = info;
    if (!records && !density_payload && !material_payload && (info.n_bricks || info.n_density || info.n_material)) { std::fclose(f); return BLOK_OK; }      // the sizes alone
    if ((info.n_bricks && !records) || (info.n_density && !density_payload) || (info.n_material && !material_payload)) return close_fail("null array with a non-zero count");
    bool ok = !info.n_bricks || std::fread(records, sizeof *records, info.n_bricks, f) == info.n_bricks;
    ok = ok && (!info.n_density || std::fread(density_payload, sizeof(uint32_t), info.n_density, f) == info.n_density);
    ok = ok && (!info.n_material || std::fread(material_payload, sizeof(uint32_t), info.n_material, f) == info.n_material);
    if (!ok) return close_fail("read failed");
    std::fclose(f);
    return blok_bricks_validate(&info, records, density_payload, material_payload, err, err_len);
}

}  // extern "C"
