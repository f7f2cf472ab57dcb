// The surface of a voxel volume as merged quads on the host (include/blok_world.h: blok_quads_extract, blok_quads_write_obj): the
// contract of blok_hip_volume_extract_quads (blok_hip.h) over host arrays, through the predicates the kernels use
// (../common/quads_core.h), plane by plane and cell by cell.
#include "blok_world.h"
#include "../common/quads_core.h"

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace Q = blok::quads;

extern "C" {

int blok_quads_extract(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags, blok_quad* out, uint64_t capacity,
                       uint64_t* out_n_quads, uint64_t* out_n_faces) {
    if (out_n_quads) *out_n_quads = 0;
    if (out_n_faces) *out_n_faces = 0;
    if (flags & ~(BLOK_QUADS_IGNORE_MATERIAL | BLOK_QUADS_COUNT_ONLY)) return BLOK_ERR_INVALID_ARG;
    if ((region_lo == nullptr) != (region_hi == nullptr)) return BLOK_ERR_INVALID_ARG;
    if (capacity && !out) return BLOK_ERR_INVALID_ARG;
    const int64_t dims[3] = {nx, ny, nz};
    const int32_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = region_lo ? int64_t(region_lo[a]) - org[a] : 0;
        hi[a] = region_hi ? int64_t(region_hi[a]) - org[a] : dims[a];
        if (lo[a] > hi[a]) return BLOK_ERR_INVALID_ARG;
    }
    for (int a = 0; a < 3; ++a) if (lo[a] < 0 || hi[a] > dims[a]) return BLOK_ERR_UNSUPPORTED;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    if (lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) return BLOK_OK;
    if (!density || !material_ids) return BLOK_ERR_INVALID_ARG;
    const bool ignore = flags & BLOK_QUADS_IGNORE_MATERIAL, count_only = flags & BLOK_QUADS_COUNT_ONLY;

    const auto is_filled = [&](int64_t x, int64_t y, int64_t z) {      // outside the box: empty
        if (x < 0 || y < 0 || z < 0 || x >= dims[0] || y >= dims[1] || z >= dims[2]) return false;
        return Q::filled(density[static_cast<size_t>(x + (y + z * dims[1]) * dims[0])]);
    };
    uint64_t n_quads = 0, n_faces = 0;
    std::vector<Q::Cell> plane;
    for (uint32_t face = 0; face < 6u; ++face) {
        const int a = Q::normal_axis(face), u = Q::u_axis(a), v = Q::v_axis(a), sign = Q::normal_sign(face);
        const int64_t ns = hi[a] - lo[a], nu = hi[u] - lo[u], nv = hi[v] - lo[v];
        plane.assign(static_cast<size_t>(nu * nv), Q::Cell{0u, 0u});
        const auto at = [&](int64_t cu, int64_t cv) -> Q::Cell {      // a cell outside the region belongs to no run
            if (cu < 0 || cu >= nu || cv < 0 || cv >= nv) return Q::Cell{0u, 0u};
            return plane[static_cast<size_t>(cu + cv * nu)];
        };
        // the row holds a run with the cells u0..u1 of `like`'s key, and it ends at both
        const auto identical_run = [&](int64_t u0, int64_t u1, int64_t cv, const Q::Cell& like) {
            if (cv < 0 || cv >= nv) return false;
            for (int64_t cu = u0; cu <= u1; ++cu) if (!Q::same(at(cu, cv), like)) return false;
            return !Q::same(at(u0 - 1, cv), like) && !Q::same(at(u1 + 1, cv), like);
        };
        for (int64_t s = 0; s < ns; ++s) {
            bool any = false;
            for (int64_t cv = 0; cv < nv; ++cv)
                for (int64_t cu = 0; cu < nu; ++cu) {
                    int64_t p[3];
                    p[a] = lo[a] + s; p[u] = lo[u] + cu; p[v] = lo[v] + cv;
                    int64_t q[3] = {p[0], p[1], p[2]};
                    q[a] += sign;
                    const bool f = is_filled(p[0], p[1], p[2]);
                    const Q::Cell c = Q::cell(f, f && is_filled(q[0], q[1], q[2]),
                                              material_ids[static_cast<size_t>(p[0] + (p[1] + p[2] * dims[1]) * dims[0])], ignore);
                    plane[static_cast<size_t>(cu + cv * nu)] = c;
                    n_faces += c.exposed;
                    any = any || c.exposed;
                }
            if (!any) continue;
            for (int64_t cv = 0; cv < nv; ++cv)
                for (int64_t cu = 0; cu < nu; ++cu) {
                    const Q::Cell c = at(cu, cv);
                    if (!Q::starts_run(c, at(cu - 1, cv))) continue;
                    int64_t u1 = cu;
                    while (!Q::ends_run(at(u1, cv), at(u1 + 1, cv))) ++u1;
                    if (!identical_run(cu, u1, cv - 1, c)) {      // not linked to the row below: a quad starts here
                        int64_t dv = 1;
                        while (identical_run(cu, u1, cv + dv, c)) ++dv;
                        if (!count_only && n_quads < capacity) {
                            blok_quad r{};
                            r.lo[a] = static_cast<int32_t>(org[a] + lo[a] + s + (sign > 0 ? 1 : 0));
                            r.lo[u] = static_cast<int32_t>(org[u] + lo[u] + cu);
                            r.lo[v] = static_cast<int32_t>(org[v] + lo[v] + cv);
                            r.du = static_cast<uint32_t>(u1 - cu + 1); r.dv = static_cast<uint32_t>(dv);
                            r.material = c.key; r.face = face; r.reserved = 0u;
                            out[n_quads] = r;
                        }
                        ++n_quads;
                    }
                    cu = u1;
                }
        }
    }
    if (out_n_quads) *out_n_quads = n_quads;
    if (out_n_faces) *out_n_faces = n_faces;
    return BLOK_OK;
}

int blok_quads_write_obj(const char* path, const blok_quad* quads, uint64_t n, const blok_material_library* lib, char* err, size_t err_len) {
    const auto fail = [&](const std::string& msg) {
        if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
        return BLOK_ERR_INVALID_ARG;
    };
    if (!path || (n && !quads)) return fail("write_obj: null argument");
    for (uint64_t i = 0; i < n; ++i)
        if (quads[i].face > 5u || !quads[i].du || !quads[i].dv) return fail("write_obj: record " + std::to_string(i) + " is not a quad");
    const std::string obj_path(path);
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return fail("cannot open '" + obj_path + "' for writing");
    if (lib) {
        // the sibling library: the same name with the extension .mtl, one entry per material in use
        const size_t slash = obj_path.find_last_of('/'), dot = obj_path.find_last_of('.');
        const std::string stem = (dot != std::string::npos && (slash == std::string::npos || dot > slash)) ? obj_path.substr(0, dot) : obj_path;
        const std::string mtl_path = stem + ".mtl";
        std::map<uint32_t, bool> used;
        for (uint64_t i = 0; i < n; ++i) used[quads[i].material] = true;
        std::FILE* m = std::fopen(mtl_path.c_str(), "wb");
        if (!m) { std::fclose(f); return fail("cannot open '" + mtl_path + "' for writing"); }
        for (const auto& kv : used) {
            blok_material_desc d;
            blok_material_library_get(lib, kv.first, &d);
            std::fprintf(m, "newmtl m%u\nKd %.9g %.9g %.9g\n", kv.first, d.albedo[0], d.albedo[1], d.albedo[2]);
        }
        if (std::fclose(m) != 0) { std::fclose(f); return fail("write to '" + mtl_path + "' failed"); }
        std::fprintf(f, "mtllib %s\n", mtl_path.substr(slash == std::string::npos ? 0 : slash + 1).c_str());
    }
    struct Key {
        int32_t x, y, z;
        bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; }
    };
    struct Hash {
        size_t operator()(const Key& k) const {
            uint64_t h = static_cast<uint32_t>(k.x) * 0x9E3779B97F4A7C15ull;
            h ^= static_cast<uint32_t>(k.y) * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
            h ^= static_cast<uint32_t>(k.z) * 0x165667B19E3779F9ull + (h << 6) + (h >> 2);
            return static_cast<size_t>(h);
        }
    };
    // vertices are shared between quads and numbered by first use: quads in the given order, corners in winding order
    std::unordered_map<Key, uint64_t, Hash> index;
    bool have_material = false;
    uint32_t material = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const blok_quad& q = quads[i];
        int32_t c[4][3];
        Q::corners(q.lo, q.du, q.dv, q.face, c);
        uint64_t id[4];
        for (int k = 0; k < 4; ++k) {
            const Key key{c[k][0], c[k][1], c[k][2]};
            const auto it = index.find(key);
            if (it != index.end()) { id[k] = it->second; continue; }
            id[k] = index.size() + 1u;
            index.emplace(key, id[k]);
            std::fprintf(f, "v %d %d %d\n", key.x, key.y, key.z);
        }
        if (!have_material || q.material != material) {
            std::fprintf(f, "usemtl m%u\n", q.material);
            have_material = true; material = q.material;
        }
        std::fprintf(f, "f %llu %llu %llu %llu\n", static_cast<unsigned long long>(id[0]), static_cast<unsigned long long>(id[1]),
                     static_cast<unsigned long long>(id[2]), static_cast<unsigned long long>(id[3]));
    }
    const bool bad = std::ferror(f) != 0;
    if (std::fclose(f) != 0 || bad) return fail("write to '" + obj_path + "' failed");
    return BLOK_OK;
}

}  // extern "C"
