// Wavefront OBJ / MTL import (include/blok_world.h: blok_obj_load_*): triangles and per-triangle material ids for
// blok_hip_volume_voxelize_mesh.  Geometry (v, f) and the material statements the voxel store can carry (Kd, Ke, Pr, Pm); texture
// coordinates, normals, groups and smoothing are read past.
#include "blok_world.h"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

struct blok_mesh {
    std::vector<float> positions;
    std::vector<uint32_t> triangles;
    std::vector<uint32_t> materials;
};

namespace {

enum : uint8_t { kEmissive = 3 };

struct Fail {
    std::string msg;
};

std::vector<std::string> tokens(const std::string& line) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t')) ++i;
        const size_t j = i;
        while (i < line.size() && line[i] != ' ' && line[i] != '\t') ++i;
        if (i > j) out.push_back(line.substr(j, i - j));
    }
    return out;
}

// Lines without the line ending (LF or CRLF; a missing final newline is fine) and without comments.
template <class Fn> void for_lines(const char* text, size_t len, Fn fn) {
    size_t at = 0, number = 0;
    while (at < len) {
        size_t end = at;
        while (end < len && text[end] != '\n') ++end;
        std::string line(text + at, end - at);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        fn(++number, line);
        at = end + 1;
    }
}

float number(const std::string& s, const char* what, size_t line) {
    errno = 0;
    char* end = nullptr;
    const float v = std::strtof(s.c_str(), &end);
    if (s.empty() || *end != '\0' || errno == ERANGE || !std::isfinite(v))
        throw Fail{std::string(what) + " line " + std::to_string(line) + ": malformed number '" + s + "'"};
    return v;
}

struct Mtl {
    std::unordered_map<std::string, uint32_t> ids;
};

void parse_mtl(const char* text, size_t len, blok_material_library* lib, Mtl& out) {
    std::vector<blok_material_desc> descs;
    std::vector<std::string> names;
    for_lines(text, len, [&](size_t n, const std::string& line) {
        const auto t = tokens(line);
        if (t.empty()) return;
        if (t[0] == "newmtl") {
            if (t.size() < 2) throw Fail{"mtl line " + std::to_string(n) + ": newmtl without a name"};
            blok_material_desc d;
            blok_material_desc_init(&d);
            std::snprintf(d.name, sizeof(d.name), "%s", t[1].c_str());
            descs.push_back(d);
            names.push_back(t[1]);
            return;
        }
        if (t[0] != "Kd" && t[0] != "Ke" && t[0] != "Pr" && t[0] != "Pm") return;
        if (descs.empty()) throw Fail{"mtl line " + std::to_string(n) + ": " + t[0] + " before newmtl"};
        blok_material_desc& d = descs.back();
        const size_t want = (t[0] == "Kd" || t[0] == "Ke") ? 3 : 1;
        if (t.size() < want + 1) throw Fail{"mtl line " + std::to_string(n) + ": " + t[0] + " needs " + std::to_string(want) + " values"};
        float v[3] = {0, 0, 0};
        for (size_t k = 0; k < want; ++k) v[k] = number(t[k + 1], "mtl", n);
        if (t[0] == "Kd") for (int k = 0; k < 3; ++k) d.albedo[k] = v[k];
        else if (t[0] == "Ke") {
            if (v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f) {
                for (int k = 0; k < 3; ++k) d.emission[k] = v[k];
                d.type = kEmissive;
                d.emission_power = 1.0f;
            }
        } else if (t[0] == "Pr") d.roughness = v[0];
        else d.metallic = v[0];
    });
    for (size_t i = 0; i < descs.size(); ++i)
        out.ids[names[i]] = lib ? blok_material_library_add_or_find(lib, &descs[i]) : 0u;
}

bool read_file(const std::string& path, std::string& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::ostringstream s;
    s << f.rdbuf();
    out = s.str();
    return true;
}

// mtl_dir: the directory of the .obj (load_file), or null with the MTL text given (load_memory).
int parse_obj(const char* text, size_t len, const std::string* mtl_dir, const char* mtl, size_t mtl_len, blok_material_library* lib,
              blok_mesh** out, char* err, size_t err_len) {
    if (!out || (len && !text)) return BLOK_ERR_INVALID_ARG;
    *out = nullptr;
    auto* m = new (std::nothrow) blok_mesh();
    if (!m) return BLOK_ERR_OOM;
    try {
        Mtl lib_mtl;
        bool have_mtllib = false;
        uint32_t current = 0;
        if (!mtl_dir && mtl) { parse_mtl(mtl, mtl_len, lib, lib_mtl); have_mtllib = true; }
        for_lines(text, len, [&](size_t n, const std::string& line) {
            const auto t = tokens(line);
            if (t.empty()) return;
            const std::string at = "obj line " + std::to_string(n) + ": ";
            if (t[0] == "v") {
                if (t.size() < 4) throw Fail{at + "a vertex needs x y z"};
                for (int k = 1; k <= 3; ++k) m->positions.push_back(number(t[k], "obj", n));
                if (t.size() > 4) (void)number(t[4], "obj", n);                 // w: checked, ignored
            } else if (t[0] == "f") {
                if (t.size() < 4) throw Fail{at + "a face needs at least three vertices"};
                const int64_t count = static_cast<int64_t>(m->positions.size() / 3);
                std::vector<uint32_t> idx;
                for (size_t k = 1; k < t.size(); ++k) {
                    const std::string s = t[k].substr(0, t[k].find('/'));
                    errno = 0;
                    char* end = nullptr;
                    const long long i = std::strtoll(s.c_str(), &end, 10);
                    if (s.empty() || *end != '\0' || errno == ERANGE) throw Fail{at + "malformed vertex index '" + t[k] + "'"};
                    if (i == 0) throw Fail{at + "vertex index 0"};
                    const int64_t r = i > 0 ? i - 1 : count + i;
                    if (r < 0 || r >= count) throw Fail{at + "vertex index " + s + " out of range (" + std::to_string(count) + " vertices so far)"};
                    idx.push_back(static_cast<uint32_t>(r));
                }
                for (size_t k = 1; k + 1 < idx.size(); ++k) {                     // a fan from the first vertex
                    m->triangles.insert(m->triangles.end(), {idx[0], idx[k], idx[k + 1]});
                    m->materials.push_back(current);
                }
            } else if (t[0] == "mtllib") {
                if (t.size() < 2) throw Fail{at + "mtllib without a file name"};
                if (have_mtllib || !mtl_dir) return;                            // the first library only; load_memory: the given text
                have_mtllib = true;
                std::string body;
                const std::string path = (mtl_dir->empty() ? std::string() : *mtl_dir + "/") + t[1];
                if (!read_file(path, body)) throw Fail{at + "cannot open material library '" + path + "'"};
                parse_mtl(body.data(), body.size(), lib, lib_mtl);
            } else if (t[0] == "usemtl") {
                const auto it = t.size() > 1 ? lib_mtl.ids.find(t[1]) : lib_mtl.ids.end();
                current = it == lib_mtl.ids.end() ? 0u : it->second;            // undefined: the default material
            }
            // vt, vn, o, g, s, l, p and anything unknown: ignored
        });
    } catch (const Fail& f) {
        if (err && err_len) std::snprintf(err, err_len, "%s", f.msg.c_str());
        delete m;
        return BLOK_ERR_INVALID_ARG;
    } catch (const std::bad_alloc&) {
        delete m;
        return BLOK_ERR_OOM;
    }
    *out = m;
    return BLOK_OK;
}

}  // namespace

extern "C" {

int blok_obj_load_file(const char* path, blok_material_library* lib, blok_mesh** out, char* err, size_t err_len) {
    if (!path || !out) return BLOK_ERR_INVALID_ARG;
    std::string body;
    if (!read_file(path, body)) {
        if (err && err_len) std::snprintf(err, err_len, "cannot open '%s'", path);
        return BLOK_ERR_INVALID_ARG;
    }
    const std::string p(path);
    const size_t slash = p.find_last_of('/');
    const std::string dir = slash == std::string::npos ? std::string(".") : p.substr(0, slash);
    return parse_obj(body.data(), body.size(), &dir, nullptr, 0, lib, out, err, err_len);
}

int blok_obj_load_memory(const char* obj, size_t obj_len, const char* mtl, size_t mtl_len, blok_material_library* lib, blok_mesh** out,
                         char* err, size_t err_len) {
    return parse_obj(obj, obj_len, nullptr, mtl, mtl_len, lib, out, err, err_len);
}

void blok_mesh_free(blok_mesh* m) { delete m; }
size_t blok_mesh_vertex_count(const blok_mesh* m) { return m ? m->positions.size() / 3 : 0; }
size_t blok_mesh_triangle_count(const blok_mesh* m) { return m ? m->materials.size() : 0; }
const float* blok_mesh_positions(const blok_mesh* m) { return m && !m->positions.empty() ? m->positions.data() : nullptr; }
const uint32_t* blok_mesh_triangles(const blok_mesh* m) { return m && !m->triangles.empty() ? m->triangles.data() : nullptr; }
const uint32_t* blok_mesh_materials(const blok_mesh* m) { return m && !m->materials.empty() ? m->materials.data() : nullptr; }

}  // extern "C"
