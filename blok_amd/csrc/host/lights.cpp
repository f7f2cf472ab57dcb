// Emissive quads as a light table on the host (include/blok_world.h: blok_lights_from_quads, blok_lights_check): the contract of
// blok_hip_lights_from_quads and blok_hip_set_lights (blok_hip.h) over host arrays, through the predicates the kernels use
// (../common/lights_core.h).
#include "blok_world.h"
#include "../common/lights_core.h"

#include <cstdio>
#include <vector>

namespace L = blok::lights;

extern "C" {

int blok_lights_from_quads(const blok_quad* quads, uint64_t n_quads, const blok_material* materials, size_t n_materials, blok_light* out,
                           uint64_t capacity, float voxel_size, blok_lights_info* out_info) {
    if (out_info) *out_info = blok_lights_info{};
    if ((n_quads && !quads) || (capacity && !out) || !materials || !n_materials) return BLOK_ERR_INVALID_ARG;
    std::vector<uint32_t> glows(L::kSetWords), owned(L::kSetWords, 0u);
    L::emissive_set(materials, n_materials, glows.data());
    const uint32_t n_mat = static_cast<uint32_t>(n_materials < L::kSetBits ? n_materials : L::kSetBits);
    uint64_t n = 0, faces = 0;
    for (uint64_t i = 0; i < n_quads; ++i) {
        const blok_quad& q = quads[i];
        if (!L::keeps(q.material, glows.data(), n_mat)) continue;
        if (n < capacity) {
            blok_light& l = out[n];
            for (int c = 0; c < 3; ++c) l.lo[c] = q.lo[c];
            l.du = q.du; l.dv = q.dv; l.material = q.material; l.face = q.face; l.cum = static_cast<uint32_t>(faces);
        }
        const uint32_t m = L::material_index(q.material, n_mat);
        owned[m >> 5] |= 1u << (m & 31u);
        n += 1; faces += static_cast<uint64_t>(q.du) * q.dv;
    }
    if (n >= 0x80000000ull || faces > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    if (out_info) {
        out_info->n = static_cast<uint32_t>(n); out_info->n_faces = faces; out_info->bytes = n * sizeof(blok_light);
        for (const uint32_t w : owned) out_info->n_owned += static_cast<uint32_t>(__builtin_popcount(w));
        out_info->area_world = static_cast<float>(faces) * voxel_size * voxel_size;
    }
    return BLOK_OK;
}

int blok_lights_check(const blok_light* lights, uint64_t n, blok_lights_info* out_info, char* err, size_t err_len) {
    static const char* const kRules[] = {"", "face above 5", "du or dv is 0", "cum is not the running sum of du * dv", "2^31 or more lights, or 2^32 or more unit faces",
                                         "a corner outside [-32768, 32768]"};
    if (out_info) *out_info = blok_lights_info{};
    if (err && err_len) err[0] = '\0';
    if (n && !lights) return BLOK_ERR_INVALID_ARG;
    uint64_t faces = 0, index = 0;
    const int rule = L::check_table(lights, n, &faces, &index);
    if (rule) {
        if (err && err_len) std::snprintf(err, err_len, "light %llu: %s", static_cast<unsigned long long>(index), kRules[rule]);
        return rule == 4 ? BLOK_ERR_UNSUPPORTED : BLOK_ERR_INVALID_ARG;
    }
    if (out_info) { out_info->n = static_cast<uint32_t>(n); out_info->n_faces = faces; out_info->bytes = n * sizeof(blok_light); }
    return BLOK_OK;
}

}  // extern "C"
