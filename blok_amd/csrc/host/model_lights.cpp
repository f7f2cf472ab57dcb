// Emissive models as lights on the host (include/blok_world.h: blok_model_lights, blok_instance_light_record): the contract of
// blok_hip_model_lights (blok_hip.h, "emissive models as lights") for the model blok_hip_model_create makes of a voxel list — the same tree
// (../hip/tree_build.cpp), walked brick by brick through the functions the kernels run (../common/lights_core.h).
#include "blok_world.h"
#include "../common/lights_core.h"
#include "../hip/tree.h"

#include <vector>

namespace L = blok::lights;

extern "C" {

int blok_model_lights(const int32_t* xyz, const uint32_t* material_ids, size_t n, const blok_material* materials, size_t n_materials, blok_light* out,
                      uint64_t capacity, uint64_t* out_n) {
    if (out_n) *out_n = 0;
    if (!xyz || !material_ids || n == 0 || (capacity && !out) || !materials || !n_materials) return BLOK_ERR_INVALID_ARG;
    std::vector<blok::VoxelRec> voxels(n);
    for (size_t i = 0; i < n; ++i) voxels[i] = blok::VoxelRec{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], material_ids[i]};
    blok::HostTree tree;
    const char* why = "";
    if (!blok::build_tree(voxels, tree, &why)) return BLOK_ERR_UNSUPPORTED;
    std::vector<uint32_t> glows(L::kSetWords);
    L::emissive_set(materials, n_materials, glows.data());
    const uint32_t n_mat = static_cast<uint32_t>(n_materials < L::kSetBits ? n_materials : L::kSetBits);
    const blok::TreeNode* nodes = tree.nodes.data();
    const auto load = [nodes](uint32_t i) { return L::Node{nodes[i].mask_lo | (static_cast<uint64_t>(nodes[i].mask_hi) << 32), nodes[i].base}; };
    const L::ModelTree<decltype(load)> t{load, static_cast<uint32_t>(tree.nodes.size()), tree.materials.data(), static_cast<uint32_t>(tree.materials.size()),
                                         tree.levels, {tree.origin[0], tree.origin[1], tree.origin[2]}};
    uint64_t total = 0;
    std::vector<blok_light> brick(6 * 64);
    for (uint32_t i = L::first_brick(t); i < t.n_nodes; ++i) {
        uint64_t open[6], glowing;
        uint32_t b[3];
        L::Node node;
        const uint32_t count = L::brick_lights(t, i, glows.data(), n_mat, open, &glowing, b, &node);
        if (!count) continue;
        L::brick_write_lights(t, node, b, open, glowing, 0u, brick.data());
        for (uint32_t k = 0; k < count; ++k, ++total)
            if (total < capacity) { out[total] = brick[k]; out[total].cum = static_cast<uint32_t>(total); }
    }
    if (total >= 0x80000000ull) return BLOK_ERR_UNSUPPORTED;
    if (out_n) *out_n = total;
    return BLOK_OK;
}

void blok_instance_light_record(const blok_instance* instance, uint32_t scale_log2, const blok_light* model_face, blok_light* out) {
    if (instance && model_face && out) *out = L::instance_light_record(*instance, scale_log2 > 8u ? 8u : scale_log2, *model_face);
}

}  // extern "C"
