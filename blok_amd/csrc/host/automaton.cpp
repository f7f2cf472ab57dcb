// Neighbour-count rules stepped over host arrays (include/blok_world.h: blok_automaton_voxels): the contract of blok_hip_volume_automaton
// (blok_hip.h) as a plain double-buffered loop per cell — the definition — through the check, the offsets and the vote the kernels use
// (../common/automaton_core.h).  The whole-brick arithmetic of that header is not used here: tests/host_harness/automaton_main.cpp runs it
// beside this loop.
#include "blok_world.h"
#include "../common/automaton_core.h"
#include "../common/region_core.h"

#include <cstdint>
#include <vector>

namespace K = blok::automaton;

extern "C" {

int blok_automaton_check(const blok_automaton_rule* rule, char* err, size_t err_len) {
    const int failed = K::check(rule);
    if (err && err_len) {
        const char* text = K::rule_text(failed);
        size_t i = 0;
        for (; text[i] && i + 1 < err_len; ++i) err[i] = text[i];
        err[i] = '\0';
    }
    return failed ? BLOK_ERR_INVALID_ARG : BLOK_OK;
}

int blok_automaton_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                          const int32_t region_lo[3], const int32_t region_hi[3], const blok_automaton_rule* rule, uint64_t* out_step_counts,
                          blok_automaton_info* out_info) {
    if (K::check(rule) != 0) return BLOK_ERR_INVALID_ARG;
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t lo[3], hi[3];
    const int rc = blok::region::status(blok::region::local(origin, dims, region_lo, region_hi, lo, hi));
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    const int32_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    blok_automaton_info info;
    K::plan(o, lo, hi, rule->flags, &info);
    if (out_step_counts)
        for (uint32_t k = 0; k < 2u * rule->steps; ++k) out_step_counts[k] = 0u;
    if (!info.ext[0] || !info.ext[1] || !info.ext[2]) {
        if (out_info) *out_info = info;
        return BLOK_OK;
    }
    if (!density || !material_ids) return BLOK_ERR_INVALID_ARG;
    const size_t cells = size_t(nx) * ny * nz;
    const auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return (size_t(z) * ny + y) * nx + x; };
    const bool solid = (rule->flags & BLOK_AUTOMATON_BOX_IS_SOLID) != 0u, fixed = (rule->flags & BLOK_AUTOMATON_FIXED_MATERIAL) != 0u;
    std::vector<uint8_t> before(cells);                    // the state every cell of a step is decided from
    std::vector<float> next_density;                       // the region's cells after the step, x fastest
    std::vector<uint32_t> next_ids;
    const size_t region_cells = size_t(info.ext[0]) * info.ext[1] * info.ext[2];
    next_density.resize(region_cells); next_ids.resize(region_cells);
    for (uint32_t step = 0; step < rule->steps; ++step) {
        for (size_t i = 0; i < cells; ++i) before[i] = density[i] > 0.0f ? 1u : 0u;
        uint64_t n_born = 0, n_died = 0;
        size_t r = 0;
        for (uint32_t z = lo[2]; z < hi[2]; ++z)
            for (uint32_t y = lo[1]; y < hi[1]; ++y)
                for (uint32_t x = lo[0]; x < hi[0]; ++x, ++r) {
                    const size_t c = at(x, y, z);
                    uint32_t n = 0u, voters = 0u, ids[26];
                    for (uint32_t i = 0; i < rule->neighbourhood; ++i) {
                        int32_t d[3];
                        K::offset(i, d);
                        const int64_t qx = int64_t(x) + d[0], qy = int64_t(y) + d[1], qz = int64_t(z) + d[2];
                        ids[i] = 0u;
                        if (qx < 0 || qy < 0 || qz < 0 || qx >= int64_t(nx) || qy >= int64_t(ny) || qz >= int64_t(nz)) { n += solid ? 1u : 0u; continue; }
                        const size_t q = at(uint32_t(qx), uint32_t(qy), uint32_t(qz));
                        if (before[q]) { ++n; voters |= 1u << i; ids[i] = material_ids[q]; }
                    }
                    next_density[r] = density[c]; next_ids[r] = material_ids[c];
                    if (before[c] && !((rule->survive >> n) & 1u)) { next_density[r] = 0.0f; next_ids[r] = 0u; ++n_died; }
                    else if (!before[c] && ((rule->birth >> n) & 1u)) {
                        next_density[r] = rule->density;
                        next_ids[r] = fixed ? rule->material : K::vote([&](uint32_t i) { return ids[i]; }, rule->neighbourhood, voters, rule->material);
                        ++n_born;
                    }
                }
        info.steps_run = step + 1u;
        if (!n_born && !n_died) break;                      // a fixed point: this step counts, no later one runs
        r = 0;
        for (uint32_t z = lo[2]; z < hi[2]; ++z)
            for (uint32_t y = lo[1]; y < hi[1]; ++y)
                for (uint32_t x = lo[0]; x < hi[0]; ++x, ++r) {
                    const size_t c = at(x, y, z);
                    if (before[c] || next_density[r] > 0.0f) { density[c] = next_density[r]; material_ids[c] = next_ids[r]; }      // (an empty cell that stays empty keeps its bits)
                }
        info.n_born += n_born; info.n_died += n_died;
        if (out_step_counts) { out_step_counts[2u * step] = n_born; out_step_counts[2u * step + 1u] = n_died; }
    }
    for (uint32_t z = lo[2]; z < hi[2]; ++z)
        for (uint32_t y = lo[1]; y < hi[1]; ++y)
            for (uint32_t x = lo[0]; x < hi[0]; ++x) info.n_filled += density[at(x, y, z)] > 0.0f ? 1u : 0u;
    if (out_info) *out_info = info;
    return BLOK_OK;
}

}  // extern "C"
