// Posed models on the host (include/blok_world.h: blok_pose_from_instance, blok_pose_from_matrix, blok_affine_from_pose): making the
// record the posed tracer takes (blok_hip.h, "Posed models"), folding one into the record blok_hip_volume_stamp_affine takes, and
// (blok_pose_motion_record) the motion record of a pose between two frames, from the core the device shares.
#include "blok_world.h"
#include "../common/affine_core.h"
#include "../common/pose_core.h"
#include "../common/pose_motion_core.h"

#include <cmath>
#include <cstdint>

namespace A = blok::affine;
namespace P = blok::pose;

extern "C" {

int blok_pose_from_instance(const blok_instance* placement, float vs, blok_pose* out) {
    if (!placement || !out || !blok::stamp::well_formed(*placement) || !std::isfinite(vs) || !(vs > 0.0f)) return BLOK_ERR_INVALID_ARG;
    blok_pose p{};
    p.model = placement->model;
    for (uint32_t k = 0; k < 3u; ++k) {
        p.m[k][placement->axis[k]] = ((placement->flip >> k) & 1u) ? -1.0f : 1.0f;
        p.pivot[k] = static_cast<float>(placement->offset[k]) * vs;          // the product of the instance's own ray rule (instance_core.h)
    }
    if (P::floats_rule(p) != P::kFine) return BLOK_ERR_INVALID_ARG;
    *out = p;
    return BLOK_OK;
}

int blok_pose_from_matrix(const double forward[12], const double pivot_local[3], uint32_t model, blok_pose* out) {
    if (!forward || !out) return BLOK_ERR_INVALID_ARG;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(forward[i])) return BLOK_ERR_INVALID_ARG;
    const double pl[3] = {pivot_local ? pivot_local[0] : 0.0, pivot_local ? pivot_local[1] : 0.0, pivot_local ? pivot_local[2] : 0.0};
    for (int i = 0; i < 3; ++i) if (!std::isfinite(pl[i])) return BLOK_ERR_INVALID_ARG;
    const double* F = forward;
    const double f[3][3] = {{F[0], F[1], F[2]}, {F[4], F[5], F[6]}, {F[8], F[9], F[10]}}, T[3] = {F[3], F[7], F[11]};
    // the inverse as adjugate / determinant (as blok_affine_from_matrix)
    double c[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[j][i] = f[i1][j1] * f[i2][j2] - f[i1][j2] * f[i2][j1];
        }
    const double det = f[0][0] * c[0][0] + f[0][1] * c[1][0] + f[0][2] * c[2][0];
    double scale = 1.0;
    for (int i = 0; i < 3; ++i) scale *= std::sqrt(f[i][0] * f[i][0] + f[i][1] * f[i][1] + f[i][2] * f[i][2]);
    if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * scale)) return BLOK_ERR_INVALID_ARG;
    blok_pose p{};
    p.model = model;
    double off[3];
    for (int j = 0; j < 3; ++j) {
        const double w = f[j][0] * pl[0] + f[j][1] * pl[1] + f[j][2] * pl[2] + T[j];      // where the local pivot lies in the world
        p.pivot[j] = static_cast<float>(w);
        off[j] = static_cast<double>(p.pivot[j]) - w;
    }
    for (int k = 0; k < 3; ++k) {
        double lk = pl[k];
        for (int j = 0; j < 3; ++j) {
            const double inv = c[k][j] / det;
            p.m[k][j] = static_cast<float>(inv);
            lk += inv * off[j];
        }
        p.local[k] = static_cast<float>(lk);
    }
    if (P::floats_rule(p) != P::kFine) return BLOK_ERR_INVALID_ARG;
    *out = p;
    return BLOK_OK;
}

int blok_affine_from_pose(const blok_pose* pose, float vs, uint32_t scale_log2, blok_affine* out) {
    if (!pose || !out || !std::isfinite(vs) || !(vs > 0.0f) || scale_log2 > A::kMaxScaleLog2) return BLOK_ERR_INVALID_ARG;
    if (P::floats_rule(*pose) != P::kFine) return BLOK_ERR_INVALID_ARG;
    blok_affine a{};
    a.model = pose->model;
    const double v = vs, cell = std::ldexp(v, static_cast<int>(scale_log2));
    double centre[3];
    for (int j = 0; j < 3; ++j) {
        const double fl = std::floor(static_cast<double>(pose->pivot[j]) / v);
        if (!(fl >= -2147483648.0 && fl <= 2147483647.0)) return BLOK_ERR_INVALID_ARG;
        a.anchor[j] = static_cast<int32_t>(fl);
        centre[j] = (fl + 0.5) * v - static_cast<double>(pose->pivot[j]);
    }
    for (int k = 0; k < 3; ++k) {
        double tk = pose->local[k];
        for (int j = 0; j < 3; ++j) {
            const double mk = std::rint(std::ldexp(static_cast<double>(pose->m[k][j]), 16 - static_cast<int>(scale_log2)));
            if (!(std::fabs(mk) <= static_cast<double>(A::kMaxM))) return BLOK_ERR_INVALID_ARG;
            a.m[k][j] = static_cast<int32_t>(mk);
            tk += static_cast<double>(pose->m[k][j]) * centre[j];
        }
        tk = std::rint(tk / cell * 65536.0);
        if (!(std::fabs(tk) <= static_cast<double>(A::kMaxT))) return BLOK_ERR_INVALID_ARG;
        a.t[k] = static_cast<int64_t>(tk);
    }
    *out = a;
    return BLOK_OK;
}

int blok_pose_motion_record(const blok_pose* cur, const blok_pose* prev, int model_usable, blok_pose_motion* out) {
    if (!cur || !out) return BLOK_ERR_INVALID_ARG;
    P::motion_record(*cur, prev ? *prev : *cur, prev != nullptr, model_usable != 0, *out);
    return BLOK_OK;
}

}  // extern "C"
