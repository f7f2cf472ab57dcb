// Launchers of the image-space chain (post_core.h); one lane = one pixel, 64x4-pixel workgroups (one wave per row
// segment: coalesced 16-B-per-lane plane reads).
#ifndef BLOK_POST_KERNELS_H
#define BLOK_POST_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blok_hip.h"

namespace blok {
struct TemporalArgs;
struct VarianceArgs;
struct AtrousArgs;
struct TaaArgs;
struct SharpenArgs;
struct TemporalInstancedArgs;
struct InstanceMotionArgs;
struct TemporalPosedArgs;
struct PosedMotionArgs;
struct ModelDesc;
void launch_temporal(const TemporalArgs& a, hipStream_t stream);
void launch_temporal_instanced(const TemporalInstancedArgs& a, hipStream_t stream);   // the temporal pass of a frame with instances
void launch_instance_motion(const InstanceMotionArgs& a, hipStream_t stream);         // object motion of tracked instance pixels
void launch_temporal_posed(const TemporalPosedArgs& a, hipStream_t stream);           // the temporal pass of a frame with poses
void launch_posed_motion(const PosedMotionArgs& a, hipStream_t stream);               // object motion of tracked pose and instance pixels
// one blok_pose_motion record per pose of `cur` against `prev` (pose_motion.h), one lane per pose; out: n_cur records
void launch_pose_motion_prepare(const blok_pose* cur, uint32_t n_cur, const blok_pose* prev, uint32_t n_prev, const ModelDesc* models, uint32_t n_models,
                                blok_pose_motion* out, hipStream_t stream);
void launch_variance(const VarianceArgs& a, hipStream_t stream);
void launch_atrous(const AtrousArgs& a, hipStream_t stream);
void launch_taa(const TaaArgs& a, hipStream_t stream);
void launch_sharpen(const SharpenArgs& a, hipStream_t stream);
// half / half2 planes -> float planes (state download for tests and tools)
void launch_widen(const uint16_t* src, float* dst, size_t n, hipStream_t stream);
}  // namespace blok
#endif
