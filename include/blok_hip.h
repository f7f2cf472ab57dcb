/*
 * blok_hip.h — C ABI of the MI355X (gfx950) voxel ray-march backend for blok.
 *
 * This is the drop-in boundary.  blok has no plugin ABI; a backend is whatever
 * `App` calls on it (reference blok/src/app.cpp:73-128,130-192) and whatever
 * `Renderer::addWorld` consumes (reference blok/include/renderer.hpp:40-72).
 * Each entry point below names the reference interface it stands in for.
 *
 * Conventions
 *   - every function returns BLOK_OK (0) or a negative blok_status; the text of the
 *     last failure is available from blok_hip_last_error(ctx) (ctx may be NULL for
 *     create-time failures).  The reference throws std::runtime_error instead
 *     (reference blok/src/main.cpp:19-22); the C++ HipTracer wrapper rethrows.
 *   - plain pointers and sizes only; caller owns every host array, the context owns
 *     every device copy (same ownership split as reference renderer.hpp:195 +
 *     renderer_init.cpp:123-169).
 *   - a context is bound to one device and is not thread-safe (the reference is
 *     single-threaded: one context, one frame in flight on the compute path,
 *     reference blok/src/cuda_tracer.cu:539).
 *   - there is NO CPU fallback: without a gfx950 device / code object every entry
 *     point that would compute fails with BLOK_ERR_NO_DEVICE.
 */
#ifndef BLOK_HIP_H
#define BLOK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ records */

/* = blok::SvoNode, reference blok/include/svo.hpp:23-28.  16 B.
 * childMask bit i set <=> child i non-empty (reference blok/src/svo.cpp:99);
 * leaf <=> childMask == 0 (reference assets/shaders/intersect.rint:136). */
typedef struct blok_svo_node {
    uint32_t child_mask;
    uint32_t first_child; /* chunk-relative index of child 0, 8 siblings contiguous; 0xFFFFFFFF none */
    uint32_t material_id;
    float    occupancy;   /* >0 filled */
} blok_svo_node;

/* = blok::SubChunkGpu, reference blok/include/resources.hpp:170-184.  48 B. */
typedef struct blok_sub_chunk {
    uint32_t node_offset;     /* start of the parent chunk's nodes in the global array */
    uint32_t root_node_index; /* relative to node_offset */
    uint32_t node_count;      /* nodes in the parent chunk */
    uint32_t start_depth;
    float    world_min[3];
    float    sub_chunk_size;
    float    world_max[3];
    float    pad0;
} blok_sub_chunk;

/* = blok::MaterialGpu, reference blok/include/material.hpp:88-114.  32 B.
 * flags = metal<<24 | rough<<16 | type<<12 | alpha4<<8 | spec. */
typedef struct blok_material {
    float    albedo[3];
    uint32_t flags;
    float    emission[3];
    float    ior;
} blok_material;

/* = CameraCUDA, the reference's own compute-backend camera contract
 * (reference blok/src/cuda_tracer.cu:51-58, filled at :404-415 from blok::Camera,
 * reference blok/include/camera.hpp:25-42). */
typedef struct blok_camera {
    float pos[3];
    float fwd[3];
    float right[3];
    float up[3];
    float tan_half_fov; /* tanf(0.5*fov) */
    float aspect;       /* width / height of the FULL frame */
} blok_camera;

/* First-hit record, 16 B per ray.  What closest-hit sees of a procedural hit in the
 * reference: gl_HitTEXT, hitAttribs.materialId, gl_HitKindEXT
 * (reference assets/shaders/intersect.rint:138-141, hit.rchit:58-74), plus the voxel
 * that produced it.  Miss: t = -1 (reference miss.rmiss:25-27), hit = 0, face = 0xFF. */
typedef struct blok_hit {
    float    t;
    uint32_t material_id;
    int16_t  voxel[3];    /* world voxel coordinates of the leaf */
    uint8_t  face;        /* 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z  (reference hit.rchit:46-53) */
    uint8_t  hit;         /* 1 hit, 0 miss */
} blok_hit;

/* Explicit ray, for secondary rays and edge-case tests (same interval semantics as
 * traceRayEXT: reference assets/shaders/raygen.rgen:217-229). */
typedef struct blok_ray {
    float org[3];
    float tmin;
    float dir[3];
    float tmax;
} blok_ray;

typedef enum blok_status {
    BLOK_OK              =  0,
    BLOK_ERR_INVALID_ARG = -1,
    BLOK_ERR_NO_DEVICE   = -2, /* no gfx950 device, or the HIP runtime failed */
    BLOK_ERR_HIP         = -3, /* a HIP call failed; message has the call and code */
    BLOK_ERR_NO_WORLD    = -4, /* trace before upload */
    BLOK_ERR_UNSUPPORTED = -5, /* world not on the unit-voxel integer lattice, leaf above voxel level, ... */
    BLOK_ERR_OOM         = -6,
    BLOK_ERR_INTERNAL    = -7  /* a bound the library proves for itself did not hold: a defect of the library, never of the caller */
} blok_status;

/* Reference constants of the primary trace (reference assets/shaders/raygen.rgen:225,227). */
#define BLOK_RAY_TMIN 0.001f
#define BLOK_RAY_TMAX 10000.0f

typedef struct blok_hip_ctx blok_hip_ctx;

/* ---------------------------------------------------------------- lifecycle */

/* = CudaTracer::CudaTracer(w,h) + init()   (reference blok/include/cuda_tracer.hpp:25-28,
 *   blok/src/cuda_tracer.cu:425-448).  Binds the context to `device_ordinal`. */
int blok_hip_create(blok_hip_ctx** out_ctx, int device_ordinal, uint32_t width, uint32_t height);

/* = CudaTracer::resize (reference blok/src/cuda_tracer.cu:557-575). */
int blok_hip_resize(blok_hip_ctx* ctx, uint32_t width, uint32_t height);

/* = CudaTracer::shutdown / Renderer::cleanupWorld (reference blok/src/cuda_tracer.cu:577-602,
 *   blok/src/renderer_init.cpp:123-169). */
void blok_hip_destroy(blok_hip_ctx* ctx);

const char* blok_hip_last_error(const blok_hip_ctx* ctx);

/* A caller that is about to destroy a HIP stream it has passed to *_device entries tells the context first: the context keeps scratch
 * buffers and launch markers per stream (so that frames in flight on different streams never share any) and would otherwise keep them
 * until blok_hip_destroy.  Blocks until the device is idle.  No reference counterpart (the reference renders on one queue). */
int blok_hip_release_stream(blok_hip_ctx* ctx, void* hip_stream);

/* ------------------------------------------------------------------- world */

/* ChunkManager's voxelSize for the NEXT blok_hip_upload_world or blok_hip_upload_dense (reference blok/src/chunk_manager.cpp:19-25: voxel coordinates
 * times voxelSize are the world coordinates in every SubChunkGpu).  Default 1 (the reference app, app.cpp:37).  Powers of two
 * in [1/256, 256] are supported: the structure is built on the voxel lattice and the walk scales its integer planes, every
 * product exact, so first hits stay bit-exact; hit records carry the voxel's lattice coordinates.  Any other size returns
 * BLOK_ERR_UNSUPPORTED: its box planes are not exactly representable, and the reference's own result then depends on the
 * rounding of every intermediate box, which no other traversal order reproduces.  The shadow rays' last-occluder map and the
 * resident volume exist for size 1 only. */
int blok_hip_set_voxel_size(blok_hip_ctx* ctx, float voxel_size);

/* = Renderer::addWorld / updateWorld  (reference blok/include/renderer.hpp:40-72,
 *   uploadSvoBuffers + uploadMaterialBuffer, blok/src/renderer_upload.cpp:237-312).
 * Takes the three host arrays of WorldSvoGpu (reference blok/include/resources.hpp:195-203)
 * exactly as packChunksToGpuSvo emits them (reference blok/src/chunk_manager.cpp:234-314),
 * copies them to HBM and builds the traversal structure there (this also replaces
 * buildChunkBlas/buildChunkTlas, reference blok/src/renderer_raytracing.cpp:15-254).
 * Replaces any previous world. */
int blok_hip_upload_world(blok_hip_ctx* ctx,
                          const blok_svo_node* nodes, size_t n_nodes,
                          const blok_sub_chunk* sub_chunks, size_t n_sub_chunks,
                          const blok_material* materials, size_t n_materials);

/* Dense form (BASELINE.json configs[0..1]): material_ids[x + y*nx + z*nx*ny], 0 = empty,
 * i.e. the reference's dense store with density>0 <=> id != 0
 * (reference blok/include/chunk.hpp:35-36, blok/src/chunk_manager.cpp:57-59,330-348).
 * origin = world coordinate of voxel (0,0,0), in voxels: with blok_hip_set_voxel_size s, cell c covers world [(origin + c) s, (origin + c + 1) s)
 * (since ABI 1.16; before, the size was taken for blok_hip_upload_world alone). */
int blok_hip_upload_dense(blok_hip_ctx* ctx, const uint32_t* material_ids,
                          uint32_t nx, uint32_t ny, uint32_t nz, const int32_t origin[3],
                          const blok_material* materials, size_t n_materials);
/* Dense-grid path (BASELINE.json configs[1]: "256^3 dense grid ... primary-ray DDA ... coalesced HBM, no SVO"; no reference
 * counterpart, the reference has no DDA): when on at the time of blok_hip_upload_dense, the grid itself stays on the device in
 * 8x8x8-cell tiles with one occupancy bit per tile (staged into LDS by the kernel), and blok_hip_trace_primary* (rectangle
 * entries) walk it with a two-level DDA over the same canonical plane sequence instead of the derived tree; the tile / ray /
 * path entries keep using the tree.  Records are identical either way (tests/test_gpu_parity.py).  Default off. */
int blok_hip_set_dense_dda(blok_hip_ctx* ctx, int enabled);

/* Sizes of the device-resident world, for accounting (bytes). */
typedef struct blok_world_stats {
    uint64_t n_voxels;          /* filled leaves */
    uint64_t n_ref_nodes;       /* reference SvoNode records uploaded */
    uint64_t n_sub_chunks;
    uint64_t n_tree_nodes;      /* 16-B 4x4x4 nodes of the derived structure */
    uint64_t tree_bytes;        /* nodes + material side array */
    uint32_t levels;            /* 4^levels voxels per axis */
    int32_t  origin[3];         /* world coordinate of the structure's corner */
} blok_world_stats;
int blok_hip_world_stats(const blok_hip_ctx* ctx, blok_world_stats* out);

/* -------------------------------------------------------------------- trace */

/* = CudaTracer::drawFrame(cam, ...) restricted to the primary hit
 *   (reference blok/src/cuda_tracer.cu:484-555) == raygen.rgen bounce 0 / sample 0
 *   -> traceRayEXT -> intersect.rint -> hit.rchit
 *   (reference assets/shaders/raygen.rgen:194-229).
 * Traces the pixel rectangle [x0,x0+w) x [y0,y0+h) of the ctx-sized frame (tile-able for
 * the multi-GPU partition) and copies the w*h records row-major to `out_hits_host`.
 * Blocking, like the reference's cudaDeviceSynchronize (cuda_tracer.cu:539). */
int blok_hip_trace_primary(blok_hip_ctx* ctx, const blok_camera* cam,
                           uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                           blok_hit* out_hits_host);

/* Same work, device-resident outputs, asynchronous on `hip_stream` (a hipStream_t, or NULL for the default
 * stream).  `out_hits_dev` (w*h 16-B records) and `out_rgba_dev` (w*h RGBA8 pixels: the frame through
 * hit.rchit's material fetch, reference assets/shaders/hit.rchit:58-67; the CUDA backend's output format,
 * reference blok/src/cuda_tracer.cu:385-386) are device pointers; either may be NULL, not both.
 * This is the entry the benchmark times and the one a graph capture may record (no allocation, no host
 * sync inside). */
int blok_hip_trace_primary_device(blok_hip_ctx* ctx, const blok_camera* cam,
                                  uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                  void* out_hits_dev, void* out_rgba_dev, void* hip_stream);

/* Interleaved-tile form of the multi-GPU partition: rank r of n traces the tiles
 * (tile x tile pixels, row-major tile index i) with i % n == r and writes them densely,
 * tile after tile, each tile row-major; each output holds
 * blok_hip_tiles_for_rank(...) * tile*tile elements (edge tiles are padded with misses / sky). */
uint32_t blok_hip_tiles_for_rank(uint32_t width, uint32_t height, uint32_t tile,
                                 uint32_t rank, uint32_t n_ranks);
int blok_hip_trace_tiles_device(blok_hip_ctx* ctx, const blok_camera* cam,
                                uint32_t tile, uint32_t rank, uint32_t n_ranks,
                                void* out_hits_dev, void* out_rgba_dev, void* hip_stream);
/* Root side: scatter n_ranks gathered tile buffers (rank-major, each padded to `tiles_per_rank_max`
 * tiles) of `elem_bytes`-sized elements (16: hit records, 4: RGBA8) back into a row-major
 * width*height frame. */
int blok_hip_untile_device(blok_hip_ctx* ctx, const void* gathered_dev, uint32_t elem_bytes, uint32_t tile,
                           uint32_t n_ranks, uint32_t tiles_per_rank_max,
                           void* out_frame_dev, void* hip_stream);

/* Sparse framebuffer exchange for the tile partition (no reference counterpart: blok is single-GPU): most
 * of a frame's tiles can be sky, and only bytes cross xGMI slowly.  compact: from a rank's dense RGBA8 tile buffer (as
 * blok_hip_trace_tiles_device writes it) to  word 0 = number of tiles with at least one non-sky pixel, then one record
 * {local tile index, tile*tile pixels} per such tile, in no particular order; `out_words_dev` holds
 * blok_hip_compact_words(tile, n_tiles) 32-bit words.  A prefix of 1 + S * (1 + tile*tile) words carries the first S records.
 * scatter (on the root): writes the context's width x height RGBA8 frame: the tiles the ranks' records hold (rank r's buffer
 * starts at word r * rank_stride_words; at most max_records records each are looked at; local tile index j of rank r is frame
 * tile r + j * n_ranks) and the sky colour everywhere else.  Both asynchronous on `hip_stream`. */
size_t blok_hip_compact_words(uint32_t tile, uint32_t n_tiles);
int blok_hip_compact_tiles_device(blok_hip_ctx* ctx, const void* rgba_tiles_dev, uint32_t tile, uint32_t n_tiles,
                                  void* out_words_dev, void* hip_stream);
int blok_hip_scatter_tiles_device(blok_hip_ctx* ctx, const void* gathered_dev, uint32_t n_ranks, size_t rank_stride_words,
                                  uint32_t tile, uint32_t max_records, void* out_frame_rgba_dev, void* hip_stream);

/* Several frames per call (no reference counterpart: the reference issues one traceRaysKHR per frame,
 * blok/src/renderer_raytracing.cpp:666-685, on one GPU).  At N ranks one frame's share of the tiles is 1/N of a launch whose
 * duration is mostly latency, and every call and collective costs host time, so a rank traces up to BLOK_MAX_TILE_FRAMES
 * consecutive frames — cams[0 .. n_frames), one camera each — in ONE beam + trace launch pair and exchanges them together.
 * Frame f of a dense tile buffer starts `frame_stride_tiles` tiles behind frame f - 1; the root's output frames are contiguous
 * (width*height elements each).  Each call equals n_frames calls of the one-frame
 * entry above it, bit for bit. */
#define BLOK_MAX_TILE_FRAMES 8
int blok_hip_trace_tile_frames_device(blok_hip_ctx* ctx, const blok_camera* cams, uint32_t n_frames,
                                      uint32_t tile, uint32_t rank, uint32_t n_ranks, uint32_t frame_stride_tiles,
                                      void* out_hits_dev, void* out_rgba_dev, void* hip_stream);
/* gathered: rank r's block starts at tile r * tiles_per_rank_max, frame f inside it at tile f * frame_stride_tiles */
int blok_hip_untile_frames_device(blok_hip_ctx* ctx, const void* gathered_dev, uint32_t elem_bytes, uint32_t tile,
                                  uint32_t n_ranks, uint32_t tiles_per_rank_max, uint32_t n_frames, uint32_t frame_stride_tiles,
                                  void* out_frames_dev, void* hip_stream);
/* Sparse exchange of n_frames frames.  compact: `out_words_dev` holds n_frames * blok_hip_compact_words(tile, n_tiles) words:
 * n_frames count words, then the records INTERLEAVED by frame — record slot j of frame f at word
 * n_frames + (j * n_frames + f) * (1 + tile*tile) — so that the first S slots of all frames are one contiguous prefix of
 * n_frames * (1 + S * (1 + tile*tile)) words: what travels (n_frames = 1 is the one-frame layout above).
 * scatter (root): rank r's prefix starts at word r * rank_stride_words; writes n_frames contiguous width*height RGBA8 frames: a
 * tile some record holds gets its pixels, every other tile the sky colour, no pixel is written twice.  tile_state_dev (optional):
 * n_frames * ceil(width/tile) * ceil(height/tile) bytes that belong to `out_frames_rgba_dev` — zero while the buffer is all sky —
 * in which the call keeps "this tile of this frame buffer holds something other than sky"; with it a sky tile that stays sky is
 * not written at all (the root's assembly is on every frame's critical path).  NULL: every tile is written. */
int blok_hip_compact_tile_frames_device(blok_hip_ctx* ctx, const void* rgba_tiles_dev, uint32_t tile, uint32_t n_tiles,
                                        uint32_t n_frames, uint32_t frame_stride_tiles, void* out_words_dev, void* hip_stream);
int blok_hip_scatter_tile_frames_device(blok_hip_ctx* ctx, const void* gathered_dev, uint32_t n_ranks, size_t rank_stride_words,
                                        uint32_t tile, uint32_t max_records, uint32_t n_frames,
                                        void* out_frames_rgba_dev, void* tile_state_dev, void* hip_stream);

/* The same exchange with 16 bits per pixel.  A shaded pixel is a function of (material id, face) or the sky, and every rank holds
 * the material table, so a pixel can travel as  code = min(material id, n_materials) * 8 + face  (0xFFFF = sky), made from the
 * rank's FIRST-HIT tiles (what blok_hip_trace_tile(_frame)s_device writes to out_hits_dev) and expanded on the root through the
 * function the trace kernels shade with: the assembled RGBA8 frames are bit-identical, the bytes on the wire half.
 * blok_hip_exchange_code_bits: 16 if the uploaded material table allows it ((n_materials + 1) * 8 <= 0xFFFF), else 0 (use the
 * RGBA8 entries).  Buffers as above with records of 1 + tile*tile/2 words: blok_hip_compact_code_words(tile, n_tiles) words per frame. */
uint32_t blok_hip_exchange_code_bits(const blok_hip_ctx* ctx);
size_t blok_hip_compact_code_words(uint32_t tile, uint32_t n_tiles);
int blok_hip_compact_hit_tile_frames_device(blok_hip_ctx* ctx, const void* hit_tiles_dev, uint32_t tile, uint32_t n_tiles,
                                            uint32_t n_frames, uint32_t frame_stride_tiles, void* out_words_dev, void* hip_stream);
int blok_hip_scatter_code_tile_frames_device(blok_hip_ctx* ctx, const void* gathered_dev, uint32_t n_ranks, size_t rank_stride_words,
                                             uint32_t tile, uint32_t max_records, uint32_t n_frames,
                                             void* out_frames_rgba_dev, void* tile_state_dev, void* hip_stream);

/* The reference's per-pixel sample / bounce loop and G-buffer: raygen.rgen:167-414 with hit.rchit, miss.rmiss
 * and shadow.rmiss (reference assets/shaders/).  Planes are float4 per pixel of the rectangle, row-major; any
 * pointer may be NULL.  color = (rgb, 1); world_pos = (first-hit position, depth); normal_roughness;
 * albedo_metallic (raygen.rgen:392-407; the reference stores the last two as RGBA16F / RGBA8).
 * spp = FrameUBO.sampleCount (8 in the reference, renderer_denoising.cpp:683), max_bounces = MAX_BOUNCES
 * (2, raygen.rgen:211), frame_index = FrameUBO.frameCount (seeds the RNG, raygen.rgen:92-99). */
typedef struct blok_gbuffer {
    float* color;
    float* world_pos;
    float* normal_roughness;
    float* albedo_metallic;
} blok_gbuffer;
int blok_hip_trace_paths_device(blok_hip_ctx* ctx, const blok_camera* cam,
                                uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                uint32_t spp, uint32_t max_bounces, uint32_t frame_index,
                                const blok_gbuffer* planes_dev, void* hip_stream);
/* The same frame with the G-buffer in the reference's own image formats (raygen.rgen:55-59; created at
 * blok/src/renderer_denoising.cpp:110-170): colour RGBA32F, world position + depth RGBA32F, normal + roughness RGBA16F, albedo +
 * metallic RGBA8 (unorm), motion vectors RG16F written by the path kernel itself (computeMotionVector, raygen.rgen:150-155,
 * 409-413, from prev_view_proj = FrameUBO::prevViewProj, column-major; 0 on the sky).  48 B/pixel instead of 64.  Any plane may
 * be NULL; a motion plane needs prev_view_proj.  Conversions as the image stores do them: binary16 round to nearest even, unorm8
 * = floor(clamp(x, 0, 1) * 255 + 0.5).  blok_hip_denoise_ref_device takes these planes; blok_hip_draw_frame_rt uses them. */
typedef struct blok_gbuffer_ref {
    float*    color;             /* RGBA32F */
    float*    world_pos;         /* RGBA32F: xyz, depth */
    uint16_t* normal_roughness;  /* RGBA16F */
    uint32_t* albedo_metallic;   /* RGBA8: r | g << 8 | b << 16 | metallic << 24 */
    uint16_t* motion;            /* RG16F */
} blok_gbuffer_ref;
int blok_hip_trace_paths_ref_device(blok_hip_ctx* ctx, const blok_camera* cam,
                                    uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                    uint32_t spp, uint32_t max_bounces, uint32_t frame_index,
                                    const float prev_view_proj[16], const blok_gbuffer_ref* planes_dev, void* hip_stream);
/* Blocking form with host planes. */
int blok_hip_trace_paths(blok_hip_ctx* ctx, const blok_camera* cam,
                         uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                         uint32_t spp, uint32_t max_bounces, uint32_t frame_index,
                         const blok_gbuffer* planes_host);

/* = the tonemap pass of the post-process chain (reference assets/shaders/tonemap.comp:97-143, dispatched at
 * blok/src/renderer_postprocess.cpp:588-612): HDR float4 -> RGBA8.  Reference defaults: exposure 1.0,
 * saturation_boost 1.15, tonemap_operator 1 = Khronos PBR Neutral (0 = soft clip)
 * (reference blok/include/renderer_postprocess.hpp:110-113). */
int blok_hip_tonemap_device(blok_hip_ctx* ctx, const float* hdr_rgba_dev, uint32_t n_pixels, float exposure,
                            float saturation_boost, int tonemap_operator, void* out_rgba8_dev, void* hip_stream);
int blok_hip_tonemap(blok_hip_ctx* ctx, const float* hdr_rgba_host, uint32_t n_pixels, float exposure,
                     float saturation_boost, int tonemap_operator, uint32_t* out_rgba8_host);

/* Explicit rays (secondary rays; edge-case tests). n rays in, n records out, host arrays. */
int blok_hip_trace_rays(blok_hip_ctx* ctx, const blok_ray* rays_host, size_t n,
                        blok_hit* out_hits_host);

/* Shade first hits to RGBA8 (normal/albedo debug view through hit.rchit's material fetch,
 * reference assets/shaders/hit.rchit:55-76): out_rgba8_host[w*h]. */
int blok_hip_shade_rgba8(blok_hip_ctx* ctx, const blok_camera* cam,
                         uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                         uint32_t* out_rgba8_host);

/* = CudaTracer::drawFrame in the compute backend's progressive mode (reference blok/src/cuda_tracer.cu:484-555 with the
 * kernel's accumulate / ACES / gamma tail, :372-386, :209-216, :95-99): traces spp_per_frame samples per pixel of the
 * reference's sample/bounce loop with the RNG frame index = frames accumulated so far, adds the frame's average to the
 * accumulation buffer (xyz running sum, w = frames), clears that buffer first when any camera component moved by more
 * than 1e-5 (camChanged, :456-472) and writes the ACES-tonemapped, gamma-2.2 RGBA8 image of the running average to
 * out_rgba8_host (may be NULL).  Blocking. */
int blok_hip_draw_frame_accumulate(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp_per_frame, uint32_t max_bounces,
                                   uint32_t* out_rgba8_host, uint32_t* out_frames_accumulated);
/* The accumulation buffer: width*height float4 (xyz sum, w frames). */
int blok_hip_accum_download(blok_hip_ctx* ctx, float* out_rgba32f_host);
/* = CudaTracer::resetAccum (reference blok/src/cuda_tracer.cu:450-454). */
int blok_hip_reset_accum(blok_hip_ctx* ctx);

/* Milliseconds of the most recent trace kernel, measured with HIP events recorded on the
 * launch stream around the kernel only (valid after that stream has been synchronised). */
int blok_hip_last_kernel_ms(blok_hip_ctx* ctx, float* out_ms);

/* ---- image-space chain behind the path tracer -----------------------------------------------
 * Denoiser (temporal accumulation -> variance -> a-trous iterations), TAA resolve and sharpen as HIP kernels; the tonemap
 * pass between TAA and sharpen is blok_hip_tonemap_device.  Reference: assets/shaders/temporal_reproject.comp, variance.comp,
 * atrous.comp, taa.comp, sharpen.comp; orchestration blok/src/renderer_denoising.cpp:714-776, renderer_postprocess.cpp:505-556.
 * All planes are full-frame (ctx width x height), row-major, in device memory; calls enqueue on hip_stream and return. */
typedef struct blok_denoise_settings {       /* = Denoiser::Settings, blok/include/renderer_denoising.hpp:49-66 */
    float temporal_alpha, moment_alpha, variance_clip_gamma;
    float depth_threshold, normal_threshold;
    float phi_color, phi_normal, phi_depth;
    int32_t atrous_iterations;               /* <= 5 (DenoiserPipeline::MAX_ATROUS_ITERATIONS) */
    float variance_boost;
    int32_t min_history_length;
} blok_denoise_settings;
void blok_denoise_settings_default(blok_denoise_settings* out);
/* = Denoiser::denoise + copyCurrentGeometryToHistory + swapHistoryBuffers (renderer_denoising.cpp:714-776, 833-866, 690-697)
 * for one frame.  planes: float4 planes as blok_hip_trace_paths_device writes them (color, world_pos, normal_roughness;
 * albedo_metallic unused).  motion_dev: float2 per pixel, or NULL = the motion vectors of raygen.rgen:150-155,409-413 computed
 * from world_pos and prev_view_proj (column-major 4x4, = FrameUBO::prevViewProj).  frame_count = FrameUBO::frameCount
 * (0: no history is read).  settings NULL = defaults.  out_color_dev: float4 per pixel = Denoiser::getOutputImage(). */
int blok_hip_denoise_device(blok_hip_ctx* ctx, const blok_gbuffer* planes_dev, const float* motion_dev,
                            const float prev_view_proj[16], uint32_t frame_count, const blok_denoise_settings* settings,
                            float* out_color_dev, void* hip_stream);
/* The same for planes in the reference's image formats (blok_gbuffer_ref; motion NULL = computed from world_pos). */
int blok_hip_denoise_ref_device(blok_hip_ctx* ctx, const blok_gbuffer_ref* planes_dev, const float prev_view_proj[16],
                                uint32_t frame_count, const blok_denoise_settings* settings, float* out_color_dev, void* hip_stream);
/* Host copies of the denoiser's state after the last blok_hip_denoise_device (blocking; NULL pointers are skipped):
 * history colour float4, moments float2, history length float, variance float, motion vectors float2 (per pixel). */
int blok_hip_denoise_state(blok_hip_ctx* ctx, float* history_color, float* moments, float* history_length,
                           float* variance, float* motion);
/* = PostProcess TAA pass (taa.comp; renderer_postprocess.cpp:526-534,558-589): color_dev float4 in, out_color_dev float4 out;
 * the TAA history is kept by the context.  motion_dev: float2 per pixel or NULL = the motion vectors of the last
 * blok_hip_denoise_device call.  Defaults of the reference: feedback_min 0.93, feedback_max 0.98. */
int blok_hip_taa_device(blok_hip_ctx* ctx, const float* color_dev, const float* motion_dev, float feedback_min,
                        float feedback_max, uint32_t frame_count, float* out_color_dev, void* hip_stream);
/* = PostProcess sharpen pass (sharpen.comp; renderer_postprocess.cpp:548-555,619-642): RGBA8 in, RGBA8 out; default strength 0.5. */
int blok_hip_sharpen_device(blok_hip_ctx* ctx, const uint32_t* rgba8_dev, float strength, uint32_t* out_rgba8_dev, void* hip_stream);
/* Column-major (GLM layout) view-projection of a camera basis, such that ndc.xy * 0.5 + 0.5 of (M * vec4(p, 1)) is the screen
 * position of world point p under the basis' own primary-ray mapping: what FrameUBO::prevViewProj is to the reference's
 * shaders (temporal_reproject.comp:108-113), for callers that keep camera bases instead of matrices. */
void blok_camera_view_proj(const blok_camera* cam, float out_view_proj[16]);
/* = Renderer::drawFrame's ray-tracing path (reference blok/src/renderer_draw.cpp: trace -> Denoiser::denoise -> PostProcess::process):
 * one frame of the sample/bounce loop (spp samples, the reference forces 8; max_bounces, the reference's MAX_BOUNCES is 2) into
 * planes owned by the context, then denoiser, TAA (feedback 0.93..0.98), tonemap (Khronos PBR neutral, exposure 1, saturation
 * 1.15) and sharpen (0.5) with the reference's default settings; the previous frame's camera supplies prevViewProj and the frame
 * counter (RNG frame index, FrameUBO::frameCount) advances by one per call; blok_hip_post_reset restarts it.  Blocking.
 * out_rgba8_host: width*height RGBA8, may be NULL. */
int blok_hip_draw_frame_rt(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                           const blok_denoise_settings* settings, uint32_t* out_rgba8_host, uint32_t* out_frame_count);
/* Forget the denoiser and TAA histories (swapchain recreate: Denoiser::resize / PostProcess::resize). */
int blok_hip_post_reset(blok_hip_ctx* ctx);

/* ---- device-resident dense voxel store (edits and the rebuild they trigger, on the GPU) ----
 * The reference keeps Chunk::density / Chunk::materialIds on the host (blok/src/chunk.hpp:33-42), edits them with
 * setVoxelMaterial (chunk_manager.cpp:316-328) and applyBrush (brush.cpp:13-63), rebuilds dirty chunks' SVOs on the CPU
 * (chunk_manager.cpp:106-140), repacks (:213-314) and re-uploads (renderer_upload.cpp:237-312).  Here one box of the world
 * [origin, origin + (nx, ny, nz)) lives in HBM with the same two arrays (x fastest, then y, then z), edits are kernels
 * with the reference's float arithmetic, and blok_hip_volume_rebuild derives the traversal structure on the device from
 * "density > 0" (chunk_manager.cpp:121) and installs it as the context's world.  voxel_size must be 1; chunk_size is
 * ChunkManager's chunk edge (the brush computes voxel centres per chunk).  Edits outside the box are refused
 * (BLOK_ERR_UNSUPPORTED, nothing written).  All calls are blocking. */
int blok_hip_volume_create(blok_hip_ctx* ctx, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                           uint32_t chunk_size, float voxel_size);
int blok_hip_volume_destroy(blok_hip_ctx* ctx);
/* Whole-box upload / download of the two arrays; a null pointer uploads zeros / skips the download. */
int blok_hip_volume_upload(blok_hip_ctx* ctx, const float* density, const uint32_t* material_ids);
int blok_hip_volume_download(blok_hip_ctx* ctx, float* density, uint32_t* material_ids);
/* = ChunkManager::setVoxelMaterial for n world voxels xyz[3*i..], in order (a later entry of the same voxel wins);
 * material_ids null = 0, density null = 1. */
int blok_hip_volume_set_voxels(blok_hip_ctx* ctx, const int32_t* xyz, const uint32_t* material_ids, const float* density, size_t n);
/* = applyBrush (brush.cpp:13-63): mode 0 ADD density = max(density, value), 1 SUBTRACT density = min(density, value),
 * inside the sphere around `center` (world units), voxel centres as the reference computes them. */
int blok_hip_volume_apply_brush(blok_hip_ctx* ctx, const float center[3], float radius, float value, int mode);
/* (BLOK_SHAPE_ADD on a BLOK_SHAPE_ELLIPSOID, below, is NOT this brush: the brush keeps the reference's float voxel centres, computed per
 * chunk, and refuses a sphere that leaves the box; the shapes are integer rules and clip.) */
/* = rebuildDirtyChunks + packChunksToGpuSvo + Renderer::updateWorld for the box: installs the world made of the voxels with
 * density > 0 and their material ids, with the given material table. */
int blok_hip_volume_rebuild(blok_hip_ctx* ctx, const blok_material* materials, size_t n_materials);

/* ---- mesh voxelization into the resident volume (ABI 1.4) ----
 * Writes a triangle mesh into the box.  Host arrays: positions xyz per vertex (world units; the volume's voxel_size is 1), three
 * vertex indices per triangle, one material id per triangle or NULL (then `material` for all).
 *  - Snapping: every coordinate becomes q = rint(x * 256) (round half to even), a 64-bit integer; the box origin is origin * 256.  All
 *    later decisions are exact integer arithmetic on q, relative to each triangle's first vertex.  Shared vertices snap alike, so a
 *    closed mesh stays closed.
 *  - Limits (BLOK_ERR_INVALID_ARG, nothing written): a non-finite coordinate or |x| > 2^23 in a referenced vertex; an index >=
 *    n_vertices; a triangle whose snapped extent on an axis exceeds 2048 voxels; density not finite or <= 0; an unknown mode; a null
 *    array with a non-zero count.  With extents <= 2048 voxels (2^19 snapped units), edges are below 2^19, the normal's components below
 *    2^39, and the plane test's largest term below 3 * 2^39 * (2^20 + 2^13) < 2^61: int64 holds every product.  Volumes above 2^32 cells
 *    are refused (BLOK_ERR_UNSUPPORTED), as blok_hip_volume_set_voxels refuses them.  No volume: BLOK_ERR_NO_WORLD.
 *  - Surface set S: voxel (i, j, k) iff its closed cube [i, i+1] x [j, j+1] x [k, k+1] meets the closed snapped triangle (exact
 *    separating-axis test; a zero axis never separates, so a degenerate triangle is voxelized as the segment or point it is).  A
 *    triangle lying exactly in a lattice plane marks both neighbouring layers.
 *  - Interior set I (BLOK_VOXELIZE_SOLID only): voxel (i, j, k) iff an odd number of triangles cross its column (j + 1/2, k + 1/2) at
 *    x <= i + 1/2.  Triangles whose yz projection has zero area never count.  A column point on a projected edge or vertex counts for
 *    a triangle iff it would for the point moved by (+e, -e^2), e -> 0, after orienting the projection counter-clockwise (a top-left
 *    rule: a point on an edge (dy, dz) counts iff dz < 0, or dz == 0 and dy < 0).  A column through an edge or vertex shared by a
 *    closed edge-manifold mesh therefore counts like a column beside it.  Crossings left of the box count.  Open meshes get whatever
 *    the parity gives: the columns right of an unpaired crossing are filled up to the end of the box.
 *  - Written: S (surface mode) or S u I (solid mode), inside the box; other voxels are untouched (setVoxelMaterial's set semantics).
 *    A written voxel gets `density` and, on S, the material of the lowest-indexed triangle that overlaps it; interior-only voxels get
 *    `material`.  S and I depend neither on triangle order nor on vertex order or winding; the result is bit-identical from run to run.
 *  - Afterwards the masks, occupancy words and dirty flags are those blok_hip_volume_set_voxels leaves for the same writes; the next
 *    blok_hip_volume_rebuild installs the world.  Blocking.  out_n_voxels (may be NULL): voxels written. */
#define BLOK_VOXELIZE_SURFACE 0
#define BLOK_VOXELIZE_SOLID   1
int blok_hip_volume_voxelize_mesh(blok_hip_ctx* ctx, const float* positions, size_t n_vertices, const uint32_t* triangles, size_t n_triangles,
                                  const uint32_t* triangle_materials, uint32_t material, float density, int mode, uint64_t* out_n_voxels);

/* ---- procedural terrain into the resident volume (ABI 1.5) ----
 * A pure integer function of the world voxel coordinate (X, Y, Z): bit-identical on the host (blok_terrain_eval, blok_world.h) and on the
 * device, seamless across regions and boxes at any origin.  All arithmetic is unsigned 64-bit unless said otherwise; `>>` on a signed
 * coordinate is an arithmetic shift (floor), `&` takes its two's-complement low bits.  fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B;
 * h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16 (32-bit).  hash3(x, y, z, s) = fmix32(x * 0x9E3779B1 ^ y * 0x85EBCA77 ^ z * 0xC2B2AE3D ^ s),
 * 32-bit, coordinates as their low 32 bits.
 *  - fade(f, c): t = f << (16 - c); s = (t * t * (196608 - 2 t)) >> 32.   lerp16(a, b, s) = (a * (65536 - s) + b * s) >> 16.
 *  - 2-D value noise, cell 2^c, salt k: i = X >> c, j = Z >> c, sx = fade(X & (2^c - 1), c), sz alike; lattice value
 *    g(i, j) = hash3(i, 0x100 + k, j, seed) & 0xFFFF; v2 = lerp16(lerp16(g(i,j), g(i+1,j), sx), lerp16(g(i,j+1), g(i+1,j+1), sx), sz).
 *  - 3-D value noise, cell 2^c, salt word w: g(i, j, k) = hash3(i, j, k, seed ^ w) & 0xFFFF, indices (X, Y, Z) >> c; lerp16 along x,
 *    then y, then z, each with its axis' fade.
 *  - fBm of K octaves from cell 2^c: octave k = 0..K-1 has cell 2^(c-k) and weight 2^(K-1-k); fbm = (sum weight * value) / (2^K - 1).
 *  - H(X, Z) = base_height + ((fbm2(height_octaves, height_cell_log2; salts 0..K-1) * amplitude) >> 16), int32.
 *  - cave(X, Y, Z): cave_octaves > 0 and Y <= H - cave_roof and fbm3(cave_octaves, cave_cell_log2; salt words 0x51ED0000 + k) <
 *    cave_threshold.   solid(X, Y, Z) = Y <= H(X, Z) and not cave.  Nothing bounds it below.
 *  - material, d = H - Y: d == 0 surface; d <= soil_depth soil; else ore if the one-octave 3-D noise (cell 2^ore_cell_log2, salt word
 *    0x0BE00000) > ore_threshold, else rock.
 *  - Written, for every voxel of the region (world voxels, half-open; both NULL = the whole box): without flags a solid voxel gets
 *    (density, material) and every other voxel (0.0f, 0).  SHELL: "solid" becomes "solid with at least one of its six neighbours not
 *    solid", neighbours judged by the function (not by the store or the region).  CLOSE_SIDES: an x or z neighbour outside the region
 *    counts as not solid (y is not closed).  ADD: voxels that would get (0, 0) are not touched.
 *  - BLOK_ERR_INVALID_ARG, nothing written: height_octaves not in 1..8 or > height_cell_log2 + 1; height_cell_log2 > 12; cave_octaves > 4
 *    or > cave_cell_log2 + 1; cave_cell_log2 > 12; ore_cell_log2 > 12; a threshold > 65536; amplitude > 65536; |base_height| > 2^24;
 *    density not finite or <= 0; unknown flag bits; CLOSE_SIDES without SHELL; exactly one region pointer NULL; lo > hi on an axis.  A
 *    region that leaves the box, or a volume above 2^32 cells: BLOK_ERR_UNSUPPORTED, as the other edits answer.  No volume:
 *    BLOK_ERR_NO_WORLD.  An empty region is BLOK_OK.
 *  - Afterwards masks, occupancy words, dirty flags and the edited box are those blok_hip_volume_set_voxels leaves for the same writes;
 *    the next blok_hip_volume_rebuild installs the world.  Blocking.  out_n_voxels (may be NULL): filled voxels written. */
typedef struct blok_terrain_params {
    uint32_t seed;
    int32_t  base_height;                 /* world y of the lowest possible surface voxel */
    uint32_t amplitude;                   /* the surface lies in [base_height, base_height + amplitude) */
    uint32_t height_cell_log2, height_octaves;
    uint32_t cave_cell_log2, cave_octaves;      /* cave_octaves 0 = no caves */
    uint32_t cave_threshold;              /* 0..65536 */
    uint32_t cave_roof;                   /* caves only where y <= H - cave_roof */
    uint32_t soil_depth;
    uint32_t ore_cell_log2, ore_threshold;      /* ore_threshold 65536 = no ore */
    uint32_t surface_material, soil_material, rock_material, ore_material;
    float    density;                     /* written into filled voxels; finite and > 0 */
    uint32_t flags;
} blok_terrain_params;
#define BLOK_TERRAIN_SHELL        1u   /* write only filled voxels that have an empty 6-neighbour */
#define BLOK_TERRAIN_CLOSE_SIDES  2u   /* with SHELL: x/z neighbours outside the region count as empty */
#define BLOK_TERRAIN_ADD          4u   /* write filled voxels only; leave every other voxel as it is */
int blok_hip_volume_generate_terrain(blok_hip_ctx* ctx, const blok_terrain_params* params, const int32_t region_lo[3],
                                     const int32_t region_hi[3], uint64_t* out_n_voxels);

/* ---- the volume's surface as merged quads (ABI 1.6) ----
 * Integer arithmetic on the two arrays of the volume: the result is a pure function of (arrays, box origin, region, flags), bit-identical
 * on the host (blok_quads_extract, blok_world.h) and on the device.
 *  - Filled: a voxel is filled iff its density > 0 (the rebuild's rule; NaN and negative densities are empty).
 *  - Exposed face: faces are numbered as blok_hit::face (0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z).  Face f of a filled voxel p inside the region is
 *    exposed iff the neighbour p + n_f is not filled.  A neighbour outside the region but inside the box is judged by the store, so
 *    regions extracted side by side give exactly the faces of one extraction over their union.  A neighbour outside the box is empty.
 *  - Key: the voxel's material id; with BLOK_QUADS_IGNORE_MATERIAL 0 for every face (collider meshes).
 *  - Plane axes: for a face with normal axis a, u is the lower of the two other axes and v the higher: x -> (y, z), y -> (x, z),
 *    z -> (x, y).
 *  - Runs: for one face number, plane (the voxel coordinate along a) and row v, a run is a maximal set of cells consecutive along u,
 *    inside the region, that are all exposed with the same key.
 *  - Quads: two runs in rows v and v + 1 of the same face number and plane are identical iff they have the same first cell, last cell
 *    and key.  A quad is a maximal stack of identical runs in consecutive rows.  A row holds at most one run starting at a given cell,
 *    so stacks are unique: run-length merging plus vertical merging of equal runs.  (Not the sequential "greedy" rectangle cover: this
 *    rule is order-free, has one answer, and both the origin and the extent of a quad are local predicates.)
 *  - Corners: the rectangle is lo + [0, du] e_u + [0, dv] e_v.  Counter-clockwise seen from outside: c0 = lo, c1 = lo + du e_u,
 *    c2 = c1 + dv e_v, c3 = lo + dv e_v when (e_u x e_v) . n_f > 0 (faces 0, 3, 4), otherwise c0, c3, c2, c1.  The triangles are
 *    (c0, c1, c2) and (c0, c2, c3) of that order.
 *  - Order: quads are sorted by (face, lo[a], lo[v], lo[u]) ascending; with the rules above this order is total.
 *  - Counts: n_faces is the number of exposed unit faces and equals the sum of du * dv over the quads.  Both counts are 64-bit.
 *  - Bounds: quads <= exposed faces <= 6 * filled voxels.  The worst case is a checkerboard, 3 quads per cell of the region, so the
 *    result is sized by a counting pass, never by a bound.
 *  - blok_hip_volume_extract_quads: the region is in world voxels, half open; both pointers NULL = the whole box.  Blocking.  The quad
 *    array stays in device memory, owned by the context: a snapshot that later edits do not touch.  The next extraction replaces it;
 *    blok_hip_volume_destroy, a new blok_hip_volume_create and blok_hip_destroy free it.  With BLOK_QUADS_COUNT_ONLY only the two counts
 *    are produced and nothing is kept (an earlier snapshot stays).  Either count pointer may be NULL.
 *  - blok_hip_volume_quads_download copies records [first, first + count) of the snapshot, so a large result can be fetched in pieces.
 *  - Errors, each leaving the previous snapshot as it was.  BLOK_ERR_INVALID_ARG: unknown flag bits, exactly one region pointer NULL,
 *    lo > hi on an axis.  BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume above 2^32 cells, a region with 2^31 or more
 *    rows in total over the six face numbers.  BLOK_ERR_NO_WORLD: no volume.  An empty region is BLOK_OK with zero counts (and, without
 *    COUNT_ONLY, an empty snapshot).  BLOK_ERR_OOM: a failed device allocation.  The download answers BLOK_ERR_INVALID_ARG when there is
 *    no snapshot, the range goes past its end, or out_host is NULL with count > 0. */
typedef struct blok_quad {
    int32_t  lo[3];     /* lowest LATTICE corner, world units: lo[a] = voxel coordinate (+1 for faces 0, 2, 4), lo[u], lo[v] = first cell */
    uint32_t du, dv;    /* extent in cells along u and v, both >= 1 */
    uint32_t material;  /* the key */
    uint32_t face;      /* 0..5 */
    uint32_t reserved;  /* 0 */
} blok_quad;
#define BLOK_QUADS_IGNORE_MATERIAL 1u   /* key 0 for every face */
#define BLOK_QUADS_COUNT_ONLY      2u   /* produce the counts only; keep nothing */
int blok_hip_volume_extract_quads(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                                  uint64_t* out_n_quads, uint64_t* out_n_faces);
int blok_hip_volume_quads_download(blok_hip_ctx* ctx, blok_quad* out_host, uint64_t first, uint64_t count);

/* ---- emissive voxels as lights (ABI 1.26) ----
 * Without a light table a path-traced frame aims at one light only, the sun, and an emissive voxel lights its surroundings only when a
 * bounce ray happens to hit it.  A context that holds a light table samples it at every eligible hit of every path-traced entry.
 *  - A light is a rectangle of du x dv exposed unit faces: a blok_quad whose `reserved` word is `cum`, the exclusive prefix sum of du * dv
 *    in table order.  Same lattice, plane axes and face numbering as a quad; world position = lattice x voxel size.  The total A of
 *    du * dv must be < 2^32 and the number of lights < 2^31 (BLOK_ERR_UNSUPPORTED otherwise), so selecting a face is integer work with one
 *    right answer: pick = (r * A) >> 32 for a 32-bit random r, the light is the last with cum <= pick, the cell (pick - cum) % du,
 *    (pick - cum) / du.
 *  - Beside the table the context keeps A, area_world = float(A) * vs * vs, and the OWNED set: the material indices that occur in the
 *    table (index of an id as a hit forms it: min(id, 65535), then 0 when beyond the material table).
 *  - CONTRACT: an installed table holds EVERY exposed world face of every owned material.  The lit loop counts an owned material's
 *    emission through the table wherever a diffuse bounce ray finds it in the world, and by the hit everywhere else (first hits, specular
 *    rays, models, materials the table does not own); a table that misses faces of an owned material loses their light on diffuse paths.
 *  - blok_hip_lights_from_quads builds the table on the device from the context's quads snapshot (blok_hip_volume_extract_quads): a quad
 *    is kept iff the material its key maps to in the context's CURRENT material table is emissive (dot(emission, 1) > 0.01, the path loop's
 *    test); order is the quads' order.  flags must be 0.  Bit-identical to blok_lights_from_quads (blok_world.h) over the same quads and
 *    materials.  Errors, each leaving the previous table in place: BLOK_ERR_NO_WORLD without a world; BLOK_ERR_INVALID_ARG without a quads
 *    snapshot or a material table, for a snapshot taken with BLOK_QUADS_IGNORE_MATERIAL, for flags != 0; BLOK_ERR_UNSUPPORTED for the
 *    limits above; BLOK_ERR_OOM.  A result of no lights installs the empty table, which is the same as clearing.  Blocking.
 *  - blok_hip_set_lights installs a host-built table (a world that is not a volume: blok_quads_extract, then blok_lights_from_quads).
 *    Checked: face < 6; du, dv >= 1; cum equal to the running sum; A < 2^32; every corner inside [-32768, 32768].  A failed check is
 *    BLOK_ERR_INVALID_ARG (BLOK_ERR_UNSUPPORTED for A or n above the limits) and leaves the previous table.  n = 0 or NULL clears.
 *  - blok_hip_lights_info reports what is installed (zeros without a table); blok_hip_lights_download copies records
 *    [first, first + count), in pieces as the other snapshots do (BLOK_ERR_INVALID_ARG for a range past the end).  out_info may be NULL.
 *  - Life: the table is the context's.  Edits, a new quads extraction and blok_hip_volume_scroll leave it alone — a stale table is the
 *    caller's matter, as a stale instance table is.  blok_hip_destroy frees it.  It is CLEARED by every call that installs another world
 *    or material table (blok_hip_upload_world, blok_hip_upload_dense, blok_hip_volume_rebuild, and what removes the world): the owned set
 *    is a statement about that table.  So: rebuild, extract quads, then build the lights.
 *  - Frames: while a table with n >= 1 is installed every path-traced entry (blok_hip_trace_paths*, their instanced and posed forms, the
 *    blok_hip_draw_frame_rt* chain) runs the lit loop; they all launch through one dispatch point, and there is no path-traced entry that
 *    ignores the table.  With no table every entry runs the kernel it ran before, bit for bit.  The rule of the lit loop is DESIGN.md §32. */
typedef struct blok_light {
    int32_t  lo[3];     /* as blok_quad */
    uint32_t du, dv;
    uint32_t material;
    uint32_t face;
    uint32_t cum;       /* exposed unit faces of the lights before this one */
} blok_light;
typedef struct blok_lights_info {
    uint64_t n_faces;   /* A */
    uint64_t bytes;     /* of the table in device memory (host build: of the records) */
    uint32_t n;         /* lights */
    uint32_t n_owned;   /* material indices in the owned set */
    float    area_world;
    uint32_t reserved;  /* 0 */
} blok_lights_info;
int blok_hip_lights_from_quads(blok_hip_ctx* ctx, uint32_t flags, blok_lights_info* out_info);
int blok_hip_set_lights(blok_hip_ctx* ctx, const blok_light* lights_host, uint32_t n, blok_lights_info* out_info);
int blok_hip_lights_info(blok_hip_ctx* ctx, blok_lights_info* out_info);
int blok_hip_lights_download(blok_hip_ctx* ctx, blok_light* out_host, uint64_t first, uint64_t count);

/* ---- the light grid: per-cell lists over the world's light table (ABI 1.29) ----
 * The pick above is uniform over every face of the table, wherever the shading point is.  A light grid says, for every cell of a coarse
 * lattice, which lights are near it, and while a grid is installed every path-traced entry picks through it: a fourth draw chooses, with
 * probability share / 256 where the shading point's cell has a list, a face of that list, else a face of the whole domain as before, and
 * the density of the mixture stands where 1 / A stood, so the estimator's expectation is unchanged (DESIGN.md §34 has the rule).  With no
 * grid every entry runs the kernel it ran before, bit for bit.  A launch that samples lit lattice instances ("emissive models as lights":
 * a model light table and an instance table with n > 0) keeps its own kernel and the global pick over A_total, grid or no grid.
 *  - Parameters: cell_log2 = c in 2..12 (cells of 2^c world voxels on the world lattice: cell = voxel >> c, arithmetic), reach = R in
 *    0..3 cells, share = s in 1..255 (the local strategy's probability in 1/256; the build stores it).  flags must be 0.
 *  - A light's cells: on its plane axis a = face >> 1 the emitting voxel is lo[a] - 1 for a + face and lo[a] for a - face; in the plane
 *    the voxels are [lo_u, lo_u + du - 1] and [lo_v, lo_v + dv - 1].  cmin_k, cmax_k are those bounds >> c.
 *  - in(L, g) iff cmin_k(L) - R <= g_k <= cmax_k(L) + R on every axis k: the one predicate.
 *  - The box: cell_lo_k = min over the lights of cmin_k - R, cell_hi_k = max of cmax_k + R, dim_k = cell_hi_k - cell_lo_k + 1; cell
 *    (x, y, z), relative to cell_lo, has index (z * dim_y + y) * dim_x + x.
 *  - Per cell g: the lights with in(L, g) in ascending table index, as items {light, lcum}, lcum the exclusive prefix sum of du * dv
 *    within the list; faces[g] the list's total; start[n_cells + 1] the CSR offsets into the items.
 *  - Limits (BLOK_ERR_UNSUPPORTED): n_cells > 2^24, n_items >= 2^28.
 *  - blok_hip_build_light_grid builds the grid on the device over the installed world light table and installs it in place of an earlier
 *    one.  Bit-identical in all three arrays to blok_light_grid_build (blok_world.h).  Blocking.  Errors, each leaving the previous grid in
 *    place: BLOK_ERR_INVALID_ARG without a world light table, for a parameter out of range, for flags != 0; BLOK_ERR_UNSUPPORTED for the
 *    limits; BLOK_ERR_OOM.  out may be NULL.
 *  - blok_hip_light_grid_info reports the installed grid (zeros without one).  blok_hip_light_grid_download copies elements
 *    [first, first + count) of one array: what = 0 start (n_cells + 1 uint32), 1 faces (n_cells uint32), 2 items (n_items
 *    blok_light_grid_item); BLOK_ERR_INVALID_ARG without a grid, for another `what`, for a range past the end.  blok_hip_light_grid_clear
 *    drops the grid.
 *  - Life: the grid is a statement about one light table.  Everything that installs or clears the world's light table drops it
 *    (blok_hip_lights_from_quads, blok_hip_set_lights, and every call that clears the table: see "Life" above).  Edits and scrolls leave it
 *    alone: a stale grid is the caller's matter, as a stale table is. */
typedef struct blok_light_grid_item { uint32_t light, lcum; } blok_light_grid_item;
typedef struct blok_light_grid_info {
    int32_t  cell_lo[3]; uint32_t dim[3];
    uint32_t cell_log2, reach, share, n_nonempty;
    uint64_t n_cells, n_items, bytes;   /* bytes: of the three arrays */
    uint32_t max_items;                 /* the longest list */
    uint32_t reserved;                  /* 0 */
} blok_light_grid_info;
int blok_hip_build_light_grid(blok_hip_ctx* ctx, uint32_t cell_log2, uint32_t reach, uint32_t share, uint32_t flags, blok_light_grid_info* out);
int blok_hip_light_grid_info(blok_hip_ctx* ctx, blok_light_grid_info* out);
int blok_hip_light_grid_download(blok_hip_ctx* ctx, uint32_t what, void* out_host, uint64_t first, uint64_t count);
int blok_hip_light_grid_clear(blok_hip_ctx* ctx);

/* TAA jitter of the primary rays of all following frames, in pixels (each within +-0.5; NULL or {0,0} = none, the default and
 * the parity / benchmark contract).  The reference applies its Halton(2,3) - 0.5 sequence through the projection matrix
 * (getJitteredProjection, blok/src/renderer_postprocess.cpp:254-268: proj[2][0..1] += 2 j / size, handed to raygen.rgen as
 * invProj, blok/src/renderer_draw.cpp:64-81); in the basis form of this backend that is the same ray as NDC + 2 j / size, i.e. a
 * sub-pixel offset of +j pixels.  blok_taa_jitter (blok_world.h) gives the sequence.  blok_hip_draw_frame_rt applies entry
 * (frame mod 16) by itself (blok_hip_set_rt_taa_jitter(ctx, 0) = PostProcess::Settings::enableTAA false for the jitter). */
int blok_hip_set_taa_jitter(blok_hip_ctx* ctx, const float jitter_px[2]);
int blok_hip_set_rt_taa_jitter(blok_hip_ctx* ctx, int enabled);
/* Enable/disable the per-launch HIP event pair (default off: nothing but the kernel is
 * enqueued by the *_device entries). */
int blok_hip_set_timing(blok_hip_ctx* ctx, int enabled);

/* Library/ABI version: (major<<16)|minor.  1.1: instanced voxel models (below).  1.2: path-traced frames with instances.
 * 1.3: object motion vectors for moving instances.  1.4: mesh voxelization into the resident volume.
 * 1.5: procedural terrain into the resident volume.  1.6: the volume's surface as merged quads.
 * 1.7: models stamped into the resident volume, regions of it captured as models.
 * 1.8: connected components of the resident volume, one of them captured as a model.
 * 1.9: placed models swept against the resident volume (overlap, free travel along an axis).
 * 1.10: the resident volume saved, restored and undone as a sparse brick stream.
 * 1.11: the capped squared distance field of the resident volume; grow, shrink and hollow by it.
 * 1.12: the step field of the resident volume flooded from seeds; fill, seal, paint and clear by it.
 * 1.13: the column height field of the resident volume; models scattered onto it as an instance table.
 * 1.14: the resident volume's box scrolled through the world in device memory.
 * 1.15: a table of integer shapes (box, ellipsoid, capsule, cylinder; set, keep, erase, paint, replace, add, subtract) applied to the
 *       resident volume in one pass.
 * 1.16: the resident volume reduced to a pyramid of coarser levels (counts and a voted material id per cell); a level as a model.
 * 1.17: a power-of-two scale on instanced models (blok_hip_model_set_scale): a coarse level traced at its true size beside the world.
 * 1.18: models resampled into the resident volume through an affine map (blok_hip_volume_stamp_affine): any rotation, scale, mirror, shear.
 * 1.19: neighbour-count rules stepped over the resident volume (blok_hip_volume_automaton): smooth, despeckle, fill pits, caves, Life.
 * 1.20: procedural terrain reduced to coarse levels without a volume (blok_hip_terrain_reduce): the far field built at any time.
 * 1.21: a view at rest restarts every listed ray where its own counted walk ended (blok_hip_debug.h: blok_hip_set_beam_cache mode 4, the default).
 * 1.22: instanced models traced under any rotation, scale, mirror or shear (blok_pose; blok_hip_trace_primary_posed*, blok_hip_trace_rays_posed*).
 * 1.23: posed models in the path-traced frame, with true world normals (blok_hip_trace_paths_posed*, blok_hip_draw_frame_rt_posed).
 * 1.24: a packed frame of a view at rest in one launch, the misses written beside the walk (blok_hip_debug.h: blok_hip_set_packed_fill).
 * 1.25: object motion for posed models in the path-traced chain (blok_pose_motion; blok_hip_posed_motion_device, blok_hip_denoise_posed*,
 *       blok_hip_draw_frame_rt_posed_motion).  (Planned as 1.24; that number went to the packed frame first.)
 * 1.26: emissive voxels as lights: a light table built from the quads snapshot and sampled at every hit of the path loop (blok_light;
 *       blok_hip_lights_from_quads, blok_hip_set_lights, blok_hip_lights_info, blok_hip_lights_download).
 * 1.27: a view at rest re-enters every listed ray at the node its restarted walk ends in (blok_hip_debug.h: blok_hip_set_beam_cache mode 5, the default).
 * 1.28: emissive models as lights: a light table per model built from its own tree, sampled through the lattice instances of a path-traced
 *       launch by a per-launch prefix over the instance table (blok_hip_model_lights*, blok_hip_instance_lights_info).
 * 1.29: the light grid: per-cell lists of the world's lights, built on the device (blok_light_grid_item, blok_light_grid_info;
 *       blok_hip_build_light_grid, blok_hip_light_grid_info, blok_hip_light_grid_download, blok_hip_light_grid_clear), and the lit
 *       path loop's pick mixed between the shading point's own list and the whole table. */
uint32_t blok_hip_abi_version(void);

/* ------------------------------------------------------------- instanced voxel models
 * No reference counterpart yet: the reference's TLAS holds one instance with an identity transform
 * (blok/src/renderer_raytracing.cpp:142-157) and its todo list asks for "one BLAS per chunk, multiple TLAS instances".
 *
 * Model.  A voxel set with material ids, uploaded once and kept in HBM as its own 64-tree in its own local lattice.  It uses the
 *   world's material table and the world's voxel size (vs).
 * Instance.  blok_instance below: {model, offset (voxels), axis (a permutation of 0, 1, 2), flip (3 bits)}, 32 bytes.
 * Ray into local space.  With s_k = -1 if flip bit k is set, else +1, for local axis k:
 *     o'_k = s_k * fl(o[axis[k]] - offset[axis[k]] * vs),   d'_k = s_k * d[axis[k]],   tmin and tmax unchanged.
 * Walk.  The transformed ray walks the model's tree by the canonical rule of DESIGN.md §3 (unchanged).
 * Record back to world space.  t and material_id unchanged; world voxel w[axis[k]] = offset[axis[k]] + v'_k if flip bit k is clear,
 *   offset[axis[k]] - 1 - v'_k if it is set; local face 2k + n becomes world face 2 * axis[k] + (n XOR flip_k).
 * Composition.  Candidates in the order: the world, then instance 0, 1, 2, ...; a candidate replaces the current record only if its t
 *   is strictly smaller.  A tie goes to the world, then to the lowest instance index.  (Each instance walks with tmax = the best t so
 *   far, and the walk accepts t < tmax: the order falls out of the walk.)
 * Limits.  Every instance's world box must lie in the int16 lattice of the hit records ([-32768, 32768) on every axis); axis must be a
 *   permutation, flip < 8, the reserved words zero, the model id one that exists.  The entries with host instance tables fail with
 *   BLOK_ERR_INVALID_ARG otherwise; the device entries cannot look at their table without a host synchronise, so their kernels skip
 *   any instance that fails these checks (check a table with blok_hip_check_instances).
 * Scaled models.  A model has a scale exponent e, 0 <= e <= 8, default 0 (blok_hip_model_set_scale): one model voxel is a cube of 2^e world
 *   voxels, wherever the model is placed.  With vm = vs * 2^e:
 *   - Ray into local space: unchanged.  The offset stays in world voxels and need not be a multiple of 2^e.
 *   - Walk: the canonical walk over the model's tree with voxel size vm and 1 / vm (exact powers of two); the local box test uses vm too.
 *   - Record back to world space: t, material_id and the face rule unchanged.  The voxel is the hit cell's lowest world voxel:
 *     w[axis[k]] = offset[axis[k]] + v'_k * 2^e if flip bit k is clear, offset[axis[k]] - (v'_k + 1) * 2^e if it is set (64-bit sums
 *     before the record narrows them).  The instance id says which model was hit, and so which cell size.
 *   - World span of an instance whose model box is [lo, hi) on the local axis that maps to world axis a, with o = offset[a]:
 *     [o + lo * 2^e, o + hi * 2^e), or [o - hi * 2^e, o - lo * 2^e) when flipped.  The lattice limit below, the screen bins and the
 *     BVH's leaf boxes use it.
 *   - Limit: vm <= 256, checked where a table is checked (host tables: BLOK_ERR_INVALID_ARG naming the instance; device tables: skipped).
 *   - Composition, the tie rule, the any-hit shadow rule and the BVH's ordering rule are unchanged, and so is the object-motion map
 *     (it does not contain the scale).
 *   Not built: negative exponents (a model traced at any real scale, turned or sheared, is a blok_pose, "Posed models" below, since ABI
 *   1.22, and in the path-traced frame since ABI 1.23).  (A scaled model is baked into the resident volume by blok_hip_volume_stamp_affine, since ABI 1.18:
 *   blok_affine_from_instance, blok_world.h, folds a placement and the exponent into its record; the other volume entries refuse one, below.)
 * Instance ids.  Each pixel or ray gets the index of the winning instance, or BLOK_INSTANCE_NONE for the world or a miss.
 * Scope.  The primary frame, explicit rays and the path-traced frame (blok_hip_trace_paths_instanced*, blok_hip_draw_frame_rt_instanced
 *   below); the sun map, blok_hip_draw_frame_accumulate and the tile and multi-GPU entries stay world-only (they never receive an
 *   instance table); an instance that has stopped moving can be baked into the resident volume (blok_hip_volume_stamp_models below). */
typedef struct blok_instance {
    uint32_t model;
    int32_t  offset[3];   /* voxels, world lattice */
    uint8_t  axis[3];     /* local axis k is world axis axis[k] */
    uint8_t  flip;        /* bit k: local axis k runs against world axis axis[k] */
    uint32_t reserved[3]; /* zero */
} blok_instance;
#define BLOK_INSTANCE_NONE 0xFFFFFFFFu

/* Builds a model from n voxels (xyz[3*i..], local lattice; duplicates: the last one wins) and
 * uploads it (every listed voxel is filled); *out_model is its id (ids are never reused).  Both calls may synchronise the device. */
int blok_hip_model_create(blok_hip_ctx* ctx, const int32_t* xyz, const uint32_t* material_ids, size_t n, uint32_t* out_model);
int blok_hip_model_destroy(blok_hip_ctx* ctx, uint32_t model);
/* The model's scale exponent ("Scaled models" above).  Every entry that makes a model (blok_hip_model_create, the volume's capture_model,
 * capture_component and lod_model) makes one of scale 0.  set_scale blocks, may synchronise the device and updates the device model
 * store.  BLOK_ERR_INVALID_ARG: an unknown or destroyed model, scale_log2 > 8, a NULL output.  set_scale also empties the previous-frame
 * table that the context keeps for blok_hip_draw_frame_rt_instanced_motion, as blok_hip_post_reset does: the next frame treats its
 * instances as untracked, because the object-motion map is wrong across a change of scale.  Callers of the *_device motion entries
 * (blok_hip_instance_motion_device, blok_hip_denoise_instanced*_device) hold both tables themselves and own that rule themselves.
 * Volume entries that take a placement or a model id (blok_hip_volume_stamp_models, blok_hip_volume_sweep_models, the entries of
 * blok_hip_volume_scatter_models) return BLOK_ERR_UNSUPPORTED for a live model whose scale is not 0; nothing is touched.  The one volume
 * entry that takes a model of any exponent is blok_hip_volume_stamp_affine: it ignores the exponent, its matrix carries all scale. */
int blok_hip_model_set_scale(blok_hip_ctx* ctx, uint32_t model, uint32_t scale_log2);
int blok_hip_model_scale(blok_hip_ctx* ctx, uint32_t model, uint32_t* out_scale_log2);

/* ---- emissive models as lights (ABI 1.28) ----
 * The light table above ("emissive voxels as lights") holds faces of the WORLD.  A model can carry a table of its own, in its own cells,
 * so that a lattice instance of it (blok_instance) is a light wherever it is placed and however often it moves, with nothing rebuilt.
 * While some live model has a table, every path-traced entry that brings a lattice instance table with n > 0 (blok_hip_trace_paths_instanced*,
 * blok_hip_trace_paths_posed*, the blok_hip_draw_frame_rt_instanced* and _posed* chain) samples world and instance faces in one pick and
 * counts a lit instance's emission once (DESIGN.md §33 has the rule); with or without a world table.  With no model table, or no instance
 * table, every entry runs the kernel it ran before, bit for bit.  Poses are no part of this (their areas are real): they count by hits.
 *  - blok_hip_model_lights builds, on the device and from the model's own tree, the table of the model's exposed emissive UNIT faces:
 *    a filled model voxel whose material index (min(id, 65535), then 0 when beyond the material table) is emissive in the context's CURRENT
 *    material table contributes face f iff the model's neighbouring cell in that direction is empty.  The world and other instances play no
 *    part.  One blok_light per face: du = dv = 1, cum = the record's index, lo in the model's local lattice with the plane coordinate as in
 *    blok_quad (+1 for faces 0, 2, 4), material the voxel's id, face as in blok_quad.  Order: the model's material array (bricks in the
 *    tree's order, cells in ascending bit order x | y << 2 | z << 4), face 0..5 within a voxel.  flags must be 0.  A result of no faces
 *    installs no table (an earlier one of that model goes).  Bit-identical to blok_model_lights (blok_world.h) for the model
 *    blok_hip_model_create makes of the same list.  Blocking.  Errors, each leaving the model's previous table in place:
 *    BLOK_ERR_INVALID_ARG for an unknown or destroyed model, without a material table, for flags != 0; BLOK_ERR_OOM.
 *  - blok_hip_model_lights_info: n = n_faces = the records, bytes, area_world = 0 (a model has no place), n_owned = 0; zeros without a
 *    table.  blok_hip_model_lights_download copies records [first, first + count) in pieces as the other downloads do;
 *    blok_hip_model_lights_clear drops the model's table.  All three: BLOK_ERR_INVALID_ARG for an unknown or destroyed model.
 *  - Life: a table is freed by blok_hip_model_destroy and kept by blok_hip_model_set_scale (the records are in model cells).  ALL model
 *    tables are dropped by every call that installs another world or material table, the calls that clear the world's light table: a
 *    table is a statement about which ids glow.
 *  - The record of an instance's face (blok_instance_light_record, blok_world.h): for model cell c and scale exponent e the cell's lowest
 *    world voxel on world axis axis[k] is offset + c_k * 2^e, or offset - (c_k + 1) * 2^e when flip bit k is set; the world face is
 *    2 * axis[k] + (n XOR flip_k); the plane coordinate is that low voxel for a - face and low + 2^e for a + face; du = dv = 2^e; material
 *    unchanged; cum 0.  64-bit integer work; one model face is exactly 4^e world unit faces.
 *  - The prefix of an instance table: faces_i = n(model_i) << 2e if instance i is usable (the kernels' rule: well formed, a live model of a
 *    usable voxel size, world box inside the int16 lattice) and its model has a table, else 0; icum is the exclusive scan, n + 1 words, and
 *    icum[i + 1] != icum[i] says "instance i is lit".  With A_world the faces of the installed world table (0 without one), A_inst the sum
 *    and A_total = A_world + A_inst: if A_total >= 2^32 instance lights are DISABLED for that table — every faces_i is 0, A_inst = 0,
 *    A_total = A_world, disabled = 1 — and nothing fails.  area_world = (float(A_total) * vs) * vs.  The extended pick is
 *    pick = (r * A_total) >> 32: below A_world the world's light; else p = pick - A_world, the instance the last i with icum[i] <= p,
 *    off = p - icum[i], the model's record table[off >> 2e], the cell off & (4^e - 1) of its world rectangle.
 *  - blok_hip_instance_lights_info runs the prefix kernel over a host table (the records are not checked: unusable ones count 0) and
 *    returns the header, and the n + 1 words where out_icum_host is not NULL.  Blocking.  BLOK_ERR_INVALID_ARG: a NULL table with n > 0, a
 *    NULL out. */
typedef struct blok_instance_lights_info {
    uint64_t a_inst;     /* A_inst: world unit faces of the lit instances */
    uint64_t a_total;    /* A_world + A_inst */
    float    area_world; /* (float(A_total) * vs) * vs */
    uint32_t n_lit;      /* instances with faces_i > 0 */
    uint32_t disabled;   /* 1: A_world + the instances' faces reached 2^32, the table carries no light */
    uint32_t reserved;   /* 0 */
} blok_instance_lights_info;
int blok_hip_model_lights(blok_hip_ctx* ctx, uint32_t model, uint32_t flags, blok_lights_info* out_info);
int blok_hip_model_lights_info(blok_hip_ctx* ctx, uint32_t model, blok_lights_info* out_info);
int blok_hip_model_lights_download(blok_hip_ctx* ctx, uint32_t model, blok_light* out_host, uint64_t first, uint64_t count);
int blok_hip_model_lights_clear(blok_hip_ctx* ctx, uint32_t model);
int blok_hip_instance_lights_info(blok_hip_ctx* ctx, const blok_instance* instances_host, uint32_t n, blok_instance_lights_info* out,
                                  uint32_t* out_icum_host);
/* BLOK_OK if every instance of a host table passes the limits above, else BLOK_ERR_INVALID_ARG naming the first that does not. */
int blok_hip_check_instances(blok_hip_ctx* ctx, const blok_instance* instances_host, uint32_t n_instances);

/* The primary frame of blok_hip_trace_primary_device composed with instances.  The world pass is that entry's launch, unchanged; then,
 * on the same stream and only if n_instances > 0, a binning kernel (instances per 32x32-pixel bin of the rectangle) and a kernel that
 * walks each pixel's candidate instances.  instances_dev: n_instances records in device memory, read in stream order (a caller may
 * change the table every frame without a host synchronise).  Outputs as blok_hip_trace_primary_device plus out_instance_dev (w*h
 * uint32): any may be NULL, not all.  After the first call at a given size the call allocates nothing and does not synchronise. */
int blok_hip_trace_primary_instanced_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                            const blok_instance* instances_dev, uint32_t n_instances,
                                            void* out_hits_dev, void* out_rgba_dev, uint32_t* out_instance_dev, void* hip_stream);
/* Blocking form with host arrays (the table is checked first); any output may be NULL, not all. */
int blok_hip_trace_primary_instanced(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                     const blok_instance* instances_host, uint32_t n_instances,
                                     blok_hit* out_hits_host, uint32_t* out_rgba_host, uint32_t* out_instance_host);
/* Explicit rays against world plus instances (picking, line of sight, secondary rays): n rays in, n records and/or n instance ids out. */
int blok_hip_trace_rays_instanced(blok_hip_ctx* ctx, const blok_ray* rays_host, size_t n, const blok_instance* instances_host,
                                  uint32_t n_instances, blok_hit* out_hits_host, uint32_t* out_instance_host);
int blok_hip_trace_rays_instanced_device(blok_hip_ctx* ctx, const blok_ray* rays_dev, size_t n, const blok_instance* instances_dev,
                                         uint32_t n_instances, blok_hit* out_hits_dev, uint32_t* out_instance_dev, void* hip_stream);

/* ------------------------------------------------------------- posed models (ABI 1.22)
 * A blok_pose places a model under ANY affine map: a rotation by any angle, a real scale, a mirror, a shear.  It is traced, not baked
 * (blok_hip_volume_stamp_affine bakes); a lattice instance (blok_instance above) stays the cheaper record where it is enough.
 *
 * Pose.  blok_pose below, 64 bytes: the model, the map m from WORLD to LOCAL space (row k gives local axis k), a world point `pivot` and
 *   the local point `local` it lands on.  All lengths are world units (not voxels): one model voxel is vm = vs * 2^e wide in local space,
 *   e the model's scale exponent ("Scaled models" above).
 * Ray into local space.  Every operation rounded separately to float, nothing fused, in this order:
 *     r_j  = fl(o_j - pivot_j)
 *     o'_k = fl( fl( fl( fl(m_k0 r_0) + fl(m_k1 r_1) ) + fl(m_k2 r_2) ) + local_k )
 *     d'_k = fl( fl( fl(m_k0 d_0) + fl(m_k1 d_1) ) + fl(m_k2 d_2) )
 *   tmin and tmax unchanged.  The direction is NOT renormalised: an affine map of the ray keeps its parameter, so t means the same in the
 *   world, in a lattice instance and in a pose, and "strictly smaller t" composes them.  (The canonical walk of DESIGN.md §3 puts no
 *   condition on the length of d.)  A ray whose o' or d' has a component that is not finite does not enter that pose.
 * Walk.  The canonical walk over the model's tree at the model's own voxel size vm, exactly as for a lattice instance.
 * Record.  t and material_id unchanged, hit = 1.  voxel is the MODEL'S LOCAL voxel (a turned cell has no world voxel) and face the LOCAL
 *   face code 2k + n (n = 0: the face whose outward normal is +local axis k, n = 1: -local axis k, as in every record).  World normal:
 *   normals transform by the transpose of the world -> local map, so the outward world normal of local face 2k + n is parallel to
 *   s * (m_k0, m_k1, m_k2), s = +1 for n = 0 and -1 for n = 1 (normalise it; under a singular m it may be zero).
 * RGBA of the primary frame.  Shading needs one of the six world faces: of the vector s * (m_k0, m_k1, m_k2) the component of largest
 *   magnitude (ties: the lowest axis) names the axis a, and the shade face is 2a if that component is >= 0 (or -0), 2a + 1 if it is < 0.
 *   The record keeps the local face.
 * Composition.  Candidates in the order: the world, instances 0 .. n-1, poses 0 .. p-1; a candidate replaces the record only with a
 *   strictly smaller t (each walks with tmax = the best t so far).  Ties go to the world, then the lattice instances, then the lowest pose.
 * Ids.  out_instance = BLOK_POSE_ID | index for a pixel / ray that a pose wins; the instance index or BLOK_INSTANCE_NONE otherwise.
 * Limits.  All 15 floats finite; |m_kj| <= 1024, |pivot_j| <= 2^20, |local_k| <= 2^20; the model exists and its voxel size vm <= 256;
 *   the model's own voxel box lies in [-32768, 32768) (the record's voxel is int16).  At most 2^31 - 1 poses.  A singular m is legal: the
 *   rule needs no inverse.  Host tables fail with BLOK_ERR_INVALID_ARG naming the first pose that breaks a limit (blok_hip_check_poses does
 *   this check alone); the kernels of the device-table entries skip such a pose.
 * Scope.  The primary frame, explicit rays and, since ABI 1.23, the path-traced frame (blok_hip_trace_paths_posed*,
 *   blok_hip_draw_frame_rt_posed, below).  Object motion, the sun map, blok_hip_draw_frame_accumulate and the tile and multi-GPU entries stay
 *   as they are and never receive a pose table.  A posed model that has stopped can be baked about where it was seen: blok_affine_from_pose
 *   (blok_world.h). */
typedef struct blok_pose {     /* 64 bytes */
    uint32_t model;
    float    m[3][3];          /* world -> local: row k gives local axis k */
    float    pivot[3];         /* a world point (world units, not voxels) */
    float    local[3];         /* where the pivot lies in local space (world units: one model voxel is vm = vs * 2^e wide) */
} blok_pose;
#define BLOK_POSE_ID 0x80000000u   /* out_instance = BLOK_POSE_ID | index for a pixel / ray a pose wins */

/* BLOK_OK if every pose of a host table passes the limits above, else BLOK_ERR_INVALID_ARG naming the first that does not. */
int blok_hip_check_poses(blok_hip_ctx* ctx, const blok_pose* poses_host, uint32_t n_poses);
/* blok_hip_trace_primary_instanced_device, then, on the same stream and only if n_poses > 0, a binning kernel (poses per 32x32-pixel bin:
 * the bounding box of each pose's preimage in the world, widened by an argued margin) and a kernel that walks each pixel's
 * candidate poses and composes in place.  The frame is DEFINED as if every pose were tested for every pixel.  Either table may be empty;
 * with n_poses == 0 the outputs are byte for byte those of blok_hip_trace_primary_instanced_device.  Both tables are read in stream
 * order.  Outputs: any may be NULL, not all.  After the first call at a given size the call allocates nothing and does not synchronise. */
int blok_hip_trace_primary_posed_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                        const blok_instance* instances_dev, uint32_t n_instances, const blok_pose* poses_dev, uint32_t n_poses,
                                        void* out_hits_dev, void* out_rgba_dev, uint32_t* out_instance_dev, void* hip_stream);
/* Blocking form with host arrays (both tables are checked first). */
int blok_hip_trace_primary_posed(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                 const blok_instance* instances_host, uint32_t n_instances, const blok_pose* poses_host, uint32_t n_poses,
                                 blok_hit* out_hits_host, uint32_t* out_rgba_host, uint32_t* out_instance_host);
/* Explicit rays against the world, the instances and the poses: every pose is tested for every ray. */
int blok_hip_trace_rays_posed(blok_hip_ctx* ctx, const blok_ray* rays_host, size_t n, const blok_instance* instances_host, uint32_t n_instances,
                              const blok_pose* poses_host, uint32_t n_poses, blok_hit* out_hits_host, uint32_t* out_instance_host);
int blok_hip_trace_rays_posed_device(blok_hip_ctx* ctx, const blok_ray* rays_dev, size_t n, const blok_instance* instances_dev, uint32_t n_instances,
                                     const blok_pose* poses_dev, uint32_t n_poses, blok_hit* out_hits_dev, uint32_t* out_instance_dev,
                                     void* hip_stream);

/* Path-traced frames with instances: blok_hip_trace_paths* with every ray of the path loop composed with the instances by the rule above.
 *   Primary and bounce rays: the closest hit of world and instances.  Shadow rays: any hit; the instances are asked only when the world
 *   walk found nothing, and over the shadow ray's whole interval (the sun map caps the world walk alone).  The G-buffer is the composed
 *   first hit (sample 0, bounce 0); out_instance (w*h uint32, may be NULL) holds that hit's instance or BLOK_INSTANCE_NONE.
 * Each launch first builds a BVH over the table on the stream (one workgroup; up to 4096 instances, above that every ray loops over the
 *   table — slower, same result), so the table may change every frame without a host synchronise.  Off for such launches: the bounce
 *   rounds' tail pool (ray batching mode 3 behaves as mode 2) and blok_hip_set_path_start's resume.  The motion plane of these entries
 *   stays camera-only, and so does blok_hip_draw_frame_rt_instanced: an instance that moves between frames gets no object motion there,
 *   so the denoiser and TAA may ghost behind it.  Object motion comes from the entries of the next block.
 * n_instances == 0 is blok_hip_trace_paths*'s launch, unchanged, plus out_instance filled with BLOK_INSTANCE_NONE.  Device entries skip
 *   instances that fail the limits; the host entries check the table first. */
int blok_hip_trace_paths_instanced_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                          uint32_t spp, uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev,
                                          uint32_t n_instances, const blok_gbuffer* planes_dev, uint32_t* out_instance_dev, void* hip_stream);
int blok_hip_trace_paths_instanced_ref_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                              uint32_t spp, uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev,
                                              uint32_t n_instances, const float prev_view_proj[16], const blok_gbuffer_ref* planes_dev,
                                              uint32_t* out_instance_dev, void* hip_stream);
/* Blocking form with host planes and a host table (checked first). */
int blok_hip_trace_paths_instanced(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                                   uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_host, uint32_t n_instances,
                                   const blok_gbuffer* planes_host, uint32_t* out_instance_host);
/* blok_hip_draw_frame_rt with the path pass above (host table, checked first): the same post state and frame counter. */
int blok_hip_draw_frame_rt_instanced(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                                     const blok_denoise_settings* settings, const blok_instance* instances_host, uint32_t n_instances,
                                     uint32_t* out_rgba8_host, uint32_t* out_frame_count);

/* Path-traced frames with poses (ABI 1.23): the entries above with a pose table behind the instances.
 * Order.  Every ray of the path loop is composed in the order of "Posed models": the world, instances 0 .. n-1, poses 0 .. p-1.  A candidate
 *   replaces the record only with a strictly smaller t; ties go to the world, then the instances, then the lowest pose.  A pose's ray goes
 *   over by the rule of "Ray into local space", unchanged, and its walk is the model's own canonical walk, unchanged.
 * Primary and bounce rays.  The closest hit of all three; the poses are asked with tmax = the best t so far.
 * Shadow rays.  Any hit.  The instances are asked only if the world walk found nothing, and the poses only if the instances found nothing;
 *   both on the uncapped interval [0.001, 1000) (the sun map caps the world walk alone).
 * The normal of a posed hit.  Local face 2k + n of pose P, s = +1 for n = 0 and -1 for n = 1, every operation rounded separately to float:
 *     v_j = s * m_kj          q = fl(fl(fl(v_0 v_0) + fl(v_1 v_1)) + fl(v_2 v_2))
 *   If !(q > 0) (a zero row of a singular m, or underflow) the normal is the axis normal of the shade face of "RGBA of the primary frame".
 *   Otherwise len = sqrt(q) correctly rounded and n_j = fl(v_j / len) + 0.0f (every zero is +0, as in an axis normal).  Then the path
 *   loop's own statements on n: the flip against the ray, the G-buffer, the shadow ray's origin hit_pos + n * 0.001, n.l.  For a pose
 *   made by blok_pose_from_instance (also of a model under blok_hip_model_set_scale) this is the lattice instance's axis normal bit for
 *   bit, and the whole frame is that of the same placements given as instances.
 * The sampling frame.  tangent = normalize(cross(up, n)), bitangent = cross(n, tangent) for every hit of such a launch (for an axis normal
 *   the division is by 1: world and instance hits keep their values).
 * G-buffer.  The composed first hit (sample 0, bounce 0); world_pos = o + t d; normal_roughness holds the normal above; out_instance holds
 *   BLOK_POSE_ID | index where a pose wins, the instance index or BLOK_INSTANCE_NONE otherwise.  The motion plane of these entries stays
 *   camera-only on pose pixels, so under them a moving pose may ghost in the denoiser and TAA; object motion for poses comes from the
 *   entries of "Object motion for posed models" below (since ABI 1.25).
 * The frame is DEFINED as if every pose were tested for every ray.  Each launch first builds a second BVH, over the poses, on the stream (one
 *   workgroup; up to 4096 poses, above that every ray loops over the table; leaf boxes argued in pose_tlas_core.h; a table with a usable
 *   pose whose box has no bound — a near-singular m — loops too): slower, the same result.  blok_hip_debug.h: blok_hip_set_pose_tlas.
 * Empty tables.  With n_poses == 0 each entry is the instanced entry of the same name: the same launches, the same bytes.  With
 *   n_instances == 0 and poses present the posed kernel runs with no instance tree.
 * Errors as the instanced entries', in their order; a bad pose of a host table is named as blok_hip_check_poses names it, outputs untouched.
 *   Device tables skip what the host entries refuse.  Both tables are read in stream order; after the first call at a given size the
 *   device entries allocate nothing and do not synchronise.
 * blok_hip_draw_frame_rt_posed: blok_hip_draw_frame_rt_instanced's chain over this path pass (host tables, both checked first): the same
 *   post state and frame counter, camera-only motion; like that entry it empties the previous table of
 *   blok_hip_draw_frame_rt_instanced_motion. */
int blok_hip_trace_paths_posed_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                                      uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev, uint32_t n_instances,
                                      const blok_pose* poses_dev, uint32_t n_poses, const blok_gbuffer* planes_dev, uint32_t* out_instance_dev,
                                      void* hip_stream);
int blok_hip_trace_paths_posed_ref_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                                          uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev, uint32_t n_instances,
                                          const blok_pose* poses_dev, uint32_t n_poses, const float prev_view_proj[16],
                                          const blok_gbuffer_ref* planes_dev, uint32_t* out_instance_dev, void* hip_stream);
int blok_hip_trace_paths_posed(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                               uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_host, uint32_t n_instances,
                               const blok_pose* poses_host, uint32_t n_poses, const blok_gbuffer* planes_host, uint32_t* out_instance_host);
int blok_hip_draw_frame_rt_posed(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces, const blok_denoise_settings* settings,
                                 const blok_instance* instances_host, uint32_t n_instances, const blok_pose* poses_host, uint32_t n_poses,
                                 uint32_t* out_rgba8_host, uint32_t* out_frame_count);

/* Object motion for moving instances (ABI 1.3).
 * Tracking.  Instance i of this frame's table `cur` is tracked when i < n_prev, prev[i].model == cur[i].model and both records pass the
 *   limits above with that model; otherwise it is untracked (it appeared this frame or changed model).
 * The map.  A first-hit point p (world_pos plane) on a tracked instance was, one frame earlier, at p_prev with normal n_prev: for each local
 *   axis k, with a = cur.axis[k], b = prev.axis[k] and c = s * s' (the signs of cur's and prev's flip bit k),
 *     p_prev[b] = fl(c * p[a] + float(prev.offset[b] - c * cur.offset[a]) * voxel_size)      n_prev[b] = c * n[a]
 *   (one rounding per axis; equal offset, axis and flip: p_prev = p and n_prev = n with no arithmetic, so a stationary instance gets
 *   exactly the camera-only motion).  Object motion = (px + 0.5) / width - uv of prev_view_proj * (p_prev, 1), and the same in y: the
 *   operations of the path kernel's motion plane.
 * blok_hip_instance_motion_device: the pixels of a rectangle whose first hit is a tracked instance get their object motion, in motion_h_dev
 *   (RG16F, binary16 round to nearest even) and/or motion_dev (float2); it runs after blok_hip_trace_paths_instanced_ref_device to correct
 *   that entry's motion plane.  Every other pixel (world, sky, untracked instance) is left untouched.  Planes and the id plane are w*h,
 *   the rectangle's own; cur_dev / prev_dev are device tables read in stream order.
 * blok_hip_denoise_instanced_device / _ref_device: blok_hip_denoise_device / _ref_device with the frame's id plane (width*height) and both
 *   tables; the same post state and frame counter.  World pixels are denoised exactly as before.  A tracked instance's pixel: without a
 *   motion plane its motion is the object motion; its history is compared at p_prev / n_prev in place of the pixel's position and normal
 *   (the small-motion reprojection, the position and the normal tests).  An untracked instance's pixel uses no history (length 1).
 * blok_hip_draw_frame_rt_instanced_motion: blok_hip_draw_frame_rt_instanced with object motion: path pass (with an id plane), motion
 *   correction, the instanced temporal pass, then the rest of the chain unchanged.  The context keeps the previous frame's table; it is
 *   empty after blok_hip_post_reset and after a frame drawn by blok_hip_draw_frame_rt or blok_hip_draw_frame_rt_instanced.  With no
 *   instances the frame is blok_hip_draw_frame_rt's.
 * Errors: BLOK_ERR_INVALID_ARG for a null id plane, a null table with a non-zero count, no motion output, a rectangle outside the frame or
 *   no prev_view_proj; host tables are checked like the other host entries; device entries treat records that fail the limits as untracked. */
int blok_hip_instance_motion_device(blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* world_pos_dev,
                                    const uint32_t* instance_ids_dev, const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev,
                                    uint32_t n_prev, const float prev_view_proj[16], uint16_t* motion_h_dev, float* motion_dev, void* hip_stream);
int blok_hip_denoise_instanced_device(blok_hip_ctx* ctx, const blok_gbuffer* planes_dev, const float* motion_dev, const float prev_view_proj[16],
                                      uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* instance_ids_dev,
                                      const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                      float* out_color_dev, void* hip_stream);
int blok_hip_denoise_instanced_ref_device(blok_hip_ctx* ctx, const blok_gbuffer_ref* planes_dev, const float prev_view_proj[16],
                                          uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* instance_ids_dev,
                                          const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                          float* out_color_dev, void* hip_stream);
int blok_hip_draw_frame_rt_instanced_motion(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                                            const blok_denoise_settings* settings, const blok_instance* instances_host, uint32_t n_instances,
                                            uint32_t* out_rgba8_host, uint32_t* out_frame_count);

/* Object motion for posed models (ABI 1.25): what the block above is for lattice instances, for poses.
 * Tracking.  Pose i of this frame's table `cur` is tracked when i < n_prev, prev[i].model == cur[i].model, both records pass the limits of
 *   "Posed models" with that model, and either the two 64-byte records are byte-equal (state 1 below, which needs no inverse), or prev[i].m
 *   is invertible by the test below and every float of the motion record comes out finite (state 2).  Otherwise the pose is untracked: it
 *   appeared, changed model, or was singular one frame ago.  cur[i].m may be singular: it is only applied forward.  A change of a model's
 *   scale exponent changes what a pose's local space means: blok_hip_model_set_scale empties the context's previous pose table, as it
 *   empties the instance one, and callers of the *_device entries keep that rule themselves.
 * The motion record.  blok_pose_motion below, 128 bytes, one per pose, computed once per launch (not per pixel): state (0 untracked,
 *   1 identity, 2 moving), a, c, n and the two pivots; in states 0 and 1 every other word is zero.
 *   State 1: the two pose records are byte-equal (-0.0 against +0.0 is not).  Then p_prev = p and n_prev = n with no arithmetic, so an unmoved
 *   pose gets exactly the camera-only motion, as an unmoved instance does.
 *   State 2, in DOUBLE, every operation rounded separately in this order, nothing fused, no square root (m = prev.m, M = cur.m):
 *     C = adj(m):  C00 = m11 m22 - m12 m21   C01 = m02 m21 - m01 m22   C02 = m01 m12 - m02 m11
 *                  C10 = m12 m20 - m10 m22   C11 = m00 m22 - m02 m20   C12 = m02 m10 - m00 m12
 *                  C20 = m10 m21 - m11 m20   C21 = m01 m20 - m00 m21   C22 = m00 m11 - m01 m10
 *     det = (m00 C00 + m01 C10) + m02 C20          s_k = (m_k0^2 + m_k1^2) + m_k2^2
 *     invertible iff det det > 2^-40 ((s_0 s_1) s_2)      (the floor of the screen bins' pose_world_box, squared so that no root is needed)
 *     id = 1.0 / det      inv_jk = C_jk id      A_ij = (inv_i0 M_0j + inv_i1 M_1j) + inv_i2 M_2j
 *     dl = double(cur.local) - double(prev.local)      c_i = (inv_i0 dl_0 + inv_i1 dl_1) + inv_i2 dl_2
 *     n = the cofactor matrix of the double A (n_ij = adj(A)_ji, adj and det(A) by the formulas above), every entry negated when det(A) < 0
 *   (normals go over by A^-T = cof(A) / det(A); the per-pixel normalisation removes the magnitude, the cofactor form needs no second inverse
 *   and is defined for a singular cur).  Each value is rounded to float once; pivot_cur = cur.pivot, pivot_prev = prev.pivot.
 * The per-pixel map.  A first-hit point p (world_pos plane) with unit normal n on a pose in state 2, all operations float, rounded
 *   separately, in the manner of "Ray into local space":
 *     r_j      = fl(p_j - pivot_cur_j)
 *     q_i      = fl( fl( fl( fl(a_i0 r_0) + fl(a_i1 r_1) ) + fl(a_i2 r_2) ) + c_i )
 *     p_prev_i = fl(pivot_prev_i + q_i)
 *     v_i      = fl( fl( fl(n_i0 n_0) + fl(n_i1 n_1) ) + fl(n_i2 n_2) )
 *     qq       = fl( fl( fl(v_0 v_0) + fl(v_1 v_1) ) + fl(v_2 v_2) )
 *     n_prev   = !(qq > 0) ? n : fl(v_i / sqrt(qq))            (sqrt correctly rounded)
 *   Working from the pivots keeps r small for a model far from the origin.  Object motion = (px + 0.5) / width - uv of
 *   prev_view_proj * (p_prev, 1), and the same in y: the operations of blok_hip_instance_motion_device.
 * Ids.  The id plane of the posed path entries: BLOK_POSE_ID | index selects a pose, any other id but BLOK_INSTANCE_NONE an instance, which
 *   is handled by the rule of the block above, unchanged: a frame that holds both kinds runs one pass.
 * blok_hip_posed_motion_device: blok_hip_instance_motion_device for both kinds; it corrects the motion plane of
 *   blok_hip_trace_paths_posed_ref_device.  Pixels of tracked instances and tracked poses get their object motion (a pose in state 1: the
 *   camera-only motion recomputed); world, sky and untracked pixels are left untouched.
 * blok_hip_denoise_posed_device / _ref_device: the instanced denoise entries plus both pose tables: the same post state and frame
 *   counter.  A tracked pose pixel uses p_prev / n_prev exactly where a tracked instance pixel does; an untracked pose pixel takes no
 *   history (length 1); world and instance pixels run the existing statements.
 * All three first run a kernel that builds the records (one lane per pose) into the stream's scratch: no host synchronise, nothing
 *   allocated after the first call at a size.  All four tables are read in stream order.
 * blok_hip_draw_frame_rt_posed_motion: blok_hip_draw_frame_rt_posed's chain with the id plane written, the records built once, then the
 *   motion pass, then the posed temporal pass.  The context keeps the previous frame's instance table AND pose table; both are emptied by
 *   blok_hip_post_reset, by blok_hip_model_set_scale and by a frame of any other blok_hip_draw_frame_rt* entry.  With n_poses == 0 it is
 *   blok_hip_draw_frame_rt_instanced_motion's frame.
 * blok_pose_motion_record (blok_world.h) builds one record on the host, bit for bit; blok_hip_debug_pose_motion_records (blok_hip_debug.h)
 *   reads the kernel's back.
 * Errors as the instanced motion entries', in their order and texts (a null pose table with a non-zero count comes right after the instance
 *   tables); a bad pose of a host table is named as blok_hip_check_poses names it, outputs untouched; device tables treat what fails as
 *   untracked.
 * Not built: a history plane of ids; motion for the accumulate, tile and multi-GPU entries; non-rigid tracking beyond the index rule. */
typedef struct blok_pose_motion {   /* 128 bytes */
    uint32_t state;                 /* 0 untracked, 1 identity, 2 moving */
    float    a[3][3];
    float    c[3];
    float    n[3][3];
    float    pivot_cur[3];
    float    pivot_prev[3];
    uint32_t reserved[4];           /* zero */
} blok_pose_motion;
int blok_hip_posed_motion_device(blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* world_pos_dev,
                                 const uint32_t* ids_dev, const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                 const blok_pose* cur_poses_dev, uint32_t n_cur_poses, const blok_pose* prev_poses_dev, uint32_t n_prev_poses,
                                 const float prev_view_proj[16], uint16_t* motion_h_dev, float* motion_dev, void* hip_stream);
int blok_hip_denoise_posed_device(blok_hip_ctx* ctx, const blok_gbuffer* planes_dev, const float* motion_dev, const float prev_view_proj[16],
                                  uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* ids_dev,
                                  const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                  const blok_pose* cur_poses_dev, uint32_t n_cur_poses, const blok_pose* prev_poses_dev, uint32_t n_prev_poses,
                                  float* out_color_dev, void* hip_stream);
int blok_hip_denoise_posed_ref_device(blok_hip_ctx* ctx, const blok_gbuffer_ref* planes_dev, const float prev_view_proj[16],
                                      uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* ids_dev,
                                      const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                      const blok_pose* cur_poses_dev, uint32_t n_cur_poses, const blok_pose* prev_poses_dev, uint32_t n_prev_poses,
                                      float* out_color_dev, void* hip_stream);
int blok_hip_draw_frame_rt_posed_motion(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                                        const blok_denoise_settings* settings, const blok_instance* instances_host, uint32_t n_instances,
                                        const blok_pose* poses_host, uint32_t n_poses, uint32_t* out_rgba8_host, uint32_t* out_frame_count);

/* ------------------------------------------------------------- models into the resident volume and back (ABI 1.7)
 * The two stores of voxel data in HBM — the resident volume and the instanced models — joined on the device.  Integer arithmetic only: one
 * right answer, bit-identical on the host (blok_stamp_voxels / blok_capture_voxels, blok_world.h) and on the device.  Both calls block.
 *
 * blok_hip_volume_stamp_models writes placed models into the volume.  The model is read where it lives (its tree), never as a voxel list.
 *  - Placement: a blok_instance.  A filled model voxel v' (local lattice, the coordinates given to blok_hip_model_create) lands on the world
 *    voxel of "Record back to world space" above: w[axis[k]] = offset[axis[k]] + v'_k, or offset[axis[k]] - 1 - v'_k when flip bit k is set.
 *    A baked instance therefore lies exactly where the traced one was seen.  The sums are 64-bit before clipping.
 *  - Written set: the mapped filled voxels inside the volume's box; voxels outside are clipped silently, a placement wholly outside writes
 *    nothing.  BLOK_STAMP_SET: density[w] = density, ids[w] = the model voxel's material.  BLOK_STAMP_KEEP: the same, only where the
 *    volume's voxel is empty (density > 0 is false: 0, negative and NaN are empty).  BLOK_STAMP_ERASE: density[w] = 0.0f, ids[w] = 0 (the
 *    density argument is ignored).  Empty model cells never touch the volume.
 *  - Order: the result equals n_placements successive calls in table order (a later placement wins over an earlier one).
 *  - out_n_voxels (may be NULL): voxels written, summed over the placements; for KEEP the voxels that were empty and got filled.
 *  - Afterwards masks, occupancy words and dirty flags are those blok_hip_volume_set_voxels leaves for the same writes, refreshed over each
 *    placement's clipped box (never over their union); the next blok_hip_volume_rebuild installs the world.
 *  - Errors, nothing written.  BLOK_ERR_INVALID_ARG: a placement that fails what blok_hip_check_instances checks (same messages), an
 *    unknown mode, for SET and KEEP a density that is not finite or <= 0, a null table with a non-zero count.  BLOK_ERR_NO_WORLD: no
 *    volume.  BLOK_ERR_UNSUPPORTED: a volume above 2^32 cells.  n_placements == 0 is BLOK_OK.
 *
 * blok_hip_volume_capture_model makes a region of the volume a model, without downloading it.
 *  - Region: world voxels, half open; both pointers NULL = the whole box (the convention of blok_hip_volume_extract_quads).
 *  - The new model is exactly the one blok_hip_model_create builds from the list {(w - region_lo, ids[w]) : w in region, density[w] > 0}
 *    (with NULL pointers region_lo is the box's origin): the same node and material arrays byte for byte, the same levels, origin and box.
 *    A filled voxel with material id 0 is a filled voxel.  *out_model is the next model id.
 *  - out_n_voxels (may be NULL): the model's voxels.
 *  - BLOK_CAPTURE_CUT: after the model exists the captured voxels are cleared in the volume (density 0, id 0) and the masks refreshed.  If
 *    the model cannot be built, nothing is cut.
 *  - Errors.  BLOK_ERR_INVALID_ARG: exactly one region pointer NULL, lo > hi on an axis, unknown flag bits, out_model NULL.
 *    BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume above 2^32 cells, or a region that holds no filled voxel (then no model
 *    is created, no id consumed, *out_n_voxels = 0).  BLOK_ERR_NO_WORLD: no volume. */
#define BLOK_STAMP_SET   0   /* write every filled model voxel */
#define BLOK_STAMP_KEEP  1   /* ... only where the volume is empty */
#define BLOK_STAMP_ERASE 2   /* clear the volume where the model is filled */
int blok_hip_volume_stamp_models(blok_hip_ctx* ctx, const blok_instance* placements_host, uint32_t n_placements,
                                 int mode, float density, uint64_t* out_n_voxels);
#define BLOK_CAPTURE_CUT 1u   /* afterwards clear the captured voxels in the volume (density 0, id 0) */
int blok_hip_volume_capture_model(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                                  uint32_t* out_model, uint64_t* out_n_voxels);

/* ------------------------------------------------------------- models resampled into the resident volume through an affine map (ABI 1.18)
 * What blok_hip_volume_stamp_models cannot do — a rotation by any angle, an enlargement or reduction by any factor, a mirror, a shear —
 * is one operation: every cell of the volume asks the model which voxel lies under its centre.  Integer arithmetic only: one right answer,
 * bit-identical on the host (blok_affine_stamp_voxels, blok_world.h) and on the device.  The call blocks.
 *  - Record: blok_affine below, the map from the WORLD to the MODEL.  m in units of 2^-16 model voxel per world voxel; t the model-space
 *    position of the CENTRE of world voxel `anchor`, in units of 2^-16 model voxel.  blok_affine_from_instance and blok_affine_from_matrix
 *    (blok_world.h) make records from a placement or from a forward matrix.
 *  - Sampling.  For a world voxel w, every product and sum in 64 bits:  P_k(w) = t_k + sum_j m[k][j] * (w_j - anchor_j),  v_k = P_k >> 16
 *    (an arithmetic shift: a floor).
 *  - Written set.  The cell w is touched iff w lies in the region cut with the volume's box (region: world voxels, half open, both pointers
 *    NULL = the whole box) and the model has a voxel at v in its local lattice (the coordinates given to blok_hip_model_create).  Such a
 *    cell gets what blok_hip_volume_stamp_models writes for that model voxel in the same mode (BLOK_STAMP_SET / KEEP / ERASE, `density`);
 *    nothing else changes.  A point sample per cell: no holes, no cell written twice.  A singular m is legal: rank 2 extrudes, m = 0 fills
 *    the region with one voxel's material if t lands on a filled voxel and writes nothing otherwise.
 *  - Scale exponents.  The model's exponent (blok_hip_model_set_scale) is ignored, models of any exponent are taken: the matrix carries all
 *    scale.
 *  - Order: the result equals n successive calls in table order.  out_n_voxels (may be NULL): cells written, summed over the records; for
 *    KEEP the cells that were empty and got filled.
 *  - Afterwards masks, occupancy words and dirty flags are those blok_hip_volume_set_voxels leaves for the same writes, refreshed over each
 *    record's own clipped box (never over their union); the next blok_hip_volume_rebuild installs the world.
 *  - Errors, nothing written.  BLOK_ERR_INVALID_ARG: an unknown or destroyed model, a non-zero reserved word, |m[k][j]| > 2^22,
 *    |t_k| > 2^40, an anchor from which some cell of the volume's box lies 2^20 or more away on an axis, an unknown mode, for SET and KEEP a
 *    density that is not finite or <= 0, a null table with n > 0, exactly one region pointer NULL, lo > hi on an axis.
 *    BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume above 2^32 cells.  BLOK_ERR_NO_WORLD: no volume.  n == 0 is BLOK_OK. */
typedef struct blok_affine {
    uint32_t model;
    int32_t  anchor[3];   /* a world voxel */
    int32_t  m[3][3];     /* world -> model, 2^-16 model voxel per world voxel */
    uint32_t reserved[5]; /* zero */
    int64_t  t[3];        /* model-space position of the centre of world voxel `anchor`, 2^-16 model voxel */
} blok_affine;            /* 96 bytes */
int blok_hip_volume_stamp_affine(blok_hip_ctx* ctx, const blok_affine* table_host, uint32_t n, const int32_t region_lo[3],
                                 const int32_t region_hi[3], int mode, float density, uint64_t* out_n_voxels);

/* ------------------------------------------------------------- connected components of the resident volume (ABI 1.8)
 * Which voxels hang together, answered on the device, and one such piece lifted out as a model.  Integer arithmetic only: one right
 * answer, bit-identical on the host (blok_components_label, blok_world.h) and on the device.  All calls block.
 *  - Filled: a voxel is filled iff its density > 0 (the rebuild's rule; 0, negative and NaN densities are empty).
 *  - Adjacency: two filled voxels of the region are adjacent iff they differ by one in exactly one coordinate (face adjacency, 6
 *    neighbours).  Voxels touching only by an edge or a corner are not adjacent.  Voxels outside the region connect nothing: two pieces
 *    joined only through a voxel outside the region are two components.
 *  - Component: a class of the transitive closure of adjacency over the region's filled voxels.
 *  - Index and label: a region voxel has the linear index r = (x - lo.x) + (y - lo.y) rx + (z - lo.z) rx ry (x fastest, as in the
 *    arrays; rx, ry the region's extents).  The label of a component is the smallest r among its voxels.  The label array holds, per
 *    region cell in index order, the cell's component label; empty cells hold BLOK_LABEL_EMPTY.
 *  - Records: one blok_component per component, sorted by label ascending (labels are distinct, so the order is total).  `touches` is how
 *    a caller decides what is anchored: for a region standing on its floor "floating" is !(touches & 1 << 3); for a region inside a larger
 *    world it is "touches none of the five faces that continue into the world".  Bit f is set iff the bounds reach the region's side f.
 *  - blok_hip_volume_label_components: the region is in world voxels, half open; both pointers NULL = the whole box (the convention of
 *    blok_hip_volume_extract_quads).  flags must be 0.  Either count pointer may be NULL.  The snapshot — label array, record table and
 *    region — stays in device memory, owned by the context; later edits do not touch it.  The next labelling replaces it;
 *    blok_hip_volume_destroy, a new blok_hip_volume_create and blok_hip_destroy free it.
 *  - blok_hip_volume_components_download copies records [first, first + count), blok_hip_volume_labels_download cells
 *    [first, first + count) of the region, so a large snapshot can be fetched in pieces.
 *  - blok_hip_volume_capture_component makes a model of the snapshot's voxels with this label that are still filled in the volume NOW,
 *    with the volume's current material ids: exactly the model blok_hip_model_create builds from the list
 *    {(w - rec.lo, ids[w]) : label[w] == label, density[w] > 0}, rec.lo being the record's lo, returned in out_origin (may be NULL): the
 *    same node and material arrays byte for byte, the same levels, origin and box.  An instance {model, offset = out_origin, identity}
 *    shows the piece exactly where it was.  Membership is judged against the current volume, so there is no staleness rule: after a CUT
 *    of one component the snapshot still serves the others.  BLOK_COMPONENT_CUT then clears those voxels (density 0, id 0) and refreshes
 *    masks, occupancy words and dirty flags over the record's box, as BLOK_CAPTURE_CUT does.  If the model cannot be built, nothing is cut.
 *  - Errors, each leaving the previous snapshot and the volume as they were.  BLOK_ERR_INVALID_ARG: unknown flag bits, exactly one region
 *    pointer NULL, lo > hi on an axis; for the downloads no snapshot, a range past the end, or NULL with count > 0; for the capture no
 *    snapshot, out_model NULL, or a label that is not a record's label.  BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume
 *    above 2^32 cells, a region of 2^32 cells (the sentinel would be an index); for the capture none of the component's voxels still
 *    filled (then no model is made, no id consumed, *out_n_voxels = 0).  BLOK_ERR_NO_WORLD: no volume.  BLOK_ERR_OOM: a failed
 *    allocation.  An empty region, or one without filled voxels, is BLOK_OK with zero counts and an empty snapshot. */
#define BLOK_LABEL_EMPTY 0xFFFFFFFFu
typedef struct blok_component {
    uint32_t label;        /* = index of the component's first voxel in x-fastest order */
    uint32_t touches;      /* bit f (blok_hit::face numbering 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z): the component has a voxel in the region's
                              outermost layer on that side */
    uint64_t n_voxels;
    int32_t  lo[3], hi[3]; /* tight bounds of its voxels, world voxels, half open */
} blok_component;          /* 40 bytes */
int blok_hip_volume_label_components(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                                     uint64_t* out_n_components, uint64_t* out_n_voxels);
int blok_hip_volume_components_download(blok_hip_ctx* ctx, blok_component* out_host, uint64_t first, uint64_t count);
int blok_hip_volume_labels_download(blok_hip_ctx* ctx, uint32_t* out_host, uint64_t first, uint64_t count);
#define BLOK_COMPONENT_CUT 1u   /* afterwards clear the captured voxels in the volume (density 0, id 0) */
int blok_hip_volume_capture_component(blok_hip_ctx* ctx, uint32_t label, uint32_t flags, uint32_t* out_model, int32_t out_origin[3],
                                      uint64_t* out_n_voxels);

/* ------------------------------------------------------------- placed models swept against the resident volume (ABI 1.9)
 * Where a model may move: does it, placed here, hit anything, and how far can it travel along an axis before it does?  Answered from the
 * models' trees and the volume's brick masks where they lie in HBM.  Integer arithmetic only: one right answer, bit-identical on the host
 * (blok_sweep_voxels, blok_world.h) and on the device.  The call blocks.
 *  - Placement: a blok_instance.  A filled model voxel v' (local lattice) lands on the world voxel w(v') of "Record back to world space"
 *    above — the stamp's mapping, so a piece stamped at a swept position lies exactly where the sweep saw it.  The sums are 64-bit.
 *  - Direction: blok_hit::face numbering, 0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z; e is its unit vector.
 *  - Filled cell: inside the volume's box a cell is filled iff its density > 0 (0, negative and NaN densities are empty).  Outside the
 *    box a cell is empty; with BLOK_SWEEP_BOX_IS_SOLID it is filled (the box's walls and floor stop the model).
 *  - n_overlap: the number of filled model voxels v' whose cell w(v') is filled: what the placement itself intersects.
 *  - free(v'): the largest k <= max_distance such that the cells w(v') + s e, s = 1 .. k, are all empty.  The start cell w(v') itself is
 *    not looked at.
 *  - travel: the minimum of free(v') over the model's filled voxels.  The model translated by any s in 1 .. travel overlaps nothing; if
 *    `blocked` (travel < max_distance), the translate by travel + 1 overlaps something.  max_distance == 0 is the pure overlap test;
 *    any uint32 is a legal max_distance: once a column has left the box it is all empty (or all filled, with the flag), so the work is
 *    bounded by the box.
 *  - Independence: each placement is swept against the volume as it is now, independently of the other placements (model against model is
 *    not tested); out_results_host[i] belongs to placements_host[i].  The number of kernel launches does not depend on n_placements.
 *  - Side effects: none on the volume — arrays, masks, occupancy words, dirty flags, the edited box stay as they are — and none on a
 *    components or quads snapshot.
 *  - Errors, nothing written to out_results_host.  BLOK_ERR_INVALID_ARG: a placement that fails what blok_hip_check_instances checks (same
 *    messages), direction > 5, unknown flag bits, a null table or a null result array with a non-zero count.  BLOK_ERR_NO_WORLD: no
 *    volume.  BLOK_ERR_UNSUPPORTED: a volume above 2^32 cells.  n_placements == 0 is BLOK_OK. */
#define BLOK_SWEEP_BOX_IS_SOLID 1u   /* cells outside the volume's box count as filled (default: as empty) */
typedef struct blok_sweep_result {
    uint64_t n_overlap;   /* filled model voxels that land on a filled cell at the placement itself */
    uint32_t travel;      /* 0 .. max_distance */
    uint32_t blocked;     /* 1 iff travel < max_distance */
} blok_sweep_result;      /* 16 bytes */
int blok_hip_volume_sweep_models(blok_hip_ctx* ctx, const blok_instance* placements_host, uint32_t n_placements,
                                 uint32_t direction, uint32_t max_distance, uint32_t flags, blok_sweep_result* out_results_host);

/* ------------------------------------------------------------- the resident volume as a sparse brick stream (ABI 1.10)
 * Save, load, undo and copy/paste without the dense download: a region of the volume becomes a stream of its non-empty 4^3 bricks, kept
 * as a snapshot in HBM and downloadable in pieces, and a stream is written back from the snapshot or from host arrays.  A pure integer
 * function of the two arrays: one right answer, bit-identical on the host (blok_bricks_encode / blok_bricks_decode, blok_world.h) and on
 * the device.  All calls block.
 *  - Region: world voxels, half open; both pointers NULL = the whole box (the convention of blok_hip_volume_extract_quads).  Its extents
 *    are ext[3].
 *  - Bricks are counted from the region's lo, not from the box: brick (bx, by, bz) holds the region cells 4b .. 4b+3 on each axis, cut by
 *    the region; nb[a] = ceil(ext[a] / 4); its index is bx + nb[0] * (by + nb[1] * bz).  Bit b = x + 4y + 16z of a brick's mask is its cell
 *    (x, y, z): the bit order of the volume's own brick masks.
 *  - Stored cell.  Default: a cell is stored iff its density's 32-bit pattern is not 0 or its material id is not 0, so -0.0f, negative
 *    and NaN densities are stored, and so are ids left behind under a SUBTRACT brush.  BLOK_BRICKS_FILLED_ONLY: a cell is stored iff
 *    density > 0, the rebuild's rule.  A brick is stored iff it has a stored cell.
 *  - Record: one blok_brick_record per stored brick, sorted by brick index ascending (indices are distinct, so the order is total).
 *    kind bit 0: all stored cells of the brick have the same density bit pattern; then `density` is that pattern and the brick adds
 *    nothing to the density payload.  Otherwise `density` is the index of the brick's first entry in the density payload, and the brick
 *    adds popcount(mask) entries (bit patterns) in ascending bit order.  kind bit 1 and `material`: the same for ids, in the material
 *    payload.  Payload indices are running sums in record order; they fit uint32_t because a volume has at most 2^32 cells and a stored
 *    brick has at least one cell.  The totals are 64-bit.
 *  - blok_hip_volume_encode_bricks has no effect on the volume or on the quads and components snapshots.  The stream stays in device
 *    memory, owned by the context; later edits do not touch it.  The next encode replaces it; blok_hip_volume_destroy, a new
 *    blok_hip_volume_create and blok_hip_destroy free it.  The result is the same in the keyed and the row-major brick layout.
 *    out_info may be NULL.
 *  - blok_hip_volume_bricks_download copies records [first, first + count); blok_hip_volume_brick_payload_download copies payload entries
 *    [first, first + count), plane 0 the density payload, 1 the material payload.  blok_hip_volume_bricks_info returns the snapshot's info.
 *  - blok_hip_volume_restore_bricks writes the HBM snapshot into [dst_lo, dst_lo + ext); dst_lo NULL = where it was taken.
 *    blok_hip_volume_decode_bricks does the same from host arrays.  Default: every cell of the destination is written: stored cells get
 *    their values, every other cell gets (+0.0f, 0).  BLOK_BRICKS_KEEP_OTHERS: only stored cells are written (a paste).  After a
 *    default-mode encode, the default-mode restore to the same place reproduces both arrays bit for bit; after a FILLED_ONLY encode it
 *    reproduces them where density > 0 and writes (0, 0) elsewhere.
 *  - Afterwards masks, occupancy words, dirty flags and the edited box are those blok_hip_volume_set_voxels leaves for the same writes,
 *    the write counts as one that may have filled voxels, and the next blok_hip_volume_rebuild installs the world.
 *  - Validation of a host stream, on the host, before anything is uploaded or written: version 1; known flag bits; records strictly
 *    ascending by brick; brick < nb[0] nb[1] nb[2]; mask != 0 with no bit outside the region (the last brick on an axis may be partial);
 *    kind <= 3; a non-uniform plane's index equal to the running sum; the four totals equal to what the records imply.  The message names
 *    the first record that fails.
 *  - Errors, each leaving the volume and the previous snapshot as they were.  BLOK_ERR_INVALID_ARG: unknown flag bits, exactly one region
 *    pointer NULL, lo > hi on an axis, no snapshot (restore, info and the downloads), a download range past the end, plane > 1, a null
 *    array with a non-zero count, a host stream that fails validation.  BLOK_ERR_UNSUPPORTED: a region or destination that leaves the
 *    box, a volume above 2^32 cells.  BLOK_ERR_NO_WORLD: no volume.  BLOK_ERR_OOM: a failed device allocation.  An empty region, or a
 *    region with nothing stored, is BLOK_OK with zero counts and an empty snapshot; restoring an empty snapshot in default mode clears
 *    the destination. */
#define BLOK_BRICKS_FILLED_ONLY 1u   /* encode: store the cells with density > 0 only (default: every cell that is not (+0.0f, 0)) */
#define BLOK_BRICKS_KEEP_OTHERS 1u   /* restore / decode: write stored cells only (default: every other cell of the destination gets (0, 0)) */
typedef struct blok_brick_record {
    uint64_t mask;         /* bit x + 4y + 16z: cell (x, y, z) of the brick is stored */
    uint32_t brick;        /* bx + nb[0] * (by + nb[1] * bz), bricks counted from the region's lo */
    uint32_t kind;         /* bit 0: one density pattern, bit 1: one material id */
    uint32_t density;      /* the pattern, or the index of the brick's first density payload entry */
    uint32_t material;     /* the id, or the index of the brick's first material payload entry */
} blok_brick_record;       /* 24 bytes */
typedef struct blok_bricks_info {
    uint32_t version;      /* 1 */
    uint32_t flags;        /* the encode's flags */
    int32_t  lo[3];        /* the region, world voxels */
    uint32_t ext[3];
    uint64_t n_bricks, n_density, n_material, n_voxels;      /* records, payload entries, stored cells */
} blok_bricks_info;        /* 64 bytes */
int blok_hip_volume_encode_bricks(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                                  blok_bricks_info* out_info);
int blok_hip_volume_bricks_info(blok_hip_ctx* ctx, blok_bricks_info* out_info);
int blok_hip_volume_bricks_download(blok_hip_ctx* ctx, blok_brick_record* out_host, uint64_t first, uint64_t count);
int blok_hip_volume_brick_payload_download(blok_hip_ctx* ctx, uint32_t plane, uint32_t* out_u32_host, uint64_t first, uint64_t count);
int blok_hip_volume_restore_bricks(blok_hip_ctx* ctx, const int32_t dst_lo[3], uint32_t flags);
int blok_hip_volume_decode_bricks(blok_hip_ctx* ctx, const blok_bricks_info* info, const blok_brick_record* records,
                                  const uint32_t* density_payload, const uint32_t* material_payload, const int32_t dst_lo[3], uint32_t flags);

/* ------------------------------------------------------------- the distance field of the resident volume (ABI 1.11)
 * How far a cell is from the surface: the squared Euclidean distance to the nearest filled (or empty) cell, capped at a radius, as a
 * snapshot in HBM, and the three edits that threshold it — grow and shrink by a ball, hollow.  Read from the brick masks where they lie,
 * never from the densities.  A pure integer function of density > 0: one right answer, bit-identical on the host (blok_distance_field /
 * blok_distance_edit, blok_world.h) and on the device.  All calls block.
 *  - Cell state.  Inside the volume's box a cell is filled iff density > 0; zero, negative and NaN densities are empty.
 *  - Outside the box a cell is empty; with BLOK_DISTANCE_BOX_IS_SOLID it is filled (the sweep's rule).
 *  - Sources.  By default the filled cells; with BLOK_DISTANCE_TO_EMPTY the empty cells.  Sources are taken from the whole box and its
 *    outside, not only from the region: a source one cell outside the region counts.
 *  - Value.  R = max_radius lies in 0 .. 255.  For a region cell c, D(c) is the minimum of |s - c|^2 over all sources s with
 *    |s - c|^2 <= R^2, where |s - c|^2 is the integer sum of the three squared coordinate differences, and BLOK_DISTANCE_FAR (0xFFFF)
 *    when there is no such source.  D(c) == 0 iff c is itself a source.  R^2 <= 65025, so every value fits a uint16_t beside the sentinel.
 *  - Region: world voxels, half open; both pointers NULL = the whole box (the convention of blok_hip_volume_extract_quads).
 *  - Snapshot: one uint16_t per region cell, x fastest, then y, then z (the labels' index order), in device memory, owned by the context.
 *    Later edits do not touch it; the next field replaces it; blok_hip_volume_destroy, a new blok_hip_volume_create and blok_hip_destroy
 *    free it.  Taking a field has no effect on the volume or on the quads, components and bricks snapshots.  The result is the same in
 *    the keyed and the row-major brick layout.  out_info may be NULL.
 *  - Info: n_zero, n_near and n_far count the region cells with D == 0, with 0 < D <= R^2, and with FAR.
 *  - blok_hip_volume_distance_download copies cells [first, first + count); blok_hip_volume_distance_info returns the snapshot's info.
 *  - blok_hip_volume_edit_by_distance thresholds the snapshot at the squared distance d2, over the snapshot's region only.  Membership is
 *    judged against the volume as it is NOW (as blok_hip_volume_capture_component does), so there is no staleness rule.
 *      BLOK_DISTANCE_GROW: the snapshot must be a to-filled field; every region cell with 1 <= D <= d2 that is empty now gets
 *        (density, material).
 *      BLOK_DISTANCE_SHRINK: the snapshot must be a to-empty field; every region cell with 1 <= D <= d2 that is filled now gets (0.0f, 0);
 *        density and material are ignored.
 *      BLOK_DISTANCE_HOLLOW: the snapshot must be a to-empty field; every region cell with D > d2, FAR included, that is filled now gets
 *        (0.0f, 0): what remains is the shell within d2 of empty space.
 *    d2 <= R^2 of the snapshot is required: beyond that the snapshot cannot decide D <= d2.  d2 is a squared distance on purpose: 1 is the
 *    6-neighbourhood, 2 the 18-neighbourhood, 3 the 26-neighbourhood, r^2 a ball of radius r.  *out_n_voxels (may be NULL) is the number
 *    of cells written.  The snapshot is not updated by the edit.
 *  - After an edit masks, occupancy words, dirty flags and the edited box are those blok_hip_volume_set_voxels leaves for the same writes,
 *    refreshed over the snapshot's region; GROW counts as a write that may have filled voxels; the next blok_hip_volume_rebuild installs
 *    the world.
 *  - Errors, each leaving the volume and the previous snapshot as they were.  BLOK_ERR_INVALID_ARG: unknown flag bits, exactly one region
 *    pointer NULL, lo > hi on an axis, max_radius > 255, no snapshot (info, download and edit), a download range past the end, a NULL
 *    array with count > 0, an unknown op, an op that needs the other kind of field, d2 above the snapshot's R^2, for GROW a density that
 *    is not finite or <= 0.  BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume above 2^32 cells, a region of more than
 *    2^31 tiles of 64 x 32 cells (no volume that can be created today has one).  BLOK_ERR_NO_WORLD: no volume.
 *    BLOK_ERR_OOM: a failed device allocation.  An empty region is BLOK_OK with zero counts and an empty snapshot; every edit on an empty
 *    snapshot writes nothing. */
#define BLOK_DISTANCE_TO_EMPTY     1u   /* the sources are the empty cells (default: the filled cells) */
#define BLOK_DISTANCE_BOX_IS_SOLID 2u   /* cells outside the volume's box count as filled (default: as empty) */
#define BLOK_DISTANCE_FAR 0xFFFFu       /* no source within max_radius */
#define BLOK_DISTANCE_GROW   0
#define BLOK_DISTANCE_SHRINK 1
#define BLOK_DISTANCE_HOLLOW 2
typedef struct blok_distance_info {
    uint32_t version;      /* 1 */
    uint32_t flags;        /* the field's flags */
    int32_t  lo[3];        /* the region, world voxels */
    uint32_t ext[3];
    uint32_t max_radius;   /* R */
    uint32_t reserved;     /* 0: pads the counts to 8 bytes */
    uint64_t n_zero, n_near, n_far;      /* region cells with D == 0, with 0 < D <= R^2, with FAR */
} blok_distance_info;      /* 64 bytes */
int blok_hip_volume_distance_field(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t max_radius,
                                   uint32_t flags, blok_distance_info* out_info);
int blok_hip_volume_distance_info(blok_hip_ctx* ctx, blok_distance_info* out_info);
int blok_hip_volume_distance_download(blok_hip_ctx* ctx, uint16_t* out_host, uint64_t first, uint64_t count);
int blok_hip_volume_edit_by_distance(blok_hip_ctx* ctx, int op, uint32_t d2, float density, uint32_t material, uint64_t* out_n_voxels);

/* ------------------------------------------------------------- the flood of the resident volume from seeds (ABI 1.12)
 * Reachability through the volume: the least number of 6-neighbour steps from a seed set to every cell through passable cells, capped, as
 * a snapshot in HBM, and the four edits that threshold it — fill (pour, plug), seal what the flood did not reach, paint and clear what it
 * did.  A pure integer function of density > 0 and, with BLOK_FLOOD_SAME_MATERIAL, of the material ids: one right answer, bit-identical
 * on the host (blok_flood_field / blok_flood_edit, blok_world.h) and on the device.  All calls block.
 *  - Cell state.  Inside the volume's box a cell is filled iff density > 0; zero, negative and NaN densities are empty.
 *  - Region: world voxels, half open; both pointers NULL = the whole box.  A cell outside the region is impassable: a path never leaves
 *    the region.
 *  - Passable cells.  By default the region cells that are empty; with BLOK_FLOOD_THROUGH_FILLED the filled ones; with
 *    BLOK_FLOOD_SAME_MATERIAL (legal only together with THROUGH_FILLED) the filled ones whose material id equals `material`.  Without
 *    SAME_MATERIAL `material` is ignored.
 *  - Seeds.  The n_seeds world cells seeds_xyz_host[3 i ..], and with flag bit BLOK_FLOOD_SEED_FACE(f) every passable cell of the
 *    region's outermost layer on side f (blok_hit::face numbering: 0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z).  A listed seed that is not
 *    passable is ignored; duplicates are harmless.  A listed seed outside the region is BLOK_ERR_INVALID_ARG, the message names the first
 *    one, and nothing changes.  No seed at all is BLOK_OK with every value FAR.
 *  - Value.  K = max_steps lies in 0 .. 65534.  D(c) is the length of the shortest chain of passable cells from a seed to c, consecutive
 *    cells differing by one in exactly one coordinate.  The value of c is D(c) if that is at most K, and BLOK_FLOOD_FAR (0xFFFF)
 *    otherwise; impassable cells hold FAR.  D(c) == 0 iff c is a passable seed.
 *  - Snapshot: one uint16_t per region cell, x fastest, then y, then z, in device memory, owned by the context beside the distance
 *    snapshot and with the same life: later edits do not touch it; the next flood replaces it; blok_hip_volume_destroy, a new
 *    blok_hip_volume_create and blok_hip_destroy free it.  Taking it changes nothing in the volume and nothing in the quads, components,
 *    bricks and distance snapshots.  The result is the same in the keyed and the row-major brick layout.  out_info may be NULL.
 *  - Info: farthest is the largest value that is not FAR, or 0; n_seed counts the cells with D == 0, n_reached those with 0 < D <= K,
 *    n_unreached the passable cells that hold FAR.  farthest < max_steps proves that the flood ended on its own and not at the cap: a
 *    passable cell with FAR next to a reached one would have taken farthest + 1 <= max_steps at the most.  Then n_unreached counts
 *    exactly the passable cells no chain reaches, which is what BLOK_FLOOD_FILL_UNREACHED relies on to seal cavities and nothing else.
 *    Nothing in the info depends on how the device scheduled the work.
 *  - blok_hip_volume_flood_download copies cells [first, first + count); blok_hip_volume_flood_info returns the snapshot's info.
 *  - blok_hip_volume_edit_by_flood works over the snapshot's region and judges each cell by the volume as it is NOW (the rule of
 *    blok_hip_volume_edit_by_distance); the snapshot is not updated by an edit.
 *      BLOK_FLOOD_FILL: needs a through-empty field; every region cell with D <= d that is empty now gets (density, material): water up
 *        to the region's top, or a plug.
 *      BLOK_FLOOD_FILL_UNREACHED: needs a through-empty field; every region cell with FAR that is empty now gets (density, material);
 *        d is ignored.  After a flood from the six faces that ended on its own this seals the cavities.
 *      BLOK_FLOOD_PAINT: needs a THROUGH_FILLED field; every region cell with D <= d that is filled now gets the id `material`; its
 *        density is untouched.
 *      BLOK_FLOOD_CLEAR: needs a THROUGH_FILLED field; every region cell with D <= d that is filled now gets (0.0f, 0).
 *    d <= max_steps of the snapshot is required (FILL_UNREACHED ignores d).  *out_n_voxels (may be NULL) is the number of cells written.
 *  - After an edit masks, occupancy words, dirty flags and the edited box are those blok_hip_volume_set_voxels leaves for the same writes,
 *    refreshed over the snapshot's region; PAINT changes no mask and still marks the bricks it wrote dirty, so the next rebuild gathers
 *    the new ids; the FILL ops count as writes that may have filled voxels.
 *  - Errors, each leaving the volume and the previous snapshot as they were.  BLOK_ERR_INVALID_ARG: unknown flag bits, SAME_MATERIAL
 *    without THROUGH_FILLED, max_steps > 65534, exactly one region pointer NULL, lo > hi on an axis, a NULL seed array with n_seeds > 0,
 *    a listed seed outside the region, no snapshot (info, download and edit), a download range past the end, a NULL array with
 *    count > 0, an unknown op, an op on the wrong kind of field, d above the snapshot's max_steps, for the FILL ops a density that is not
 *    finite or <= 0.  BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume above 2^32 cells.  BLOK_ERR_NO_WORLD: no volume.
 *    BLOK_ERR_OOM: a failed device allocation.  BLOK_ERR_INTERNAL: the flood did not end within max_steps + 2 rounds, the bound
 *    DESIGN.md §20 proves (the library stops there and never loops further).  An empty region is BLOK_OK with zero counts and an empty
 *    snapshot; every edit on an empty snapshot writes nothing. */
#define BLOK_FLOOD_THROUGH_FILLED 1u    /* the passable cells are the filled ones (default: the empty ones) */
#define BLOK_FLOOD_SAME_MATERIAL  2u    /* ... and only those whose id equals `material`; needs THROUGH_FILLED */
#define BLOK_FLOOD_SEED_FACE(f) (1u << (8 + (f)))      /* every passable cell of the region's outermost layer on side f (0..5) is a seed */
#define BLOK_FLOOD_FAR 0xFFFFu          /* not reached within max_steps, or impassable */
#define BLOK_FLOOD_MAX_STEPS 65534u
#define BLOK_FLOOD_FILL           0
#define BLOK_FLOOD_FILL_UNREACHED 1
#define BLOK_FLOOD_PAINT          2
#define BLOK_FLOOD_CLEAR          3
typedef struct blok_flood_info {
    uint32_t version;      /* 1 */
    uint32_t flags;        /* the field's flags */
    int32_t  lo[3];        /* the region, world voxels */
    uint32_t ext[3];
    uint32_t max_steps;    /* K */
    uint32_t farthest;     /* the largest value that is not FAR, or 0 */
    uint64_t n_seed, n_reached, n_unreached;      /* region cells with D == 0, with 0 < D <= K, passable ones with FAR */
} blok_flood_info;         /* 64 bytes */
int blok_hip_volume_flood_field(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], const int32_t* seeds_xyz_host,
                                uint64_t n_seeds, uint32_t max_steps, uint32_t flags, uint32_t material, blok_flood_info* out_info);
int blok_hip_volume_flood_info(blok_hip_ctx* ctx, blok_flood_info* out_info);
int blok_hip_volume_flood_download(blok_hip_ctx* ctx, uint16_t* out_host, uint64_t first, uint64_t count);
int blok_hip_volume_edit_by_flood(blok_hip_ctx* ctx, int op, uint32_t d, float density, uint32_t material, uint64_t* out_n_voxels);

/* ------------------------------------------------------------- the column field of the resident volume, and scatter (ABI 1.13)
 * Where the ground is, and what to put on it, without a download: for every column of a region along an axis the first filled cell met
 * from one end and that cell's material id, as a snapshot in HBM; and scatter, which turns that snapshot into a sorted table of
 * blok_instance placements in HBM by a seeded, seamless, pure integer rule.  The table is traced where it lies (the *_instanced_device
 * entries) or downloaded and stamped (blok_hip_volume_stamp_models).  One right answer, bit-identical on the host (blok_column_field /
 * blok_scatter, blok_world.h) and on the device.  All calls block.
 * The column field.
 *  - Cell state.  A cell is filled iff density > 0.  The tops are read from the brick masks (which every edit leaves equal to that
 *    rule), never from the densities; the material plane reads one id per column that hits.
 *  - Region: world voxels, half open; both pointers NULL = the whole box.  The field sees only cells inside the region.
 *  - Columns.  With p < q the two axes other than `axis`, the column of region-local (cp, cq) has index cp + ext[p] * cq;
 *    n_columns = ext[p] * ext[q].
 *  - Value.  top is the region-local coordinate along `axis`, counted from lo[axis], of the first filled cell met from the entry face: by
 *    default the face at hi, travelling -axis (the highest filled cell); with BLOK_COLUMNS_FROM_LOW the face at lo, travelling +axis (the
 *    lowest).  A column without a filled cell holds BLOK_COLUMNS_NONE.  A box's extent is at most 16384, so the value fits a uint16_t.
 *  - Material plane: the material id of the top cell; 0 for a column with NONE.
 *  - Snapshot: plane 0 is one uint16_t per column, plane 1 one uint32_t, in device memory, owned by the context beside the distance
 *    snapshot and with the same life: later edits do not touch it; the next field replaces it; blok_hip_volume_destroy, a new
 *    blok_hip_volume_create and blok_hip_destroy free it.  Taking it changes nothing in the volume and nothing in the quads, components,
 *    bricks, distance and flood snapshots.  The result is the same in the keyed and the row-major brick layout.  out_info may be NULL.
 *  - Info: n_hit counts the columns with a top; min_top and max_top range over them (BLOK_COLUMNS_NONE and 0 when none hit).
 *  - blok_hip_volume_columns_download copies elements [first, first + count) of a plane; blok_hip_volume_columns_info returns the info.
 *  - Errors, each leaving the volume, the previous snapshot and the previous scatter table as they were.  BLOK_ERR_INVALID_ARG: unknown
 *    flag bits, axis > 2, exactly one region pointer NULL, lo > hi on an axis, no snapshot (info and download), a download range past the
 *    end, plane > 1, a NULL array with count > 0.  BLOK_ERR_UNSUPPORTED: a region that leaves the box, a volume above 2^32 cells.
 *    BLOK_ERR_NO_WORLD: no volume.  BLOK_ERR_OOM: a failed device allocation.  An empty region is BLOK_OK with zero counts. */
#define BLOK_COLUMNS_FROM_LOW 1u      /* enter at the region's lo face and travel +axis (default: enter at hi, travel -axis) */
#define BLOK_COLUMNS_NONE 0xFFFFu     /* no filled cell in the column */
typedef struct blok_columns_info {
    uint32_t version;      /* 1 */
    uint32_t flags;
    int32_t  lo[3];        /* the region, world voxels */
    uint32_t ext[3];
    uint32_t axis;         /* 0, 1, 2 */
    uint32_t min_top, max_top;   /* over the columns that hit; BLOK_COLUMNS_NONE and 0 when none hit */
    uint32_t reserved;     /* 0 */
    uint64_t n_columns, n_hit;
} blok_columns_info;       /* 64 bytes */
int blok_hip_volume_column_field(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t axis, uint32_t flags,
                                 blok_columns_info* out_info);
int blok_hip_volume_columns_info(blok_hip_ctx* ctx, blok_columns_info* out_info);
/* plane 0: uint16_t tops, plane 1: uint32_t material ids */
int blok_hip_volume_columns_download(blok_hip_ctx* ctx, uint32_t plane, void* out_host, uint64_t first, uint64_t count);

/* Scatter.
 *  - Input: the current column snapshot, which must have axis == 1 and no BLOK_COLUMNS_FROM_LOW (up is +y).  Nothing else of the volume is
 *    read, and the models are not looked at: blok_hip_check_instances on the downloaded table remains the caller's check, and the
 *    *_instanced_device entries skip instances that fail their limits.
 *  - Hash.  hash3(x, y, z, s) = fmix32(x * 0x9E3779B1 ^ y * 0x85EBCA77 ^ z * 0xC2B2AE3D ^ s) with murmur3's 32-bit finaliser fmix32 (the
 *    terrain's hash), all in uint32_t.  For world column (X, Z) and c = cell_log2: cx = X >> c, cz = Z >> c (arithmetic shifts), S = 1 << c,
 *    h1 = hash3((uint32_t)cx, 0x5CA70001, (uint32_t)cz, seed), h2 = hash3((uint32_t)cx, 0x5CA70002, (uint32_t)cz, seed).
 *  - Candidate.  Cell (cx, cz) has one candidate column, X = (cx << c) + (h1 & (S - 1)), Z = (cz << c) + ((h1 >> 8) & (S - 1)).  A cell
 *    counts toward n_cells iff its candidate lies in the snapshot's region: a world column gets the same decision whatever region was
 *    taken, so placement is seamless in the way the terrain is.
 *  - Tests, in order; the first that fails is counted in n_rejected[0..4].  0 probability: (h1 >> 16) < probability.  1 none: the
 *    candidate's top != NONE.  2 band: min_y <= lo[1] + top <= max_y.  3 material: BLOK_SCATTER_ANY_MATERIAL, or the material plane equals
 *    surface_material.  4 footprint: for every column (X + dx, Z + dz) with |dx|, |dz| <= radius that lies inside the region (columns
 *    outside it are ignored: take the field `radius` wider for seamless footprints), with top' its value as stored: top' <= top + max_rise
 *    unless max_rise == 0xFFFF, and top' != NONE && top' + max_drop >= top unless max_drop == 0xFFFF.  (NONE is 0xFFFF: a column without a
 *    filled cell fails a rise limit as well as a drop limit.)
 *  - Placement, integer arithmetic on the values above.  W = the sum of the weights.  The entry is the first whose cumulative weight
 *    exceeds (h2 & 0xFFFF) % W.  r = ROTATE ? (h2 >> 16) & 3 : 0; m = MIRROR ? (h2 >> 18) & 1 : 0.  axis = (r & 1) ? {2, 1, 0} : {0, 1, 2};
 *    flip = {0, 4, 5, 1}[r] ^ m.  The target cell is T = (X, lo[1] + top + 1 - sink, Z).  For each local axis k with world axis A = axis[k]:
 *    offset[A] = T[A] - anchor[k] when flip bit k is clear, T[A] + 1 + anchor[k] when it is set, so that by "Record back to world space"
 *    above the entry's anchor voxel lands exactly on T.  model is the entry's, reserved is zero.  The four (axis, flip) pairs without
 *    the mirror are the four proper rotations about +y.
 *  - Table: blok_instance records sorted by the candidate's column index, ascending (the indices are distinct), in device memory, owned by
 *    the context.  The next scatter replaces it; a new column field, blok_hip_volume_destroy, a new blok_hip_volume_create and
 *    blok_hip_destroy free it.  blok_hip_volume_scatter_device gives the table where it lies (null for an empty one), valid until then.
 *    out_info may be NULL.
 *  - Errors, each leaving the previous table as it was.  BLOK_ERR_INVALID_ARG: a NULL context, parameter record or entry array; unknown
 *    flag bits or non-zero reserved words; cell_log2 > 8, probability > 65536, radius > 8, max_rise or max_drop above 0xFFFF; n_entries of
 *    0 or above BLOK_SCATTER_MAX_ENTRIES; a weight of 0 or above 65535; min_y > max_y; no column snapshot, or one with another axis or
 *    FROM_LOW; no table (info, download, device); a download range past the end; a NULL array with count > 0.  BLOK_ERR_OOM: a failed
 *    device allocation. */
#define BLOK_SCATTER_ANY_MATERIAL 1u   /* ignore surface_material */
#define BLOK_SCATTER_ROTATE       2u   /* one of the four rotations about +y, chosen by the hash */
#define BLOK_SCATTER_MIRROR       4u   /* also mirror local x, chosen by the hash */
#define BLOK_SCATTER_MAX_ENTRIES 16u
typedef struct blok_scatter_entry {
    uint32_t model;
    uint32_t weight;       /* 1..65535 */
    int32_t  anchor[3];    /* the model voxel (local lattice) that lands on the target cell */
    int32_t  sink;         /* the target cell is this many cells below the first empty cell above the top */
} blok_scatter_entry;      /* 24 bytes */
typedef struct blok_scatter_params {
    uint32_t seed, flags;
    uint32_t cell_log2;          /* c in 0..8: one candidate per 2^c x 2^c cell of world (x, z) */
    uint32_t probability;        /* 0..65536; 65536 = every candidate */
    uint32_t surface_material;
    int32_t  min_y, max_y;       /* world y of the top cell, inclusive band */
    uint32_t radius;             /* 0..8: footprint half-width in columns */
    uint32_t max_rise, max_drop; /* 0..0xFFFF; 0xFFFF = no limit */
    uint32_t reserved[6];        /* zero */
} blok_scatter_params;           /* 64 bytes */
typedef struct blok_scatter_info {
    uint32_t version, flags;     /* 1, the parameters' flags */
    uint64_t n_cells, n_placed;
    uint64_t n_rejected[5];      /* first failing test: probability, none, band, material, footprint */
    uint64_t reserved;           /* 0 */
} blok_scatter_info;             /* 72 bytes */
int blok_hip_volume_scatter_models(blok_hip_ctx* ctx, const blok_scatter_params* params, const blok_scatter_entry* entries_host,
                                   uint32_t n_entries, blok_scatter_info* out_info);
int blok_hip_volume_scatter_info(blok_hip_ctx* ctx, blok_scatter_info* out_info);
int blok_hip_volume_scatter_download(blok_hip_ctx* ctx, blok_instance* out_host, uint64_t first, uint64_t count);
/* The table where it lies, for the *_instanced_device entries; valid until the next scatter / column field / volume. */
int blok_hip_volume_scatter_device(blok_hip_ctx* ctx, const blok_instance** out_dev, uint64_t* out_count);

/* ------------------------------------------------------------- the scroll of the resident volume (ABI 1.14)
 * Moves the volume's box through the world in HBM, by a whole number of bricks, so that the box can follow the camera: every world voxel
 * that stays inside keeps its two 32-bit values exactly, the cells that come into view are empty and reported as up to three boxes (the
 * caller's to fill: blok_hip_volume_generate_terrain, blok_hip_volume_decode_bricks), and the cells that drop out are reported too (plan
 * first, then blok_hip_volume_encode_bricks them).  One right answer, bit-identical on the host (blok_scroll_plan / blok_scroll_voxels,
 * blok_world.h) and on the device.  All calls block.
 * Move.
 *  - The box becomes [origin + delta, origin + delta + dims).  dims, chunk_size, voxel size and brick layout are unchanged.
 *  - Each component of delta is a multiple of 4, so bricks stay bricks.
 *  - A world voxel in both boxes keeps the bit pattern of its density and its id: -0.0f, negative and NaN densities, ids under density 0.
 *  - Every other cell of the new box holds (+0.0f, 0).
 *  - delta = (0, 0, 0) is valid and changes nothing.  It doubles as "where is the box".
 * Boxes.  Take C to be the per-axis intersection of the old and new extents.
 *  - If C is empty on any axis (|delta[a]| >= dims[a]), nothing is kept: exposed is one box, the whole new box, and leaving is one box,
 *    the whole old box.
 *  - Otherwise exposed lists, in this order and only where non-empty: the z slab (new x, new y, z in new \ C), the y slab (new x, y in
 *    new \ C, z in C), the x slab (x in new \ C, y in C, z in C).  leaving is the same construction with the old box's extents.
 *  - The listed boxes are disjoint and cover new \ old, or old \ new, exactly.
 * Afterwards.
 *  - Brick masks, occupancy words, dirty flags and, in the row-major layout, the non-empty flags are what blok_hip_volume_upload of the
 *    new arrays would leave, for ragged last bricks too: a mask bit never refers to a cell outside the box.
 *  - Every brick counts as changed for the next rebuild; no material ids are taken from the previous build's array.
 *  - The edit log notes the whole box as an edit that may have filled voxels.
 *  - The installed world is untouched until the next blok_hip_volume_rebuild, as behind any edit.  That rebuild sees a changed lattice
 *    and searches the sun map anew.
 * Snapshots are of world cells.  The quads hold no position and stay.  The brick stream holds its region in world voxels and stays:
 * blok_hip_volume_restore_bricks(NULL) keeps meaning "where it was taken", and is BLOK_ERR_UNSUPPORTED, with the snapshot kept, if that
 * region has left the box.  The components, the distance field, the flood field and the columns with their scatter table follow the box
 * when their region still lies wholly in the new box, and are freed otherwise: their entries then answer "no snapshot" as after a new
 * volume.
 * Memory.  The move is out of place: a second pair of dense arrays (8 bytes per cell: 8 GiB for a 1024^3 box) and a second mask array live
 * for the duration of the call; the volume adopts them and the old ones are freed once the device has finished.  (An in-place move, with
 * an ordering per axis, is next.)
 * BLOK_SCROLL_PLAN_ONLY runs the same checks and fills the same info, counts included, and writes nothing.  out_info may be NULL.
 * Errors, each leaving the volume, its origin and every snapshot as they were.  BLOK_ERR_INVALID_ARG: NULL delta, a component that is not
 * a multiple of 4, unknown flag bits.  BLOK_ERR_UNSUPPORTED: the new box leaves the int16 lattice [-32768, 32768] (blok_hip_volume_create's
 * rule).  BLOK_ERR_NO_WORLD: no volume.  BLOK_ERR_OOM: the call's scratch could not be allocated. */
#define BLOK_SCROLL_PLAN_ONLY 1u      /* fill out_info, change nothing */
typedef struct blok_scroll_box { int32_t lo[3], hi[3]; } blok_scroll_box;     /* world voxels, half open; 24 bytes */
typedef struct blok_scroll_info {
    int32_t  origin[3];               /* the box's corner after the call (PLAN_ONLY: as it would be) */
    int32_t  delta[3];
    uint32_t n_exposed, n_leaving;    /* 0..3 */
    blok_scroll_box exposed[3];       /* new box minus old box: now (+0.0f, 0), the caller's to fill */
    blok_scroll_box leaving[3];       /* old box minus new box: gone after the call */
    uint64_t n_cells_kept;            /* cells that lie in the old box and in the new */
    uint64_t n_filled_before, n_filled_kept;   /* voxels with density > 0 in the old box / among the kept cells */
} blok_scroll_info;                   /* 200 bytes */
int blok_hip_volume_scroll(blok_hip_ctx* ctx, const int32_t delta[3], uint32_t flags, blok_scroll_info* out_info);

/* ------------------------------------------------------------- a table of shapes applied to the resident volume (ABI 1.15)
 * What a voxel editor does first: fill a box, draw a line, paint a material over a region.  blok_hip_volume_apply_shapes takes a table of
 * primitives, each with its own operation; the result equals the table applied one shape at a time, in order, and is computed in one pass
 * that reads and writes each touched cell once, however many shapes overlap it.  One right answer, bit-identical on the host
 * (blok_shapes_voxels, blok_world.h) and on the device.  The call blocks.
 * Coordinates are in HALF-voxel units: world coordinate = a / 2, and the centre of world voxel w is c = 2 w + 1.  A centre or a corner can
 * so sit on a voxel centre, a face or a corner, and every test is an exact integer test on c.  With dx = c - a:
 *  - BOX: a[k] <= c[k] <= b[k] on all axes (a = 2 lo, b = 2 hi is the half-open voxel box [lo, hi)).  r is zero.
 *  - ELLIPSOID: centre a, radii r[3], b zero: |dx_k| <= r_k on every axis and sum_k dx_k^2 prod_{j != k} r_j^2 <= prod_j r_j^2.  A zero radius
 *    flattens it with no special case: both sides of the sum are then 0, and what remains is the rectangle, the segment or the point of
 *    the other axes' |dx_k| <= r_k.
 *  - CAPSULE: segment a -> b, radius r[0], r[1] = r[2] = 0.  d = b - a, p = c - a, dd = d.d, s = p.d.  dd == 0 or s <= 0: |p|^2 <= r^2; else
 *    s >= dd: |c - b|^2 <= r^2; else |p|^2 dd - s^2 <= r^2 dd.  a == b is the sphere; a chain of capsules is a stroke without gaps.
 *  - CYLINDER: the same d, p, s, a != b: 0 <= s <= dd and |p|^2 dd - s^2 <= r^2 dd.
 * Operations, on a voxel inside the shape and inside the volume's box (filled = density > 0, the rebuild's rule); each counts one write:
 *  - SET: density = value, id = material.  KEEP: the same where the voxel is empty.  ERASE: density = 0.0f, id = 0.
 *  - PAINT: id = material where the voxel is filled.  REPLACE: id = material where it is filled and id == match.  The density is untouched.
 *  - ADD: density = density < value ? value : density.  SUBTRACT: density = value < density ? value : density.  The id is untouched.
 * Voxels outside the box are clipped silently; a shape wholly outside writes nothing.  *out_n_written (may be NULL) is the number of
 * writes by these rules summed over the shapes in order: a voxel under three SET shapes counts three.  n_shapes == 0 is BLOK_OK.
 * Afterwards masks, occupancy words and dirty flags are what blok_hip_volume_set_voxels leaves for the same writes, refreshed per group of
 * shapes whose brick-aligned boxes overlap: two far-apart shapes do not refresh what lies between them.  Snapshots are treated as behind
 * blok_hip_volume_stamp_models.
 * BLOK_ERR_INVALID_ARG, nothing written, the message names the first offending index: a or b outside [-2^17, 2^17]; a radius above 1024;
 * |b - a| above 4096 on an axis of a CAPSULE or CYLINDER; an unknown kind or op; non-zero reserved words or fields the kind does not use;
 * a BOX with a > b on an axis; a CYLINDER with a == b; a value that is not finite, or <= 0 for SET and KEEP; a NULL table with a non-zero
 * count; n_shapes > BLOK_SHAPES_MAX.  BLOK_ERR_NO_WORLD: no volume.  BLOK_ERR_UNSUPPORTED: a volume above 2^32 cells. */
#define BLOK_SHAPE_BOX       0u
#define BLOK_SHAPE_ELLIPSOID 1u
#define BLOK_SHAPE_CAPSULE   2u
#define BLOK_SHAPE_CYLINDER  3u
#define BLOK_SHAPE_SET      0u
#define BLOK_SHAPE_KEEP     1u
#define BLOK_SHAPE_ERASE    2u
#define BLOK_SHAPE_PAINT    3u
#define BLOK_SHAPE_REPLACE  4u
#define BLOK_SHAPE_ADD      5u
#define BLOK_SHAPE_SUBTRACT 6u
#define BLOK_SHAPES_MAX 65536u
typedef struct blok_shape {
    uint32_t kind;                    /* BLOK_SHAPE_BOX .. _CYLINDER */
    uint32_t op;                      /* BLOK_SHAPE_SET .. _SUBTRACT */
    int32_t  a[3], b[3];              /* half-voxel units */
    uint32_t r[3];                    /* half-voxel units */
    uint32_t material, match;
    float    value;
    uint32_t reserved[2];             /* zero */
} blok_shape;                         /* 64 bytes */
int blok_hip_volume_apply_shapes(blok_hip_ctx* ctx, const blok_shape* shapes_host, uint32_t n_shapes, uint64_t* out_n_written);

/* ------------------------------------------------------------- the resident volume reduced to a pyramid of coarser levels (ABI 1.16)
 * The cheap, coarse copy a far field needs: blok_hip_volume_reduce halves a region of the volume `levels` = K times (1 <= K <= 5) and keeps
 * the K coarse levels as a snapshot in device memory.  Nothing of the volume or of any other snapshot changes.
 *  - Level 0 is the volume restricted to the region [region_lo, region_hi) (world voxels, half open; both NULL = the whole box).  A cell
 *    is filled iff density > 0 (read from the brick masks, as the column and distance fields do), its id is its material id, and a filled
 *    cell is exposed iff at least one of its six neighbours is empty: a neighbour inside the box has the volume's real state whether or
 *    not it lies in the region, a neighbour outside the box counts as filled (the faces of the box expose nothing).  A cell outside the
 *    region contributes nothing.
 *  - Level j (1 <= j <= K) is world-aligned: cell C covers the level-(j-1) cells 2C + (dx, dy, dz), i.e. the world voxels
 *    [C 2^j, (C+1) 2^j).  Its grid runs, per axis, from clo = lo >> j (arithmetic: the floor) to chi = (hi + 2^j - 1) >> j, cext = chi - clo;
 *    an empty region has cext = 0 on every axis at every level.  Per cell: n = the sum of the children's n (filled fine cells, at most
 *    32768), e = the sum of the children's e (exposed filled fine cells), and id = the vote of the children: the voters are the children
 *    with e > 0, weighted by e, when BLOK_LOD_VOTE_EXPOSED is set and the cell's e > 0, otherwise the children with n > 0, weighted by n;
 *    weights of equal ids add, the largest sum wins, a tie goes to the smallest id, no voter gives 0.  (A hierarchical vote, not the exact
 *    mode of the 8^j fine cells: each level needs only the level below, and the K levels of one call nest.  An id of 0 on a filled cell is
 *    a filled cell, as everywhere else.)
 *  - Snapshot: per level 1..K three planes over the level's grid, x fastest (index (Cx - clo[0]) + cext[0] ((Cy - clo[1]) + cext[1] (Cz -
 *    clo[2]))): plane 0 n (uint16_t), plane 1 e (uint16_t), plane 2 id (uint32_t).  It is a record of world cells, like the brick stream:
 *    later edits and scrolls leave it alone, the next reduce replaces it, blok_hip_volume_destroy, a new blok_hip_volume_create and
 *    blok_hip_destroy free it.  blok_hip_volume_lod_info returns the info, blok_hip_volume_lod_download copies elements [first, first +
 *    count) of one plane of one level.
 *  - Info, 360 bytes: bytes 0-15 version (1), flags, levels, a reserved zero; 16-27 the region's corner lo, 28-39 its extent ext (world
 *    voxels); then five 64-byte records, level j at byte 40 + 64 (j - 1): clo[3], cext[3], n_cells (= the product of cext), n_filled
 *    (cells with n > 0), n_exposed (cells with e > 0), sum_n and sum_e (the same at every level: the region's filled and exposed voxels).
 *    Records above `levels` are zero.
 *  - blok_hip_volume_lod_model: the cells of `level` with n >= min_count (1 <= min_count <= 8^level) become a new model, byte for byte the
 *    one blok_hip_model_create builds from the voxels {(C - clo, id[C])}; it is built on the device, no voxel list exists on the host.
 *    *out_n_voxels (may be NULL) takes their number.  A level that holds no such cell gives BLOK_ERR_UNSUPPORTED: no model is created and no
 *    id is consumed.
 *  - Errors, each leaving the volume, the previous snapshot and the model store as they were: BLOK_ERR_INVALID_ARG for levels 0 or above
 *    BLOK_LOD_MAX_LEVELS, unknown flag bits, exactly one region pointer NULL, lo > hi, no snapshot (info, download, model), a level 0 or
 *    above the snapshot's, a plane above 2, a range past the end, NULL with count > 0, min_count 0 or above 8^level, a NULL out_model;
 *    BLOK_ERR_UNSUPPORTED for a region that leaves the box or a volume above 2^32 cells; BLOK_ERR_NO_WORLD without a volume (reduce);
 *    BLOK_ERR_OOM.  An empty region is BLOK_OK with zero counts and an empty snapshot.  out_info may be NULL. */
#define BLOK_LOD_VOTE_EXPOSED 1u      /* exposed cells alone vote where a coarse cell has any */
#define BLOK_LOD_MAX_LEVELS 5u
typedef struct blok_lod_level {
    int32_t  clo[3];                  /* the level's grid: first cell, in units of 2^level world voxels */
    uint32_t cext[3];
    uint64_t n_cells, n_filled, n_exposed, sum_n, sum_e;
} blok_lod_level;                     /* 64 bytes */
typedef struct blok_lod_info {
    uint32_t version, flags, levels, reserved;
    int32_t  lo[3];                   /* the region, world voxels */
    uint32_t ext[3];
    blok_lod_level level[5];          /* level j at [j - 1] */
} blok_lod_info;                      /* 360 bytes */
int blok_hip_volume_reduce(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t levels, uint32_t flags,
                           blok_lod_info* out_info);
int blok_hip_volume_lod_info(blok_hip_ctx* ctx, blok_lod_info* out_info);
int blok_hip_volume_lod_download(blok_hip_ctx* ctx, uint32_t level, uint32_t plane, void* out_host, uint64_t first, uint64_t count);
int blok_hip_volume_lod_model(blok_hip_ctx* ctx, uint32_t level, uint32_t min_count, uint32_t* out_model, uint64_t* out_n_voxels);

/* ------------------------------------------------------------- procedural terrain reduced to coarse levels without a volume (ABI 1.20)
 * blok_hip_terrain_reduce evaluates the terrain function (blok_terrain_params, above) over the world region [region_lo, region_hi) and
 * reduces it `levels` times in one pass, without writing a voxel anywhere: it fills the snapshot blok_hip_volume_reduce fills, so
 * blok_hip_volume_lod_info, _lod_download and _lod_model work behind it unchanged and the snapshot has the same life.  It needs no
 * volume; a volume that exists is neither read nor written, and no other snapshot changes.  The call blocks.
 *  - Without BLOK_LOD_SEAMLESS the planes and the info are, byte for byte, what blok_hip_volume_generate_terrain(params, NULL, NULL)
 *    followed by blok_hip_volume_reduce(NULL, NULL, levels, flags) leaves on a volume whose box is exactly the region (origin region_lo,
 *    dims region_hi - region_lo): the faces of the region expose nothing.
 *  - With BLOK_LOD_SEAMLESS a filled voxel is exposed iff the function says one of its six neighbours is empty, wherever the region ends:
 *    the result of reduce(region_lo, region_hi, levels, flags & BLOK_LOD_VOTE_EXPOSED) on a volume whose box is the region grown by one
 *    voxel on every side and filled the same way.  Promise: for regions whose corners are multiples of 2^levels, the planes of a union
 *    of regions are the concatenation of the parts' planes (a ring of coarse boxes can be built and refreshed in strips).
 *  - info.flags holds the flags as passed; everything else in the info is the composition's.
 *  - BLOK_ERR_INVALID_ARG: NULL params, parameters blok_terrain_validate refuses, params->flags != 0 (SHELL, CLOSE_SIDES and ADD describe
 *    writes into a volume), a NULL region pointer, lo > hi on an axis, levels 0 or above BLOK_LOD_MAX_LEVELS, unknown flag bits.
 *    BLOK_ERR_UNSUPPORTED: a coordinate beyond +-2^30, an extent above 65536 on an axis, 2^31 or more level-1 cells.  BLOK_ERR_OOM.
 *    Every error leaves the previous snapshot in place.  lo == hi on an axis is BLOK_OK with an empty snapshot.  out_info may be NULL. */
#define BLOK_LOD_SEAMLESS 2u          /* terrain_reduce only: neighbours judged by the function, not by the region's faces */
int blok_hip_terrain_reduce(blok_hip_ctx* ctx, const blok_terrain_params* params, const int32_t region_lo[3], const int32_t region_hi[3],
                            uint32_t levels, uint32_t flags, blok_lod_info* out_info);

/* ------------------------------------------------------------- neighbour-count rules stepped over the resident volume (ABI 1.19)
 * The one edit that decides a cell from its own 3 x 3 x 3 neighbourhood: smooth (the majority of the neighbourhood), despeckle, fill pits,
 * the cellular-automaton caves behind a terrain's noise, 3-D Life-like rules.  blok_hip_volume_automaton steps a rule over a region of the
 * volume in place.  The neighbour counts are taken from the brick masks where they lie, never from the densities.  A pure integer function
 * of density > 0 and the ids: one right answer, bit-identical on the host (blok_automaton_voxels, blok_world.h) and on the device, the
 * same in the keyed and the row-major brick layout.  The call blocks.
 *  - Cell state.  Inside the volume's box a cell is filled iff density > 0; zero, negative and NaN densities are empty (§19's rule).
 *  - Outside the box a cell is empty; with BLOK_AUTOMATON_BOX_IS_SOLID it is filled.
 *  - Outside the region a cell inside the box counts with its real state and is never written: it is frozen across all steps.
 *  - Region: world voxels, half open; both pointers NULL = the whole box.  It need not be brick aligned.
 *  - Neighbourhood: 6 (the faces), 18 (and the edges) or 26 (and the corners): the cells at squared distance <= 1, 2, 3.
 *  - A step is synchronous: every region cell is decided from the state BEFORE the step.  With n the number of filled cells among the cell's
 *    neighbourhood, a filled cell with bit n of `survive` clear dies, an empty cell with bit n of `birth` set is born.  A cell that dies
 *    gets (0.0f, 0), as BLOK_DISTANCE_SHRINK writes; a cell that is born gets (rule.density, id); every other cell keeps both of its 32-bit
 *    values bit for bit — an empty cell its NaN or negative density and its stale id.
 *  - The id of a born cell.  With BLOK_AUTOMATON_FIXED_MATERIAL it is rule.material.  Otherwise the cells of its neighbourhood that lie
 *    inside the box and were filled before the step — those that die in this step included — cast one vote each for their stored id; the
 *    most votes win, a tie goes to the smallest id (§24's rule); with no voter (only the solid outside, or bit 0 of `birth`) the id is
 *    rule.material.  The ids of empty cells never vote.
 *  - Steps.  Step k + 1 reads what step k left.  The call stops after the first step that changes nothing; that step counts in steps_run.
 *  - out_step_counts (may be NULL) takes 2 * rule.steps values: the cells born and the cells that died in step k at [2 k] and [2 k + 1],
 *    zero for the steps past steps_run.
 *  - Info (out_info may be NULL): the region, steps_run, n_born and n_died summed over the steps run, n_filled the filled region cells
 *    after the last of them.
 *  - After the call masks, occupancy words, dirty flags and the edited box are those blok_hip_volume_set_voxels leaves for the same writes,
 *    refreshed over the region after every step that wrote; the writes count as ones that may have filled voxels iff birth != 0.
 *    Snapshots and labels are untouched.  The next blok_hip_volume_rebuild installs the world.
 *  - Errors, each leaving the volume untouched.  BLOK_ERR_INVALID_ARG: a NULL rule, a neighbourhood other than 6, 18, 26, a bit of
 *    `survive` or `birth` above the neighbourhood's size, unknown flag bits, reserved != 0, steps outside 1 .. 255, birth != 0 with a
 *    density that is not finite or <= 0, exactly one region pointer NULL, lo > hi on an axis.  BLOK_ERR_UNSUPPORTED: a region that leaves
 *    the box, a volume above 2^32 cells.  BLOK_ERR_NO_WORLD: no volume.  BLOK_ERR_OOM: a failed device allocation (16 bytes per brick of
 *    the region, for the call).  An empty region is BLOK_OK with zero counts and steps_run = 0. */
#define BLOK_AUTOMATON_BOX_IS_SOLID   1u   /* cells outside the volume's box count as filled (default: as empty) */
#define BLOK_AUTOMATON_FIXED_MATERIAL 2u   /* a born cell gets rule.material; nobody votes */
typedef struct blok_automaton_rule {
    uint32_t neighbourhood; /* 6 (faces), 18 (+ edges), 26 (+ corners): the cells at squared distance <= 1, 2, 3 */
    uint32_t survive;       /* bit n: a filled cell with n filled neighbours stays filled */
    uint32_t birth;         /* bit n: an empty cell with n filled neighbours becomes filled */
    uint32_t flags;         /* BLOK_AUTOMATON_* */
    float    density;       /* what a born cell gets; finite and > 0 when birth != 0 */
    uint32_t material;      /* a born cell's id with FIXED_MATERIAL, else the id when nobody votes */
    uint32_t steps;         /* 1 .. 255 */
    uint32_t reserved;      /* 0 */
} blok_automaton_rule;      /* 32 bytes */
typedef struct blok_automaton_info {
    uint32_t version;       /* 1 */
    uint32_t flags;         /* the rule's flags */
    int32_t  lo[3];         /* the region, world voxels */
    uint32_t ext[3];
    uint32_t steps_run;
    uint32_t reserved;      /* 0 */
    uint64_t n_born, n_died, n_filled;   /* summed over the steps run; filled region cells after the last */
} blok_automaton_info;      /* 64 bytes */
int blok_hip_volume_automaton(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], const blok_automaton_rule* rule,
                              uint64_t* out_step_counts, blok_automaton_info* out_info);

/* ------------------------------------------------------------- several devices, one process
 * The tile partition of the frame over the GPUs of one node driven from one host thread (no reference
 * counterpart — blok is single-GPU): one context and one stream per device in `device_ordinals` (the first is the root), the
 * world replicated on each, every device traces tiles rank, rank + G, ... of the tile x tile grid, the RGBA8 tiles are gathered
 * on the root and un-permuted into the row-major frame; first-hit records stay on the device that traced them.
 * Transport: RCCL when allow_rccl != 0, librccl is found at run time (dlopen; no link-time dependency) and the devices are
 * distinct — one communicator per device (ncclCommInitAll), one ncclGroupStart/End per frame with every peer's ncclSend and the
 * root's ncclRecvs, each on its device's stream; otherwise hipMemcpyPeerAsync from every peer into the root's buffer (also how
 * a one-GPU box rehearses several ranks: the same ordinal may be listed more than once); one device: none.
 * blok_hip_multi_transport() says which ("rccl", "peer-copy", "none").  The per-device contexts are ordinary contexts
 * (blok_hip_multi_context) for settings such as blok_hip_set_beam. */
typedef struct blok_hip_multi blok_hip_multi;
int  blok_hip_multi_create(blok_hip_multi** out, const int* device_ordinals, uint32_t n_devices, uint32_t width, uint32_t height,
                           uint32_t tile, int allow_rccl);
void blok_hip_multi_destroy(blok_hip_multi* m);
const char* blok_hip_multi_last_error(const blok_hip_multi* m);      /* NULL: the last failed create on this thread */
uint32_t blok_hip_multi_device_count(const blok_hip_multi* m);
const char* blok_hip_multi_transport(const blok_hip_multi* m);
blok_hip_ctx* blok_hip_multi_context(blok_hip_multi* m, uint32_t rank);
/* = Renderer::addWorld on every device (replicated). */
int  blok_hip_multi_upload_world(blok_hip_multi* m, const blok_svo_node* nodes, size_t n_nodes, const blok_sub_chunk* sub_chunks,
                                 size_t n_sub_chunks, const blok_material* materials, size_t n_materials);
/* One frame, asynchronous: enqueues trace, exchange and un-permute; *out_rgba8_dev_on_root (may be NULL) = the root's
 * width x height RGBA8 frame, valid after blok_hip_multi_synchronize.  blok_hip_multi_draw_frame = that + synchronise + copy. */
int  blok_hip_multi_draw_frame_device(blok_hip_multi* m, const blok_camera* cam, const uint32_t** out_rgba8_dev_on_root);
int  blok_hip_multi_synchronize(blok_hip_multi* m);
int  blok_hip_multi_draw_frame(blok_hip_multi* m, const blok_camera* cam, uint32_t* out_rgba8_host);
/* Rank `rank`'s first-hit records of the last synchronised frame, in its tile order (blok_hip_tiles_for_rank x tile^2). */
/* Several frames per call (1..BLOK_MAX_TILE_FRAMES cameras, one launch pair per device; the frames lie one after the other in
 * the root's buffer / in out_rgba8_host), and how the tiles reach the root:
 *   "sparse-pull" (mode 1; the default, mode -1, whenever it can be had): every device compacts its tiles with a hit into 16-bit
 *       (material, face) code records in its own memory and the root's assembly kernel reads counts and records straight out of
 *       the peers' memory through peer mappings and expands them — nothing staged, no size on the host, only live records cross
 *       a link, bit-identical frames.  Needs peer access from the root to every device (refused with BLOK_ERR_UNSUPPORTED
 *       otherwise) and a material table that fits the codes (else the call uses "dense").
 *   "dense" (mode 0): the RGBA8 tiles of every rank travel whole (blok_hip_multi_transport), then an un-permute kernel. */
int  blok_hip_multi_set_exchange(blok_hip_multi* m, int mode);
const char* blok_hip_multi_exchange(const blok_hip_multi* m);        /* what the next call will use: "sparse-pull" or "dense" */
int  blok_hip_multi_draw_frames_device(blok_hip_multi* m, const blok_camera* cams, uint32_t n_frames, const uint32_t** out_rgba8_dev_on_root);
int  blok_hip_multi_draw_frames(blok_hip_multi* m, const blok_camera* cams, uint32_t n_frames, uint32_t* out_rgba8_host);
/* first-hit records of the first frame of the last call */
int  blok_hip_multi_download_hits(blok_hip_multi* m, uint32_t rank, blok_hit* out_host, size_t capacity_records);

#ifdef __cplusplus
}
#endif
#endif /* BLOK_HIP_H */
