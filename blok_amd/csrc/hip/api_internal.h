// Internals shared by the translation units of the C ABI (api.hip, api_post.hip, api_volume.hip): the context, the error
// macro and the helpers defined in api.hip.  Not installed; include/blok_hip.h is the interface.
#ifndef BLOK_API_INTERNAL_H
#define BLOK_API_INTERNAL_H
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "blok_hip.h"
#include "blok_hip_debug.h"
#include "device_buffer.h"
#include "gpu_build.h"
#include <hip/hip_fp16.h>
#include "post_kernels.h"
#include "post_core.h"
#include "reference_world.h"
#include "trace_kernels.h"
#include "dense_kernels.h"
#include "launch_policy.h"
#include "beam_cache.h"
#include "tile_order.h"
#include "path_args.h"
#include "tree.h"
#include "instance_core.h"
#include "../common/lights_core.h"

// Every device array, pinned array and event of the context is a member that owns it (device_buffer.h): the context's destructor is its
// teardown, a reset is the assignment of a fresh value, and every grow-on-demand site is one reserve() that names what must finish first.
struct blok_hip_ctx {
    int device = 0;
    uint32_t width = 0, height = 0;
    // derived structure in HBM: the tree as the kernels' arguments read it, and its owners — empty while the arrays are the resident volume's
    uint4* d_nodes = nullptr;
    uint32_t* d_tree_materials = nullptr;
    blok::DeviceArray<uint4> own_nodes;
    blok::DeviceArray<uint32_t> own_tree_materials;
    blok::DeviceArray<blok_material> d_materials;
    size_t n_materials = 0;
    bool has_world = false;
    bool built_on_device = false;     // structure built by gpu_build.hip (else tree_build.cpp on the host)
    uint32_t world_version = 0;        // counts uploads and rebuilds: scheduling state measured on another world is dropped (TileOrder::key)
    uint32_t tree_version = 0;         // counts every tree installed, a rebuild of the resident volume included (which keeps world_version, and with it the view's order): what was computed FROM the tree is dropped (beam_cache.h)
    bool tree_owned_by_volume = false; // d_nodes / d_tree_materials belong to the resident volume's scratch (gpu_build.h): own_nodes / own_tree_materials are empty
    bool force_host_build = false;
    blok_world_stats stats{};
    float voxel_size = 1.0f;            // for the next blok_hip_upload_world / blok_hip_upload_dense (blok_hip_set_voxel_size)
    float world_voxel_size = 1.0f;      // of the installed world
    float pending_voxel_size = 1.0f;    // handed from blok_hip_upload_world / blok_hip_upload_dense to install_tree
    // dense-grid path (dense_kernels.hip): the uploaded id grid in 8^3-cell tiles and one occupancy bit per tile; kept when
    // blok_hip_set_dense_dda was on at blok_hip_upload_dense, and then used by the rectangle entries of the primary trace
    bool dense_dda = false, has_dense = false;
    blok::DeviceArray<uint32_t> d_dense_tiled, d_dense_bits;
    uint32_t dense_tiles[3] = {0, 0, 0};
    int32_t dense_origin[3] = {0, 0, 0};
    // scratch frame for the host-output entry points
    blok::DeviceArray<blok_hit> d_frame;
    // progressive accumulation (CudaTracer::m_dAccum / m_frameIndex / m_prevCam, reference cuda_tracer.hpp:51-55)
    blok::DeviceArray<float> d_accum, d_color;
    size_t accum_pixels = 0;
    uint32_t accum_frames = 0;
    blok_camera prev_cam{};
    bool has_prev_cam = false;
    // image-space chain (post_core.h): history ping-pong [2] and per-frame planes, all width x height
    struct Post {
        size_t pixels = 0;
        uint32_t width = 0, height = 0;      // the frame shape the planes were allocated for
        blok::DeviceArray<float> hist_color[2], moments[2], world_pos[2];
        blok::DeviceArray<uint16_t> hist_len[2];
        blok::DeviceArray<float> unit_normals[2];       // float4: normalize(binary16 normal)
        blok::DeviceArray<uint16_t> motion;             // half2
        blok::DeviceArray<float> variance, ping, pong, taa_hist[2];
        blok::DeviceArray<float> widen;                 // scratch for state downloads
        int cur = 0, taa_cur = 0;
        bool has_motion = false;
        // blok_hip_draw_frame_rt: the frame's own planes and its camera history
        blok::DeviceArray<float> rt_planes[2], rt_denoised, rt_resolved;        // [0] colour, [1] world position
        blok::DeviceArray<uint16_t> rt_normal_roughness_h, rt_motion_h;          // RGBA16F, RG16F
        blok::DeviceArray<uint32_t> rt_albedo_metallic_u8;                       // RGBA8
        blok::DeviceArray<uint32_t> rt_ldr, rt_final;
        uint32_t rt_frame = 0;
        blok_camera rt_prev_cam{};
        // blok_hip_draw_frame_rt_instanced_motion: the first-hit instance plane, and the number of records of the previous frame's table
        // (rt_prev_instances; 0 after a reset or a frame without object motion)
        blok::DeviceArray<uint32_t> rt_ids;
        uint32_t rt_prev_n = 0;
        // blok_hip_draw_frame_rt_posed_motion: ... and of the previous frame's pose table (rt_prev_poses; 0 after a reset, a change of a model's
        // scale or a frame of any other entry)
        uint32_t rt_prev_n_poses = 0;
    } post;
    // blok_hip_draw_frame_rt_instanced(_motion): the frame's instance table in device memory (records), grown on demand, and the previous
    // frame's (the motion entry swaps the two after each frame); outside `post`, which ensure_post may reallocate after the upload
    blok::DeviceArray<blok_instance> rt_instances, rt_prev_instances;
    blok::DeviceArray<blok_pose> rt_poses;       // blok_hip_draw_frame_rt_posed: the frame's pose table in device memory, grown on demand
    blok::DeviceArray<blok_pose> rt_prev_poses;  // blok_hip_draw_frame_rt_posed_motion: the previous frame's (swapped with rt_poses after each frame)
    // device-resident dense store (gpu_build.h: GpuVolume)
    blok::GpuVolume volume;
    bool has_volume = false;
    bool volume_keyed_layout = true;   // blok_hip_set_volume_layout: the next blok_hip_volume_create may use the keyed brick layout (gpu_build.h)
    // the snapshots (gpu_build.h: each knows whether it was taken), each replaced by the next of its kind, all freed with the volume
    // (free_volume_snapshots)
    blok::GpuQuads quads;                // of the last blok_hip_volume_extract_quads
    blok::GpuComponents components;      // of the last blok_hip_volume_label_components
    blok::GpuBricks bricks;              // of the last blok_hip_volume_encode_bricks
    blok::GpuDistance distance;          // of the last blok_hip_volume_distance_field
    blok::GpuFlood flood;                // of the last blok_hip_volume_flood_field
    blok::GpuColumns columns;            // of the last blok_hip_volume_column_field
    blok::GpuScatter scatter;            // of the last blok_hip_volume_scatter_models: it goes with the column snapshot it was made from
    blok::GpuLod lod;                    // of the last blok_hip_volume_reduce
    // emissive voxels as lights (blok_hip.h; api_volume.hip): the table, the owned set (lights_core.h: kSetWords words) and the totals; n == 0:
    // no table.  Cleared by free_world: the owned set is a statement about the world and material table it was built for.
    struct Lights {
        blok::DeviceArray<blok_light> table;
        blok::DeviceArray<uint32_t> owned;
        uint32_t n = 0, n_owned = 0;
        uint64_t n_faces = 0;
        float area_world = 0.0f;
    } lights;
    // the light grid over that table (blok_hip.h: "the light grid"; api_volume.hip): installed iff info.n_cells != 0.  Dropped by
    // clear_lights, so by everything that installs or clears the table.
    struct LightGrid {
        blok::DeviceArray<uint32_t> start, faces;
        blok::DeviceArray<blok_light_grid_item> items;
        blok_light_grid_info info{};
    } light_grid;
    std::vector<uint32_t> material_glows;             // the emissive indices of the installed material table, a bit each (install_materials)
    std::vector<unsigned char> volume_materials;      // the material table the last blok_hip_volume_rebuild installed (compared, not re-uploaded, when unchanged)
    // "last occluder" map of the shadow rays (beam.h: prism_far), rebuilt with every world
    blok::DeviceArray<float> d_sun_map;
    bool sun_map_enabled = true, has_sun_map = false;
    uint32_t sun_loose_edits = 0; int32_t sun_loose_lo[3] = {0, 0, 0}, sun_loose_hi[3] = {0, 0, 0};      // edits since the map was last made tight, and the union of their boxes (update_sun_map)
    bool sun_tighten_pending = false; uint32_t sun_tighten_u0 = 0, sun_tighten_u1 = 0, sun_tighten_v0 = 0, sun_tighten_v1 = 0;      // texels still to be made tight, a band of rows per edit (update_sun_map)
    blok::Event sun_event; bool sun_event_pending = false;                                            // behind the latest patch of the map
    uint32_t ray_batching = 3;          // PathArgs::batch_kinds (blok_hip_set_ray_batching); 3 = 2 + the bounce rounds' tail pool
    uint32_t tail_cap = 24, tail_cap_parked = 32;                 // trips after which a bounce round / a round over parked rays stops (BLOK_TAIL_CAPS overrides, experiments)
    bool pose_tlas = true;                                // blok_hip_set_pose_tlas: posed path launches build and walk the pose BVH (false: the linear loop)
    bool path_resume = false, path_fine_beam = true;      // PathArgs::resume_secondary / fine_beam (blok_hip_set_path_start)
    blok::SunMapArgs sun{};
    // beam pre-pass (beam.h): start parameters per beam tile, one buffer per stream (launches on one stream are
    // ordered, frames in flight on different streams must not share)
    uint32_t beam_tile = 32;
    uint32_t beam_budget = 0;           // 0 = beam.h's default visit budget
    bool miss_in_walk = true;           // who writes the pixels of tiles the pre-pass found empty (blok_hip_set_miss_writer)
    struct StreamScratch {             // per launch stream
        blok::DeviceArray<float> beam;                                   // two-launch form: start parameters per beam tile
        blok::DeviceArray<uint32_t> ctl; blok::DeviceArray<unsigned long long> entries;      // one-launch form: work queue (trace_kernels.h: FrameQueue)
        blok::DeviceArray<unsigned long long> slots; uint32_t serial = 0;   // joint launch: published beam results
        blok::DeviceArray<uint32_t> gave_up;                              // joint and list launches: waves that gave up a bounded wait (sticky; blok_hip_frame_queue_stalls)
        // list launches (trace_kernels.h: LiveList): entries, control words, serial, and the pinned words the searches leave the segments' lengths in
        blok::DeviceArray<unsigned long long> list_entries; size_t list_capacity = 0;   // entries per segment: the stride of the launches
        blok::DeviceArray<unsigned long long> list_ctl;
        uint32_t list_serial = 0;
        blok::PinnedArray<uint32_t> list_hint; bool list_hint_valid = false; uint32_t list_hint_key = 0;
        blok::DeviceArray<uint32_t> tile_map;                            // sparse exchange, root: frame tile -> record (zero between launches)
        blok::DeviceBytes tail_pool;                                      // path launches: the bounce rounds' tail pool (path_core.h: TailRecord[blocks][kTailCapacity]), grown on demand
        blok::DeviceArray<uint32_t> inst_bins;                           // instanced frames: the binning kernel's lists (instance_core.h: kBinWords words per bin), grown on demand
        blok::DeviceArray<blok_hit> inst_hits;                           // instanced frames without a record output: the world records the instance pass reads
        blok::DeviceArray<uint32_t> pose_bins;                           // posed frames: the posed binning kernel's lists (the same layout), grown on demand
        blok::DeviceBytes pose_tlas;                                      // posed path launches: the pose BVH (pose_tlas_core.h), grown on demand
        blok::DeviceArray<blok_pose_motion> pose_motion;                 // posed motion passes: one record per pose (pose_motion.h), grown on demand
        blok::DeviceBytes tlas;                                           // instanced path launches: the instance BVH (tlas_core.h: TlasNode), grown on demand
        blok::DeviceArray<uint32_t> inst_lights;                         // ... with model light tables: the launch's prefix, 8 words of header (blok_instance_lights_info), then icum (n + 1 words), grown on demand
    };
    std::unordered_map<hipStream_t, StreamScratch> beam_buffers;
    // The beam bounds of views at rest (beam_cache.h: key, admission, slots; api_launch.hip: the hazards).  A slot's buffer is written by the
    // searches of ONE launch (the fill) and read by the walks of later launches of the same view, on any stream: the first reader on another
    // stream waits for `ready`, and a slot is refilled only behind the held markers of every stream (api_launch.hip: hold_markers).
    // Allocated by blok_hip_create / _resize for the finest beam tile over the whole frame, so that no launch allocates.
    // A second buffer of the same size per slot holds the view's finer bounds, one per wave tile (beam_cache.h: plan_beam_refine): written by
    // ONE launch behind its walk (the refine kernel, `refined` behind it), read by the walks of the view's later launches under the same two
    // rules — a refill waits for every stream's held markers, which covers the readers of both buffers.
    // The modes (blok_hip_set_beam_cache) are switches of the policy's facts: 1 the beam bounds, 2 `refine`, 3 `packed`, 4 the policy's
    // own_starts, 5 its node_restart.  What a launch then does is one value (beam_cache.h: RestingWalk), made by plan_resting_launch and
    // acted on by api_launch.hip's plan_resting / issue_resting / finish_resting.
    struct BeamCache {
        bool enabled = true;                                // blok_hip_set_beam_cache
        bool refine = true;                                 // ... with the finer bounds (mode 2)
        blok::BeamCachePolicy policy{};
        // What one launch wrote on its stream and later launches read on any: the event behind the writer, and who need not wait any more.
        struct Produced {
            blok::Event done;                               // behind the launch that wrote
            hipStream_t producer = nullptr;                 // ... and its stream
            bool settled = true;                            // `done` has been seen complete: nobody waits any more
            static constexpr uint32_t kWaited = 8;
            hipStream_t waited[kWaited] = {}; uint32_t n_waited = 0;      // streams that already wait for `done` (or are behind it)
        };
        struct Slot {
            blok::DeviceArray<float> d_beam, d_fine;
            Produced filled, refined;
            bool used = false;                              // filled at least once: launches that read it may be in flight
            // the view's packed list and its group table (trace_kernels.h: the packed walk), built behind the count launch on its stream and
            // adopted once `list_done` has been seen complete, so no reader ever waits; rebuilt only behind a refill, under the rule above
            blok::DeviceArray<uint32_t> d_list, d_table;
            blok::DeviceArray<float> d_start;               // mode 4: every entry's own start parameter, in list order (written by the same build)
            blok::DeviceArray<uint32_t> d_node;             // mode 5: ... and the node its restarted walk ends in (trace_core.h: restart_node_word), in list order
            uint32_t n_words = 0, n_groups = 0;             // the table's words as built (kPackGroups per area); its non-empty groups, as read from h_groups at adoption
        } slots[blok::kBeamCacheSlots];
        bool packed = true;                                 // ... with the packed walk (mode 3)
        blok::DeviceArray<uint8_t> d_trips;                 // the count launch's trips, a byte per pixel of the frame: one build at a time reads it
        blok::DeviceArray<float> d_ray_start;               // mode 4: ... and every ray's restart parameter, a float per pixel; the policy's own_starts is the mode
        blok::DeviceArray<uint8_t> d_restarts;              // ... and the trips of the walk restarted there, a byte per pixel: what a mode-4 build sorts by
        blok::DeviceArray<uint32_t> d_ray_node;             // mode 5: ... and the node word of every ray, a word per pixel; the policy's node_restart is the mode
        uint64_t node_hits = 0;                             // blok_hip_beam_cache_node_counters: packed hits that ran packed_frame_node_kernel
        blok::DeviceArray<uint32_t> d_words;                // ... its table before the sort (kPackGroups words per area)
        blok::DeviceBytes d_sort_temp; size_t sort_temp_bytes = 0;
        blok::PinnedArray<uint32_t> h_groups;               // pinned, one word per slot: the table's length, written by the device before list_done
        blok::Event list_done;                              // behind the build in flight (policy.building)
        size_t list_capacity = 0, words_capacity = 0;       // entries per list; words per table
        uint64_t list_builds = 0;                           // blok_hip_beam_cache_list_builds
        uint64_t start_hits = 0, start_other_key = 0;       // blok_hip_beam_cache_start_counters: packed hits that walked from the starts; ... that found another start key
        uint32_t packed_fill = BLOK_PACKED_FILL;            // blok_hip_set_packed_fill: fill units per workgroup of a packed frame's one launch; 0 = the fill in a launch of its own
        uint64_t one_launch_frames = 0, fill_only_workgroups = 0;      // blok_hip_packed_fill_counters
        int last_starts = 0;                                // the latest rectangle launch: 0 no starts, 1 it walked from them (or counted them), 2 it found another start key
        int last_list = 0;                                  // the latest rectangle launch: 0 no list, 1 it counted and issued the build, 2 it walked packed
        uint32_t last_w = 0, last_h = 0;                    // ... and its rectangle (blok_hip_beam_cache_download_list)
        size_t capacity = 0;                                // floats per buffer
        uint64_t hits = 0, fills = 0, refines = 0;          // blok_hip_beam_cache_counters, blok_hip_beam_cache_refines
        int last_action = 0, last_slot = -1; uint32_t last_n_beams = 0;      // the latest rectangle launch: 0 searched, 1 searched into last_slot, 2 walked from it (blok_hip_beam_cache_download)
        int last_fine = 0; uint32_t last_n_fine = 0;        // ... and its finer bounds: 0 none, 1 it issued their searches, 2 it walked from them (blok_hip_beam_cache_download_fine)
    } beam_cache;
    // Longest-first scheduling of the walk for a camera at rest (tile_order.h; rectangle launches of the static forms): every walk wave
    // leaves the clocks it spent in d_cost (one buffer per context, for the launch geometry in `key`).  Every `interval` launches a
    // radix sort of a snapshot of those costs follows the frame on its stream: it writes the order buffer that is NOT in use, and a later
    // launch adopts it once hipEventQuery says it is complete — no launch ever waits.  Decisions: launch_policy.h plan_order.
    struct TileOrder {
        bool enabled = true;
        bool rank_tiles = true;                            // ... also for a rank's tile launches (blok_hip_set_rank_tile_ordering)
        uint32_t interval = 8, interval_now = 8;          // interval_now: of a view that has no order of its own yet (a slot carries its own)
        blok::DeviceArray<uint32_t> d_cost, d_iota;
        blok::DeviceArray<uint32_t> d_keys_in, d_keys;      // the sort's snapshot of the costs, and its sorted keys
        blok::DeviceBytes d_temp;
        size_t temp_bytes = 0, capacity = 0;                // capacity: wave tiles that EVERY buffer of the order has room for (0 until all are there)
        // Round 4: a small CACHE of orders per launch geometry, one slot per view (round 3 kept two buffers — the order in use and the one
        // being sorted — so a caller alternating between two fixed views, stereo eyes or a camera cycle, walked in row-major order for ever).
        // A slot holds an order sorted from the clocks of the view `cam` (own-view: used by launches from that view only) or from dilated
        // clocks (made to be carried to the next view by a shift: only the latest such order is of any use).
        static constexpr int kSlots = 4;
        struct Slot {
            blok::DeviceArray<uint32_t> d_order, d_rank_of;
            bool valid = false, dilated = false;
            uint32_t live = 0, radius = 0;                 // leading entries that walked (as read at adoption); dilation it was sorted with
            blok_camera cam{};                             // the view its clocks were measured under
            float inv_depth[2] = {};                       // mean and sigma of that frame's live beam tiles' inverse start parameters (dilated orders)
            uint32_t frames_since_sort = 0, interval_now = 8;      // launches that walked in it; re-sort interval of its view (doubles while the view rests)
            uint64_t last_use = 0;                         // serial of the latest launch that walked in it
        } slots[kSlots];
        blok::PinnedArray<uint32_t> h_live;                 // pinned, kSlots words: how many leading entries of the slot's order walked (written by the device)
        blok::PinnedArray<float> h_depth;                   // pinned, kSlots x 64 x 3 floats: partial count, sum, sum of squares of the live beam tiles' inverse start parameters
        uint32_t key[7] = {};                               // launch rectangle, frame size, world version
        int current = -1, target = 0;                       // the slot adopted last (-1: none yet); the slot a pending sort writes
        bool pending = false;
        bool orphan = false;                                // a sort of a previous launch geometry may still be running (the next sort waits for it)
        uint32_t still_frames = 0, prefix_limit = 0;
        uint64_t launch_serial = 0, hold_serial = 0;        // orderable launches so far; ... at the latest hold_markers (what the held markers are behind)
        blok_camera last_cam{};                             // camera of the last launch
        blok_camera recent[4] = {}; uint32_t n_recent = 0, revisit_streak = 0;  // cameras of the latest launches; consecutive launches from a view seen among them (alternating views are views at rest)
        blok_camera pending_cam{}; bool pending_dilated = false; uint32_t pending_radius = 0, pending_interval = 8;      // of the sort in flight
        blok::Event done;
        // a camera in motion (launch_policy.h): orders sorted from dilated clocks, carried to the next view by a whole-tile shift
        bool moving = true;                                 // blok_hip_set_moving_order
        blok::DeviceBytes d_class_scratch;                  // tile_order.h: count table and class bytes of the counting sort
        bool have_residual = false; float last_residual = 0.0f;     // what the latest shift left over (sizes the next dilation)
        bool debug_shift = false; uint32_t debug_sx = 0, debug_sy = 0;      // blok_hip_debug_force_order_shift: every ordered launch uses this shift (tests)
        blok::DeviceArray<uint32_t> d_fallback;             // wave tiles the search waves of the latest prefix launch walked themselves (cleared in stream order before it)
        blok::PinnedArray<uint32_t> h_fallback;             // pinned: ... copied here behind the launch
        uint32_t last_fallback = 0;                         // ... as read before the next launch (blok_hip_last_fallback_tiles)
        bool alone_before = false;                          // the previous orderable launch had the device to itself
        int last_use = 0; uint32_t last_sx = 0, last_sy = 0;        // the latest launch: 0 natural order, 1 an order of its own view, 2 a carried one (blok_hip_last_order_use)
        int chosen = -1;                                    // the slot the latest launch walked in (-1: none)
    } order;
    // list launches, rectangle frames: clocks per wave tile of the last frame of this launch geometry, and the camera they were measured under (trace_kernels.h: cost classes)
    blok::DeviceArray<uint32_t> d_list_cost; uint32_t list_cost_key[6] = {};
    blok_camera list_prev_cam{}; bool list_has_prev_cam = false;
    bool list_classes = true;           // blok_hip_set_list_classes
    uint32_t* debug_clocks = nullptr;   // blok_hip_set_debug_wave_clocks (caller's device memory)
    int launch_form = blok::kFormAuto;  // blok_hip_set_fused (launch_policy.h: LaunchForm)
    int last_launch_kind = -1;          // launch_policy.h: LaunchKind of the latest rectangle / tile launch (blok_hip_last_launch_kind)
    uint32_t frame_parts = 32, frame_chunk = 1;      // FrameQueue::n_parts / chunk (BLOK_FRAME_PARTS / BLOK_FRAME_CHUNK override, for experiments)
    int cu_count = 0;
    int frame_blocks_per_cu[2][16] = {};   // [mode][levels], 0 = not asked yet
    // TAA jitter of the next frames' primary rays, in pixels (blok_hip_set_taa_jitter); blok_hip_draw_frame_rt sets it per frame
    float jitter_px[2] = {0.0f, 0.0f};
    bool rt_taa_jitter = true;          // PostProcess::Settings::enableTAA (renderer_postprocess.hpp:103)
    // instanced voxel models (api_instances.hip): descriptors indexed by model id (a destroyed model keeps its slot with nodes == null),
    // the owners of their arrays under the same index, their device copy, and the LDS stack slots the deepest live model needs
    struct Models {
        // (with what the kernels never look at and their descriptor has no room for: the arrays' lengths, and the model's box in its own
        // voxels, of which the descriptor's box is the 2^e-fold)
        struct Arrays {
            blok::DeviceArray<uint4> nodes; blok::DeviceArray<uint32_t> materials;
            uint32_t n_nodes = 0, n_materials = 0;
            int32_t box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
        };
        std::vector<blok::ModelDesc> desc;
        std::vector<Arrays> own;
        blok::DeviceArray<blok::ModelDesc> d_desc;      // the kernels' copy: nodes = null also where vs * 2^e is above the limit ...
        float uploaded_voxel_size = 1.0f;               // ... for this voxel size of the world (models_follow_voxel_size)
        uint32_t stack_levels = 1;
        // emissive models as lights (blok_hip.h): a model's table under its id (shorter than desc while the later models have none), the
        // number of tables, and the kernels' copy, one entry per model id (written by upload_model_lights behind every change)
        struct LightTable { blok::DeviceArray<blok_light> table; uint32_t n = 0; };
        std::vector<LightTable> lights;
        uint32_t n_light_tables = 0;
        blok::DeviceArray<uint32_t> d_glows;            // the emissive set of the installed material table (lights_core.h: kSetWords words), kept while any model has a table
        blok::DeviceArray<blok::lights::ModelLightTable> d_lights; uint32_t n_lights_uploaded = 0;      // (models made since have no table: ids at or beyond it count as none)
    } models;
    // timing
    blok::Event ev_begin, ev_end;
    bool timing = false, timed = false;
    std::string error;
};

namespace blok_api {

int set_error(blok_hip_ctx* ctx, int status, const std::string& msg);

#define BLOK_HIP_TRY(ctx, call)                                                                    \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_error(ctx, e_ == hipErrorOutOfMemory ? BLOK_ERR_OOM : BLOK_ERR_HIP,         \
                             std::string(#call) + ": " + hipGetErrorString(e_));                   \
    } while (0)

// A call that fills `owner` right after a reserve() replaced it (a zero fill, a first upload): if it fails, the owner is emptied first, so
// that the next call starts over and no kernel ever reads words nobody wrote.
#define BLOK_HIP_TRY_FILL(ctx, owner, call)                                                        \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (owner).reset();                                                                       \
            return set_error(ctx, e_ == hipErrorOutOfMemory ? BLOK_ERR_OOM : BLOK_ERR_HIP,         \
                             std::string(#call) + ": " + hipGetErrorString(e_));                   \
        }                                                                                          \
    } while (0)

// The one device block of a blocking entry, staged: the entry names its segments (each starts on a 256-byte boundary), stage() allocates
// the block once and uploads the non-empty inputs, the entry makes its device call with at() / wanted(), and collect() downloads the
// outputs the host asked for, synchronises the device and names a HIP failure after the entry.  The block is freed with the object.
class StagedBlock {
public:
    template <class T> struct Seg { size_t part; };
    template <class T> Seg<T> input(const T* host, size_t count) { return {add(count * sizeof(T), host, nullptr)}; }
    template <class T> Seg<T> output(T* host, size_t count) { return {add(count * sizeof(T), nullptr, host)}; }       // host may be null
    template <class T> Seg<T> scratch(size_t count) { return {add(count * sizeof(T), nullptr, nullptr)}; }
    template <class T> T* at(Seg<T> s) const { return reinterpret_cast<T*>(d.get() + parts_[s.part].offset); }
    // ... of an output: null where the host asked for none
    template <class T> T* wanted(Seg<T> s) const { return parts_[s.part].down ? at(s) : nullptr; }

    int stage(blok_hip_ctx* ctx, const char* entry) {
        size_t bytes = 0;
        for (Part& p : parts_) { p.offset = bytes; bytes += (p.bytes + 255u) / 256u * 256u; }
        BLOK_HIP_TRY(ctx, d.reserve(bytes, blok::FreeAfter::nothing()));
        hipError_t e = hipSuccess;
        for (const Part& p : parts_)
            if (e == hipSuccess && p.up && p.bytes) e = hipMemcpy(d + p.offset, p.up, p.bytes, hipMemcpyHostToDevice);
        return report(ctx, entry, e);
    }
    // rc: what the device call returned.  Its failure wins over a HIP failure here; the device is synchronised either way.
    int collect(blok_hip_ctx* ctx, const char* entry, int rc) {
        hipError_t e = hipSuccess;
        for (const Part& p : parts_)
            if (rc == BLOK_OK && e == hipSuccess && p.down) e = hipMemcpy(p.down, d + p.offset, p.bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        return rc != BLOK_OK ? rc : report(ctx, entry, e);
    }

private:
    struct Part { size_t offset, bytes; const void* up; void* down; };
    size_t add(size_t bytes, const void* up, void* down) { parts_.push_back(Part{0, bytes, up, down}); return parts_.size() - 1; }
    static int report(blok_hip_ctx* ctx, const char* entry, hipError_t e) {
        if (e == hipSuccess) return BLOK_OK;
        return set_error(ctx, e == hipErrorOutOfMemory ? BLOK_ERR_OOM : BLOK_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e));
    }
    std::vector<Part> parts_;
    blok::DeviceArray<unsigned char> d;
};

// Is `model` the id of a live model of the context's store?
inline bool known_model(const blok_hip_ctx* ctx, uint32_t model) { return model < ctx->models.desc.size() && ctx->models.desc[model].nodes; }

void free_world(blok_hip_ctx* ctx);
void clear_lights(blok_hip_ctx* ctx);                   // api_volume.hip: no light table from here on
void clear_model_lights(blok_hip_ctx* ctx);             // api_instances.hip: no model has a light table from here on
void adopt_tree(blok_hip_ctx* ctx, const blok::GpuTree& gpu);
int install_materials(blok_hip_ctx* ctx, const blok_material* materials, size_t n_materials);
int install_tree(blok_hip_ctx* ctx, const blok::HostTree& tree, const blok_material* materials, size_t n_materials);
int rebuild_sun_map(blok_hip_ctx* ctx);
int update_sun_map(blok_hip_ctx* ctx, const int32_t lo[3], const int32_t hi[3], bool same_lattice, bool may_add);
int ensure_frame(blok_hip_ctx* ctx, size_t records);
blok::TraceArgs base_args(const blok_hip_ctx* ctx, const blok_camera* cam);
int prepare_beam(blok_hip_ctx* ctx, blok::RayMode mode, blok::TraceArgs& args, hipStream_t stream, uint32_t tiles_of_rank, uint32_t* n_beams);
int prepare_queue(blok_hip_ctx* ctx, blok::RayMode mode, const blok::TraceArgs& args, hipStream_t stream, uint32_t n_beams, blok::FrameQueue* queue, uint32_t* n_blocks);
int check_trace(blok_hip_ctx* ctx, const blok_camera* cam);
// The instances of an instanced path launch (null: world only): a device table of n records and the optional id plane.
struct PathInstances { const blok_instance* table; uint32_t n; uint32_t* ids; };
// The poses of a posed path launch (null, or n == 0: none): a device table of n records, traced behind the instances.
struct PathPoses { const blok_pose* table; uint32_t n; };
// With a light table installed (ctx->lights.n >= 1) every launch runs the lit kernel, whatever tables the entry brought.  With a model light
// table (ctx->models.n_light_tables >= 1) every launch that brings instances runs the placed lit kernel behind the launch's prefix kernel.
int launch_path_frame(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                      uint32_t max_bounces, uint32_t frame_index, const blok::PathArgs& planes, void* hip_stream, const PathInstances* inst = nullptr,
                      const PathPoses* poses = nullptr);
// api_launch.hip
int beam_buffer(blok_hip_ctx* ctx, hipStream_t stream, size_t n, float** out);
int order_buffers(blok_hip_ctx* ctx, uint32_t blocks, hipStream_t stream);
int beam_cache_buffers(blok_hip_ctx* ctx);              // at create / resize: the slots' buffers for the frame size (a blocking entry)
int beam_list_buffers(blok_hip_ctx* ctx);               // ... and the packed walk's, when it is switched on (a blocking entry)
void settle_beam_cache(blok_hip_ctx* ctx);               // behind a device-wide synchronisation: every slot's producer has finished
int live_list(blok_hip_ctx* ctx, blok::TraceArgs& args, hipStream_t stream, uint32_t n_searches, uint32_t per_search);
int launch_timed(blok_hip_ctx* ctx, blok::RayMode mode, blok::TraceArgs args, uint32_t blocks, hipStream_t stream, uint32_t tiles_of_rank = 0,
                 const blok::TileFrames* frames = nullptr);
// api_volume.hip: the one place the context's snapshots are freed (a new volume, a destroyed one, the context's end)
void free_volume_snapshots(blok_hip_ctx* ctx);
// ... and the one place they follow a scroll of the box by `delta`, or are freed where they cannot (blok_hip_volume_scroll)
void scroll_volume_snapshots(blok_hip_ctx* ctx, const int32_t delta[3]);
// api_instances.hip
// The limits of blok_hip.h for a host table: BLOK_OK or BLOK_ERR_INVALID_ARG naming the first instance that breaks one.
int check_instance_table(blok_hip_ctx* ctx, const blok_instance* inst, uint32_t n);
// The volume entries' rule for a model id they are handed (a placement's, a scatter entry's): BLOK_ERR_UNSUPPORTED for a live model whose
// scale is not 0 (baking a scaled model is not built), else BLOK_OK.  An unknown id is the caller's other checks' business.
int refuse_scaled_model(blok_hip_ctx* ctx, const char* op, uint32_t model);
// The tail of every entry that makes a model (blok_hip_model_create, blok_hip_volume_capture_model): takes the two device arrays into the
// store under the next id, refreshes the device copy of the descriptors and the stack depth the kernels need.  Synchronises the device.
// On failure the arrays are freed (they are `own`'s from the call on) and no id is consumed.
int add_model(blok_hip_ctx* ctx, const blok::ModelDesc& m, blok_hip_ctx::Models::Arrays own, uint32_t* out_model);
// After a world with another voxel size was installed: the device copy of the descriptors is written again if some scaled model's voxel
// size has come above or below the limit with it (it then waits for the device first).  Nothing to do while every model has scale 0.
int models_follow_voxel_size(blok_hip_ctx* ctx);
// The id plane and both tables of an object-motion pass (instance_motion.h) with the context's model store and voxel size.
blok::MotionTables motion_tables(const blok_hip_ctx* ctx, const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev,
                                 uint32_t n_prev);
// Null tables with non-zero counts and the pose count's limit, for device tables (the messages every placed entry gives).
int check_placed_device_tables(blok_hip_ctx* ctx, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses);
// The poses' motion records of a posed motion pass (pose_motion.h), built on `stream` into its scratch: *out is null when n_cur == 0.
int prepare_pose_motion(blok_hip_ctx* ctx, const blok_pose* cur, uint32_t n_cur, const blok_pose* prev, uint32_t n_prev, hipStream_t stream,
                        const blok_pose_motion** out);
// ... and its tables: motion_tables with the records of n_cur_poses poses.
blok::PoseMotionTables pose_motion_tables(const blok_hip_ctx* ctx, const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev,
                                          uint32_t n_prev, const blok_pose_motion* records, uint32_t n_cur_poses);
// blok_hip_posed_motion_device behind its checks and the records' build.
int posed_motion_pass(blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* world_pos_dev, const blok::PoseMotionTables& tables,
                      const float prev_view_proj[16], uint16_t* motion_h_dev, float* motion_dev, hipStream_t stream);
void forget_device_activity(const blok_hip_ctx* ctx, bool one_stream = false, hipStream_t stream = nullptr);
bool rect_inside(const blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
// The root's assembly of a sparse exchange (blok_hip_scatter_*_tile_frames_device): the ranks' buffers either side by side in
// `gathered_dev` or, rank_ptrs_dev != null, wherever a device array of n_ranks pointers says (peer-mapped memory of other devices).
int scatter_frames(blok_hip_ctx* ctx, bool codes, const void* gathered_dev, const void* const* rank_ptrs_dev, uint32_t n_ranks, size_t rank_stride_words,
                   uint32_t tile, uint32_t max_records, uint32_t n_frames, void* out_frames_rgba_dev, void* tile_state_dev, void* hip_stream);

}  // namespace blok_api
#endif
