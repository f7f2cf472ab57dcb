/* blok_hip_debug.h — diagnostics, test hooks and tuning knobs of libblok_hip.so.
 *
 * NOT part of the drop-in surface: a reference-side binding includes blok_hip.h only, whose entries are the ones
 * SURVEY.md section 8(b) derives from CudaTracer (blok/include/cuda_tracer.hpp:23-58) and Renderer (blok/include/renderer.hpp:29-77).
 * What is here has no reference counterpart: switches between launch forms and schedules that were measured against each other
 * (every setting gives the same frames), read-backs the tests and the experiment scripts use, and hooks that force
 * paths a working system rarely takes.  The library exports them all the same; nothing here is needed to render.
 */
#ifndef BLOK_HIP_DEBUG_H
#define BLOK_HIP_DEBUG_H

#include "blok_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ structure build */
/* The traversal structure is built on the device (blok_amd/csrc/hip/gpu_build.hip).  Worlds outside what those
 * kernels cover (empty worlds, sub-chunks smaller than 4 voxels or of mixed sizes) are built by the general host
 * path instead; blok_hip_set_host_build(ctx, 1) forces that path (used by tests to compare the two). */
int blok_hip_set_host_build(blok_hip_ctx* ctx, int enabled);
int blok_hip_world_built_on_device(const blok_hip_ctx* ctx);   /* 1 / 0 */
/* Copies the device-resident structure back: n_tree_nodes 16-byte nodes and n_voxels material ids
 * (see blok_world_stats); either output may be NULL.  For tests and debugging. */
int blok_hip_download_tree(const blok_hip_ctx* ctx, void* nodes_out, size_t node_capacity,
                           uint32_t* materials_out, size_t material_capacity);

/* ------------------------------------------------------------ resident volume */
/* Diagnostic: 0 = the next blok_hip_volume_create keeps its brick masks in row-major order and rebuilds by scanning, keying and sorting
 * all bricks (the general path, ~2.4 ms for a 1024^3 box); 1 (default) = bricks indexed by their tree key under a pyramid of occupancy
 * words, rebuilt by scans over the pyramid (~0.2 ms), whenever the box's 64^(levels-1) mask words are affordable.  Both give the same
 * node and material arrays, byte for byte (tests/test_brush.py). */
int blok_hip_set_volume_layout(blok_hip_ctx* ctx, int keyed);
/* Diagnostic / test hook: how the resident volume's brick masks have been refreshed since blok_hip_volume_create, one count per refresh
 * (an upload, a brush, a set_voxels call, ...): [0] keyed layout, the path of an edit — a wave per brick of the edit's range and the
 * occupancy words above it in one workgroup — [1] keyed layout, the path of a range of more than 65 536 bricks or 4096 level-2 cells —
 * a lane per brick, a launch per level — [2] general layout.  Every path computes the same masks (tests/test_volume_rebuild_gpu.py). */
int blok_hip_volume_refresh_counts(blok_hip_ctx* ctx, uint64_t out_counts[3]);
/* Diagnostic: how the device reached the last flood snapshot (blok_hip_volume_flood_field): out_counts[0] = the rounds run (launches over a
 * non-empty list of active bricks), [1] = the bricks taken off those lists, summed.  Both depend on how the device scheduled the waves,
 * which is why neither is part of blok_flood_info.  BLOK_ERR_INVALID_ARG without a snapshot. */
int blok_hip_volume_flood_counters(blok_hip_ctx* ctx, uint64_t out_counts[2]);

/* ------------------------------------------------------------ path kernel */
/* Scheduling knob of the path kernel (no reference counterpart): 0 = every lane walks whatever ray it has pending; 1 = a wave walks
 * one kind of ray at a time (primary, else shadow, else bounce); 2 = one kind at a time and the oldest sample first, so the
 * pixels of a wave stay in step sample by sample.  Per-lane work and results are identical in these three (tests/test_paths.py).
 * 3 (default, round 4) = 2 and the bounce rounds' tail pool (from 4 samples per pixel on, two bounces or more, rays from the root): a round
 * of last-segment rays is cut off after 24 trips of the walk, the rays still walking are parked and walked 64 at a time in rounds of
 * their own, and their terms reach the pixels' sums later — the same terms in another order (colour inside a hundredth of the test
 * tolerance of mode 2's, G-buffer bit-identical, launches deterministic; 64 spp at 4K 35 -> 30 ms). */
int blok_hip_set_ray_batching(blok_hip_ctx* ctx, int enabled);
/* Where the path kernel's walks start (round 4; no reference counterpart: raygen.rgen:217-229, 282-298 hand every ray to traceRayEXT).
 * wave_tile_beam (default 1): every 8x8-pixel wave tile searches a start parameter of its own once per launch, on top of its 32x32 beam
 * tile's, from 8 samples per pixel on: all spp primary rays of its pixels start behind it (4K over 1024^3, 64 spp: 46.7 -> 44.5 ms; 8 spp: 6.06 -> 5.90;
 * 2 spp would lose: 1.68 -> 1.82).
 * resume_from_anchor (default 0 — built, exact, and slower): a pixel's rays enter the walk from the ancestors of its latest reported
 * voxel — the shadow and bounce rays start a hair off it (raygen.rgen:284, :376), the next sample's primary ray ends near it — instead
 * of descending from the root: the start voxel is found with the walk's own plane rule and verified, the lowest common ancestor comes
 * from an LDS copy of the hit's ancestor stack, and ancestors that hold nothing the ray can still reach are left at once
 * (blok_amd/csrc/hip/trace_core.h: walk_resume).  It takes 13 % off the secondary rays' iterations and gives nothing back: the descents it
 * saves are the ones every lane of the wave takes together, the set-up it adds runs per ray (profiles/r04_paths_start_ab.txt).  Kept as a
 * second instantiation of the kernel, so the default carries none of its state.
 * Frames are identical bit for bit in all four combinations (tests/test_paths.py). */
int blok_hip_set_path_start(blok_hip_ctx* ctx, int resume_from_anchor, int wave_tile_beam);
/* "Last occluder" map of the path kernel's shadow rays (no reference counterpart): all shadow rays share the shader's constant sun
 * direction (raygen.rgen:142,185), so with every world the backend records, per 4-voxel texel of the plane perpendicular to
 * it, how far along that direction voxels exist at all; a shadow ray's tmax is capped there (rays above the last occluder skip
 * their walk).  Results are identical with and without it (tests/test_paths.py).  Default on. */
int blok_hip_set_sun_map(blok_hip_ctx* ctx, int enabled);

/* ------------------------------------------------------------ frame launches: pre-pass, order, launch form */
/* Beam pre-pass of the frame kernels (no reference counterpart; the reference culls per ray in Vulkan RT hardware,
 * blok/src/renderer_raytracing.cpp:15-254): before a rectangle / tile launch, one wave per beam_tile_pixels^2 pixels finds a
 * conservative start parameter for that tile's rays, and tiles whose frustum meets no voxel are written as misses without
 * a walk.  Results are identical with and without it (tests/test_gpu_parity.py).  0 turns it off; default 32. */
int blok_hip_set_beam(blok_hip_ctx* ctx, uint32_t beam_tile_pixels);
/* Longest-first scheduling of the walk for a camera at rest (default: on, re-sorted every 8 launches; rectangle launches of at least
 * 4096 wave tiles behind the pre-pass, static launch forms 0, 2, 3): every wave of the walk leaves the clocks it spent; every N-th launch a
 * 16-bit radix sort of a snapshot of those costs (129 600 keys at 4K) follows the frame on its stream, a later launch adopts the finished
 * order, and the walk's workgroups take their tiles in it, so the long grazing-ray waves — each a quarter of the launch long, whatever
 * their priority — start first instead of forming the launch's tail.  The order also tells which tiles need a walk wave at all: launch
 * forms 2 and 3 dispatch walk waves for the tiles that walked when the order was made only, and a tile that has become live since is
 * walked by its search wave.  An order of a view's own clocks is used for that view only (the same camera up to float noise: 0.0006 degree,
 * a thousandth of a voxel): ordering by a stale cost is no better than row-major even one frame later, and the prefix of a view that has crept
 * away leaves the new silhouettes to the search waves (profiles/r03_stale_cost_order_experiment.txt, r03_moving_order_solitary_frames.txt);
 * any camera in motion, however slow, gets an order of another kind (blok_hip_set_moving_order below).
 * A view at rest is re-sorted ever less often (the interval doubles up to 64 launches).
 * Pure scheduling: any order gives the same frame (tests/test_gpu_parity.py).  No reference counterpart
 * (renderer_raytracing.cpp:666-685 leaves scheduling to the driver).  0 = off; N > 0 = re-sort every N launches.
 * Measured (4K over 1024^3, one frame at a time): walk alone 216 us row-major, 168 us in this order. */
int blok_hip_set_tile_ordering(blok_hip_ctx* ctx, int resort_every_n_frames);
/* The same for a camera in MOTION (round 3; default on): the heavy tiles of the next frame are near the heavy tiles of this one, not on
 * them.  After a frame that had the device to itself (and whose predecessor had too), a counting sort in three small launches keys every tile by the largest clocks within a few tiles of it (2-8, sized
 * by what the previous shift left over), and the next launch carries that order to its own view by ONE whole-tile shift of the screen
 * — entry (tx, ty) names tile (tx + sx, ty + sy) modulo the grid, still a permutation — computed on the host from the two cameras and
 * the depth range of the frame the order was measured on (blok_amd/csrc/hip/launch_policy.h: plan_shift).  Used while what the shift
 * leaves over (parallax, the stretch of a rotation towards the screen's edge) stays within twice the dilation; beyond that, and beside
 * frames in flight on other streams, a moving camera's launches keep row-major order as before.  Pure scheduling, as above.
 * Measured (4K over 1024^3, walk alone, camera orbiting by 1-2 degrees per frame): 209-216 us row-major, 171-178 us carried order, 167-170
 * us in the order of the frame's own clocks (profiles/r03_moving_order_experiment.txt).  0 = off. */
int blok_hip_set_moving_order(blok_hip_ctx* ctx, int enabled);
/* The same scheduling for a RANK's tile launches (blok_hip_trace_tiles_device / _tile_frames_device, 4096 wave tiles per frame or more;
 * round 4, default on): the rank's wave tiles are walked longest first and, in the automatic launch form, walk workgroups are dispatched for
 * the live prefix only — for a view at rest (all cameras of a several-frame launch the same view): a whole-tile shift of the screen does
 * not map a rank's round-robin share of the tiles onto itself, so a camera in motion keeps the natural order there.  Pure scheduling
 * (tests/test_gpu_parity.py).  0 = off (round 3's launches). */
int blok_hip_set_rank_tile_ordering(blok_hip_ctx* ctx, int enabled);
/* Diagnostic / test hook: the counting sort that follows a moving camera's frames, run on the caller's host arrays — cost[tiles_x * tiles_y]
 * (row-major wave tiles), dilation radius <= 8, optionally n_beams start parameters (>= 1e38 = none) — and read back: out_order (tiles by
 * descending class of the largest cost within `radius` tiles: 64 classes, four to the octave from 256 up, 0 = nothing near; within a class by
 * 16x16-tile block of the grid, row-major, then row-major inside the block), its inverse, *out_live = entries of classes > 0, and
 * out_depth_sums3 = (count, sum, sum of squares) of 1 / max(start parameter, 1) over the beam tiles that have one (may be null). */
int blok_hip_debug_class_order(blok_hip_ctx* ctx, const uint32_t* cost_host, uint32_t tiles_x, uint32_t tiles_y, uint32_t radius, const float* beam_host, uint32_t n_beams,
                               uint32_t* out_order_host, uint32_t* out_rank_of_host, uint32_t* out_live, float* out_depth_sums3);
/* Diagnostic: wave tiles the search waves of the latest TIMED prefix launch (blok_hip_set_timing) walked themselves (tiles live now that had
 * no walk workgroup: a changed view); read it after synchronising.  -1 = null context or nothing allocated yet. */
int64_t blok_hip_last_fallback_tiles(const blok_hip_ctx* ctx);
/* Test hook: every launch that walks in an order (of either kind) applies this whole-tile shift to it (taken modulo the launch's grid)
 * instead of the one the cameras give — any shift of any order is a permutation of the tiles, so the frames must not change. */
int blok_hip_debug_force_order_shift(blok_hip_ctx* ctx, int enabled, uint32_t shift_x, uint32_t shift_y);
/* Diagnostic: what the latest rectangle launch walked in — 0 row-major order, 1 an order of its own view, 2 an order carried over from
 * another view by the shift returned through the pointers (wave tiles, modulo the grid; either may be null); -1 = null context. */
int blok_hip_last_order_use(const blok_hip_ctx* ctx, int32_t* out_shift_x, int32_t* out_shift_y);
/* Diagnostic: the most walk waves a launch over the order's live prefix dispatches (0 = no limit).  Whatever is cut off is walked by the
 * search waves; the frame is the same (the tests use it to exercise that path). */
int blok_hip_set_joint_prefix_limit(blok_hip_ctx* ctx, uint32_t max_walk_waves);
/* Who writes the miss pixels of the tiles the pre-pass found empty (two-launch form): 1 (default) = the walk launch's waves of
 * those tiles — they are launched anyway and have nothing else to do — 0 = the pre-pass wave of the tile, 1 024 pixels each, which
 * puts ~120 MB of stores on the pre-pass's critical path (4K, 73 % sky).  Never changes a result. */
int blok_hip_set_miss_writer(blok_hip_ctx* ctx, int in_walk);
/* The beam bounds of a view at rest: 1 = a rectangle launch of the automatic form whose camera, rectangle,
 * beam settings and world are those of the launch before it, byte for byte, leaves its start parameters in one of four slots of the
 * context, and every later launch of that view walks from them without searching; 2 (default) = as 1, and the view's K-th such launch
 * (blok_hip_set_beam_refine_after) issues, behind its walk, one search per 8 x 8 wave tile of its live beam tiles, whose answers the
 * launches after it walk from — a shorter walk, and none for a wave tile that is empty by its own search (only where the beam tile is a
 * whole number, more than one, of wave tiles per side); 0 = every launch searches (the launches of a library without the cache, one for
 * one); 3 = as 2, and the view's walked pixels are regrouped by the length of their walks: the N-th launch that walks from the finer bounds
 * (blok_hip_set_beam_list_after) also counts every ray's trips and issues, behind its walk, the build of a list — per 32 x 32 pixels,
 * the pixels by descending count, 64 to a group — and of a table of the groups, heaviest first; the first later launch that finds the build
 * finished walks one group per wave from then on, with neither the view's order nor its live prefix (rectangles up to 65 534 pixels a side;
 * allocates the lists' buffers, about 17 bytes per pixel of the frame, and waits for the device); 4 (default since ABI 1.21) = as 3, and
 * the count launch also leaves, for every ray, the ray parameter at which it entered the cell its answer lies in (a hit's t; the entry of a
 * miss's last cell inside the world) and the trips of the walk from the root started there (at most the tree's levels); the list is sorted by
 * those, which leaves it nearly in pixel order, and carries every entry's start beside it; a packed launch whose jitter, tmin and tmax are the
 * count launch's, bit for bit, walks every listed ray from its own start — from the root to that cell — and any other packed launch of the
 * view walks the same list from the finer bounds as under 3 (another 21 bytes per pixel of the frame); 5 (default since ABI 1.27) = as 4,
 * and the count launch also leaves, for every ray, the tree node that walk from its own start ends in — the brick of a hit, the parent of a
 * miss's last cell — with that cell's level, as one word, carried beside every entry's start; a packed launch that walks from the starts then
 * loads that node directly and makes the walk's last trip alone, and a wave with a ray this does not settle (a ray of a live tile that misses
 * the world box) walks as under 4 (another 8 bytes per pixel; a tree of 2^29 nodes or more runs as 4).  In every case the slots are emptied.
 * blok_hip_last_launch_kind goes on reporting the form the launch policy chose for the
 * device's state, also for a launch that walked from kept bounds (a plain trace launch).  Never changes a result. */
int blok_hip_set_beam_cache(blok_hip_ctx* ctx, int mode);
/* N: a refined view's rays are counted by its N-th launch from the finer bounds (0 = the default, 16: what the count launch and the build
 * cost over what a packed frame gains), or the first after it at which no other view's build is in flight. */
int blok_hip_set_beam_list_after(blok_hip_ctx* ctx, uint32_t hits);
/* The side of the packed list's areas in pixels (32): an area's stretch of the list has its square of entries, its share of the table a
 * 64th of that in words. */
uint32_t blok_hip_pack_area(void);
/* Launches so far that counted and issued a list's build (at most one per set of finer bounds). */
int blok_hip_beam_cache_list_builds(const blok_hip_ctx* ctx, uint64_t* out_builds);
/* Read-back of the list: *out_state = 0 the latest rectangle launch had nothing to do with one, 1 it counted and issued the build, 2 it
 * walked packed; for states 1 and 2, *out_n_areas = the areas of its rectangle (blok_hip_pack_area pixels a side: 32; row-major), *out_n_groups = the table's non-empty
 * groups, and into the buffers that are given: the list, 1 024 entries per area (x | y << 16 in the rectangle, 0xFFFFFFFF = padding, entries
 * beyond an area's last group undefined); the table, 16 words per area, of which the first *out_n_groups are (largest trip count of the
 * group + 1) << 20 | area * 16 + group of the area, descending, and the rest 0; the trips of the context's latest count launch, one byte per
 * pixel of the rectangle, defined for the listed pixels (those of state 1's launch; a later count launch for another view overwrites them).
 * Waits for the device; launches nothing and changes nothing.  Any pointer may be null. */
int blok_hip_beam_cache_download_list(blok_hip_ctx* ctx, int* out_state, uint32_t* out_n_areas, uint32_t* out_n_groups, uint32_t* out_list_host_or_null, size_t list_capacity,
                                      uint32_t* out_table_host_or_null, size_t table_capacity, uint8_t* out_trips_host_or_null, size_t trips_capacity);
/* Mode 4's read-back, for the slot blok_hip_beam_cache_download_list reads: *out_state = 0 the latest rectangle launch had nothing to do with
 * starts, 1 it counted them or walked from them, 2 it walked packed under another start key (from the finer bounds); and into the buffers
 * that are given, for a slot whose list carries starts: every entry's start parameter in list order, 1 024 floats per area (defined where the
 * list holds an entry that is not padding), and the restarted trips of the context's latest count launch, one byte per pixel of the
 * rectangle, defined for the listed pixels.  Waits for the device; launches nothing and changes nothing.  Any pointer may be null. */
int blok_hip_beam_cache_download_starts(blok_hip_ctx* ctx, int* out_state, float* out_starts_host_or_null, size_t starts_capacity, uint8_t* out_restarts_host_or_null,
                                        size_t restarts_capacity);
/* Packed launches so far that walked from the starts, and that found another start key; either pointer may be null. */
int blok_hip_beam_cache_start_counters(const blok_hip_ctx* ctx, uint64_t* out_from_starts, uint64_t* out_other_key);
/* Mode 5's read-back, for the same slot: *out_has_nodes = 1 if its list carries node words; and into the buffers that are given, for such a
 * slot: every entry's word in list order, 1 024 per area (defined where the list holds an entry that is not padding), and the words of the
 * context's latest count launch, one per pixel of the rectangle, defined for the listed pixels.  A word is the index of a node of the tree
 * (blok_hip_download_tree's order) in its low 29 bits and the level of the cell of the ray's last trip — a child of that node — in its top
 * three; 0xFFFFFFFF for a ray that made no trip.  Waits for the device; launches nothing and changes nothing.  Any pointer may be null. */
int blok_hip_beam_cache_download_nodes(blok_hip_ctx* ctx, int* out_has_nodes, uint32_t* out_entry_words_host_or_null, size_t entry_capacity, uint32_t* out_pixel_words_host_or_null,
                                       size_t pixel_capacity);
/* Packed launches so far that re-entered their rays at the node words (they count as launches from the starts too). */
int blok_hip_beam_cache_node_counters(const blok_hip_ctx* ctx, uint64_t* out_from_nodes);
/* How a packed launch (modes 3 and 4, a list with at least one group) writes the miss pixels of the wave tiles that are empty by the finer
 * bounds (ABI 1.24): 0 = a fill launch in front of the walk launch, as before; k >= 1 = ONE launch, in which the walk's
 * workgroups also write fill units — 64 consecutive pixels of a row of the rectangle, one to a lane — at most k to a workgroup, with
 * workgroups behind the walk's that only fill where the units need them (the default: BLOK_PACKED_FILL in trace_kernels.h).  Every other
 * launch — the count launch, an all-sky view's, modes 0 to 2, tiles, captures — is as before.  Never changes a result. */
int blok_hip_set_packed_fill(blok_hip_ctx* ctx, uint32_t units_per_wave);
/* Packed launches so far that were issued as one launch, and the workgroups of those launches that only filled; either pointer may be null. */
int blok_hip_packed_fill_counters(const blok_hip_ctx* ctx, uint64_t* out_one_launch_frames, uint64_t* out_fill_only_workgroups);
/* Launches so far that walked from kept bounds (hits) and that searched into a slot (fills); either pointer may be null. */
int blok_hip_beam_cache_counters(const blok_hip_ctx* ctx, uint64_t* out_hits, uint64_t* out_fills);
/* ... and that issued a view's finer searches behind their walk (at most one per fill; such a launch counts as a hit too). */
int blok_hip_beam_cache_refines(const blok_hip_ctx* ctx, uint64_t* out_refines);
/* K: a kept view's finer bounds are searched behind the walk of its K-th hit since it was filled (0 = the default, 16: what the searches
 * cost over what a frame gains from them), so that a camera which rests only briefly pays nothing for them. */
int blok_hip_set_beam_refine_after(blok_hip_ctx* ctx, uint32_t hits);
/* Read-back for the tests that check the kept bounds as numbers: *out_action = what the latest rectangle launch did — 0 it searched (or ran
 * without a pre-pass), 1 it searched into a slot, 2 it walked from a slot without searching — *out_n_beams = its beam tiles (0 for action
 * 0), and with a buffer of `capacity` floats, for actions 1 and 2, that slot's start parameters, row-major as blok_hip_beam_prepass returns
 * them.  Waits for the device; launches nothing and changes nothing.  Any pointer may be null.  (blok_hip_beam_prepass itself never looks
 * at the slots: it always searches, whatever blok_hip_set_beam_cache says.) */
int blok_hip_beam_cache_download(blok_hip_ctx* ctx, int* out_action, uint32_t* out_n_beams, float* out_t0_host_or_null, size_t capacity);
/* The same for the finer bounds of that slot (blok_hip_beam_cache_download goes on returning the beam tiles' bounds): *out_state = 0 the
 * latest rectangle launch had nothing to do with them, 1 it issued their searches behind its walk, 2 it walked from them; *out_n_tiles =
 * the 8 x 8 wave tiles of its rectangle (0 for state 0), and for states 1 and 2 their start parameters, row-major: >= 3e38 where the wave
 * tile's own search or its beam tile's found nothing, else the larger of the two bounds. */
int blok_hip_beam_cache_download_fine(blok_hip_ctx* ctx, int* out_state, uint32_t* out_n_tiles, float* out_t0_host_or_null, size_t capacity);
/* Node visits one beam search may spend (0 = the default, 256; searches average 35).  A search that runs out answers with the
 * lower bound over the cells it has not visited yet — valid, only less tight — never "none", so the frame is the same whatever
 * the budget (tests/test_gpu_parity.py runs with budgets of 1-64 visits against an unlimited search).  The pre-pass lasts as
 * long as its longest search, so the budget bounds its duration; too small a budget is paid for by the walk (beam.h). */
int blok_hip_set_beam_budget(blok_hip_ctx* ctx, uint32_t max_node_visits);
/* Launch form of a rectangle / tile frame (no reference counterpart: blok/src/renderer_raytracing.cpp:666-685 issues one
 * traceRaysKHR per frame); results are identical in every form (tests/test_gpu_parity.py):
 *   0  two launches: the beam kernel, then one walk wave per 8x8 pixels;
 *   1  one persistent launch with work queues: resident waves first take beam tiles, append the wave-sized sub-tiles of the live
 *      ones to per-part queues with an atomic reservation, then take walk tasks from those queues with one ticket each (measures
 *      slower on MI355X: same-address atomics run at 88 M/s);
 *   2  joint launch: the search waves and the walk waves are ONE grid, statically — workgroups are dispatched in index order, the
 *      searches first; a walk wave waits (bounded) only while its own tile's search is still running, so the chip starts walking
 *      when the first searches end, not when the last one does.  With a longest-first order in force (blok_hip_set_tile_ordering)
 *      walk waves are dispatched only for the tiles that walked when the order was made; a tile that has become live since is walked
 *      by its search wave.  Not for frames in flight on several streams: the waiting waves hold slots other frames' waves would
 *      use, and several joint launches in flight can wait for each other's searches in a circle until they give up (bounded; the
 *      frame stays exact);
 *   3  (default) automatic: 2 for a launch that has the DEVICE to itself — no frame launch of another stream or context of this
 *      process still pending on it — else 0, over the order's live prefix when an order is in force;
 *   4  list-fed joint launch: as 2, but the walk waves take their 8x8-pixel tiles from the frame's LIVE LISTS — a search that finds
 *      its beam tile live appends the tile's wave tiles, with their start parameter, to lists by cost class (blok_hip_set_list_classes;
 *      one 64-bit add per list reserves the slots), walk wave k of a list takes its entries k, k + n, ... — so no wave is launched for
 *      a dead tile and no pixel depends on an earlier frame: the walk grid is sized from the previous launch's lists (a hint only; any
 *      size walks every entry).  A walk wave that waits in vain (bounded, ~1 ms) leaves its entries to a clean-up launch behind the frame;
 *   5  the same lists in two launches: the beam kernel fills them, the walk waves take them (nothing waits).
 * Measured at 4K over 1024^3, a launch alone, camera at rest / orbiting by 1 degree per frame (profiles/r03_*): form 0 0.29 / 0.29 ms,
 * 2 with the order 0.20 / (no order) 0.24, 4 0.23 / 0.26, 5 0.26 / 0.29 — the lists lose to the measured order because entries arrive in
 * the order the searches finish, the heavy tiles last; they stay as the forms that need nothing from earlier frames. */
int blok_hip_set_fused(blok_hip_ctx* ctx, int enabled);
/* Health check of forms 1, 2 and 4: synchronises the device and returns how many waves ever gave up a bounded wait (0 in a working
 * system).  Form 1: for a queue entry (~0.5 s; frames since context creation may then be incomplete).  Form 2: for their tile's
 * search (such a wave starts at the ray origin instead: the frame is still exact).  Form 4: for a list entry (walked by the clean-up
 * launch: the frame is still exact). */
int blok_hip_frame_queue_stalls(blok_hip_ctx* ctx, uint32_t* out_stalled_waves);
/* Diagnostics of the pre-pass and the walk's scheduling (no reference counterpart).  blok_hip_beam_prepass: the pre-pass alone over a
 * rectangle — per beam tile (row-major, blok_hip_set_beam pixels each) its start parameter (>= 3e38 = no ray of the tile can hit
 * anything) and, optionally, the node visits its search spent — to host arrays of `capacity` elements.
 * blok_hip_trace_wave_tiles_device: walks exactly the listed 8x8-pixel wave tiles of the rectangle (index = row * ceil(w / 8) + column),
 * walk workgroup j taking entry j, each ray starting at its tile's t0 (NULL = at the ray origin; a value beyond the true first hit
 * would lose it — use what blok_hip_beam_prepass returned for the tile's beam tile); pixels of tiles not listed are left as they are.
 * A frame assembled from the two equals blok_hip_trace_primary_device's (tests/test_gpu_parity.py).
 * blok_hip_set_debug_wave_clocks: device array of one word per wave tile that list-fed walk waves leave their clock count in (NULL = off). */
int blok_hip_beam_prepass(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                          float* out_t0_host, uint32_t* out_visits_host_or_null, size_t capacity);
int blok_hip_trace_wave_tiles_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                     const uint32_t* tiles_host, const float* t0_host_or_null, size_t n_tiles,
                                     void* out_hits_dev_or_null, void* out_rgba8_dev_or_null, void* hip_stream);
int blok_hip_set_debug_wave_clocks(blok_hip_ctx* ctx, void* clocks_dev_or_null);
/* Read-back of the shadow rays' last-occluder map (blok_hip_set_sun_map above) for the tests that check it as numbers: the map's frame
 * exactly as the kernels use it, in float32 — texel (iu, iv) covers [u0 + iu texel, u0 + (iu + 1) texel] x [v0 + iv texel, ...] of (u . p, v . p)
 * and holds an upper bound of s . p over the filled voxels of that column — and the bookkeeping of the edits since it was last tight
 * (api.hip: update_sun_map).  map_out_or_null receives the nu * nv floats, row iv after row iv - 1; capacity is in floats and is not looked
 * at without a buffer.  Launches nothing and changes nothing; it waits for every raise and tighten launch enqueued so far.  Without a map
 * (no world, an empty one, a voxel size other than 1) has_map is 0 and everything else of the struct is 0. */
typedef struct blok_sun_map_info {
    float    u[3], v[3], s[3];    /* orthonormal; s = the sun direction */
    float    u0, v0, texel;
    uint32_t nu, nv;
    uint32_t has_map;
    uint32_t loose_edits;         /* edits since the map was last made tight (or since their union went to the pending rectangle) */
    uint32_t tighten_pending;     /* 1: the texels [pending_u0, pending_u1] x [pending_v0, pending_v1] are still to be searched again */
    uint32_t pending_u0, pending_u1, pending_v0, pending_v1;
} blok_sun_map_info;
int blok_hip_sun_map_download(blok_hip_ctx* ctx, blok_sun_map_info* out_info, float* map_out_or_null, size_t capacity);
/* Which kernels the latest rectangle / tile launch of the context was issued as: 0 walk alone (no pre-pass), 1 two launches, 2 queues,
 * 3 joint, 4 list-fed joint, 5 beam launch + list-fed walk; -1 before the first launch (what form 3 chose; tests and diagnostics). */
int blok_hip_last_launch_kind(const blok_hip_ctx* ctx);
/* Cost classes of the list launches (rectangle frames; default on): walk waves leave the clocks they took per wave tile, and the next
 * frame's searches put every live wave tile into one of four lists by what its place on the previous frame's screen cost, heaviest
 * list first — so the waves of grazing rays, a quarter of the launch long each, start first instead of forming its tail.  Only the
 * order depends on the previous frame; 0 = one list in the order the searches finish.  Never changes a result. */
int blok_hip_set_list_classes(blok_hip_ctx* ctx, int enabled);

/* ------------------------------------------------------------ several devices */
/* Diagnostic: deny != 0 = behave as if the root had no peer access to the other devices (sparse-pull unavailable, mode 1 refused, every
 * call takes the dense exchange over blok_hip_multi_transport); 0 = back to what the node really offers.  The frames are the same. */
int blok_hip_multi_debug_deny_peer_access(blok_hip_multi* m, int deny);

/* The instance BVH of the instanced path frame (tlas_core.h: TlasNode, 32 bytes each) for a device table of 1 .. 4096 instances: built on
 * the default stream and downloaded.  *out_count = the node count (header included); fails if capacity (nodes) is smaller. */
int blok_hip_debug_build_tlas(blok_hip_ctx* ctx, const blok_instance* instances_dev, uint32_t n_instances, void* out_nodes_host, size_t capacity,
                              uint32_t* out_count);

/* The pose BVH of the posed path frame (pose_tlas_core.h; the same TlasNode format; node 0's first word is the linear flag) for a device table
 * of 1 .. 4096 poses and the launch's camera (its position is one of the ray origins the leaf boxes are argued for): built on the default
 * stream and downloaded, as blok_hip_debug_build_tlas does. */
int blok_hip_debug_build_pose_tlas(blok_hip_ctx* ctx, const blok_camera* cam, const blok_pose* poses_dev, uint32_t n_poses, void* out_nodes_host,
                                   size_t capacity, uint32_t* out_count);
/* enabled = 0: posed path launches build no pose BVH and every ray loops over the pose table (the frame's definition); default 1.  The frames
 * are identical. */
int blok_hip_set_pose_tlas(blok_hip_ctx* ctx, int enabled);

/* The motion records of the posed motion passes (blok_hip.h, "Object motion for posed models"): the kernel that builds them, run on two HOST
 * tables (uploaded as they are, unchecked: a pose that fails a limit is untracked) with the context's model store; out_records_host takes
 * n_cur records.  Byte for byte blok_pose_motion_record's (blok_world.h).  Blocks.  BLOK_ERR_INVALID_ARG: a null table with a non-zero count,
 * 2^31 poses or more, a null output with n_cur > 0. */
int blok_hip_debug_pose_motion_records(blok_hip_ctx* ctx, const blok_pose* cur_host, uint32_t n_cur, const blok_pose* prev_host, uint32_t n_prev,
                                       blok_pose_motion* out_records_host);

/* Read-back of an instanced model (blok_hip_model_create, blok_hip_volume_capture_model), for the tests that pin a captured model byte for
 * byte: the node array (16 bytes per node, root first) and the material array (one id per voxel) as they lie in device memory, and the
 * model's lattice.  Either array pointer may be NULL (then its capacity is not looked at); out_info may be NULL.  BLOK_ERR_INVALID_ARG: an
 * unknown or destroyed model, or a capacity (in elements) below the model's count.  Blocking. */
typedef struct blok_model_info {
    uint32_t levels;              /* the tree covers 4^levels voxels per axis from origin */
    int32_t  origin[3];           /* local coordinate of the tree's corner */
    int32_t  lo[3], hi[3];        /* the box of the model's voxels, half open, local coordinates */
    uint64_t n_nodes, n_materials;
} blok_model_info;
int blok_hip_download_model(blok_hip_ctx* ctx, uint32_t model, void* nodes_out, size_t node_capacity, uint32_t* materials_out,
                            size_t material_capacity, blok_model_info* out_info);

#ifdef __cplusplus
}
#endif
#endif /* BLOK_HIP_DEBUG_H */
