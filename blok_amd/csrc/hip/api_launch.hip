// How a frame is launched (include/blok_hip.h: the trace entries; launch_policy.h: the decisions): who else is on the device, the
// orders cached per view and what keeps them (markers, sorts, shifts), the joint launch's slots, the list forms' buffers, and
// launch_timed, through which every rectangle / tile launch goes.  Split from api.hip in round 4.
#include "api_internal.h"
#include "beam.h"
#include <cstdlib>

namespace blok_api {

// ---- who else is using the device -----------------------------------------------------------------------------------------------
// A joint launch only pays when it has the device to itself (launch_policy.h), and "itself" is a property of the DEVICE, not of a
// context: two contexts on one device (two HipTracers; blok_hip_multi_* with an ordinal listed twice) must see each other's frames.
// So every frame launch leaves an event behind on its stream in a process-wide table per device, and a launch asks whether any OTHER
// (context, stream) of the device still has one pending.
namespace {
// Two markers per (context, stream), both recorded by the stream's own launches only (nothing here ever records on a stream other than
// the one being launched on: a caller may have destroyed it, or be capturing it into a graph): `last` = behind its latest frame launch;
// `held` = what `last` was when the context last asked for its launches to be remembered (hold_markers: the adoption of an order, a change
// of launch geometry) — a marker that stays put while the stream goes on launching, which is what a later sort waits for.
struct StreamMarks { blok::Event last, held; bool fresh = false; };
struct DeviceActivity {
    std::mutex lock;
    std::map<std::pair<const blok_hip_ctx*, hipStream_t>, StreamMarks> marks;
};
DeviceActivity& device_activity(int device) {
    static std::mutex table_lock;
    static auto& table = *new std::map<int, DeviceActivity>;      // never destroyed: the markers of a context nobody destroyed must not be handed back to a runtime that is shutting down
    std::lock_guard<std::mutex> g(table_lock);
    return table[device];
}
}  // namespace

static bool device_busy_elsewhere(const blok_hip_ctx* ctx, hipStream_t stream) {
    DeviceActivity& act = device_activity(ctx->device);
    std::lock_guard<std::mutex> g(act.lock);
    bool busy = false;
    for (auto& kv : act.marks) {
        if (kv.first.first == ctx && kv.first.second == stream) continue;
        for (hipEvent_t ev : {kv.second.last.get(), kv.second.held.get()})
            if (ev && hipEventQuery(ev) == hipErrorNotReady) { busy = true; break; }
        if (busy) break;
    }
    (void)hipGetLastError();                               // hipErrorNotReady is an answer, not a failure
    return busy;
}

static int note_frame_launch(blok_hip_ctx* ctx, hipStream_t stream) {
    DeviceActivity& act = device_activity(ctx->device);
    std::lock_guard<std::mutex> g(act.lock);
    StreamMarks& m = act.marks[{ctx, stream}];
    BLOK_HIP_TRY(ctx, m.last.create());
    BLOK_HIP_TRY(ctx, hipEventRecord(m.last, stream));
    m.fresh = true;
    return BLOK_OK;
}

// Every launch of this context issued so far, on any of its streams, is in front of a `held` marker from here on.  No HIP call: the
// marker a stream recorded behind its latest launch changes places with the one it held before (which that stream's next launch re-records).
static void hold_markers(const blok_hip_ctx* ctx) {
    DeviceActivity& act = device_activity(ctx->device);
    std::lock_guard<std::mutex> g(act.lock);
    for (auto& kv : act.marks)
        if (kv.first.first == ctx && kv.second.fresh) { std::swap(kv.second.last, kv.second.held); kv.second.fresh = false; }
}

// `stream` waits for the held markers of the context's OTHER streams (its own earlier work is in front of it anyway).
static int wait_for_held_markers(blok_hip_ctx* ctx, hipStream_t stream) {
    DeviceActivity& act = device_activity(ctx->device);
    std::lock_guard<std::mutex> g(act.lock);
    for (auto& kv : act.marks)
        if (kv.first.first == ctx && kv.first.second != stream && kv.second.held) BLOK_HIP_TRY(ctx, hipStreamWaitEvent(stream, kv.second.held, 0));
    return BLOK_OK;
}

void forget_device_activity(const blok_hip_ctx* ctx, bool one_stream, hipStream_t stream) {
    DeviceActivity& act = device_activity(ctx->device);
    std::lock_guard<std::mutex> g(act.lock);
    for (auto it = act.marks.begin(); it != act.marks.end();)
        if (it->first.first == ctx && (!one_stream || it->first.second == stream)) it = act.marks.erase(it);      // (and its events with it)
        else ++it;
}

// ---- longest-first order of the walk's wave tiles (api_internal.h: TileOrder; decisions in launch_policy.h: plan_order, plan_shift) ------
// Is it the same view?  An order sorted from a view's own clocks — and above all the set of tiles that walked in it, the only ones a prefix
// launch dispatches walk waves for — is that view's: a camera creeping by a quarter of a degree per frame (round 2's window) kept such
// an order in force while the silhouettes moved out from under it, and every tile that had become live was walked by its search wave,
// one after the other (measured: 0.32-0.37 ms per frame for a slow pan against 0.25 in row-major order).  So "at rest" means at rest: the
// basis within 1e-5 per component (0.0006 degree), the position within a thousandth of a voxel (and a millionth of its distance to the
// world), the same lens.  Whatever moves more is a camera in motion and gets the order made for that (launch_policy.h).
static bool camera_near(const blok_hip_ctx* ctx, const blok_camera& a, const blok_camera& b) {
    const float half = 0.5f * std::ldexp(1.0f, 2 * static_cast<int>(ctx->stats.levels)) * ctx->world_voxel_size;
    float d2 = 0.0f, r2 = 0.0f, turn = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float centre = static_cast<float>(ctx->stats.origin[k]) * ctx->world_voxel_size + half;
        d2 += (a.pos[k] - b.pos[k]) * (a.pos[k] - b.pos[k]);
        r2 += (a.pos[k] - centre) * (a.pos[k] - centre);
        turn = std::max(turn, std::max(std::fabs(a.fwd[k] - b.fwd[k]), std::max(std::fabs(a.right[k] - b.right[k]), std::fabs(a.up[k] - b.up[k]))));
    }
    const float still = 1.0e-3f * ctx->world_voxel_size;
    return turn <= 1.0e-5f && d2 <= std::max(still * still, 1.0e-12f * r2) && std::fabs(a.tan_half_fov - b.tan_half_fov) < 1e-6f && std::fabs(a.aspect - b.aspect) < 1e-6f;
}

// The order's buffers, for at least `blocks` wave tiles and never fewer than the full frame has: allocated by blok_hip_create / _resize, so
// that no *_device launch ever allocates or waits for the device on their account (the regrow below is what is left for a caller that
// resizes between launches: a device-wide wait, because frames in flight and a pending sort may use the old buffers).
int order_buffers(blok_hip_ctx* ctx, uint32_t blocks, hipStream_t stream) {
    auto& O = ctx->order;
    constexpr int kSlots = blok_hip_ctx::TileOrder::kSlots;
    const uint32_t want = std::max<uint32_t>(blocks, blok::rect_grid_blocks(ctx->width, ctx->height));
    if (O.capacity >= want) return BLOK_OK;
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());          // the one wait for all of them: the reserves below name none
    O.capacity = 0;
    const blok::FreeAfter waited = blok::FreeAfter::nothing();
    const size_t bytes = static_cast<size_t>(want) * sizeof(uint32_t);
    for (auto* a : {&O.d_cost, &O.d_iota, &O.d_keys_in, &O.d_keys}) BLOK_HIP_TRY(ctx, a->reserve(want, waited));
    for (auto& sl : O.slots) {
        sl = blok_hip_ctx::TileOrder::Slot{};
        BLOK_HIP_TRY(ctx, sl.d_order.reserve(want, waited));
        BLOK_HIP_TRY(ctx, sl.d_rank_of.reserve(want, waited));
    }
    bool fresh = false;
    BLOK_HIP_TRY(ctx, O.h_live.reserve(kSlots, waited));
    BLOK_HIP_TRY(ctx, O.h_depth.reserve(kSlots * blok::kOrderDepthPartials * 3, waited));
    BLOK_HIP_TRY(ctx, O.h_fallback.reserve(1, waited, &fresh));
    if (fresh) *O.h_fallback = 0u;
    BLOK_HIP_TRY(ctx, O.d_fallback.reserve(1, waited));
    O.temp_bytes = blok::tile_order_temp_bytes(want);
    BLOK_HIP_TRY(ctx, O.d_temp.reserve(O.temp_bytes ? O.temp_bytes : 16, waited));
    BLOK_HIP_TRY(ctx, O.d_class_scratch.reserve(blok::tile_order_class_sort_bytes_max(want), waited));
    BLOK_HIP_TRY(ctx, O.done.create());
    BLOK_HIP_TRY(ctx, blok::launch_iota(O.d_iota, want, stream));              // the identity, whatever the geometry: written once
    BLOK_HIP_TRY(ctx, hipMemsetAsync(O.d_cost, 0, bytes, stream));
    O.capacity = want;
    std::memset(O.key, 0xFF, sizeof(O.key));
    O.current = -1; O.chosen = -1; O.pending = false; O.orphan = false; O.n_recent = 0;
    return BLOK_OK;
}

// Before an orderable launch: adoption of a finished sort, the plan; fills args.order / rank_of / launched / cost_out.
// rect: a rectangle launch (else a rank's tiles: orders of a view's own clocks only — a whole-tile shift of the screen does not map a rank's
// round-robin share of the tiles onto itself); uniform_view: every camera of the launch is the same view (several frames per launch).
static int order_before_launch(blok_hip_ctx* ctx, blok::TraceArgs& args, uint32_t blocks, hipStream_t stream, bool alone, bool rect, bool uniform_view, blok::OrderPlan* plan) {
    auto& O = ctx->order;
    constexpr int kSlots = blok_hip_ctx::TileOrder::kSlots;
    const uint32_t key[7] = {rect ? args.x0 : (0x80000000u | args.tile), rect ? args.y0 : args.rank, rect ? args.w : args.n_ranks, rect ? args.h : 0u, ctx->width, ctx->height, ctx->world_version};
    if (O.capacity < blocks) { const int rc = order_buffers(ctx, blocks, stream); if (rc != BLOK_OK) return rc; }      // (never after create / resize: a rectangle has no more tiles than the frame)
    O.launch_serial += 1;
    if (std::memcmp(key, O.key, sizeof(key)) != 0) {
        // another launch geometry starts in natural order with no costs and no views; in stream order, nothing waits (a sort still pending
        // for the old geometry finishes into a slot nobody will adopt: its event is simply never asked again)
        BLOK_HIP_TRY(ctx, hipMemsetAsync(O.d_cost, 0, static_cast<size_t>(blocks) * sizeof(uint32_t), stream));
        std::memcpy(O.key, key, sizeof(key));
        O.orphan = O.orphan || O.pending;                                    // (a sort of the old geometry may still be writing an order buffer)
        // ... and frames in flight on other streams may still be READING the slots that were in use: the first sort of the new geometry,
        // whichever slot it targets, waits for the markers held from here (without this it waited for the markers of the last
        // adoption only, which cover the readers of the other buffer)
        hold_markers(ctx); O.hold_serial = O.launch_serial;
        for (auto& sl : O.slots) { sl.valid = false; sl.last_use = 0; }
        O.current = -1; O.pending = false; O.still_frames = 0; O.interval_now = O.interval; O.have_residual = false; O.n_recent = 0; O.revisit_streak = 0;
    }
    if (O.pending && hipEventQuery(O.done) == hipSuccess) {              // the sort launched some frames ago has finished
        auto& sl = O.slots[O.target];
        sl.valid = true; sl.dilated = O.pending_dilated; sl.radius = O.pending_radius; sl.cam = O.pending_cam;
        sl.live = O.h_live[O.target];                                    // written by the device before the event
        sl.frames_since_sort = 0; sl.interval_now = O.pending_interval; sl.last_use = 0;
        if (sl.dilated) {
            // the frame's depths: mean and standard deviation of its live beam tiles' inverse start parameters, from the sort's partial sums
            double cnt = 0.0, s1 = 0.0, s2 = 0.0;
            const float* part = O.h_depth + O.target * blok::kOrderDepthPartials * 3;
            for (uint32_t k = 0; k < blok::kOrderDepthPartials; ++k) { cnt += part[k * 3]; s1 += part[k * 3 + 1]; s2 += part[k * 3 + 2]; }
            const double mean = cnt > 0.0 ? s1 / cnt : 0.0, var = cnt > 0.0 ? s2 / cnt - mean * mean : 0.0;
            sl.inv_depth[0] = static_cast<float>(mean); sl.inv_depth[1] = static_cast<float>(var > 0.0 ? std::sqrt(var) : 0.0);
        }
        // an older order of the same view, and older orders made to be carried (only the latest is of use), make room
        for (int k = 0; k < kSlots; ++k)
            if (k != O.target && O.slots[k].valid && (O.slots[k].dilated || (!sl.dilated && camera_near(ctx, sl.cam, O.slots[k].cam)))) O.slots[k].valid = false;
        O.current = O.target; O.pending = false;
        // From here on the slots just retired are read by no new launch; the launches that may still be reading them are those already
        // issued, on any stream of this context.  The marker each stream left behind its latest launch is held from now: what a later sort —
        // which overwrites such a slot, many launches from now — has to wait for: long past by then, so the sort never holds up the frames in
        // flight (waiting for the streams' LATEST launches instead did: a bubble in the three-deep pipeline per sort, 5 % of a 20-frame run).
        hold_markers(ctx); O.hold_serial = O.launch_serial;
    }
    (void)hipGetLastError();                                             // hipErrorNotReady is an answer, not a failure
    // the order this launch may walk in: its own view's if the cache has one, else the one adopted last (a carried order, if it is dilated)
    int own = -1;
    for (int k = 0; k < kSlots && uniform_view; ++k)
        if (O.slots[k].valid && !O.slots[k].dilated && camera_near(ctx, args.cam, O.slots[k].cam) && (own < 0 || O.slots[k].last_use > O.slots[own].last_use)) own = k;
    const int chosen = own >= 0 ? own : O.current;
    // At rest: the previous launch's view — or, for a caller that alternates between fixed views, one of the few before it, once that has
    // happened four launches running (a camera that swings back and forth passes through a view of two launches ago at every turn: that is
    // motion, and keeps the moving camera's carried order)
    const bool rest = uniform_view && camera_near(ctx, args.cam, O.last_cam);
    bool revisit = false;
    for (uint32_t k = 0; k < O.n_recent && uniform_view && !rest && !revisit; ++k) revisit = camera_near(ctx, args.cam, O.recent[k]);
    O.revisit_streak = revisit ? O.revisit_streak + 1u : (rest ? O.revisit_streak : 0u);
    const bool seen = rest || (revisit && O.revisit_streak >= 4u);      // (a swing back through a view the camera rested in makes three in a row: four)
    blok::OrderFacts f{};
    f.enabled = true; f.have_order = chosen >= 0 && O.slots[chosen].valid;
    f.near_order_view = f.have_order && own >= 0;
    f.near_last_view = seen;
    f.sort_pending = O.pending; f.still_frames = O.still_frames;
    f.frames_since_sort = own >= 0 ? O.slots[own].frames_since_sort : 0u; f.interval = O.interval; f.interval_now = own >= 0 ? O.slots[own].interval_now : O.interval_now;
    f.moving_enabled = O.moving && rect; f.alone = alone; f.alone_before = O.alone_before; O.alone_before = alone;
    f.order_dilated = f.have_order && O.slots[chosen].dilated;
    blok::ShiftPlan shift{};
    if (f.order_dilated && f.moving_enabled && f.alone) {
        blok::ShiftFacts sf{};
        static_assert(sizeof(blok::PolicyCamera) == sizeof(blok_camera), "launch_policy.h: PolicyCamera is blok_camera");
        std::memcpy(&sf.then, &O.slots[chosen].cam, sizeof(blok_camera)); std::memcpy(&sf.now, &args.cam, sizeof(blok_camera));
        sf.inv_depth_mean = O.slots[chosen].inv_depth[0]; sf.inv_depth_sigma = O.slots[chosen].inv_depth[1];
        sf.frame_w = ctx->width; sf.frame_h = ctx->height;
        sf.tiles_x = (args.w + blok::kTileW - 1u) / blok::kTileW; sf.tiles_y = (args.h + blok::kTileH - 1u) / blok::kTileH; sf.tile_w = blok::kTileW; sf.tile_h = blok::kTileH;
        sf.radius = O.slots[chosen].radius;
        shift = blok::plan_shift(sf);
        f.shift_ok = shift.ok;
        // what the shift leaves over sizes the next dilation and the strips — also when it is too large to use, the next dilation grows with it —
        // but only when it was computed: a view plan_shift could not compare (another lens, a point behind the camera) says nothing, and
        // the next sort takes the default radius (a residual of 0 from an early exit gave the smallest radius after the largest change)
        O.have_residual = shift.measured; O.last_residual = shift.measured ? shift.residual : 0.0f;
    }
    *plan = blok::plan_order(f);
    O.still_frames = plan->still_frames; O.last_cam = args.cam;
    { for (uint32_t k = std::min<uint32_t>(O.n_recent, 3u); k > 0; --k) O.recent[k] = O.recent[k - 1]; O.recent[0] = args.cam; O.n_recent = std::min<uint32_t>(O.n_recent + 1u, 4u); }
    O.chosen = plan->use_order ? chosen : -1;
    args.order = plan->use_order ? O.slots[chosen].d_order : nullptr;
    args.cost_out = plan->measure ? O.d_cost : nullptr;
    args.order_sx = args.order_sy = 0u;
    O.last_use = plan->use_order ? (plan->shifted ? 2 : 1) : 0; O.last_sx = O.last_sy = 0u;
    if (args.order) {
        O.slots[chosen].last_use = O.launch_serial;
        args.rank_of = O.slots[chosen].d_rank_of; args.launched = O.slots[chosen].live;
        if (plan->shifted) { args.order_sx = O.last_sx = shift.sx; args.order_sy = O.last_sy = shift.sy; }
        if (O.debug_shift) {                                             // any shift of any order is a permutation: the frame must not change
            const uint32_t tiles_x = (args.w + blok::kTileW - 1u) / blok::kTileW, tiles_y = (args.h + blok::kTileH - 1u) / blok::kTileH;
            args.order_sx = O.last_sx = O.debug_sx % tiles_x; args.order_sy = O.last_sy = O.debug_sy % tiles_y;
        }
    }
    return BLOK_OK;
}

// After it: the sort, if the plan says so — on the LAUNCH stream, behind the frame (a stream of its own would be one HIP stream more than
// the hardware queues the frame streams and the null stream occupy: measured, that alone costs 18 % of the pipelined rate).
static int order_after_launch(blok_hip_ctx* ctx, const blok::TraceArgs& args, uint32_t blocks, uint32_t n_beams, hipStream_t stream, const blok::OrderPlan& plan) {
    auto& O = ctx->order;
    constexpr int kSlots = blok_hip_ctx::TileOrder::kSlots;
    if (O.chosen >= 0) { auto& sl = O.slots[O.chosen]; sl.frames_since_sort += 1; if (!sl.dilated) sl.interval_now = plan.next_interval_now; }
    else O.interval_now = plan.next_interval_now;
    if (!plan.start_sort) return BLOK_OK;
    // The slot to sort into: not the one this launch walks in; an empty one if there is one, else a retired-in-all-but-name dilated order, else
    // the view walked in longest ago.
    int target = -1;
    for (int pass = 0; pass < 3 && target < 0; ++pass)
        for (int k = 0; k < kSlots; ++k) {
            if (k == O.chosen) continue;
            const auto& sl = O.slots[k];
            const bool fits = pass == 0 ? !sl.valid : (pass == 1 ? (sl.dilated && k != O.current) : true);
            if (fits && (target < 0 || (pass == 2 && sl.last_use < O.slots[target].last_use))) { target = k; if (pass != 2) break; }
        }
    if (target < 0) return BLOK_OK;
    // Nothing still running may read the target: whatever walked in it was issued before the latest holding of the markers (an adoption, a
    // change of geometry) — or else they are held again now, behind the streams' latest launches (a cache with more views cycling than slots).
    // (>=: the launch during which the markers were held was itself issued behind them)
    if (O.slots[target].last_use >= O.hold_serial) { hold_markers(ctx); O.hold_serial = O.launch_serial; }
    O.slots[target].valid = false;
    if (O.current == target) O.current = -1;
    { const int rc = wait_for_held_markers(ctx, stream); if (rc != BLOK_OK) return rc; }
    // ... and nothing may still be WRITING it: a sort left behind by a change of launch geometry, possibly on another stream
    if (O.orphan) { BLOK_HIP_TRY(ctx, hipStreamWaitEvent(stream, O.done, 0)); O.orphan = false; }
    uint32_t radius = 0;
    auto& T = O.slots[target];
    if (plan.dilate) {
        // a camera in motion: a counting sort of the dilated clocks (three small launches; it reads the live cost buffer — any mixture of old
        // and new costs is as good a key, and what it sorts is its own copy), and the frame's depths go along for the next launch's shift
        radius = blok::plan_dilation(O.have_residual, O.last_residual);
        const uint32_t tiles_x = (args.w + blok::kTileW - 1u) / blok::kTileW, tiles_y = (args.h + blok::kTileH - 1u) / blok::kTileH;
        BLOK_HIP_TRY(ctx, blok::launch_tile_order_class_sort(O.d_cost, tiles_x, tiles_y, radius, O.d_class_scratch, T.d_order, T.d_rank_of, O.h_live + target,
                                                             args.beam, args.beam_slots, args.beam_serial, n_beams, O.h_depth + target * blok::kOrderDepthPartials * 3, stream));
    } else {
        // the sort reads a SNAPSHOT of the costs: frames in flight on other streams keep writing the live buffer, and a radix sort that saw a
        // key change between its histogram and its scatter would not produce a permutation
        BLOK_HIP_TRY(ctx, hipMemcpyAsync(O.d_keys_in, O.d_cost, static_cast<size_t>(blocks) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        BLOK_HIP_TRY(ctx, blok::launch_tile_order_sort(O.d_keys_in, O.d_keys, O.d_iota, T.d_order, O.d_temp, O.temp_bytes, blocks, stream));
        BLOK_HIP_TRY(ctx, blok::launch_tile_order_finish(T.d_order, O.d_keys, blocks, T.d_rank_of, O.h_live + target, stream));
    }
    BLOK_HIP_TRY(ctx, hipEventRecord(O.done, stream));
    O.target = target; O.pending_cam = args.cam; O.pending_dilated = plan.dilate; O.pending_radius = radius; O.pending_interval = plan.next_interval_now; O.pending = true;
    return BLOK_OK;
}

// The stream's give-up counter (joint and list forms).
static int gave_up_counter(blok_hip_ctx* ctx, hipStream_t stream, uint32_t** out) {
    auto& slot = ctx->beam_buffers[stream];
    bool fresh = false;
    BLOK_HIP_TRY(ctx, slot.gave_up.reserve(1, blok::FreeAfter::nothing(), &fresh));
    if (fresh) BLOK_HIP_TRY_FILL(ctx, slot.gave_up, hipMemsetAsync(slot.gave_up, 0, sizeof(uint32_t), stream));
    *out = slot.gave_up;
    return BLOK_OK;
}

// The stream's published-result words of a joint launch: valid when they carry this launch's serial.
static int joint_slots(blok_hip_ctx* ctx, blok::TraceArgs& args, hipStream_t stream, uint32_t n_beams) {
    auto& slot = ctx->beam_buffers[stream];
    bool fresh = false;
    BLOK_HIP_TRY(ctx, slot.slots.reserve(n_beams, blok::FreeAfter::work_on(stream), &fresh));
    if (fresh) {
        BLOK_HIP_TRY_FILL(ctx, slot.slots, hipMemsetAsync(slot.slots, 0, n_beams * sizeof(unsigned long long), stream));
        slot.serial = 0;
    }
    if (++slot.serial == 0u) slot.serial = 1u;
    args.beam_slots = slot.slots; args.beam_serial = slot.serial;
    return gave_up_counter(ctx, stream, &args.joint_gave_up);
}

// The stream's live list for a launch of n_searches search workgroups with per_search wave tiles each (trace_kernels.h: LiveList).
int live_list(blok_hip_ctx* ctx, blok::TraceArgs& args, hipStream_t stream, uint32_t n_searches, uint32_t per_search) {
    auto& slot = ctx->beam_buffers[stream];
    const size_t seg_capacity = static_cast<size_t>((n_searches + blok::kListSegments - 1u) / blok::kListSegments) * per_search;
    bool fresh = false;
    BLOK_HIP_TRY(ctx, slot.list_ctl.reserve(blok::kListSegments * blok::kListCtlWords, blok::FreeAfter::nothing(), &fresh));
    if (fresh) {      // the control words and the hint come and go together: a failure on the way leaves neither
        BLOK_HIP_TRY_FILL(ctx, slot.list_ctl, hipMemsetAsync(slot.list_ctl, 0, blok::kListSegments * blok::kListCtlWords * sizeof(unsigned long long), stream));
        BLOK_HIP_TRY_FILL(ctx, slot.list_ctl, slot.list_hint.reserve(blok::kListSegments * blok::kListClasses, blok::FreeAfter::nothing()));
        std::memset(slot.list_hint, 0, blok::kListSegments * blok::kListClasses * sizeof(uint32_t));      // read as a hint before the first launch has written it
        slot.list_hint_valid = false;
    }
    const bool wrapped = slot.list_serial + 1u >= (1u << blok::kListSerialBits);
    if (slot.list_capacity < seg_capacity || wrapped) {
        bool grown = false;
        if (slot.list_capacity < seg_capacity) {
            slot.list_capacity = 0;
            BLOK_HIP_TRY(ctx, slot.list_entries.reserve(seg_capacity * blok::kListSegments * blok::kListClasses, blok::FreeAfter::work_on(stream), &grown));
            slot.list_capacity = seg_capacity;
        }
        // every entry empty; also when the 20-bit serial starts over, so that no entry of a million launches ago can pass for a new one
        const hipError_t emptied = hipMemsetAsync(slot.list_entries, 0, slot.list_capacity * blok::kListSegments * blok::kListClasses * sizeof(unsigned long long), stream);
        if (emptied != hipSuccess && grown) { slot.list_entries.reset(); slot.list_capacity = 0; }      // (a new array nobody has used yet: the next launch starts over)
        BLOK_HIP_TRY(ctx, emptied);
        if (wrapped) slot.list_serial = 0;
    }
    slot.list_serial += 1u;
    args.list.entries = slot.list_entries; args.list.ctl = slot.list_ctl; args.list.hint = slot.list_hint;
    args.list.seg_capacity = static_cast<uint32_t>(slot.list_capacity);      // the buffer's stride (>= this launch's need)
    args.list.serial = slot.list_serial; args.list.n_searches = n_searches;
    return gave_up_counter(ctx, stream, &args.joint_gave_up);
}

// What the previous list launch on this stream left in pinned memory: per class its longest list (sizing hints, launch_policy.h).
static bool list_hint(const blok_hip_ctx* ctx, hipStream_t stream, uint32_t geometry_key, uint32_t per_class[blok::kListClasses]) {
    auto it = ctx->beam_buffers.find(stream);
    if (it == ctx->beam_buffers.end() || !it->second.list_hint || !it->second.list_hint_valid || it->second.list_hint_key != geometry_key) return false;
    for (uint32_t c = 0; c < blok::kListClasses; ++c) {
        per_class[c] = 0;
        for (uint32_t k = 0; k < blok::kListSegments; ++k) per_class[c] = std::max(per_class[c], it->second.list_hint[k * blok::kListClasses + c]);      // plain reads of words the device may be writing: hints
    }
    return true;
}

// The context's cost buffer for a rectangle launch (trace_kernels.h: cost classes): one word per wave tile of the launch geometry.
static int list_costs(blok_hip_ctx* ctx, blok::TraceArgs& args, uint32_t wave_tiles, hipStream_t stream) {
    const uint32_t key[6] = {args.x0, args.y0, args.w, args.h, ctx->width, ctx->height};
    bool fresh = false;
    BLOK_HIP_TRY(ctx, ctx->d_list_cost.reserve(wave_tiles, blok::FreeAfter::device(), &fresh));      // frames in flight on other streams still write it
    if (fresh || std::memcmp(key, ctx->list_cost_key, sizeof(key)) != 0) {      // (a larger launch is another geometry: its key differs too)
        BLOK_HIP_TRY(ctx, hipMemsetAsync(ctx->d_list_cost, 0, ctx->d_list_cost.capacity() * sizeof(uint32_t), stream));      // another geometry: nothing is known
        std::memcpy(ctx->list_cost_key, key, sizeof(key));
        ctx->list_has_prev_cam = false;
    }
    args.list.cost = ctx->d_list_cost;
    args.list.has_prev = ctx->list_has_prev_cam ? 1u : 0u;
    args.list.prev_cam = ctx->list_prev_cam;
    ctx->list_prev_cam = args.cam; ctx->list_has_prev_cam = true;        // the costs this launch leaves are those of this camera
    return BLOK_OK;
}

// ---- the beam bounds of views at rest (beam_cache.h: the key, admission, the slots; api_internal.h: BeamCache) ---------------------------
// One float per beam tile of the whole frame at the finest beam tile there is (blok_hip_set_beam: 8 pixels), per slot: no rectangle, no
// beam setting needs more, so no launch ever allocates on the cache's account.  Grown only (a device-wide wait: frames in flight may read
// the old buffers); what the slots held is dropped with them.
int beam_cache_buffers(blok_hip_ctx* ctx) {
    auto& B = ctx->beam_cache;
    const size_t want = static_cast<size_t>((ctx->width + 7u) / 8u) * ((ctx->height + 7u) / 8u);
    if (B.capacity >= want) return beam_list_buffers(ctx);      // (the same wave tiles can be more pixels: the lists' buffers count those)
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    B.capacity = 0;
    blok::beam_cache_clear(B.policy);
    for (auto& sl : B.slots) {
        sl = blok_hip_ctx::BeamCache::Slot{};
        BLOK_HIP_TRY(ctx, sl.d_beam.reserve(want, blok::FreeAfter::nothing()));      // (the wait above was for all of them)
        BLOK_HIP_TRY(ctx, sl.d_fine.reserve(want, blok::FreeAfter::nothing()));
        BLOK_HIP_TRY(ctx, sl.filled.done.create());
        BLOK_HIP_TRY(ctx, sl.refined.done.create());
    }
    B.capacity = want;
    B.list_capacity = 0;                                 // (the slots' lists went with the slots)
    return beam_list_buffers(ctx);
}

// The packed walk's buffers (trace_kernels.h), for the whole frame — no rectangle has more areas — when the packed walk is switched on: by
// blok_hip_create / _resize behind the buffers above, and by blok_hip_set_beam_cache; no launch allocates.  A device-wide wait, as above.
int beam_list_buffers(blok_hip_ctx* ctx) {
    auto& B = ctx->beam_cache;
    if (!B.packed) return BLOK_OK;
    const size_t areas = static_cast<size_t>((ctx->width + blok::kPackArea - 1u) / blok::kPackArea) * ((ctx->height + blok::kPackArea - 1u) / blok::kPackArea);
    const size_t entries = areas * blok::kPackStretch, words = areas * blok::kPackGroups, pixels = static_cast<size_t>(ctx->width) * ctx->height;
    const bool own = B.policy.own_starts, nodes = own && B.policy.node_restart;
    if (B.list_capacity >= entries && B.words_capacity >= words && B.d_trips.capacity() >= pixels &&
        (!own || (B.d_ray_start.capacity() >= pixels && B.d_restarts.capacity() >= pixels && B.slots[0].d_start.capacity() >= entries)) &&
        (!nodes || (B.d_ray_node.capacity() >= pixels && B.slots[0].d_node.capacity() >= entries))) return BLOK_OK;
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    B.list_capacity = 0; B.words_capacity = 0;
    blok::beam_cache_clear(B.policy);
    blok::beam_list_settle(B.policy);
    const blok::FreeAfter waited = blok::FreeAfter::nothing();
    for (auto& sl : B.slots) {
        BLOK_HIP_TRY(ctx, sl.d_list.reserve(entries, waited));
        BLOK_HIP_TRY(ctx, sl.d_table.reserve(words, waited));
        if (own) BLOK_HIP_TRY(ctx, sl.d_start.reserve(entries, waited));
        if (nodes) BLOK_HIP_TRY(ctx, sl.d_node.reserve(entries, waited));
        sl.n_groups = 0;
    }
    BLOK_HIP_TRY(ctx, B.d_trips.reserve(pixels, waited));
    if (own) { BLOK_HIP_TRY(ctx, B.d_ray_start.reserve(pixels, waited)); BLOK_HIP_TRY(ctx, B.d_restarts.reserve(pixels, waited)); }
    if (nodes) BLOK_HIP_TRY(ctx, B.d_ray_node.reserve(pixels, waited));
    BLOK_HIP_TRY(ctx, B.d_words.reserve(words, waited));
    B.sort_temp_bytes = blok::pack_table_temp_bytes(static_cast<uint32_t>(words));
    BLOK_HIP_TRY(ctx, B.d_sort_temp.reserve(B.sort_temp_bytes ? B.sort_temp_bytes : 16, waited));
    BLOK_HIP_TRY(ctx, B.h_groups.reserve(blok::kBeamCacheSlots, waited));
    BLOK_HIP_TRY(ctx, B.list_done.create());
    B.list_capacity = entries; B.words_capacity = words;
    return BLOK_OK;
}

void settle_beam_cache(blok_hip_ctx* ctx) {
    for (auto& sl : ctx->beam_cache.slots)
        for (auto* p : {&sl.filled, &sl.refined}) { p->settled = true; p->n_waited = 0; }
}

static blok::BeamKey beam_key(const blok_hip_ctx* ctx, blok::RayMode mode, const blok::TraceArgs& args) {
    blok::BeamKey k{};
    static_assert(sizeof(k.cam) == sizeof(blok_camera), "beam_cache.h: BeamKey::cam is blok_camera, byte for byte");
    std::memcpy(k.cam, &args.cam, sizeof(blok_camera));
    k.x0 = args.x0; k.y0 = args.y0; k.w = args.w; k.h = args.h;
    k.frame_w = args.frame_w; k.frame_h = args.frame_h;
    k.beam_tile = args.beam_tile; k.beam_budget = args.beam_budget;
    k.tuning = blok::kBeamCoarsen1 | (blok::kBeamCoarsen2 << 8) | (static_cast<uint32_t>(BLOK_BEAM_STOP_LEVEL) << 16);
    k.ray_mode = static_cast<uint32_t>(mode);
    k.levels = args.levels;
    for (int a = 0; a < 3; ++a) k.origin[a] = args.origin[a];
    std::memcpy(&k.voxel_bits, &args.voxel_size, sizeof(uint32_t));
    const uint64_t nodes = reinterpret_cast<uintptr_t>(args.nodes);
    k.nodes_lo = static_cast<uint32_t>(nodes); k.nodes_hi = static_cast<uint32_t>(nodes >> 32);
    k.world_version = ctx->world_version; k.tree_version = ctx->tree_version;
    return k;
}

// The launch that wrote what `stream` is about to read may still be running, on another stream: the first reader there waits for it.
static int wait_for_producer(blok_hip_ctx* ctx, blok_hip_ctx::BeamCache::Produced& p, hipStream_t stream) {
    if (p.settled || stream == p.producer) return BLOK_OK;
    for (uint32_t k = 0; k < p.n_waited; ++k) if (p.waited[k] == stream) return BLOK_OK;
    if (hipEventQuery(p.done) == hipSuccess) { p.settled = true; p.n_waited = 0; return BLOK_OK; }
    (void)hipGetLastError();                             // hipErrorNotReady is an answer, not a failure
    BLOK_HIP_TRY(ctx, hipStreamWaitEvent(stream, p.done, 0));
    if (p.n_waited < blok_hip_ctx::BeamCache::Produced::kWaited) p.waited[p.n_waited++] = stream;      // (more streams than that wait again next time: harmless)
    return BLOK_OK;
}

// Plan.  Before a rectangle launch of a static form: what does it do over the cache (beam_cache.h: plan_resting_launch) — search, search
// into a slot, or walk from a slot, and then how?  A build that has finished is adopted here, whatever this launch is (its length was
// written before the event).  Points args.beam at the slot's beam bounds and deals with whoever else uses it.
static int plan_resting(blok_hip_ctx* ctx, blok::RayMode mode, blok::TraceArgs& args, hipStream_t stream, blok::RestingPlan* resting) {
    auto& B = ctx->beam_cache;
    blok::RestingFacts facts{};
    facts.refine_eligible = B.refine && blok::beam_refine_applies(args) && blok::beam_refine_tiles(args) <= B.capacity;
    facts.list_eligible = B.packed && blok::pack_applies(args) && static_cast<size_t>(blok::pack_areas(args)) * blok::kPackStretch <= B.list_capacity &&
                          static_cast<size_t>(args.w) * args.h <= B.d_trips.capacity();
    if (B.policy.building >= 0) { facts.build_finished = hipEventQuery(B.list_done) == hipSuccess; (void)hipGetLastError(); }      // hipErrorNotReady is an answer, not a failure
    // mode 5: the node words beside the starts — unless the tree's node indices do not fit them, or (never: beam_list_buffers reserves
    // every slot alike, and a reservation that failed leaves no list capacity to count for) there is nowhere to put them
    facts.node_words = blok::node_words_apply(ctx->stats.n_tree_nodes) && B.d_ray_node;
    for (const auto& sl : B.slots) facts.node_words = facts.node_words && sl.d_node;
    static_assert(sizeof(args.jitter_clip) == sizeof(facts.start_key.jitter_clip), "beam_cache.h: BeamStartKey::jitter_clip is TraceArgs::jitter_clip, bit for bit");
    std::memcpy(facts.start_key.jitter_clip, args.jitter_clip, sizeof(facts.start_key.jitter_clip));
    std::memcpy(&facts.start_key.tmin, &args.tmin, sizeof(uint32_t)); std::memcpy(&facts.start_key.tmax, &args.tmax, sizeof(uint32_t));
    *resting = blok::plan_resting_launch(B.policy, beam_key(ctx, mode, args), facts);
    const blok::BeamCachePlan& plan = resting->cache;
    if (resting->list.adopted >= 0) { auto& got = B.slots[resting->list.adopted]; got.n_groups = std::min(B.h_groups[resting->list.adopted], got.n_words); }
    if (resting->walk == blok::RestingWalk::PackedNodes && !B.slots[plan.slot].d_node) resting->walk = blok::RestingWalk::PackedStarts;      // (never, as above)
    if (plan.action == blok::BeamAction::Search) return BLOK_OK;
    auto& sl = B.slots[plan.slot];
    if (plan.action == blok::BeamAction::Hit) {
        { const int rc = wait_for_producer(ctx, sl.filled, stream); if (rc != BLOK_OK) return rc; }
        if (resting->fine.use_fine) { const int rc = wait_for_producer(ctx, sl.refined, stream); if (rc != BLOK_OK) return rc; }
        B.hits += 1u;
    } else {
        // Nothing in flight may read the slot while the searches rewrite it (nor still be writing it): whatever used it was issued before
        // now, on some stream of this context, so every stream's marker is held here and this stream waits for the others' (its own
        // earlier launches are in front of it anyway).  Once per view that comes to rest, and not at all for a slot never filled.
        if (sl.used) {
            hold_markers(ctx);
            const int rc = wait_for_held_markers(ctx, stream);
            if (rc != BLOK_OK) return rc;
        }
        sl.used = true;
        sl.filled.settled = false; sl.filled.producer = stream; sl.filled.n_waited = 0;
        B.fills += 1u;
    }
    args.beam = sl.d_beam; args.beam_slots = nullptr; args.beam_serial = 0u;      // plain floats, whatever form was planned
    return BLOK_OK;
}

// A packed hit's fill units per workgroup; 0: the fill in a launch of its own.  Known only behind the adoption: a list with groups has
// the fill in the walk's grid (blok_hip_set_packed_fill), an all-sky view has the fill alone.
static uint32_t packed_fill_units(const blok_hip_ctx* ctx, const blok::RestingPlan& r) {
    return blok::resting_packed(r.walk) && ctx->beam_cache.slots[r.cache.slot].n_groups > 0u ? ctx->beam_cache.packed_fill : 0u;
}

// Issue.  A hit's launches, by r.walk -> the workgroups of a packed frame's one launch that only fill.
// No searches.  Coarse, Fine: the walk over the view's live prefix, from the kept bounds; in front of it, what the search waves do besides
// searching (the miss pixels, unless the walk writes them; the wave tiles the prefix has no workgroup for); behind it, on the view's K-th
// hit, its finer searches, once.  The packed walk, and the launch that measures for it, use neither the view's order nor its live prefix
// (the table's order stands in for both; the count launch walks every wave tile in a workgroup of its own, so that every listed pixel gets
// its count): their fill writes the misses of the empty beam tiles and of the empty wave tiles and walks nothing.
static uint32_t issue_resting(blok_hip_ctx* ctx, blok::RayMode mode, const blok::TraceArgs& args, const blok::RestingPlan& r, uint32_t blocks, uint32_t walk_blocks, uint32_t n_beams,
                              hipStream_t stream) {
    using Walk = blok::RestingWalk;
    auto& B = ctx->beam_cache;
    auto& sl = B.slots[r.cache.slot];
    const bool prefix = r.walk == Walk::Coarse || r.walk == Walk::Fine;
    blok::TraceArgs fill = args;
    if (!prefix) {
        fill.order = nullptr; fill.rank_of = nullptr; fill.launched = 0u; fill.order_sx = fill.order_sy = 0u; fill.n_strip = 0u; fill.fallback_tiles = nullptr;
        fill.miss_in_walk = 0u;
    }
    // the walk reads the finer bounds through the fields it has: a "beam tile" the size of a wave tile (the lookup in trace_block works for
    // any tile size), so a wave tile that is empty by its own bound is not walked: its misses come from the walk (miss_in_walk) or from the
    // fill wave of its beam tile, and its walk workgroup, while the order still has one, costs 0
    blok::TraceArgs walk = fill;
    if (r.walk != Walk::Coarse) { walk.beam = sl.d_fine; walk.beam_tile = blok::kWaveW; walk.beam_bx = (args.w + blok::kWaveW - 1u) / blok::kWaveW; }
    const uint32_t units = packed_fill_units(ctx, r);
    if (units == 0u && !fill.miss_in_walk) blok::launch_beam_fill(mode, fill, n_beams, r.walk != Walk::Coarse ? sl.d_fine.get() : nullptr, stream);
    if (prefix) {
        blok::launch_trace(mode, walk, walk_blocks, stream);
        if (r.fine.refine_now) blok::launch_beam_refine(args, sl.d_fine, stream);
        return 0u;
    }
    if (blok::resting_packed(r.walk))
        return blok::launch_packed(fill, {sl.d_fine, sl.d_list, sl.d_table, sl.d_start, sl.d_node, sl.n_groups},
                                   r.walk == Walk::PackedNodes ? blok::PackedFrom::Nodes : r.walk == Walk::PackedStarts ? blok::PackedFrom::Starts : blok::PackedFrom::Fine, units, stream);
    // The count.  Mode 4: it also leaves every ray's own start and restarted trips; the build sorts by those and writes the starts in list
    // order.  Mode 5: ... and the node every restarted walk ends in, gathered beside the starts.
    const bool own = r.walk != Walk::Count, nodes = r.walk == Walk::CountNodes;
    if (own) blok::launch_trace_count_own(walk, blocks, B.d_trips, B.d_ray_start, B.d_restarts, nodes ? B.d_ray_node.get() : nullptr, stream);
    else blok::launch_trace_count(walk, blocks, B.d_trips, stream);
    // the build behind it: the areas' sorted stretches, then (finish_resting) the table; its length goes to pinned memory in front of the event
    sl.n_words = blok::pack_areas(args) * blok::kPackGroups; sl.n_groups = 0u;
    blok::launch_pack_build(fill, sl.d_fine, {own ? B.d_restarts.get() : B.d_trips.get(), own ? B.d_ray_start.get() : nullptr, nodes ? B.d_ray_node.get() : nullptr},
                            {sl.d_list, B.d_words, sl.d_start, sl.d_node}, stream);
    return 0u;
}

// What the latest rectangle launch did, for api_debug.hip's read-backs, and the counters.  fill_only: what issue_resting answered.
static void note_resting(blok_hip_ctx* ctx, const blok::RestingPlan& r, const blok::TraceArgs& args, uint32_t n_beams, uint32_t fill_only) {
    auto& B = ctx->beam_cache;
    B.last_action = r.cache.action == blok::BeamAction::Hit ? 2 : r.cache.action == blok::BeamAction::Fill ? 1 : 0;
    B.last_slot = r.cache.slot; B.last_n_beams = n_beams;
    B.last_fine = r.fine.use_fine ? 2 : r.fine.refine_now ? 1 : 0;
    B.last_n_fine = B.last_fine ? blok::beam_refine_tiles(args) : 0u;
    B.last_list = r.list.use_list ? 2 : r.list.count_now ? 1 : 0;
    B.last_starts = r.starts.use == blok::BeamStarts::OtherKey ? 2 : (r.starts.use == blok::BeamStarts::Use || r.starts.count_own) ? 1 : 0;
    if (r.starts.use == blok::BeamStarts::Use) B.start_hits += 1u;
    if (r.starts.use == blok::BeamStarts::OtherKey) B.start_other_key += 1u;
    B.last_w = args.w; B.last_h = args.h;
    if (packed_fill_units(ctx, r) == 0u) return;
    B.one_launch_frames += 1u; B.fill_only_workgroups += fill_only;
    if (r.walk == blok::RestingWalk::PackedNodes) B.node_hits += 1u;
}

// Finish.  Behind the launches, with what issuing them answered: bounds nobody wrote are nobody's to keep; the event behind the finer
// searches; the table's sort and the event behind the build; the commit of both (bounds nobody can wait for, a list nobody can see
// finished, are not used); the event behind a fill.
static int finish_resting(blok_hip_ctx* ctx, const blok::RestingPlan& r, hipError_t launch_error, hipStream_t stream) {
    auto& B = ctx->beam_cache;
    auto* const sl = r.cache.action == blok::BeamAction::Search ? nullptr : &B.slots[r.cache.slot];      // (a search is told neither to refine nor to count)
    if (launch_error != hipSuccess && r.cache.action == blok::BeamAction::Fill) B.policy.valid[r.cache.slot] = false;
    hipError_t marked = launch_error, built = launch_error;
    if (r.fine.refine_now && marked == hipSuccess) marked = hipEventRecord(sl->refined.done, stream);
    if (r.list.count_now && built == hipSuccess) built = blok::launch_pack_table_sort(B.d_words, sl->d_table, B.d_sort_temp, B.sort_temp_bytes, sl->n_words, B.h_groups + r.cache.slot, stream);
    if (r.list.count_now && built == hipSuccess) built = hipEventRecord(B.list_done, stream);
    blok::commit_resting_launch(B.policy, r, marked == hipSuccess, built == hipSuccess);
    if (r.fine.refine_now && marked == hipSuccess) { sl->refined.settled = false; sl->refined.producer = stream; sl->refined.n_waited = 0; B.refines += 1u; }
    if (r.list.count_now && built == hipSuccess) B.list_builds += 1u;
    BLOK_HIP_TRY(ctx, launch_error);
    BLOK_HIP_TRY(ctx, marked);
    BLOK_HIP_TRY(ctx, built);
    if (r.cache.action == blok::BeamAction::Fill) BLOK_HIP_TRY(ctx, hipEventRecord(sl->filled.done, stream));
    return BLOK_OK;
}

// Rect / Tiles launches run the beam pre-pass first, on the same stream (tiles_of_rank: Tiles only; frames: several frames of a rank's
// tiles in one launch, `blocks` and the beam tiles then count ONE frame).
int launch_timed(blok_hip_ctx* ctx, blok::RayMode mode, blok::TraceArgs args, uint32_t blocks, hipStream_t stream,
                 uint32_t tiles_of_rank, const blok::TileFrames* frames) {
    uint32_t n_beams = 0;
    if (blocks) { const int rc = prepare_beam(ctx, mode, args, stream, tiles_of_rank, &n_beams); if (rc != BLOK_OK) return rc; }
    const uint32_t n_frames = frames ? frames->n_frames : 1u;
    if (frames && n_beams) { const int rc = beam_buffer(ctx, stream, static_cast<size_t>(n_beams) * n_frames, &args.beam); if (rc != BLOK_OK) return rc; }
    blok::LaunchFacts facts{};
    facts.form = ctx->launch_form;
    facts.has_beam = n_beams != 0;
    facts.one_wave_blocks = blok::kBlock == 64;
    facts.wave_tiles = blocks * n_frames;
    const uint32_t geometry_key = blocks * 31u + n_beams * n_frames;
    facts.have_hint = list_hint(ctx, stream, geometry_key, facts.hint);
    bool busy = false;
    // A launch that is being captured into a hipGraph is replayed with these very arguments: it gets the plain two-launch form and none of
    // the per-frame bookkeeping (event queries and records outside the graph, serial numbers, orders adopted between frames).
    bool capturing = false;
    if (stream) {
        hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &status) == hipSuccess) capturing = status != hipStreamCaptureStatusNone;
        else (void)hipGetLastError();
    }
    if (capturing) facts.form = blok::kFormTwoLaunches;
    else busy = facts.has_beam && (ctx->launch_form == blok::kFormAuto || (ctx->order.enabled && ctx->order.moving)) && device_busy_elsewhere(ctx, stream);
    facts.device_busy = busy && ctx->launch_form == blok::kFormAuto;
    blok::LaunchPlan plan = blok::plan_launch(facts);
    if (frames && (plan.kind == blok::LaunchKind::Queues || plan.kind == blok::LaunchKind::Joint)) plan.kind = blok::LaunchKind::TwoLaunches;      // several frames per launch: the two-launch or the list forms
    ctx->last_launch_kind = static_cast<int>(plan.kind);

    blok::FrameQueue queue{};
    uint32_t frame_blocks = 0;
    blok::TileFrames fr{};
    if (frames) { fr = *frames; fr.blocks_per_frame = blocks; fr.beams_per_frame = n_beams; }
    if (plan.kind == blok::LaunchKind::Joint) { const int rc = joint_slots(ctx, args, stream, n_beams); if (rc != BLOK_OK) return rc; }
    if (plan.kind == blok::LaunchKind::Queues) { const int rc = prepare_queue(ctx, mode, args, stream, n_beams, &queue, &frame_blocks); if (rc != BLOK_OK) return rc; }
    if (plan.kind == blok::LaunchKind::ListJoint || plan.kind == blok::LaunchKind::ListTwoLaunches) {
        const uint32_t per_search = (args.beam_tile / blok::kWaveW) * (args.beam_tile / blok::kWaveH);
        const int rc = live_list(ctx, args, stream, n_beams * n_frames, per_search);
        if (rc != BLOK_OK) return rc;
        for (uint32_t c = 0; c < blok::kListClasses; ++c) args.list.walkers[c] = plan.walkers_per_class[c];
        if (mode == blok::RayMode::Rect && ctx->list_classes) { const int rc2 = list_costs(ctx, args, blocks, stream); if (rc2 != BLOK_OK) return rc2; }
        auto& slot = ctx->beam_buffers[stream];
        slot.list_hint_valid = true; slot.list_hint_key = geometry_key;      // the searches of this launch write the hint
    }
    // static forms over a rectangle: longest-first order of a camera at rest, and walk waves for its live prefix only
    const bool static_form = plan.kind == blok::LaunchKind::TwoLaunches || plan.kind == blok::LaunchKind::Joint;
    // (round 4: a rank's tile launches too — one frame or several per launch — for a view at rest: ctx->order.rank_tiles)
    const bool rect = mode == blok::RayMode::Rect;
    const bool orderable = !capturing && ctx->order.enabled && static_form && ((rect && !frames) || (mode == blok::RayMode::Tiles && ctx->order.rank_tiles)) && n_beams &&
                           blocks >= blok::kOrderMinTiles && BLOK_XCD_MAP == 0 && blok::kBlock == 64;
    bool uniform_view = true;
    if (frames) for (uint32_t f = 1; f < frames->n_frames; ++f) uniform_view = uniform_view && camera_near(ctx, frames->cam[0], frames->cam[f]);
    blok::OrderPlan order_plan{};
    if (orderable) { const int rc = order_before_launch(ctx, args, blocks, stream, !busy, rect, uniform_view, &order_plan); if (rc != BLOK_OK) return rc; }
    else ctx->order.last_use = 0;
    uint32_t walk_blocks = blocks;
    if (args.order && args.rank_of && plan.may_use_prefix && args.launched <= blocks) {
        // the search wave of a beam tile that is live now walks any wave tile of its own without a walk wave (a changed view), and writes
        // the miss pixels of the empty ones
        if (ctx->order.prefix_limit && args.launched > ctx->order.prefix_limit) args.launched = ctx->order.prefix_limit;      // tests: more work for the search waves
        walk_blocks = args.launched;
        // what the previous prefix launch left to its search waves (read now: that launch is over, or nearly), counted afresh for this one
        // (a diagnostic, counted only for timed launches — blok_hip_set_timing: a clear in front of the frame and a copy behind it are two more
        // operations on the stream of every frame)
        if (ctx->timing) {
            ctx->order.last_fallback = *static_cast<volatile uint32_t*>(ctx->order.h_fallback.get());
            BLOK_HIP_TRY(ctx, hipMemsetAsync(ctx->order.d_fallback, 0, sizeof(uint32_t), stream));
            args.fallback_tiles = ctx->order.d_fallback;
        }
        // an order carried over by a shift says nothing about the strips of the screen the shift brings in: every tile there gets a walk
        // workgroup of its own, in front of the prefix (trace_kernels.h: TraceArgs::n_strip)
        if (args.order_sx || args.order_sy) {
            const uint32_t tiles_x = (args.w + blok::kTileW - 1u) / blok::kTileW, tiles_y = (args.h + blok::kTileH - 1u) / blok::kTileH;
            const bool left = args.order_sx * 2u <= tiles_x, top = args.order_sy * 2u <= tiles_y;      // the shift as a signed number: towards +x / +y brings in the low columns / rows
            // (each strip wider by what the shift leaves over near the edge it comes in through: a rotation stretches the screen there)
            const float res = ctx->order.have_residual && ctx->order.last_residual >= 0.0f ? std::min(ctx->order.last_residual, 8.0f) : 0.0f;
            const uint32_t extra = static_cast<uint32_t>(std::ceil(res));
            args.strip_nx = left ? args.order_sx : tiles_x - args.order_sx; if (args.strip_nx) args.strip_nx = std::min(args.strip_nx + extra, tiles_x);
            args.strip_ny = top ? args.order_sy : tiles_y - args.order_sy; if (args.strip_ny) args.strip_ny = std::min(args.strip_ny + extra, tiles_y);
            args.strip_x0 = left ? 0u : tiles_x - args.strip_nx;
            args.strip_y0 = top ? 0u : tiles_y - args.strip_ny;
            args.n_strip = args.strip_nx * tiles_y + (tiles_x - args.strip_nx) * args.strip_ny;
            walk_blocks += args.n_strip;
        }
    } else { args.rank_of = nullptr; args.launched = 0u; }
    if (ctx->timing && !capturing) BLOK_HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, stream));
    args.miss_in_walk = static_form && !args.rank_of && ctx->miss_in_walk ? 1u : 0u;
    // A view at rest keeps its beam bounds (beam_cache.h): rectangle launches of the automatic form — the explicit forms stay what they are
    // there to be compared with, a rank's tiles and several frames per launch are left alone — that are not being captured.
    blok::RestingPlan resting{};
    if (ctx->beam_cache.enabled && rect && !frames && !capturing && static_form && ctx->launch_form == blok::kFormAuto && n_beams && n_beams <= ctx->beam_cache.capacity) {
        const int rc = plan_resting(ctx, mode, args, stream, &resting);
        if (rc != BLOK_OK) { blok::commit_resting_launch(ctx->beam_cache.policy, resting, false, false); return rc; }
        // the searches that fill a slot write plain floats: the two-launch form, this once
        if (resting.cache.action == blok::BeamAction::Fill && plan.kind == blok::LaunchKind::Joint) { plan.kind = blok::LaunchKind::TwoLaunches; ctx->last_launch_kind = static_cast<int>(plan.kind); }
    }
    uint32_t fill_only = 0u;
    if (resting.walk != blok::RestingWalk::NotHit) fill_only = issue_resting(ctx, mode, args, resting, blocks, walk_blocks, n_beams, stream);      // last_launch_kind stays the policy's
    else
    switch (plan.kind) {
        case blok::LaunchKind::Walk:
            if (frames) blok::launch_tile_frames(args, fr, stream); else blok::launch_trace(mode, args, blocks, stream);
            break;
        case blok::LaunchKind::TwoLaunches:
            if (frames) blok::launch_tile_frames(args, fr, stream, walk_blocks);
            else { blok::launch_beam(mode, args, n_beams, stream); blok::launch_trace(mode, args, walk_blocks, stream); }
            break;
        case blok::LaunchKind::Queues: blok::launch_frame(mode, args, queue, frame_blocks, stream); break;
        case blok::LaunchKind::Joint: blok::launch_joint(mode, args, n_beams, walk_blocks, stream); break;
        case blok::LaunchKind::ListJoint: blok::launch_list_joint(mode, args, frames ? &fr : nullptr, n_beams * n_frames, plan.walkers, stream); break;
        case blok::LaunchKind::ListTwoLaunches:
            if (frames) blok::launch_beam_frames(args, fr, stream); else blok::launch_beam(mode, args, n_beams, stream);
            blok::launch_list_walk(mode, args, frames ? &fr : nullptr, plan.walkers, stream);
            break;
    }
    note_resting(ctx, resting, args, n_beams, fill_only);
    { const int rc = finish_resting(ctx, resting, hipGetLastError(), stream); if (rc != BLOK_OK) return rc; }
    if (ctx->timing && !capturing) { BLOK_HIP_TRY(ctx, hipEventRecord(ctx->ev_end, stream)); ctx->timed = true; }
    if (args.fallback_tiles) BLOK_HIP_TRY(ctx, hipMemcpyAsync(ctx->order.h_fallback, ctx->order.d_fallback, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    // (a packed launch leaves no clocks: a re-sort behind it would sort what the last one sorted — the order keeps its state and is not re-made)
    if (resting.list.use_list) order_plan.start_sort = false;
    if (orderable) { const int rc = order_after_launch(ctx, args, blocks, n_beams, stream, order_plan); if (rc != BLOK_OK) return rc; }
    if (facts.has_beam && !capturing) return note_frame_launch(ctx, stream);          // (behind the sort, if one was started: it belongs to this launch)
    return BLOK_OK;
}

}  // namespace blok_api
