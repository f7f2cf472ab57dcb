// The beam bounds of a view at rest, kept from launch to launch: which launches may reuse them, when a view is admitted, which slot it
// takes.  A pure function of a key and a little state, like launch_policy.h, so that the table can be tested on the host
// (tests/test_beam_cache_policy.py compiles this header with g++; nothing here touches HIP).  No reference counterpart: the reference
// lets Vulkan RT hardware cull boxes per ray (blok/src/renderer_raytracing.cpp:15-254) and has no pre-pass to keep.
//
// What is kept is the OUTPUT of beam_kernel alone (trace_kernels.hip; beam.h): one start parameter per beam tile, a pure function of the
// key below.  The records and the pixels of a frame are produced by walking every live tile of every frame as before; a launch that
// hits walks from the same start parameters its own searches would have found, so it writes the same bytes.  From its K-th hit on a slot
// also keeps the output of beam_refine_kernel — the same search over every wave tile's own pixels, a pure function of the same key — and
// later hits walk from those: valid lower bounds again, so the same bytes again, over a shorter walk.
#ifndef BLOK_BEAM_CACHE_H
#define BLOK_BEAM_CACHE_H
#include <stdint.h>
#include <string.h>

namespace blok {

// Every input of a rectangle launch's searches — the TraceArgs fields beam_block<Rect>, beam_start and beam_search read on the way to a
// start parameter (trace_kernels.hip, beam.h), and what stands for the memory behind them:
//   cam                          beam_start: the tile's central direction and side planes.  BYTE FOR BYTE: bounds of a nearby view are
//                                not conservative for this one (api_launch.hip's camera_near is a tolerance for scheduling, not for this)
//   x0, y0, w, h                 beam_block: the tile's pixel rectangle, cut at the launch rectangle's edge (beam_bx follows from w)
//   frame_w, frame_h             beam_start: pixel -> direction
//   beam_tile                    beam_block: the tile's size
//   beam_budget                  beam_search: node visits (0 = kBeamMaxVisits) — a search that runs out answers with a looser bound
//   tuning                       beam.h's compile-time constants that shape the answer the same way (coarsening eighths, stop level)
//   ray_mode                     Rect only is cached; in the key so that no other mode can ever match
//   levels, origin, voxel_bits   beam_search: the tree's cube; beam_start: voxel_size and its reciprocal (a power of two)
//   nodes_lo, nodes_hi           beam_search: the tree's address
//   world_version, tree_version  the tree's CONTENT: uploads count in both, a rebuild of the resident volume in tree_version alone (it
//                                keeps the view's order, api_volume.hip, but not its bounds)
// Not in the key, because no search reads it: the jitter (beam.h grows the frustum by a pixel on every side, which covers every
// sub-pixel offset), tmin / tmax, the outputs, the order and everything else that decides who writes what.
struct BeamKey {
    uint32_t cam[14];
    uint32_t x0, y0, w, h;
    uint32_t frame_w, frame_h;
    uint32_t beam_tile, beam_budget, tuning;
    uint32_t ray_mode;
    uint32_t levels;
    int32_t origin[3];
    uint32_t voxel_bits;
    uint32_t nodes_lo, nodes_hi;
    uint32_t world_version, tree_version;
};
static_assert(sizeof(BeamKey) == 33 * sizeof(uint32_t), "BeamKey is compared with memcmp: no padding");

inline bool beam_key_equal(const BeamKey& a, const BeamKey& b) { return memcmp(&a, &b, sizeof(BeamKey)) == 0; }

constexpr int kBeamCacheSlots = 4;             // as many views as the orders (api_internal.h: TileOrder::kSlots)

enum class BeamAction : int {
    Search = 0,                                // the launch runs its searches as ever
    Fill = 1,                                  // ... and they write into slot `slot`, which holds the view from here on
    Hit = 2,                                   // no searches: the walk reads slot `slot`
};
struct BeamCachePlan { BeamAction action; int slot; };

// A filled slot's finer bounds: one start parameter per wave tile, searched ONCE, behind the walk of the view's K-th hit (plan_beam_refine);
// later hits walk from them.  A camera that rests for fewer than K hits pays nothing for them.
enum class BeamRefine : uint8_t {
    None = 0,                                  // the slot holds the beam tiles' bounds only
    Now = 1,                                   // the launch that was just planned issues the finer searches (beam_refine_commit ends this state)
    Done = 2,                                  // the finer bounds are there (or on their way, on the stream of the launch that refined)
};
// The default K: the finer searches' duration over what a frame gains from them, rounded up to a power of two.  Measured at 4K over 1024^3
// (profiles/beam_refine_ab.txt): pose A 135 us over 23 us a frame = 5.9, pose B 354 us over 34 us = 10.3 (the grazing view: more live
// tiles, longer searches) -> 8 and 16; the larger, so that neither view pays for searches it has not yet earned back.
constexpr uint32_t kBeamRefineAfter = 16;
struct BeamRefinePlan { bool refine_now, use_fine; };

// A refined slot's packed list: the view's walked pixels regrouped, 64 to a wave, by the trips their walks took (trace_kernels.h: the packed
// walk).  A view at rest walks the very same rays every frame, so their lengths are measured ONCE: the slot's N-th hit from the finer bounds
// (N = list_after) walks with a counting kernel and issues the build behind it; the first later launch that finds the build finished adopts
// the list, and the slot's hits walk packed from then on.  Any assignment of pixels to lanes writes the same frame: the list is scheduling
// state and can be stale (another jitter under the same key) but never wrong — as long as it lists the pixels of THIS key's finer bounds,
// which is why it goes whenever they go.  One build is in flight at a time (it uses buffers of the context), whichever slot it is for.
enum class BeamList : uint8_t {
    None = 0,                                  // no list
    Now = 1,                                   // the launch that was just planned counts and issues the build (beam_list_commit ends this state)
    Building = 2,                              // the build is on its way, on the stream of the launch that counted
    Ready = 3,                                 // adopted: hits walk packed
};
// The default N, decided as K was: what the count launch and the build cost once over what a packed frame gains, rounded up to a power of
// two.  Measured at 4K over 1024^3 (profiles/packed_walk_ab.txt): the count launch takes 70 us (pose A) and 25 us (pose B) longer than the
// view's usual walk, the build 39 to 43 us and the table's sort about 54 us; a frame in flight gains 13 us and 7 to 9 us: ratios 12 and 14 to 17 -> 16.
// With the starts (below) the same rule gives 4 (profiles/own_start_ab.txt: about 180 and 140 us once, 54 and 60 us gained per frame in flight);
// left at 16 until it is changed together with K, with the benchmark's short per-pose windows measured.
constexpr uint32_t kBeamListAfter = 16;
struct BeamListPlan { bool count_now, use_list; int adopted; };      // adopted: the slot whose finished build this launch adopted (read its size now), or -1

// A packed list's starts: one start parameter per listed RAY, left by the count launch — the ray parameter at which that very ray entered
// the cell its answer lies in (trace_kernels.h: launch_trace_count_own) — and written beside the list by its build.  Unlike the searched
// bounds, which hold for every ray through a tile, a ray's own start holds for THAT ray and interval: the starts carry a key of their own,
// the inputs of primary_ray and of the walk's interval that the beam key leaves out, compared bit for bit.  A packed hit under another
// start key walks the same list from the finer bounds, as a list without starts does; the starts stay, and serve again when the counted
// values return.  They go wherever the list goes (beam_list_drop, a build that was not issued).
struct BeamStartKey { uint32_t jitter_clip[2], tmin, tmax; };
static_assert(sizeof(BeamStartKey) == 4 * sizeof(uint32_t), "BeamStartKey is compared with memcmp: no padding");
inline bool beam_start_key_equal(const BeamStartKey& a, const BeamStartKey& b) { return memcmp(&a, &b, sizeof(BeamStartKey)) == 0; }
enum class BeamStarts : int {
    None = 0,                                  // the launch walks no list, or a list without starts
    Use = 1,                                   // a packed hit of the counted rays: it walks from the starts
    OtherKey = 2,                              // a packed hit under another start key: from the finer bounds, this launch
};
struct BeamStartsPlan { bool count_own; BeamStarts use; };          // count_own: the launch told "count now" also leaves the starts
// Mode 5: beside its start every listed ray keeps the NODE its restarted walk ends in (trace_core.h: restart_node_word), left by the same
// count launch and gathered by the same build, and a packed hit from the starts makes that walk's last trip alone (walk_enter_node).  The
// node is a function of the ray, its interval and the tree: of the beam key (the tree's address and versions) and the start key together,
// so the words live and die with the starts — `nodes[slot]` is set where `starts[slot]` is, and only then — and serve exactly the launches
// the starts serve.

struct BeamCachePolicy {
    BeamKey key[kBeamCacheSlots];
    bool valid[kBeamCacheSlots];
    uint64_t last_use[kBeamCacheSlots];        // serial of the latest launch that filled or hit the slot
    BeamKey last;                              // key of the previous launch that asked
    bool have_last;
    uint64_t serial;                           // launches that asked so far
    BeamRefine refine[kBeamCacheSlots];        // reset by every fill (a refill, an eviction) and by beam_cache_clear
    uint32_t hits_since_fill[kBeamCacheSlots];
    uint32_t refine_after = kBeamRefineAfter;  // K (a debug setter: the tests need 1); kept by beam_cache_clear
    BeamList list[kBeamCacheSlots];            // reset with `refine`: a slot keeps its list exactly as long as it keeps its finer bounds
    uint32_t fine_hits[kBeamCacheSlots];       // hits that walked from the finer bounds since they were made
    uint32_t list_after = kBeamListAfter;      // N (a debug setter); kept by beam_cache_clear
    bool own_starts = true;                    // the lists carry starts (a mode: kept by beam_cache_clear)
    bool starts[kBeamCacheSlots];              // the slot's list (built, or being counted and built) carries starts, counted under start_key
    BeamStartKey start_key[kBeamCacheSlots];
    bool node_restart = true;                  // the lists with starts carry node words as well (mode 5: kept by beam_cache_clear)
    bool nodes[kBeamCacheSlots];               // the slot's list carries them (never without starts[slot])
    int building = -1;                         // the slot the build in flight writes (-1: none is in flight)
    bool building_stale = false;               // ... and that slot has been refilled or cleared since: the build finishes into a list nobody adopts
};

// The slot's finer bounds are gone (a refill, an eviction, a clear): its list goes with them.  A build still in flight for it stays "in
// flight" — it is writing the slot's buffers, and the context's — until a launch sees it finished.
inline void beam_list_drop(BeamCachePolicy& s, int slot) {
    s.list[slot] = BeamList::None; s.fine_hits[slot] = 0u; s.starts[slot] = false; s.nodes[slot] = false;
    if (s.building == slot) s.building_stale = true;
}

inline void beam_cache_clear(BeamCachePolicy& s) {
    for (int k = 0; k < kBeamCacheSlots; ++k) { s.valid[k] = false; s.last_use[k] = 0u; s.refine[k] = BeamRefine::None; s.hits_since_fill[k] = 0u; beam_list_drop(s, k); }
    s.have_last = false;
}

// Behind a wait for the whole device: no build is in flight any more (and a list that had not been adopted by then is not kept).
inline void beam_list_settle(BeamCachePolicy& s) {
    if (s.building >= 0 && s.building < kBeamCacheSlots && s.list[s.building] == BeamList::Building) s.list[s.building] = BeamList::None;
    s.building = -1; s.building_stale = false;
}

// Admission: a view is cached when the same key arrives a second time IN A ROW — that launch still searches, into a slot — and hits
// from the third launch on.  A camera in motion never repeats a key, so it never fills, never evicts and never pays anything.
// Slots: an empty one, else the one used longest ago.
inline BeamCachePlan plan_beam_cache(BeamCachePolicy& s, const BeamKey& k) {
    s.serial += 1u;
    const bool again = s.have_last && beam_key_equal(s.last, k);
    s.last = k; s.have_last = true;
    for (int i = 0; i < kBeamCacheSlots; ++i)
        if (s.valid[i] && beam_key_equal(s.key[i], k)) {
            s.last_use[i] = s.serial;
            if (s.hits_since_fill[i] != UINT32_MAX) s.hits_since_fill[i] += 1u;
            return {BeamAction::Hit, i};
        }
    if (!again) return {BeamAction::Search, -1};
    int target = -1;
    for (int i = 0; i < kBeamCacheSlots && target < 0; ++i) if (!s.valid[i]) target = i;
    if (target < 0) { target = 0; for (int i = 1; i < kBeamCacheSlots; ++i) if (s.last_use[i] < s.last_use[target]) target = i; }
    s.key[target] = k; s.valid[target] = true; s.last_use[target] = s.serial;
    s.refine[target] = BeamRefine::None; s.hits_since_fill[target] = 0u;
    beam_list_drop(s, target);
    return {BeamAction::Fill, target};
}

// Behind plan_beam_cache, for the same launch: does it issue the finer searches, does it walk from the finer bounds?  "Refine now" is said
// once per fill, on the slot's K-th hit (the first eligible hit from the K-th on, should K have been lowered meanwhile); never for a search
// or a fill, so never for a view that is not admitted.  eligible: the launch's geometry allows finer bounds at all and they are switched on
// (a property of the key and of the context, the same for every hit of a slot).  The launch that refines still walks from the coarse bounds.
inline BeamRefinePlan plan_beam_refine(BeamCachePolicy& s, const BeamCachePlan& p, bool eligible) {
    if (p.action != BeamAction::Hit || p.slot < 0 || p.slot >= kBeamCacheSlots || !eligible) return {false, false};
    if (s.refine[p.slot] == BeamRefine::Done) return {false, true};
    if (s.refine[p.slot] == BeamRefine::None && s.hits_since_fill[p.slot] >= (s.refine_after ? s.refine_after : 1u)) {
        s.refine[p.slot] = BeamRefine::Now;
        return {true, false};
    }
    return {false, false};
}

// The launch that was told "refine now" has issued its searches (issued: the finer bounds are kept) or could not (the slot stays as it
// was filled, and is asked again K hits later).
inline void beam_refine_commit(BeamCachePolicy& s, int slot, bool issued) {
    if (slot < 0 || slot >= kBeamCacheSlots || s.refine[slot] != BeamRefine::Now) return;
    s.refine[slot] = issued ? BeamRefine::Done : BeamRefine::None;
    if (!issued) s.hits_since_fill[slot] = 0u;
}

// Behind plan_beam_refine, for the same launch.  build_finished: the event behind the build in flight has been seen complete (asked only
// while s.building >= 0) — then the build is over whoever launches, and its slot, unless it was dropped meanwhile, has its list from this
// launch on.  Then: does this launch walk packed, or count and build?  Only a hit that walks from the finer bounds can do either; "count
// now" is said once per set of finer bounds, on its N-th such hit or the first after it at which no other build is in flight.
// eligible: the packed walk applies to the launch's geometry and is switched on.
inline BeamListPlan plan_beam_list(BeamCachePolicy& s, const BeamCachePlan& p, const BeamRefinePlan& f, bool eligible, bool build_finished) {
    BeamListPlan out{false, false, -1};
    if (s.building >= 0 && build_finished) {
        if (!s.building_stale && s.building < kBeamCacheSlots && s.list[s.building] == BeamList::Building) { s.list[s.building] = BeamList::Ready; out.adopted = s.building; }
        s.building = -1; s.building_stale = false;
    }
    if (p.action != BeamAction::Hit || p.slot < 0 || p.slot >= kBeamCacheSlots || !f.use_fine || !eligible) return out;
    if (s.list[p.slot] == BeamList::Ready) { out.use_list = true; return out; }
    if (s.list[p.slot] != BeamList::None) return out;
    if (s.fine_hits[p.slot] != UINT32_MAX) s.fine_hits[p.slot] += 1u;
    if (s.building < 0 && s.fine_hits[p.slot] >= (s.list_after ? s.list_after : 1u)) { s.list[p.slot] = BeamList::Now; out.count_now = true; }
    return out;
}

// Behind plan_beam_list, for the same launch, k its start key.  The launch told "count now" is told whether to leave the starts as well (the
// mode), and they are its key's from then on; a launch told "use the list" is told whether the list's starts are its own rays'.
inline BeamStartsPlan plan_beam_starts(BeamCachePolicy& s, const BeamCachePlan& p, const BeamListPlan& l, const BeamStartKey& k) {
    if (p.action != BeamAction::Hit || p.slot < 0 || p.slot >= kBeamCacheSlots) return {false, BeamStarts::None};
    if (l.count_now) {
        s.starts[p.slot] = s.own_starts;
        s.nodes[p.slot] = s.own_starts && s.node_restart;
        if (s.own_starts) s.start_key[p.slot] = k;
        return {s.own_starts, BeamStarts::None};
    }
    if (!l.use_list || !s.starts[p.slot]) return {false, BeamStarts::None};
    return {false, beam_start_key_equal(s.start_key[p.slot], k) ? BeamStarts::Use : BeamStarts::OtherKey};
}

// The launch that was told "count now" has issued its build and the event behind it (issued), or could not: the slot stays without a list
// and is asked again N hits later.
inline void beam_list_commit(BeamCachePolicy& s, int slot, bool issued) {
    if (slot < 0 || slot >= kBeamCacheSlots || s.list[slot] != BeamList::Now) return;
    s.list[slot] = issued ? BeamList::Building : BeamList::None;
    if (issued) { s.building = slot; s.building_stale = false; }
    else { s.fine_hits[slot] = 0u; s.starts[slot] = false; s.nodes[slot] = false; }
}

// The launch told to count the starts cannot leave node words (a tree whose node indices do not fit the word): the slot's list has starts alone.
inline void beam_nodes_decline(BeamCachePolicy& s, int slot) {
    if (slot >= 0 && slot < kBeamCacheSlots) s.nodes[slot] = false;
}
// Does a launch that plan_beam_starts told `plan` count the node words / walk from them?
inline bool beam_nodes_count(const BeamCachePolicy& s, const BeamCachePlan& p, const BeamStartsPlan& plan) {
    return plan.count_own && p.slot >= 0 && p.slot < kBeamCacheSlots && s.nodes[p.slot];
}
inline bool beam_nodes_use(const BeamCachePolicy& s, const BeamCachePlan& p, const BeamStartsPlan& plan) {
    return plan.use == BeamStarts::Use && p.slot >= 0 && p.slot < kBeamCacheSlots && s.node_restart && s.nodes[p.slot];
}

// ---- one launch over the cache: the four plans above in their order, and what they come to ------------------------------------------------
// What the policy cannot know itself.
struct RestingFacts {
    bool refine_eligible;                      // plan_beam_refine's `eligible`
    bool list_eligible;                        // plan_beam_list's `eligible`
    bool build_finished;                       // ... and its `build_finished` (asked only while s.building >= 0)
    bool node_words;                           // a count launch can leave node words: the tree's node indices fit them, and every slot has somewhere to put them
    BeamStartKey start_key;
};
// What a launch over the cache does: one value, computed here and acted on in one place (api_launch.hip: issue_resting).
enum class RestingWalk : int {
    NotHit = 0,                                // a search or a fill: the launch policy's form
    Coarse,                                    // a hit: the live prefix from the beam tiles' bounds (fine.refine_now: the finer searches behind it)
    Fine,                                      // ... from the finer bounds
    Count,                                     // every wave tile from the finer bounds, counting trips; the build behind it
    CountStarts,                               // ... leaving every ray's own start as well
    CountNodes,                                // ... and its node word
    PackedFine,                                // the list, from the finer bounds (a list without starts, or another start key)
    PackedStarts,                              // the list, every ray from its own start
    PackedNodes,                               // the list, every ray re-entered at its node
};
struct RestingPlan {
    BeamCachePlan cache{BeamAction::Search, -1};
    BeamRefinePlan fine{false, false};
    BeamListPlan list{false, false, -1};
    BeamStartsPlan starts{false, BeamStarts::None};
    RestingWalk walk = RestingWalk::NotHit;
};
inline bool resting_counts(RestingWalk w) { return w == RestingWalk::Count || w == RestingWalk::CountStarts || w == RestingWalk::CountNodes; }
inline bool resting_packed(RestingWalk w) { return w == RestingWalk::PackedFine || w == RestingWalk::PackedStarts || w == RestingWalk::PackedNodes; }

inline RestingPlan plan_resting_launch(BeamCachePolicy& s, const BeamKey& k, const RestingFacts& facts) {
    RestingPlan r;
    r.cache = plan_beam_cache(s, k);
    r.fine = plan_beam_refine(s, r.cache, facts.refine_eligible);
    r.list = plan_beam_list(s, r.cache, r.fine, facts.list_eligible, facts.build_finished);
    r.starts = plan_beam_starts(s, r.cache, r.list, facts.start_key);
    if (beam_nodes_count(s, r.cache, r.starts) && !facts.node_words) beam_nodes_decline(s, r.cache.slot);      // the slot's list has starts alone, for good
    if (r.cache.action != BeamAction::Hit) r.walk = RestingWalk::NotHit;
    else if (r.list.use_list) r.walk = r.starts.use != BeamStarts::Use ? RestingWalk::PackedFine : beam_nodes_use(s, r.cache, r.starts) ? RestingWalk::PackedNodes : RestingWalk::PackedStarts;
    else if (r.list.count_now) r.walk = !r.starts.count_own ? RestingWalk::Count : beam_nodes_count(s, r.cache, r.starts) ? RestingWalk::CountNodes : RestingWalk::CountStarts;
    else r.walk = r.fine.use_fine ? RestingWalk::Fine : RestingWalk::Coarse;
    return r;
}

// Behind the launch: what it was told to issue once has been issued (the finer searches and the event behind them; the build and its
// event), or could not be — also a launch that failed before it issued anything.
inline void commit_resting_launch(BeamCachePolicy& s, const RestingPlan& r, bool refine_issued, bool list_issued) {
    if (r.fine.refine_now) beam_refine_commit(s, r.cache.slot, refine_issued);
    if (r.list.count_now) beam_list_commit(s, r.cache.slot, list_issued);
}

}  // namespace blok
#endif
