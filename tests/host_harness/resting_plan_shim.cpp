// TEST INFRASTRUCTURE: exposes what one launch over the cache comes to in blok_amd/csrc/hip/beam_cache.h (pure C++, no HIP) — plan_resting_launch,
// its one value, the node words' decline, commit_resting_launch — to tests/test_resting_plan_policy.py.  Built with -DRESTING_PLAN_SHIM_MAIN it
// is a stand-alone program instead (a walk through the same decisions, for a sanitizer build).
#include "beam_cache.h"

extern "C" {
unsigned resting_plan_key_words() { return sizeof(blok::BeamKey) / sizeof(uint32_t); }
// K = 1 and N = `after`; own, nodes: the modes (4: own; 5: own and nodes)
void* resting_plan_new(int own, int nodes, unsigned after) {
    auto* s = new blok::BeamCachePolicy{};
    blok::beam_cache_clear(*s);
    s->refine_after = 1u; s->list_after = after; s->own_starts = own != 0; s->node_restart = nodes != 0;
    return s;
}
void resting_plan_delete(void* s) { delete static_cast<blok::BeamCachePolicy*>(s); }
void resting_plan_reset(void* s) { blok::beam_cache_clear(*static_cast<blok::BeamCachePolicy*>(s)); }
void resting_plan_settle(void* s) { blok::beam_list_settle(*static_cast<blok::BeamCachePolicy*>(s)); }
void resting_plan_set_node_restart(void* s, int nodes) { static_cast<blok::BeamCachePolicy*>(s)->node_restart = nodes != 0; }
int resting_plan_refine_state(void* s, int slot) { return static_cast<int>(static_cast<blok::BeamCachePolicy*>(s)->refine[slot]); }
int resting_plan_list_state(void* s, int slot) { return static_cast<int>(static_cast<blok::BeamCachePolicy*>(s)->list[slot]); }
int resting_plan_has_starts(void* s, int slot) { return static_cast<blok::BeamCachePolicy*>(s)->starts[slot] ? 1 : 0; }
int resting_plan_has_nodes(void* s, int slot) { return static_cast<blok::BeamCachePolicy*>(s)->nodes[slot] ? 1 : 0; }
// One launch, as api_launch.hip asks.  facts: 1 refine eligible | 2 list eligible | 4 build finished | 8 node words can be kept; the start
// key as bits; refine_issued, list_issued: what commit_resting_launch is told (either < 0: no commit, the launch is still "now").
// -> the one value (beam_cache.h: RestingWalk, 0 .. 8) | the four plans it was made from: action << 4 | refine_now << 6 | use_fine << 7 |
// count_now << 8 | use_list << 9 | count_own << 10 | use << 11 | (adopted slot + 1) << 13 | the slot has node words << 16; the slot through the pointer.
int resting_plan_launch(void* sp, const uint32_t* key, const uint32_t* start_key, int facts, int refine_issued, int list_issued, int* slot) {
    auto& s = *static_cast<blok::BeamCachePolicy*>(sp);
    blok::BeamKey k;
    memcpy(&k, key, sizeof(k));
    blok::RestingFacts f{(facts & 1) != 0, (facts & 2) != 0, (facts & 4) != 0, (facts & 8) != 0, {}};
    memcpy(&f.start_key, start_key, sizeof(f.start_key));
    const blok::RestingPlan r = blok::plan_resting_launch(s, k, f);
    const bool has_nodes = r.cache.slot >= 0 && s.nodes[r.cache.slot];      // as the plan saw them: a failed build drops them
    if (refine_issued >= 0 && list_issued >= 0) blok::commit_resting_launch(s, r, refine_issued != 0, list_issued != 0);
    *slot = r.cache.slot;
    return static_cast<int>(r.walk) | (static_cast<int>(r.cache.action) << 4) | (r.fine.refine_now ? 1 << 6 : 0) | (r.fine.use_fine ? 1 << 7 : 0) | (r.list.count_now ? 1 << 8 : 0) |
           (r.list.use_list ? 1 << 9 : 0) | (r.starts.count_own ? 1 << 10 : 0) | (static_cast<int>(r.starts.use) << 11) | ((r.list.adopted + 1) << 13) | (has_nodes ? 1 << 16 : 0);
}
}

#ifdef RESTING_PLAN_SHIM_MAIN
#include <stdio.h>
int main() {
    using W = blok::RestingWalk;
    const unsigned n = resting_plan_key_words();
    uint32_t key[64] = {};
    const uint32_t counted[4] = {0u, 0u, 0x3A83126Fu, 0x461C4000u}, jittered[4] = {0x3E800000u, 0xBE800000u, 0x3A83126Fu, 0x461C4000u};
    int slot = -1, bad = 0;
    const auto walk = [&](void* s, const uint32_t* sk, int facts, int refine_issued = 1, int list_issued = 1) {
        return static_cast<W>(resting_plan_launch(s, key, sk, facts, refine_issued, list_issued, &slot) & 15);
    };
    // the modes x node words can be kept or cannot; six views through four slots, twice round: a search, a fill, the hit that refines, the hit
    // that counts, one while the build runs, the hit that adopts, packed hits under the counted key, another key, the counted key again
    for (int own = 0; own < 2; ++own)
        for (int nodes = 0; nodes < 2; ++nodes)
            for (int can = 0; can < 2; ++can) {
                void* s = resting_plan_new(own, nodes, 1u);
                const int facts = 1 | 2 | (can ? 8 : 0);
                const bool words = own && nodes && can;
                const W count = !own ? W::Count : words ? W::CountNodes : W::CountStarts, packed = !own ? W::PackedFine : words ? W::PackedNodes : W::PackedStarts;
                for (int round = 0; round < 2; ++round)
                    for (uint32_t view = 0; view < 6; ++view) {
                        for (unsigned i = 0; i < n; ++i) key[i] = view * 977u + i;
                        bad += walk(s, counted, facts) != W::NotHit;
                        bad += walk(s, counted, facts) != W::NotHit || slot < 0 || slot >= blok::kBeamCacheSlots;
                        bad += walk(s, counted, facts) != W::Coarse || resting_plan_refine_state(s, slot) != 2;
                        bad += walk(s, counted, facts) != count || resting_plan_has_starts(s, slot) != own || resting_plan_has_nodes(s, slot) != (words ? 1 : 0);
                        bad += walk(s, jittered, facts) != W::Fine;
                        bad += walk(s, counted, facts | 4) != packed;
                        bad += walk(s, jittered, 1 | 2 | 8) != W::PackedFine;      // another start key; and node words that could be kept NOW revive nothing
                        bad += walk(s, counted, 1 | 2 | 8) != packed || resting_plan_has_nodes(s, slot) != (words ? 1 : 0);
                        bad += walk(s, counted, 1 | 2) != packed;                  // only a count launch declines
                        bad += walk(s, counted, 1) != W::Fine || walk(s, counted, 2) != W::Coarse;      // not eligible for the list; for the finer bounds
                    }
                // an issue that fails at the refine, then at the build: asked again, and a failed build leaves neither starts nor node words
                resting_plan_reset(s); resting_plan_settle(s);
                for (unsigned i = 0; i < n; ++i) key[i] = i;
                walk(s, counted, facts); walk(s, counted, facts);
                bad += walk(s, counted, facts, 0, 0) != W::Coarse || resting_plan_refine_state(s, slot) != 0;
                bad += walk(s, counted, facts) != W::Coarse || resting_plan_refine_state(s, slot) != 2;
                bad += walk(s, counted, facts, 0, 0) != count || resting_plan_list_state(s, slot) != 0 || resting_plan_has_starts(s, slot) != 0 || resting_plan_has_nodes(s, slot) != 0;
                bad += walk(s, counted, facts) != count || resting_plan_list_state(s, slot) != 2;
                resting_plan_delete(s);
            }
    printf("resting plan policy: %d mismatches\n", bad);
    return bad != 0;
}
#endif
