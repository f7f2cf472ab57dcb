// TEST INFRASTRUCTURE: exposes the packed-list part of blok_amd/csrc/hip/beam_cache.h (pure C++, no HIP) — plan_beam_list, beam_list_commit,
// beam_list_settle, N — to tests/test_beam_list_policy.py.  Built with -DBEAM_LIST_SHIM_MAIN it is a stand-alone program instead (a walk through
// the same decisions, for a sanitizer build).
#include "beam_cache.h"

extern "C" {
unsigned beam_list_key_words() { return sizeof(blok::BeamKey) / sizeof(uint32_t); }
unsigned beam_list_default_after() { return blok::kBeamListAfter; }
void* beam_list_new() { auto* s = new blok::BeamCachePolicy{}; blok::beam_cache_clear(*s); s->refine_after = 1u; return s; }
void beam_list_delete(void* s) { delete static_cast<blok::BeamCachePolicy*>(s); }
void beam_list_reset(void* s) { blok::beam_cache_clear(*static_cast<blok::BeamCachePolicy*>(s)); }
void beam_list_settle(void* s) { blok::beam_list_settle(*static_cast<blok::BeamCachePolicy*>(s)); }
void beam_list_set_after(void* s, unsigned n) { static_cast<blok::BeamCachePolicy*>(s)->list_after = n; }
unsigned beam_list_after(void* s) { return static_cast<blok::BeamCachePolicy*>(s)->list_after; }
int beam_list_state(void* s, int slot) { return static_cast<int>(static_cast<blok::BeamCachePolicy*>(s)->list[slot]); }
int beam_list_building(void* s) { const auto& p = *static_cast<blok::BeamCachePolicy*>(s); return p.building < 0 ? -1 : p.building | (p.building_stale ? 256 : 0); }
// One launch, as api_launch.hip asks: plan_resting_launch (K = 1) with what the event query said, then commit_resting_launch: the finer
// searches always issued, the build as `issued` says (< 0: no commit for a launch told to count).
// -> action (0 search, 1 fill, 2 hit) | refine_now << 4 | use_fine << 5 | count_now << 6 | use_list << 7 | (adopted slot + 1) << 8; the slot through the pointer.
int beam_list_launch(void* sp, const uint32_t* key, int eligible, int build_finished, int issued, int* slot) {
    auto& s = *static_cast<blok::BeamCachePolicy*>(sp);
    blok::BeamKey k;
    memcpy(&k, key, sizeof(k));
    const blok::RestingPlan r = blok::plan_resting_launch(s, k, {true, eligible != 0, build_finished != 0, false, {}});
    if (!r.list.count_now || issued >= 0) blok::commit_resting_launch(s, r, true, issued != 0);
    *slot = r.cache.slot;
    return static_cast<int>(r.cache.action) | (r.fine.refine_now ? 16 : 0) | (r.fine.use_fine ? 32 : 0) | (r.list.count_now ? 64 : 0) | (r.list.use_list ? 128 : 0) | ((r.list.adopted + 1) << 8);
}
}

#ifdef BEAM_LIST_SHIM_MAIN
#include <stdio.h>
#include <initializer_list>
int main() {
    void* s = beam_list_new();
    const unsigned n = beam_list_key_words();
    uint32_t key[64] = {};
    int slot = -1, bad = 0;
    // six views through four slots, twice round, N = 1, 2, 4: per visit a search, a fill, the hit that refines, N - 1 hits from the finer
    // bounds, the hit that counts, one while the build runs, the hit that adopts and walks packed, one more packed hit — every eviction
    // starts a view over
    for (unsigned after : {1u, 2u, 4u}) {
        beam_list_reset(s); beam_list_settle(s);
        beam_list_set_after(s, after);
        for (int round = 0; round < 2; ++round)
            for (uint32_t view = 0; view < 6; ++view) {
                for (unsigned i = 0; i < n; ++i) key[i] = view * 977u + i;
                bad += beam_list_launch(s, key, 1, 0, 1, &slot) != 0;
                bad += beam_list_launch(s, key, 1, 0, 1, &slot) != 1;
                bad += slot < 0 || slot >= blok::kBeamCacheSlots || beam_list_state(s, slot) != 0;
                bad += beam_list_launch(s, key, 1, 0, 1, &slot) != (2 | 16);
                for (unsigned h = 1; h < after; ++h) bad += beam_list_launch(s, key, 1, 0, 1, &slot) != (2 | 32);
                bad += beam_list_launch(s, key, 1, 0, 1, &slot) != (2 | 32 | 64);
                bad += beam_list_state(s, slot) != 2 || beam_list_building(s) != slot;
                bad += beam_list_launch(s, key, 1, 0, 1, &slot) != (2 | 32);
                bad += beam_list_launch(s, key, 1, 1, 1, &slot) != (2 | 32 | 128 | ((slot + 1) << 8));
                bad += beam_list_launch(s, key, 1, 1, 1, &slot) != (2 | 32 | 128);
                bad += beam_list_building(s) != -1;
            }
    }
    // a build that could not be issued; a geometry that is not eligible; commits for slots that do not exist; a settle in mid-build
    beam_list_reset(s); beam_list_settle(s);
    beam_list_set_after(s, 1);
    for (unsigned i = 0; i < n; ++i) key[i] = i;
    beam_list_launch(s, key, 1, 0, 1, &slot); beam_list_launch(s, key, 1, 0, 1, &slot); beam_list_launch(s, key, 1, 0, 1, &slot);
    bad += beam_list_launch(s, key, 1, 0, 0, &slot) != (2 | 32 | 64);
    bad += beam_list_state(s, slot) != 0 || beam_list_building(s) != -1;
    bad += beam_list_launch(s, key, 0, 0, 1, &slot) != (2 | 32);
    bad += beam_list_launch(s, key, 1, 0, 1, &slot) != (2 | 32 | 64);
    beam_list_settle(s);
    bad += beam_list_state(s, slot) != 0 || beam_list_building(s) != -1;
    blok::beam_list_commit(*static_cast<blok::BeamCachePolicy*>(s), -1, true);
    blok::beam_list_commit(*static_cast<blok::BeamCachePolicy*>(s), blok::kBeamCacheSlots, true);
    bad += blok::plan_beam_list(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Hit, blok::kBeamCacheSlots}, {false, true}, true, false).count_now;
    bad += blok::plan_beam_list(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Hit, -1}, {false, true}, true, false).use_list;
    beam_list_delete(s);
    printf("beam list policy: %d mismatches\n", bad);
    return bad != 0;
}
#endif
