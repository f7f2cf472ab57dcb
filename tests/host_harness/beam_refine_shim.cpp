// TEST INFRASTRUCTURE: exposes the refinement half of blok_amd/csrc/hip/beam_cache.h (pure C++, no HIP) — plan_beam_refine, beam_refine_commit,
// K — to tests/test_beam_refine_policy.py.  Built with -DBEAM_REFINE_SHIM_MAIN it is a stand-alone program instead (a walk through the same
// decisions, for a sanitizer build).
#include "beam_cache.h"

extern "C" {
unsigned beam_refine_key_words() { return sizeof(blok::BeamKey) / sizeof(uint32_t); }
unsigned beam_refine_default_after() { return blok::kBeamRefineAfter; }
void* beam_refine_new() { auto* s = new blok::BeamCachePolicy{}; blok::beam_cache_clear(*s); return s; }
void beam_refine_delete(void* s) { delete static_cast<blok::BeamCachePolicy*>(s); }
void beam_refine_reset(void* s) { blok::beam_cache_clear(*static_cast<blok::BeamCachePolicy*>(s)); }
void beam_refine_set_after(void* s, unsigned k) { static_cast<blok::BeamCachePolicy*>(s)->refine_after = k; }
unsigned beam_refine_after(void* s) { return static_cast<blok::BeamCachePolicy*>(s)->refine_after; }
int beam_refine_state(void* s, int slot) { return static_cast<int>(static_cast<blok::BeamCachePolicy*>(s)->refine[slot]); }
// One launch, as api_launch.hip asks: plan_resting_launch (no packed walk), then (issued >= 0) commit_resting_launch.
// -> action (0 search, 1 fill, 2 hit) | refine_now << 4 | use_fine << 5; the slot through the pointer.
int beam_refine_launch(void* sp, const uint32_t* key, int eligible, int issued, int* slot) {
    auto& s = *static_cast<blok::BeamCachePolicy*>(sp);
    blok::BeamKey k;
    memcpy(&k, key, sizeof(k));
    const blok::RestingPlan r = blok::plan_resting_launch(s, k, {eligible != 0, false, false, false, {}});
    if (issued >= 0) blok::commit_resting_launch(s, r, issued != 0, false);
    *slot = r.cache.slot;
    return static_cast<int>(r.cache.action) | (r.fine.refine_now ? 16 : 0) | (r.fine.use_fine ? 32 : 0);
}
}

#ifdef BEAM_REFINE_SHIM_MAIN
#include <stdio.h>
#include <initializer_list>
int main() {
    void* s = beam_refine_new();
    const unsigned n = beam_refine_key_words();
    uint32_t key[64] = {};
    int slot = -1, bad = 0;
    // six views through four slots, twice round, K = 1, 2, 3, 5: per visit a search, a fill, K - 1 plain hits, the hit that refines, two
    // hits from the finer bounds — every eviction starts a view over
    for (unsigned k_after : {1u, 2u, 3u, 5u}) {
        beam_refine_reset(s);
        beam_refine_set_after(s, k_after);
        for (int round = 0; round < 2; ++round)
            for (uint32_t view = 0; view < 6; ++view) {
                for (unsigned i = 0; i < n; ++i) key[i] = view * 977u + i;
                bad += beam_refine_launch(s, key, 1, 1, &slot) != 0;
                bad += beam_refine_launch(s, key, 1, 1, &slot) != 1;
                bad += slot < 0 || slot >= blok::kBeamCacheSlots || beam_refine_state(s, slot) != 0;
                for (unsigned h = 1; h < k_after; ++h) bad += beam_refine_launch(s, key, 1, 1, &slot) != 2;
                bad += beam_refine_launch(s, key, 1, 1, &slot) != (2 | 16);
                bad += beam_refine_launch(s, key, 1, 1, &slot) != (2 | 32);
                bad += beam_refine_launch(s, key, 1, 1, &slot) != (2 | 32);
            }
    }
    // a launch that could not issue its searches; a geometry that is not eligible; commits for slots that do not exist
    beam_refine_reset(s);
    beam_refine_set_after(s, 1);
    for (unsigned i = 0; i < n; ++i) key[i] = i;
    beam_refine_launch(s, key, 1, 1, &slot); beam_refine_launch(s, key, 1, 1, &slot);
    bad += beam_refine_launch(s, key, 1, 0, &slot) != (2 | 16);
    bad += beam_refine_state(s, slot) != 0;
    bad += beam_refine_launch(s, key, 0, 1, &slot) != 2;
    bad += beam_refine_launch(s, key, 1, 1, &slot) != (2 | 16);
    bad += beam_refine_launch(s, key, 0, 1, &slot) != 2;
    blok::beam_refine_commit(*static_cast<blok::BeamCachePolicy*>(s), -1, true);
    blok::beam_refine_commit(*static_cast<blok::BeamCachePolicy*>(s), blok::kBeamCacheSlots, true);
    bad += blok::plan_beam_refine(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Hit, blok::kBeamCacheSlots}, true).refine_now;
    bad += blok::plan_beam_refine(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Hit, -1}, true).use_fine;
    beam_refine_delete(s);
    printf("beam refine policy: %d mismatches\n", bad);
    return bad != 0;
}
#endif
