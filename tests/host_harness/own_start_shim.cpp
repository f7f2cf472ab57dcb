// TEST INFRASTRUCTURE: exposes the starts of a packed list in blok_amd/csrc/hip/beam_cache.h (pure C++, no HIP) — plan_beam_starts behind
// plan_beam_list, the start key, and everything that drops them — to tests/test_own_start_host.py.  Built with -DOWN_START_SHIM_MAIN it is a
// stand-alone program instead (a walk through the same decisions, for a sanitizer build).
#include "beam_cache.h"

extern "C" {
unsigned own_start_key_words() { return sizeof(blok::BeamKey) / sizeof(uint32_t); }
unsigned own_start_default_after() { return blok::kBeamListAfter; }
void* own_start_new(int own) { auto* s = new blok::BeamCachePolicy{}; blok::beam_cache_clear(*s); s->refine_after = 1u; s->list_after = 1u; s->own_starts = own != 0; return s; }
void own_start_delete(void* s) { delete static_cast<blok::BeamCachePolicy*>(s); }
void own_start_reset(void* s) { blok::beam_cache_clear(*static_cast<blok::BeamCachePolicy*>(s)); }
void own_start_settle(void* s) { blok::beam_list_settle(*static_cast<blok::BeamCachePolicy*>(s)); }
void own_start_set_mode(void* s, int own) { static_cast<blok::BeamCachePolicy*>(s)->own_starts = own != 0; }
int own_start_mode(void* s) { return static_cast<blok::BeamCachePolicy*>(s)->own_starts ? 1 : 0; }
int own_start_list_state(void* s, int slot) { return static_cast<int>(static_cast<blok::BeamCachePolicy*>(s)->list[slot]); }
int own_start_has(void* s, int slot) { return static_cast<blok::BeamCachePolicy*>(s)->starts[slot] ? 1 : 0; }
// One launch, as api_launch.hip asks: plan_resting_launch (K = 1) with what the event query said and the launch's start key (jitter x,
// jitter y, tmin, tmax as bits), then commit_resting_launch: the finer searches always issued, the build as `issued` says (< 0: no commit
// for a launch told to count).
// -> action (0 search, 1 fill, 2 hit) | count_now << 6 | use_list << 7 | count_own << 8 | use (0 none, 1 from the starts, 2 another key) << 9; the slot through the pointer.
int own_start_launch(void* sp, const uint32_t* key, const uint32_t* start_key, int build_finished, int issued, int* slot) {
    auto& s = *static_cast<blok::BeamCachePolicy*>(sp);
    blok::BeamKey k;
    memcpy(&k, key, sizeof(k));
    blok::BeamStartKey sk;
    memcpy(&sk, start_key, sizeof(sk));
    const blok::RestingPlan r = blok::plan_resting_launch(s, k, {true, true, build_finished != 0, true, sk});
    if (!r.list.count_now || issued >= 0) blok::commit_resting_launch(s, r, true, issued != 0);
    *slot = r.cache.slot;
    return static_cast<int>(r.cache.action) | (r.list.count_now ? 64 : 0) | (r.list.use_list ? 128 : 0) | (r.starts.count_own ? 256 : 0) | (static_cast<int>(r.starts.use) << 9);
}
}

#ifdef OWN_START_SHIM_MAIN
#include <stdio.h>
#include <initializer_list>
int main() {
    const unsigned n = own_start_key_words();
    uint32_t key[64] = {};
    const uint32_t counted[4] = {0u, 0u, 0x3A83126Fu, 0x461C4000u}, jittered[4] = {0x3E800000u, 0xBE800000u, 0x3A83126Fu, 0x461C4000u};
    const uint32_t nearer[4] = {0u, 0u, 0x3F800000u, 0x461C4000u}, shorter[4] = {0u, 0u, 0x3A83126Fu, 0x42C80000u}, minus_zero[4] = {0x80000000u, 0u, 0x3A83126Fu, 0x461C4000u};
    int slot = -1, bad = 0;
    constexpr int kHit = 2, kCount = 64, kPacked = 128, kCountOwn = 256, kUse = 1 << 9, kOther = 2 << 9;
    for (int own = 0; own < 2; ++own) {
        void* s = own_start_new(own);
        // six views through four slots, twice round: a search, a fill, the hit that refines, the hit that counts (and leaves the starts), one
        // while the build runs, the hit that adopts, packed hits under the counted key, under four other keys, and under the counted key again
        for (int round = 0; round < 2; ++round)
            for (uint32_t view = 0; view < 6; ++view) {
                for (unsigned i = 0; i < n; ++i) key[i] = view * 977u + i;
                bad += own_start_launch(s, key, counted, 0, 1, &slot) != 0;
                bad += own_start_launch(s, key, counted, 0, 1, &slot) != 1;
                bad += slot < 0 || slot >= blok::kBeamCacheSlots || own_start_has(s, slot) != 0;
                bad += own_start_launch(s, key, counted, 0, 1, &slot) != kHit;
                bad += own_start_launch(s, key, counted, 0, 1, &slot) != (kHit | kCount | (own ? kCountOwn : 0));
                bad += own_start_has(s, slot) != own;
                bad += own_start_launch(s, key, jittered, 0, 1, &slot) != kHit;
                bad += own_start_launch(s, key, counted, 1, 1, &slot) != (kHit | kPacked | (own ? kUse : 0));
                for (const uint32_t* other : {jittered, nearer, shorter, minus_zero}) bad += own_start_launch(s, key, other, 0, 1, &slot) != (kHit | kPacked | (own ? kOther : 0));
                bad += own_start_launch(s, key, counted, 0, 1, &slot) != (kHit | kPacked | (own ? kUse : 0));
                bad += own_start_list_state(s, slot) != 3 || own_start_has(s, slot) != own;
            }
        // a build that could not be issued leaves no starts; a clear drops them; a settle in mid-build drops the list and the starts stay unused
        own_start_reset(s); own_start_settle(s);
        for (unsigned i = 0; i < n; ++i) key[i] = i;
        own_start_launch(s, key, counted, 0, 1, &slot); own_start_launch(s, key, counted, 0, 1, &slot); own_start_launch(s, key, counted, 0, 1, &slot);
        bad += own_start_launch(s, key, counted, 0, 0, &slot) != (kHit | kCount | (own ? kCountOwn : 0));
        bad += own_start_has(s, slot) != 0 || own_start_list_state(s, slot) != 0;
        bad += own_start_launch(s, key, jittered, 0, 1, &slot) != (kHit | kCount | (own ? kCountOwn : 0));
        bad += own_start_launch(s, key, jittered, 1, 1, &slot) != (kHit | kPacked | (own ? kUse : 0));      // the key is the count launch's, whichever that was
        bad += own_start_launch(s, key, counted, 0, 1, &slot) != (kHit | kPacked | (own ? kOther : 0));
        own_start_reset(s);
        for (int k = 0; k < blok::kBeamCacheSlots; ++k) bad += own_start_has(s, k) != 0;
        bad += own_start_mode(s) != own;
        bad += static_cast<int>(blok::plan_beam_starts(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Hit, blok::kBeamCacheSlots}, {true, false, -1}, blok::BeamStartKey{}).count_own);
        bad += static_cast<int>(blok::plan_beam_starts(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Hit, -1}, {false, true, -1}, blok::BeamStartKey{}).use) != 0;
        bad += static_cast<int>(blok::plan_beam_starts(*static_cast<blok::BeamCachePolicy*>(s), {blok::BeamAction::Fill, 0}, {true, false, -1}, blok::BeamStartKey{}).count_own);
        own_start_delete(s);
    }
    printf("own start policy: %d mismatches\n", bad);
    return bad != 0;
}
#endif
