// TEST INFRASTRUCTURE: exposes blok_amd/csrc/hip/beam_cache.h (pure C++, no HIP) to tests/test_beam_cache_policy.py.  Built with
// -DBEAM_CACHE_SHIM_MAIN it is a stand-alone program instead (the same walk through the policy, for a sanitizer build).
#include "beam_cache.h"

extern "C" {
unsigned beam_cache_key_words() { return sizeof(blok::BeamKey) / sizeof(uint32_t); }
unsigned beam_cache_slots() { return blok::kBeamCacheSlots; }
void* beam_cache_new() { auto* s = new blok::BeamCachePolicy{}; blok::beam_cache_clear(*s); return s; }
void beam_cache_delete(void* s) { delete static_cast<blok::BeamCachePolicy*>(s); }
void beam_cache_reset(void* s) { blok::beam_cache_clear(*static_cast<blok::BeamCachePolicy*>(s)); }
// key: beam_cache_key_words() words, in the order of BeamKey's fields.  -> action (0 search, 1 fill, 2 hit); the slot through the pointer
int beam_cache_plan(void* s, const uint32_t* key, int* slot) {
    blok::BeamKey k;
    memcpy(&k, key, sizeof(k));
    const blok::BeamCachePlan p = blok::plan_beam_cache(*static_cast<blok::BeamCachePolicy*>(s), k);
    *slot = p.slot;
    return static_cast<int>(p.action);
}
}

#ifdef BEAM_CACHE_SHIM_MAIN
#include <stdio.h>
int main() {
    void* s = beam_cache_new();
    const unsigned n = beam_cache_key_words();
    uint32_t key[64] = {};
    int slot = -1, bad = 0;
    // six views, three launches each, twice round: search, fill, hit — through every slot and two evictions per round
    for (int round = 0; round < 2; ++round)
        for (uint32_t view = 0; view < 6; ++view)
            for (int k = 0; k < 3; ++k) {
                for (unsigned i = 0; i < n; ++i) key[i] = view * 977u + i;
                const int a = beam_cache_plan(s, key, &slot);
                bad += a != k || (k > 0 && (slot < 0 || slot >= static_cast<int>(beam_cache_slots())));
            }
    // every word of the key on its own
    for (unsigned i = 0; i < n; ++i) {
        beam_cache_reset(s);
        for (unsigned j = 0; j < n; ++j) key[j] = j;
        bad += beam_cache_plan(s, key, &slot) != 0; bad += beam_cache_plan(s, key, &slot) != 1; bad += beam_cache_plan(s, key, &slot) != 2;
        key[i] ^= 1u;
        bad += beam_cache_plan(s, key, &slot) != 0;
    }
    beam_cache_delete(s);
    printf("beam cache policy: %d mismatches\n", bad);
    return bad != 0;
}
#endif
