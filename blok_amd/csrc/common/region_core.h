// The region of a box that the volume entries take as two optional world corners.  The one place its rule lives: the device entries
// (hip/api_volume.hip) and the host builds (host/bricks.cpp, host/distance.cpp, host/flood.cpp) all include this header.  No HIP types.
#ifndef BLOK_REGION_CORE_H
#define BLOK_REGION_CORE_H
#include <stdint.h>

#include "blok_hip.h"

namespace blok {
namespace region {

// 0 = fine, otherwise the rule that failed.
enum Rule { kFine = 0, kOnePointerNull, kLoAboveHi, kLeavesBox };

// The box-local [lo, hi) of world region_lo / region_hi (both null: the whole box) in the box of `dims` cells whose cell (0, 0, 0) sits at
// world `origin` (null: the world's).
inline int local(const int32_t* origin, const uint32_t dims[3], const int32_t* region_lo, const int32_t* region_hi, uint32_t lo[3], uint32_t hi[3]) {
    if ((region_lo == nullptr) != (region_hi == nullptr)) return kOnePointerNull;
    for (int a = 0; a < 3; ++a) {
        const int64_t o = origin ? origin[a] : 0;
        const int64_t l = region_lo ? int64_t(region_lo[a]) - o : 0, h = region_hi ? int64_t(region_hi[a]) - o : int64_t(dims[a]);
        if (l > h) return kLoAboveHi;
        if (l < 0 || h > int64_t(dims[a])) return kLeavesBox;
        lo[a] = static_cast<uint32_t>(l); hi[a] = static_cast<uint32_t>(h);
    }
    return kFine;
}
// The status every entry answers a rule with.
inline int status(int rule) { return rule == kFine ? BLOK_OK : rule == kLeavesBox ? BLOK_ERR_UNSUPPORTED : BLOK_ERR_INVALID_ARG; }

}  // namespace region
}  // namespace blok
#endif
