// What the resident volume remembers of its edits between two rebuilds (gpu_build.h: GpuVolume::edits): the join of the edited boxes and
// one bit, whether any of those edits may have FILLED a voxel.  The shadow rays' last-occluder map is an upper bound per texel, and only a
// fill can make it fall short (api.hip: update_sun_map).  gpu_volume_commit notes, blok_hip_volume_rebuild takes; nothing else touches
// the log.  Plain C++, like beam_cache.h, so that the host can test it (tests/test_edit_log_cpu.py compiles this header with g++).
#ifndef BLOK_EDIT_LOG_H
#define BLOK_EDIT_LOG_H
#include <stdint.h>

namespace blok {

struct EditLog {
    uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};      // box-local voxels, half open; nothing noted = default-constructed (a noted box has hi > 0)
    bool may_fill = false;

    // Joins [blo, bhi) and ORs the bit.  A box that is empty on any axis wrote nothing: it notes nothing, not even its bit.
    void note(const uint32_t blo[3], const uint32_t bhi[3], bool fills) {
        if (bhi[0] <= blo[0] || bhi[1] <= blo[1] || bhi[2] <= blo[2]) return;
        const bool first = hi[0] == 0u;
        for (int a = 0; a < 3; ++a) {
            if (first || blo[a] < lo[a]) lo[a] = blo[a];
            if (first || bhi[a] > hi[a]) hi[a] = bhi[a];
        }
        may_fill = may_fill || fills;
    }

    struct Taken {
        int32_t lo[3], hi[3];      // the joined box in world voxels, half open; all zeros when nothing was noted
        bool may_fill;
        bool whole;                // the box is exactly the volume's, [0, dims)
    };
    // What was noted since the last take, for a volume of `dims` voxels whose voxel (0, 0, 0) sits at world `origin`; leaves the log
    // default-constructed.
    Taken take(const int32_t origin[3], const uint32_t dims[3]) {
        Taken t = {{0, 0, 0}, {0, 0, 0}, false, false};
        if (hi[0] != 0u) {
            t.may_fill = may_fill; t.whole = true;
            for (int a = 0; a < 3; ++a) {
                t.lo[a] = static_cast<int32_t>(origin[a] + static_cast<int64_t>(lo[a]));
                t.hi[a] = static_cast<int32_t>(origin[a] + static_cast<int64_t>(hi[a]));
                t.whole = t.whole && lo[a] == 0u && hi[a] == dims[a];
            }
        }
        *this = EditLog{};
        return t;
    }
};

}  // namespace blok
#endif
