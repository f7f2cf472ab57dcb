// TEST INFRASTRUCTURE: the resident volume's edit log (blok_amd/csrc/hip/edit_log.h) compiled for the host, as a program of its own so
// that it runs under -fsanitize=address,undefined (tests/test_edit_log_cpu.py).  Checks what the header promises: a fresh log takes as
// nothing; boxes join per axis; the bit is the OR of the notes; a note that is empty on one axis changes nothing, its bit included; take
// resets; the world conversion holds for a negative origin and for a box that reaches world 32768; "whole" means exactly [0, dims).
// Prints the number of checks that passed; a failed check prints its line and exits with 1.
#include <cstdint>
#include <cstdio>

#include "edit_log.h"

namespace {

int checks = 0;

bool same(const blok::EditLog::Taken& t, int32_t lx, int32_t ly, int32_t lz, int32_t hx, int32_t hy, int32_t hz, bool may_fill, bool whole) {
    return t.lo[0] == lx && t.lo[1] == ly && t.lo[2] == lz && t.hi[0] == hx && t.hi[1] == hy && t.hi[2] == hz && t.may_fill == may_fill && t.whole == whole;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } ++checks; } while (0)

}  // namespace

int main() {
    const int32_t zero[3] = {0, 0, 0}, minus[3] = {-5000, -64, -7}, high[3] = {16384, 32000, 32767};
    const uint32_t dims[3] = {64, 96, 32};
    blok::EditLog log;

    // a fresh log: nothing
    CHECK(same(log.take(zero, dims), 0, 0, 0, 0, 0, 0, false, false));
    CHECK(same(log.take(minus, dims), 0, 0, 0, 0, 0, 0, false, false));

    // one box, then a second: the join per axis, the OR of the bits; take resets
    const uint32_t a_lo[3] = {10, 20, 5}, a_hi[3] = {12, 30, 6};
    const uint32_t b_lo[3] = {11, 2, 7}, b_hi[3] = {40, 25, 9};
    log.note(a_lo, a_hi, false);
    CHECK(same(log.take(zero, dims), 10, 20, 5, 12, 30, 6, false, false));
    CHECK(same(log.take(zero, dims), 0, 0, 0, 0, 0, 0, false, false));
    log.note(a_lo, a_hi, false); log.note(b_lo, b_hi, false);
    CHECK(same(log.take(zero, dims), 10, 2, 5, 40, 30, 9, false, false));
    log.note(a_lo, a_hi, true); log.note(b_lo, b_hi, false);
    CHECK(same(log.take(zero, dims), 10, 2, 5, 40, 30, 9, true, false));
    log.note(b_lo, b_hi, false); log.note(a_lo, a_hi, true);
    CHECK(same(log.take(zero, dims), 10, 2, 5, 40, 30, 9, true, false));
    CHECK(same(log.take(zero, dims), 0, 0, 0, 0, 0, 0, false, false));                    // (the bit went with the box)

    // a note that is empty on one axis changes nothing, with its bit set too — on a fresh log and on one that holds a box
    for (int axis = 0; axis < 3; ++axis) {
        uint32_t e_lo[3] = {0, 0, 0}, e_hi[3] = {64, 96, 32};
        e_lo[axis] = e_hi[axis] = 3u;                                                     // lo == hi
        log.note(e_lo, e_hi, true);
        CHECK(same(log.take(zero, dims), 0, 0, 0, 0, 0, 0, false, false));
        e_lo[axis] = 0xFFFFFFFFu; e_hi[axis] = 0u;                                        // lo > hi: a box accumulator nothing was written into
        log.note(a_lo, a_hi, false); log.note(e_lo, e_hi, true);
        CHECK(same(log.take(zero, dims), 10, 20, 5, 12, 30, 6, false, false));
    }

    // world coordinates: a negative origin, and a box whose far corner lands on world 32768
    log.note(a_lo, a_hi, true);
    CHECK(same(log.take(minus, dims), -4990, -44, -2, -4988, -34, -1, true, false));
    const uint32_t big[3] = {16384, 768, 1};
    const uint32_t c_lo[3] = {16383, 0, 0}, c_hi[3] = {16384, 768, 1};                    // hi = 32768 - origin on every axis
    log.note(c_lo, c_hi, false);
    CHECK(same(log.take(high, big), 32767, 32000, 32767, 32768, 32768, 32768, false, false));

    // whole: exactly [0, dims), in one note or joined from several, whatever the origin; not one voxel less, not a box beyond
    const uint32_t w_lo[3] = {0, 0, 0};
    log.note(w_lo, dims, true);
    CHECK(same(log.take(minus, dims), -5000, -64, -7, -4936, 32, 25, true, true));
    log.note(w_lo, dims, false);
    CHECK(same(log.take(zero, dims), 0, 0, 0, 64, 96, 32, false, true));
    const uint32_t h1_hi[3] = {32, 96, 32}, h2_lo[3] = {32, 0, 0};
    log.note(w_lo, h1_hi, false); log.note(h2_lo, dims, true);
    CHECK(same(log.take(zero, dims), 0, 0, 0, 64, 96, 32, true, true));
    for (int axis = 0; axis < 3; ++axis) {
        uint32_t s_lo[3] = {0, 0, 0}, s_hi[3] = {64, 96, 32};
        s_hi[axis] -= 1u;
        log.note(s_lo, s_hi, true);
        CHECK(!log.take(zero, dims).whole);
        s_hi[axis] += 1u; s_lo[axis] = 1u;
        log.note(s_lo, s_hi, true);
        CHECK(!log.take(zero, dims).whole);
        s_lo[axis] = 0u; s_hi[axis] += 1u;
        log.note(s_lo, s_hi, true);
        CHECK(!log.take(zero, dims).whole);
    }
    std::printf("%d\n", checks);
    return 0;
}
