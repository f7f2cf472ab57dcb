// The surface of a voxel volume as merged quads: the predicates the host build (host/quads.cpp) and the kernels (hip/quads_kernels.hip)
// share.  include/blok_hip.h has the contract (blok_hip_volume_extract_quads); DESIGN.md §14 the algorithm.  Integer arithmetic only,
// __host__ __device__, no HIP types.
#ifndef BLOK_QUADS_CORE_H
#define BLOK_QUADS_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BLOK_QD __host__ __device__ inline
#else
#define BLOK_QD inline
#endif

namespace blok {
namespace quads {

// faces as blok_hit::face: 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z
BLOK_QD int normal_axis(uint32_t face) { return static_cast<int>(face >> 1); }
BLOK_QD int normal_sign(uint32_t face) { return (face & 1u) ? -1 : 1; }
// plane axes of a face with normal axis a: u the lower of the two other axes, v the higher
BLOK_QD int u_axis(int a) { return a == 0 ? 1 : 0; }
BLOK_QD int v_axis(int a) { return a == 2 ? 1 : 2; }
// (e_u x e_v) . n_f > 0: the corners c0, c1, c2, c3 are counter-clockwise seen from outside as they stand; otherwise c0, c3, c2, c1
BLOK_QD bool winding_as_is(uint32_t face) { return face == 0u || face == 3u || face == 4u; }

// A voxel is filled iff density > 0 (NaN and negative densities are empty).
BLOK_QD bool filled(float density) { return density > 0.0f; }

// One face number of one voxel: exposed, and the key it merges by (0 when not exposed).
struct Cell { uint32_t exposed; uint32_t key; };
BLOK_QD Cell cell(bool is_filled, bool neighbour_filled, uint32_t material, bool ignore_material) {
    Cell c;
    c.exposed = is_filled && !neighbour_filled ? 1u : 0u;
    c.key = (c.exposed && !ignore_material) ? material : 0u;
    return c;
}
// both exposed with the same key: the two cells belong to one run (side by side along u) or stack (one above the other along v)
BLOK_QD bool same(const Cell& a, const Cell& b) { return a.exposed && b.exposed && a.key == b.key; }
BLOK_QD bool starts_run(const Cell& c, const Cell& before) { return c.exposed && !same(c, before); }      // `before`: the cell at u - 1
BLOK_QD bool ends_run(const Cell& c, const Cell& after) { return c.exposed && !same(c, after); }          // `after`: the cell at u + 1

// ---- rows as bit words.  Bit b of word w of a row is cell u = 64 w + b.  Three words describe a row v of one face number and plane:
//   S: the cell starts a run       T: the cell ends a run       D: same(cell, the cell below it in row v - 1)
// The run that starts at u0 ends at the first T bit at or after u0.  It is LINKED to the row below (an identical run lies there) iff
// D holds over the whole run and row v - 1 has S at u0 and T at u1: D over the run makes the cells below one run's worth of equal keys,
// the two bits make that run end where this one does.
BLOK_QD uint64_t bits_from_to(uint32_t from, uint32_t to) {      // bits from..to inclusive, 0 <= from <= to <= 63
    return (~0ull << from) & (~0ull >> (63u - to));
}

// The runs of a row, word by word in u order.  open / ok / u0 carry a run across words.
struct RowWalk { uint32_t open; uint32_t ok; uint32_t u0; };
BLOK_QD void row_walk_reset(RowWalk& r) { r.open = 0u; r.ok = 0u; r.u0 = 0u; }
// One word of row v (s, t, d) and of the row below (sb, tb: zeros for the first row).  emit(u0, u1, linked) for every run that ends here.
template <class Emit>
BLOK_QD void row_walk_word(RowWalk& r, uint32_t word, uint64_t s, uint64_t t, uint64_t d, uint64_t sb, uint64_t tb, Emit&& emit) {
    uint64_t events = s | t;
    uint32_t from = 0u;      // where, in this word, the open run's cells not yet checked against D begin
    while (events) {
        const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(events));
        events &= events - 1ull;
        if ((s >> b) & 1ull) { r.open = 1u; r.ok = static_cast<uint32_t>((sb >> b) & 1ull); r.u0 = word * 64u + b; from = b; }
        if ((t >> b) & 1ull) {
            const uint64_t span = bits_from_to(from, b);
            const uint32_t linked = r.ok && (d & span) == span && ((tb >> b) & 1ull);
            emit(r.u0, word * 64u + b, linked != 0u);
            r.open = 0u;
        }
    }
    if (r.open) { const uint64_t span = bits_from_to(from, 63u); r.ok = r.ok && (d & span) == span; }
}
// Does the row hold a run identical to [u0, u1] that is linked to the row below it?  (How a quad grows upwards.)  word_of(w) returns
// the row's S, T and D words through its reference arguments.
template <class Words>
BLOK_QD bool row_has_linked_run(uint32_t u0, uint32_t u1, Words&& word_of) {
    const uint32_t w0 = u0 >> 6, w1 = u1 >> 6;
    for (uint32_t w = w0; w <= w1; ++w) {
        uint64_t s, t, d;
        word_of(w, s, t, d);
        const uint32_t from = w == w0 ? (u0 & 63u) : 0u, to = w == w1 ? (u1 & 63u) : 63u;
        const uint64_t span = bits_from_to(from, to);
        if ((d & span) != span) return false;
        if (w == w0 && !((s >> from) & 1ull)) return false;
        if (w == w1 && !((t >> to) & 1ull)) return false;
    }
    return true;
}

// The four corners of a quad in winding order (counter-clockwise seen from outside), three int32 each.
BLOK_QD void corners(const int32_t lo[3], uint32_t du, uint32_t dv, uint32_t face, int32_t out[4][3]) {
    const int a = normal_axis(face), u = u_axis(a), v = v_axis(a);
    for (int k = 0; k < 4; ++k) for (int c = 0; c < 3; ++c) out[k][c] = lo[c];
    const bool as_is = winding_as_is(face);
    const int k1 = as_is ? 1 : 3, k3 = as_is ? 3 : 1;      // c1 = lo + du e_u, c3 = lo + dv e_v
    out[k1][u] += static_cast<int32_t>(du);
    out[2][u] += static_cast<int32_t>(du); out[2][v] += static_cast<int32_t>(dv);
    out[k3][v] += static_cast<int32_t>(dv);
}

}  // namespace quads
}  // namespace blok
#endif
