// Emissive voxels as lights: what the host build (host/lights.cpp), the table kernels (hip/lights_kernels.hip) and the lit path loop
// (hip/path_core.h: shade_pixel<…, kLit>) share.  include/blok_hip.h has the contract ("Emissive voxels as lights"); DESIGN.md §32 the rule.
// The table part is integer arithmetic; the sample part is float, every operation rounded separately (no contraction).
#ifndef BLOK_LIGHTS_CORE_H
#define BLOK_LIGHTS_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_LD __host__ __device__ inline
#else
#define BLOK_LD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace blok {
namespace lights {

constexpr uint32_t kSetBits = 65536u, kSetWords = kSetBits / 32u;      // a set of material indices: one bit each
constexpr float kLightEps = 0.004f;                                     // twice the bounce ray's offset: what a light's shadow ray stops short of

// The index a material id reads the material table at (path_core.h, hit.rchit): ids above 65535 read 65535, ids beyond the table read 0.
BLOK_LD uint32_t material_index(uint32_t id, uint32_t n_materials) {
    const uint32_t c = id < 65535u ? id : 65535u;
    return c < n_materials ? c : 0u;
}
// raygen.rgen:158-160 (path_core.h: is_emissive): dot(e, 1) > 0.01, summed left to right.
BLOK_LD bool emissive(const float e[3]) { return ((e[0] * 1.0f + e[1] * 1.0f) + e[2] * 1.0f) > 0.01f; }
BLOK_LD bool in_set(const uint32_t* set, uint32_t i) { return (set[i >> 5] >> (i & 31u)) & 1u; }
// A quad becomes a light iff the material its key maps to glows (`glows`: the set of emissive material indices).
BLOK_LD bool keeps(uint32_t material, const uint32_t* glows, uint32_t n_materials) { return in_set(glows, material_index(material, n_materials)); }

// The set of emissive indices of a material table (host; one evaluation per material).
inline void emissive_set(const blok_material* materials, size_t n_materials, uint32_t* set) {
    for (uint32_t w = 0; w < kSetWords; ++w) set[w] = 0u;
    const size_t n = n_materials < kSetBits ? n_materials : kSetBits;
    for (size_t m = 0; m < n; ++m) if (emissive(materials[m].emission)) set[m >> 5] |= 1u << (m & 31u);
}

// The rules blok_hip_set_lights holds a host table to.  0: fine (then *out_faces = A); else the rule that light *out_index breaks:
// 1 face > 5, 2 du or dv 0, 3 cum is not the running sum, 4 (unsupported) A >= 2^32 or n >= 2^31, 5 a coordinate outside [-32768, 32768].
inline int check_table(const blok_light* t, uint64_t n, uint64_t* out_faces, uint64_t* out_index) {
    uint64_t sum = 0;
    *out_faces = 0; *out_index = 0;
    if (n >= 0x80000000ull) return 4;
    for (uint64_t i = 0; i < n; ++i) {
        const blok_light& l = t[i];
        *out_index = i;
        if (l.face > 5u) return 1;
        if (l.du == 0u || l.dv == 0u) return 2;
        if (sum > 0xFFFFFFFFull) return 4;
        if (l.cum != static_cast<uint32_t>(sum)) return 3;
        const int a = static_cast<int>(l.face >> 1), u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
        for (int c = 0; c < 3; ++c) if (l.lo[c] < -32768 || l.lo[c] > 32768) return 5;
        if (l.du > 65536u || l.dv > 65536u || int64_t(l.lo[u]) + l.du > 32768 || int64_t(l.lo[v]) + l.dv > 32768) return 5;
        sum += static_cast<uint64_t>(l.du) * l.dv;
    }
    if (sum > 0xFFFFFFFFull) return 4;
    *out_faces = sum;
    return 0;
}

// ---- the pick: which unit face a 32-bit random number selects, and its light ----
BLOK_LD uint32_t pick_of(uint32_t r, uint32_t n_faces) { return static_cast<uint32_t>((static_cast<uint64_t>(r) * n_faces) >> 32); }
// The last light whose cum is <= pick (cum[0] = 0, so there is one), n >= 1: 4-byte loads of the records' cum words.
BLOK_LD uint32_t find_light(const blok_light* t, uint32_t n, uint32_t pick) {
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t[mid].cum <= pick) lo = mid; else hi = mid;
    }
    return lo;
}

// The sampled point q on cell `off` of light L (off = pick - L.cum; iu = off % du, iv = off / du) and the light's normal nl = +-e_a.
// World position = lattice x vs; vs is a power of two, so the products are exact.
BLOK_LD void sample_point(const blok_light& L, uint32_t off, float u1, float u2, float vs, float q[3], float nl[3]) {
    const uint32_t iu = off % L.du, iv = off / L.du;
    const uint32_t a = L.face >> 1;
    const int32_t lo_u = a == 0u ? L.lo[1] : L.lo[0], lo_v = a == 2u ? L.lo[1] : L.lo[2], lo_a = a == 0u ? L.lo[0] : (a == 1u ? L.lo[1] : L.lo[2]);
    const float pa = static_cast<float>(lo_a) * vs;
    const float pu = (static_cast<float>(lo_u + static_cast<int32_t>(iu)) + u1) * vs;
    const float pv = (static_cast<float>(lo_v + static_cast<int32_t>(iv)) + u2) * vs;
    q[0] = a == 0u ? pa : pu;
    q[1] = a == 0u ? pu : (a == 1u ? pa : pv);
    q[2] = a == 2u ? pa : pv;
    const float s = (L.face & 1u) ? -1.0f : 1.0f;
    nl[0] = a == 0u ? s : 0.0f; nl[1] = a == 1u ? s : 0.0f; nl[2] = a == 2u ? s : 0.0f;
}

// ---- emissive models as lights (blok_hip.h: "emissive models as lights") ----
// A model's table holds its exposed emissive UNIT faces in the order of its material array (bricks in the tree's order, cells in ascending
// bit order, face 0..5 within a voxel); cum is the record's index.  The host build (host/model_lights.cpp) and the kernels (hip/lights_kernels.hip)
// run the functions below over the model's 64-tree (hip/tree.h: 16-byte nodes, root first, every level in Morton order, the bricks last).
struct Node { uint64_t mask; uint32_t base; };
// The tree as both sides hand it over: node(i) loads node i; an index at or beyond n_nodes reads as an empty node, a material at or beyond
// n_voxels as id 0, so a malformed tree costs wrong records, never a load outside the arrays.
template <class LoadNode>
struct ModelTree {
    LoadNode node; uint32_t n_nodes;
    const uint32_t* materials; uint32_t n_voxels;
    uint32_t levels; int32_t origin[3];
    BLOK_LD Node at(uint32_t i) const { return i < n_nodes ? node(i) : Node{0ull, 0u}; }
    BLOK_LD uint32_t material(uint32_t i) const { return i < n_voxels ? materials[i] : 0u; }
};
// One table per model for the kernels that read it through the model id (the instance prefix): 16 bytes, table == null or n == 0: none.
struct ModelLightTable { const blok_light* table; uint32_t n; uint32_t reserved; };

BLOK_LD uint32_t popc64(uint64_t m) { return static_cast<uint32_t>(__builtin_popcountll(m)); }
BLOK_LD uint32_t ctz64(uint64_t m) { return static_cast<uint32_t>(__builtin_ctzll(m)); }

// Where level l begins (1: the bricks): the root's level begins at 0 and every level's block at the first child of the first node above it.
template <class T> BLOK_LD uint32_t level_start(const T& t, uint32_t l) {
    uint32_t start = 0u;
    for (uint32_t k = t.levels; k > l; --k) start = t.at(start).base;
    return start;
}
template <class T> BLOK_LD uint32_t first_brick(const T& t) { return level_start(t, 1u); }
// The brick coordinates (bricks from the tree's origin) of brick node `index`: upwards, a level at a time — the parent is the last node of
// the level above whose base is <= the child's index (bases ascend within a level), the digit the child's rank among its parent's set bits.
template <class T> BLOK_LD void brick_coords(const T& t, uint32_t index, uint32_t b[3]) {
    b[0] = b[1] = b[2] = 0u;
    uint32_t child = index;
    for (uint32_t l = 2u; l <= t.levels; ++l) {
        // the parent lies in [lo, hi): level l's block (its bounds are formed again per level, a few loads every lane shares, so that no
        // array indexed by the level lives in scratch)
        uint32_t lo = level_start(t, l), hi = level_start(t, l - 1u);
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (t.at(mid).base <= child) lo = mid; else hi = mid;
        }
        const Node p = t.at(lo);
        uint64_t m = p.mask;
        for (uint32_t r = child - p.base; r != 0u && m != 0ull; --r) m &= m - 1ull;
        const uint32_t digit = m ? ctz64(m) : 0u;
        const uint32_t shift = 2u * (l - 2u);
        b[0] |= (digit & 3u) << shift; b[1] |= ((digit >> 2) & 3u) << shift; b[2] |= (digit >> 4) << shift;
        child = lo;
    }
}
// The mask of the brick at brick coordinates b (any integers: outside the tree's cube it is empty): downwards from the root.
template <class T> BLOK_LD uint64_t brick_mask_at(const T& t, int64_t bx, int64_t by, int64_t bz) {
    const int64_t edge = int64_t(1) << (2u * (t.levels - 1u));
    if (bx < 0 || by < 0 || bz < 0 || bx >= edge || by >= edge || bz >= edge) return 0ull;
    Node n = t.at(0u);
    for (uint32_t l = t.levels; l >= 2u; --l) {
        const uint32_t shift = 2u * (l - 2u);
        const uint32_t digit = static_cast<uint32_t>((bx >> shift) & 3) | (static_cast<uint32_t>((by >> shift) & 3) << 2) | (static_cast<uint32_t>((bz >> shift) & 3) << 4);
        if (!((n.mask >> digit) & 1ull)) return 0ull;
        n = t.at(n.base + popc64(n.mask & ((1ull << digit) - 1ull)));
    }
    return n.mask;
}
// The cells of a brick (mask m; its six neighbours' masks in face order +x -x +y -y +z -z) whose face f looks at an empty cell of the model:
// bit-parallel, cell bit = x | y << 2 | z << 4.
BLOK_LD void brick_open_faces(uint64_t m, const uint64_t nb[6], uint64_t open[6]) {
    constexpr uint64_t X0 = 0x1111111111111111ull, X3 = 0x8888888888888888ull, Y0 = 0x000F000F000F000Full, Y3 = 0xF000F000F000F000ull,
                       Z0 = 0x000000000000FFFFull, Z3 = 0xFFFF000000000000ull;
    open[0] = m & ~(((m >> 1) & ~X3) | ((nb[0] << 3) & X3));
    open[1] = m & ~(((m << 1) & ~X0) | ((nb[1] >> 3) & X0));
    open[2] = m & ~(((m >> 4) & ~Y3) | ((nb[2] << 12) & Y3));
    open[3] = m & ~(((m << 4) & ~Y0) | ((nb[3] >> 12) & Y0));
    open[4] = m & ~(((m >> 16) & ~Z3) | ((nb[4] << 48) & Z3));
    open[5] = m & ~(((m << 16) & ~Z0) | ((nb[5] >> 48) & Z0));
}
// What brick node `index` contributes: the cells that glow and have an open face at all (*glowing), the open cells per face, its brick
// coordinates; returns the number of its records.  Materials are read only for cells with an open face.
template <class T> BLOK_LD uint32_t brick_lights(const T& t, uint32_t index, const uint32_t* glows, uint32_t n_materials, uint64_t open[6], uint64_t* glowing,
                                                 uint32_t b[3], Node* brick) {
    *brick = t.at(index);
    brick_coords(t, index, b);
    const int64_t x = b[0], y = b[1], z = b[2];
    const uint64_t nb[6] = {brick_mask_at(t, x + 1, y, z), brick_mask_at(t, x - 1, y, z), brick_mask_at(t, x, y + 1, z),
                            brick_mask_at(t, x, y - 1, z), brick_mask_at(t, x, y, z + 1), brick_mask_at(t, x, y, z - 1)};
    brick_open_faces(brick->mask, nb, open);
    uint64_t g = 0ull;
    for (uint64_t any = open[0] | open[1] | open[2] | open[3] | open[4] | open[5]; any; any &= any - 1ull) {
        const uint32_t c = ctz64(any);
        const uint32_t id = t.material(brick->base + popc64(brick->mask & ((1ull << c) - 1ull)));
        if (keeps(id, glows, n_materials)) g |= 1ull << c;
    }
    *glowing = g;
    uint32_t n = 0u;
    for (int f = 0; f < 6; ++f) n += popc64(open[f] & g);
    return n;
}
// ... and its records, written from out[first] on (first = the records of the bricks before it): cells in ascending bit order, face 0..5.
template <class T> BLOK_LD void brick_write_lights(const T& t, const Node& brick, const uint32_t b[3], const uint64_t open[6], uint64_t glowing, uint32_t first,
                                                   blok_light* out) {
    uint32_t at = first;
    for (uint64_t cells = glowing; cells; cells &= cells - 1ull) {
        const uint32_t c = ctz64(cells);
        const uint32_t id = t.material(brick.base + popc64(brick.mask & ((1ull << c) - 1ull)));
        const int32_t v[3] = {t.origin[0] + static_cast<int32_t>(4u * b[0] + (c & 3u)), t.origin[1] + static_cast<int32_t>(4u * b[1] + ((c >> 2) & 3u)),
                              t.origin[2] + static_cast<int32_t>(4u * b[2] + (c >> 4))};
        for (uint32_t f = 0; f < 6u; ++f) {
            if (!((open[f] >> c) & 1ull)) continue;
            blok_light l;
            l.lo[0] = v[0] + ((f == 0u) ? 1 : 0); l.lo[1] = v[1] + ((f == 2u) ? 1 : 0); l.lo[2] = v[2] + ((f == 4u) ? 1 : 0);
            l.du = 1u; l.dv = 1u; l.material = id; l.face = f; l.cum = at;
            out[at++] = l;
        }
    }
}

// The world-lattice rectangle of unit face `m` (a record of a model's table: du = dv = 1) of instance I of a model of scale exponent e: the
// header's "record back to world space" rule in 64-bit integers.  du = dv = 2^e; material unchanged; cum 0.
BLOK_LD blok_light instance_light_record(const blok_instance& I, uint32_t e, const blok_light& m) {
    const uint32_t fk = m.face >> 1, fn = m.face & 1u;
    blok_light w;
    uint32_t world_face = 0u;
    // by world axis a, the local axis k with axis[k] == a by selects: the permutation is data, and an array indexed by it would live in scratch
    for (uint32_t a = 0; a < 3u; ++a) {
        const uint32_t k = I.axis[0] == a ? 0u : (I.axis[1] == a ? 1u : 2u), flip = (I.flip >> k) & 1u;
        const int32_t mlo = k == 0u ? m.lo[0] : (k == 1u ? m.lo[1] : m.lo[2]);
        const int64_t c = static_cast<int64_t>(mlo) - ((k == fk && fn == 0u) ? 1 : 0);        // the cell: a + face's plane lies one above it
        const int64_t o = I.offset[a];
        int64_t at = flip ? o - (c + 1) * (int64_t(1) << e) : o + c * (int64_t(1) << e);
        if (k == fk) { world_face = 2u * a + (fn ^ flip); if ((fn ^ flip) == 0u) at += int64_t(1) << e; }
        w.lo[a] = static_cast<int32_t>(at);
    }
    w.du = 1u << e; w.dv = 1u << e; w.material = m.material; w.face = world_face; w.cum = 0u;
    return w;
}

// ---- the per-launch prefix over an instance table ----
// faces_i = n_faces(model) << 2e for a usable instance of a model with a table, else 0; icum the exclusive scan, n + 1 words.  When
// A_world + sum(faces) reaches 2^32 the launch goes without instance lights: every faces_i 0, disabled 1.
// The scale exponent as every reader of a descriptor takes it for the prefix and the pick (the store keeps it <= 8; the one clamp for both,
// so that `off >> 2e` and icum can never disagree).
BLOK_LD uint32_t scale_exponent(uint32_t scale_log2) { return scale_log2 <= 8u ? scale_log2 : 8u; }
BLOK_LD uint64_t instance_faces(bool usable, uint32_t table_n, uint32_t e) { return usable ? static_cast<uint64_t>(table_n) << (2u * e) : 0ull; }
BLOK_LD bool instance_lights_fit(uint64_t a_world, uint64_t a_inst) { return a_world + a_inst < 0x100000000ull; }
BLOK_LD float lights_area_world(uint64_t a_total, float vs) { return (static_cast<float>(a_total) * vs) * vs; }

// ---- the light grid (blok_hip.h: "the light grid") ----
// Cells of 2^c world voxels on the world lattice; a cell's list holds the lights whose own cells lie within `reach` cells of it on every
// axis.  Integer work with one right answer: the host build (host/light_grid.cpp) and the kernels (hip/lights_kernels.hip) both run the
// functions below and nothing else decides membership.
constexpr uint32_t kGridMinLog2 = 2u, kGridMaxLog2 = 12u, kGridMaxReach = 3u;
constexpr uint64_t kGridMaxCells = 1ull << 24, kGridMaxItems = 1ull << 28;      // more cells: Unsupported; this many items or more: Unsupported
BLOK_LD bool grid_params_ok(uint32_t cell_log2, uint32_t reach, uint32_t share) {
    return cell_log2 >= kGridMinLog2 && cell_log2 <= kGridMaxLog2 && reach <= kGridMaxReach && share >= 1u && share <= 255u;
}
// The cells a light's emitting voxels lie in, both ends inclusive, before the reach.  On the plane axis the emitting voxel is lo - 1 for a
// + face and lo for a - face (instance_light_record's reading); in the plane the voxels are [lo, lo + d - 1].  >> of a negative int is
// arithmetic (C++20), so cell -1 holds voxels [-2^c, -1].
struct CellRange { int32_t lo[3], hi[3]; };
BLOK_LD CellRange light_cells(const blok_light& L, uint32_t c) {
    const uint32_t a = L.face >> 1;
    const int32_t du = static_cast<int32_t>(L.du) - 1, dv = static_cast<int32_t>(L.dv) - 1, back = (L.face & 1u) ? 0 : 1;
    CellRange r;
    r.lo[0] = a == 0u ? L.lo[0] - back : L.lo[0];                 r.hi[0] = a == 0u ? r.lo[0] : r.lo[0] + du;                       // u of faces 2..5
    r.lo[1] = a == 1u ? L.lo[1] - back : L.lo[1];                 r.hi[1] = a == 1u ? r.lo[1] : r.lo[1] + (a == 0u ? du : dv);      // u of 0..1, v of 4..5
    r.lo[2] = a == 2u ? L.lo[2] - back : L.lo[2];                 r.hi[2] = a == 2u ? r.lo[2] : r.lo[2] + dv;                       // v of faces 0..3
    for (int k = 0; k < 3; ++k) { r.lo[k] >>= c; r.hi[k] >>= c; }
    return r;
}
// in(L, g): the one predicate.  g in absolute cells.
BLOK_LD bool in_cell(const CellRange& r, uint32_t reach, int32_t gx, int32_t gy, int32_t gz) {
    const int32_t R = static_cast<int32_t>(reach);
    return r.lo[0] - R <= gx && gx <= r.hi[0] + R && r.lo[1] - R <= gy && gy <= r.hi[1] + R && r.lo[2] - R <= gz && gz <= r.hi[2] + R;
}
// The cells that list a light: its range widened by the reach; their number (below 2^32 for a light of the int16 lattice and c >= 2).
BLOK_LD uint32_t listed_extent(const CellRange& r, uint32_t reach, int k) { return static_cast<uint32_t>(r.hi[k] - r.lo[k]) + 1u + 2u * reach; }
BLOK_LD uint64_t listed_cells(const CellRange& r, uint32_t reach) {
    return static_cast<uint64_t>(listed_extent(r, reach, 0)) * listed_extent(r, reach, 1) * listed_extent(r, reach, 2);
}
// The box of all listing cells: the union of the lights' ranges, widened by the reach.  An empty box has lo > hi.
struct GridBounds { int32_t lo[3], hi[3]; };
BLOK_LD GridBounds no_bounds() { return GridBounds{{0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, {-0x7FFFFFFF - 1, -0x7FFFFFFF - 1, -0x7FFFFFFF - 1}}; }
BLOK_LD GridBounds join(const GridBounds& a, const GridBounds& b) {
    GridBounds o;
    for (int k = 0; k < 3; ++k) { o.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k]; o.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k]; }
    return o;
}
// cell_lo, dim and n_cells into *info from the union of the lights' ranges (before the reach).
BLOK_LD void grid_box(const GridBounds& b, uint32_t reach, blok_light_grid_info* info) {
    info->n_cells = 1u;
    for (int k = 0; k < 3; ++k) {
        info->cell_lo[k] = b.lo[k] - static_cast<int32_t>(reach);
        info->dim[k] = static_cast<uint32_t>(b.hi[k] - b.lo[k]) + 1u + 2u * reach;
        info->n_cells *= info->dim[k];
    }
}
// The index of listing cell number k of a light (k < listed_cells: x fastest) in a grid of that box.
BLOK_LD uint32_t listed_cell_index(const CellRange& r, uint32_t reach, uint32_t k, const int32_t cell_lo[3], const uint32_t dim[3]) {
    const uint32_t ex = listed_extent(r, reach, 0), ey = listed_extent(r, reach, 1), R = reach;
    const uint32_t x = static_cast<uint32_t>(r.lo[0] - cell_lo[0]) - R + k % ex, y = static_cast<uint32_t>(r.lo[1] - cell_lo[1]) - R + (k / ex) % ey,
                   z = static_cast<uint32_t>(r.lo[2] - cell_lo[2]) - R + k / (ex * ey);
    return (z * dim[1] + y) * dim[0] + x;
}
BLOK_LD uint64_t grid_bytes(uint64_t n_cells, uint64_t n_items) { return (n_cells + 1u) * 4u + n_cells * 4u + n_items * sizeof(blok_light_grid_item); }

}  // namespace lights
}  // namespace blok
#endif
