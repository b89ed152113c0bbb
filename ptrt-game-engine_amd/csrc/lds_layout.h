// lds_layout.h -- the dynamic LDS of every traversal launch, stated once: for each launch shape the named regions as byte
// offsets and sizes, and the total the host passes at launch.  Plain C++17, no HIP (every function is constexpr, which the
// device compiler takes as host and device): the device carves (carve_pair_lds, carve_pm1, carve_pair_lds_wg in
// pt_render.hip.h, the async and wavefront kernels) are base + offset out of these layouts, the host's byte counts
// (ptrt_render.hip.h) are their totals, and the device-free entry point ptrt_lds_layout (include/ptrt.h) hands them to
// tests/test_lds_layout.py.  DESIGN.md 2, "LDS layouts".
//
// A region is used when its size is not zero.  Regions are pairwise disjoint EXCEPT the aliases: a region whose `in_first` is
// set lies, by design, inside the span [in_first, in_last] of other regions, and the fact that makes it safe stands beside it
// (a static_assert, or a condition the host checks before it admits the scene).
#pragma once
#include <cstddef>

namespace pt {

constexpr int LDS_LIGHTS = 8; // light records (64 B each) PMODE 1 stages at most
// PMODE 3: TLAS leaves a ray may have in one fill of the pair list (a power of two <= 4) and the pairs that end a fill
#ifndef PT_TLAS_SLOTS
#define PT_TLAS_SLOTS 1
#endif
constexpr int TLAS_SLOTS = PT_TLAS_SLOTS;
constexpr int TLAS_FILL_TARGET = 64;
constexpr int PAIR_PAD = 2;   // float4 of padding in front of each mesh's packets in LDS (bank spreading)
constexpr int AS_RING = 128;  // async kernel: ring entries (u32)
constexpr int WF_RING = 256;  // wavefront trace: ring entries per wave (u32): < 64 waiting + at most 128 from one chunk
// the compacted leaf phase: 64 merge keys, and the owner lane of each of up to 64 x LEAF_PAIR_TESTS (lane, triangle) tests
constexpr int LEAF_PAIR_TESTS = 17;
constexpr int LEAF_KEY_BYTES = 64 * 8, LEAF_OWNER_BYTES = 64 * LEAF_PAIR_TESTS;
constexpr int LEAF_PAIR_BYTES = LEAF_KEY_BYTES + LEAF_OWNER_BYTES;
// the list holds 64 x the scene's largest leaf: what the host checks before a shape with the compacted leaf phase runs
constexpr bool leaf_pairs_fit(int max_leaf) { return (size_t)max_leaf * 64 <= (size_t)LEAF_OWNER_BYTES; }
static_assert(leaf_pairs_fit(LEAF_PAIR_TESTS) && !leaf_pairs_fit(LEAF_PAIR_TESTS + 1), "owner list = 64 lanes x the largest leaf");

namespace lds {

constexpr int PLANE32 = 64 * 4, PLANE64 = 64 * 8; // one word per lane
constexpr int TRI_BYTES = 48, HEAD_BYTES = 32, MESHTAB_BYTES = 16, PAD_BYTES = PAIR_PAD * 16;
constexpr int PAIR_ENTRY = 2;                  // a pair list entry: {lane, mesh order << 6} in 16 bits
constexpr int PAIRS_PER_MESH = 64 * PAIR_ENTRY; // every ray may hit every mesh
constexpr int COUNT_BYTES = 16, DIRTY_BYTES = 8; // the wave's ray totals (two 64-bit words); the closest-hit stealing's ray mask
constexpr int JIT_BYTES = 16 * 8, BN_BYTES = PLANE64, LIGHT_BYTES = 64, MAT_BYTES_SIMPLE = 48, MAT_BYTES_FULL = 96;
constexpr int PM1_MATS_MAX = 42;               // meshes whose material records PMODE 1 stages at most
constexpr int DENSE_OWNER_BYTES = 32;          // build_pairs_dense: the rank -> owner lane table of R <= 32 rays
constexpr int PM1_PARK_BYTES = 6 * PLANE32;    // lane refill [R]: a finished pixel's six generator words
constexpr int PM1_PAIR_FLOOR = 1024;           // ... which is why PMODE 1's pair list is never smaller than this
constexpr int PM1_QUERY_TAIL = 16;             // one-wave PMODE 1: bytes the host has always passed behind the pair list (unused)
static_assert(PM1_PARK_BYTES <= PLANE64 + PM1_PAIR_FLOOR, "the park fits the minima and the smallest pair list");
static_assert(COUNT_BYTES <= PAD_BYTES, "the ray totals fit the pad behind the last mesh's packets");

enum Id {
    // one copy per workgroup
    TRIS,     // PMODE 1: the leaf's triangle packets, mesh i's PAIR_PAD * i float4 later than in the arena, one pad behind the last
    MESHTAB,  // PMODE 1: per mesh order {first slot, count, flags, mesh id}
    MESHBOX,  // per mesh order the mesh record's head
    TOPNODES, // lds_nodes: the first TOP_NODES nodes of every mesh of the leaf
    JIT, LIGHTS, MATS, // PMODE 1 megakernel: the staged shading inputs its waves share
    // per wave
    BEST,     // the rays' minima, 64 x 64 bit (PMODE 3: per leaf slot)
    PAIRS,    // the (ray, mesh) pair list
    OCC,      // the any-hit flags: alias of BEST's second half, except where both kinds of ray are walked at once
    STACK, TSTACK, LEAFX, // [entry][lane] BLAS stack; PMODE 3: TLAS stack and the rays' leaf starts
    LKEY, OWNER, // the compacted leaf phase
    BN,       // PMODE 1 megakernel: the lanes' blue-noise values
    COUNT,    // the wave's ray totals; one-wave PMODE 1: alias of the last pad of TRIS
    DIRTY,    // PMODE 2: rays to trace again without stealing
    RING,     // async / wavefront: the ring of waiting items
    TAIL,     // counted, never used
    // aliases only
    LIMITS,      // any-hit traversals: the rays' limits in BEST's first half
    DENSE_OWNER, // build_pairs_dense: behind the 32 * M entries R <= 32 rays can make
    PARK,        // lane refill: across BEST and PAIRS
    N_REGIONS,
    FIRST_WAVE = BEST
};

struct Region {
    size_t off = 0, bytes = 0; // off: from the workgroup's base (ids below FIRST_WAVE) or from the wave's part
    int align = 1;             // of what is stored there
    int in_first = -1, in_last = -1;
};
struct Layout {
    Region r[N_REGIONS] = {};
    int wave_off = 0, wave_bytes = 0; // wave w's part starts at wave_off + w * wave_bytes (a workgroup has 64 KB at most)
    int waves = 1;
    size_t total = 0;
    constexpr int part(int id, int wave) const { return id >= FIRST_WAVE ? wave_off + wave * wave_bytes : 0; } // where r[id].off counts from
    constexpr size_t at(int id, int wave = 0) const { return (size_t)part(id, wave) + r[id].off; }
};
constexpr void put(Layout &L, size_t &p, int id, size_t bytes, int align) {
    L.r[id] = Region{p, bytes, align, -1, -1};
    p += bytes;
}
constexpr void alias(Layout &L, int id, size_t off, size_t bytes, int align, int in_first, int in_last) {
    L.r[id] = Region{off, bytes, align, in_first, in_last};
}
// BEST with the two planes the any-hit traversals keep in it
constexpr void put_best(Layout &L, size_t &p, size_t bytes, bool occ_inside) {
    alias(L, LIMITS, p, PLANE32, 4, BEST, BEST);
    if (occ_inside)
        alias(L, OCC, p + PLANE32, PLANE32, 4, BEST, BEST);
    put(L, p, BEST, bytes, 8);
}
constexpr void put_leaf_pairs(Layout &L, size_t &p) {
    put(L, p, LKEY, LEAF_KEY_BYTES, 8);
    put(L, p, OWNER, LEAF_OWNER_BYTES, 1);
}

constexpr size_t pm1_pair_bytes(int meshes) {
    return (size_t)meshes * PAIRS_PER_MESH > PM1_PAIR_FLOOR ? (size_t)meshes * PAIRS_PER_MESH : (size_t)PM1_PAIR_FLOOR;
}
// PMODE 1: the read-only copies at the workgroup's base; returns their end
constexpr size_t put_pm1_scene(Layout &L, int meshes, int tri_slots) {
    size_t p = 0;
    put(L, p, TRIS, (size_t)tri_slots * TRI_BYTES + (size_t)meshes * PAD_BYTES, 16);
    put(L, p, MESHTAB, (size_t)meshes * MESHTAB_BYTES, 16);
    put(L, p, MESHBOX, (size_t)meshes * HEAD_BYTES, 16);
    return p;
}
// PMODE 1: a wave's minima and pair list, with what else lives in them (put_pm1_wave: a megakernel wave's whole part)
constexpr void put_pm1_lists(Layout &L, size_t &p, int meshes) {
    alias(L, PARK, p, PM1_PARK_BYTES, 4, BEST, PAIRS);
    put_best(L, p, PLANE64, true);
    // (64 * M + 32 <= 128 * M for every M >= 1)
    alias(L, DENSE_OWNER, p + (size_t)meshes * (PAIRS_PER_MESH / 2), DENSE_OWNER_BYTES, 1, PAIRS, PAIRS);
    put(L, p, PAIRS, pm1_pair_bytes(meshes), 4);
}

constexpr size_t put_pm1_wave(Layout &L, int meshes, bool bn) { // returns the part's size
    size_t w = 0;
    put_pm1_lists(L, w, meshes);
    put(L, w, BN, bn ? BN_BYTES : 0, 8); // the lanes' blue-noise values, if staged
    put(L, w, COUNT, COUNT_BYTES, 8);
    return w;
}

// ---- one-wave pair workgroups: the device queries in PMODE 1, 2, 3 and the megakernel in PMODE 2, 3, 4 ----------------------
// `meshes`: of the single TLAS leaf (PMODE 3 stages none); `pair_cap`: PMODE 4, entries of the list both kinds of ray share.
// Behind PMODE 1 a shape is told by its counts -- a pair capacity: PMODE 4, a TLAS leaf size: PMODE 3 -- which reach the kernels'
// carve as run-time values (KParams).  Measured: told by PMODE at compile time instead, path_trace_kernel<1,true,4,1,false> does
// less (fewer instructions, six scalar spills fewer) and the showcase frame is 0.8 % slower, 3.139 against 3.11 ms; by its
// counts the kernel is the instructions it was before the layouts had a header.
constexpr Layout pair_layout(int pmode, int meshes, int tri_slots, int stack_entries, int tlas_leaf, int tlas_depth, int pair_cap) {
    Layout L;
    size_t p = 0;
    if (pmode != 4)
        pair_cap = 0;
    if (pmode != 3)
        tlas_leaf = tlas_depth = 0;
    else
        meshes = 0;
    const bool merged = pair_cap != 0, tlas = tlas_leaf != 0;
    if (pmode == 1) {
        p = put_pm1_scene(L, meshes, tri_slots);
        put_pm1_lists(L, p, meshes);
        L.r[PARK] = Region{}; // (no lane refill in a query)
        // why the totals live in LDS: path_trace_kernel; here they take the pad no mesh's packets follow
        alias(L, COUNT, (size_t)tri_slots * TRI_BYTES + (size_t)(meshes - 1) * PAD_BYTES, COUNT_BYTES, 8, TRIS, TRIS);
        put(L, p, TAIL, PM1_QUERY_TAIL, 1);
        L.total = p;
        return L;
    }
    put(L, p, MESHBOX, (size_t)meshes * HEAD_BYTES, 16);
    put_best(L, p, tlas ? (size_t)PLANE64 * TLAS_SLOTS : (size_t)PLANE64, !merged);
    put(L, p, PAIRS,
        merged ? (size_t)pair_cap * PAIR_ENTRY
        : tlas ? ((size_t)tlas_leaf * 64 + TLAS_FILL_TARGET) * PAIR_ENTRY // one TLAS leaf per ray at a time
               : (size_t)meshes * PAIRS_PER_MESH,
        4);
    if (merged)
        put(L, p, OCC, PLANE32, 4);
    put(L, p, STACK, (size_t)stack_entries * PLANE64, 8);
    put(L, p, TSTACK, (size_t)tlas_depth * PLANE64, 8);
    put(L, p, LEAFX, tlas ? (size_t)PLANE32 * TLAS_SLOTS : 0, 4);
    put_leaf_pairs(L, p);
    put(L, p, COUNT, COUNT_BYTES, 8);
    put(L, p, DIRTY, DIRTY_BYTES, 8);
    L.total = p + (tlas && tlas_depth < 1 ? PLANE64 : 0); // (the host has always counted at least one TLAS stack plane)
    return L;
}
// PMODE 4: 64 * meshes entries always fit the extension pairs; the shadow pairs get what is left of `budget` bytes, at least 64
// (one mesh per pass), at most another 64 * meshes (everything in one pass)
constexpr int merged_cap_lo(int meshes) { return 64 * meshes + 64; }
constexpr int merged_cap_hi(int meshes) { return 128 * meshes; }
constexpr int merged_pair_cap(int meshes, int stack_entries, size_t budget) {
    const size_t rest = pair_layout(4, meshes, 0, stack_entries, 0, 0, 64).total - 64 * PAIR_ENTRY; // everything but the list
    int cap = rest < budget ? (int)((budget - rest) / PAIR_ENTRY) / 64 * 64 : 0;
    cap = cap < merged_cap_lo(meshes) ? merged_cap_lo(meshes) : cap;
    return cap > merged_cap_hi(meshes) ? merged_cap_hi(meshes) : cap;
}

// ---- PMODE 1 megakernel: a workgroup of 1 or 2 waves = neighbouring tiles shares ONE copy of what is read-only -- triangle
// packets, mesh table, mesh heads, jitter table, light and material records -- and each wave has its own lists behind it.
// What is staged is the host's decision (pm1_choose), handed to the kernel in KParams::lds_extra / lds_flags / lds_wave /
// lds_wave_bytes; both sides lay the workgroup out with pm1_layout.
struct Pm1Staging {
    int lds_extra = 0, lds_flags = 0, lds_wave = 0, lds_wave_bytes = 0; // == the KParams fields
};
constexpr size_t pm1_mat_bytes(int meshes, bool full) { return (size_t)meshes * (full ? MAT_BYTES_FULL : MAT_BYTES_SIMPLE); }
constexpr Layout pm1_layout(int meshes, int tri_slots, int n_lights, bool full, int wg, const Pm1Staging &s, int lds_pad) {
    Layout L;
    put_pm1_scene(L, meshes, tri_slots);
    size_t x = (size_t)s.lds_extra;
    put(L, x, JIT, JIT_BYTES, 8);
    put(L, x, LIGHTS, (s.lds_flags & 1) ? (size_t)n_lights * LIGHT_BYTES : 0, 16);
    put(L, x, MATS, (s.lds_flags & 2) ? pm1_mat_bytes(meshes, full) : 0, 16);
    if (!(s.lds_flags & 4))
        L.r[JIT].bytes = 0;
    L.wave_off = s.lds_wave;
    L.wave_bytes = s.lds_wave_bytes;
    L.waves = wg;
    put_pm1_wave(L, meshes, (s.lds_flags & 8) != 0);
    L.total = (size_t)L.wave_off + (size_t)wg * L.wave_bytes + (size_t)lds_pad;
    return L;
}
// What a workgroup of `wg` waves stages within `budget` bytes: the shading inputs piece by piece while it stays inside.
// Returns the workgroup's bytes, 0 if even the lists are over budget.  `stage`: option bits (1 lights, 2 materials, any: the
// jitter table); `stage_bn`: the lanes' blue-noise slots as well.
constexpr size_t pm1_stage(int meshes, int tri_slots, int n_lights, bool full, int stage, bool stage_bn, int lds_pad, int wg,
                           size_t budget, bool may_stage, Pm1Staging &s) {
    Layout scene;
    const size_t wave0 = put_pm1_wave(scene, meshes, false), pad = (size_t)lds_pad, bn = put_pm1_wave(scene, meshes, stage_bn) - wave0;
    const size_t lights = (size_t)n_lights * LIGHT_BYTES, mats = pm1_mat_bytes(meshes, full);
    size_t shared = (put_pm1_scene(scene, meshes, tri_slots) + 15) & ~(size_t)15;
    if (shared + wg * wave0 + pad > budget)
        return 0;
    s.lds_extra = (int)shared;
    s.lds_flags = 0;
    size_t wave = wave0;
    if (may_stage && stage && shared + JIT_BYTES + wg * (wave0 + bn) + pad <= budget) {
        s.lds_flags = 4 | (stage_bn ? 8 : 0);
        shared += JIT_BYTES;
        wave += bn;
        if ((stage & 1) && n_lights > 0 && n_lights <= LDS_LIGHTS && shared + lights + wg * wave + pad <= budget) {
            s.lds_flags |= 1;
            shared += lights;
        }
        if ((stage & 2) && meshes <= PM1_MATS_MAX && shared + mats + wg * wave + pad <= budget) {
            s.lds_flags |= 2;
            shared += mats;
        }
    }
    s.lds_wave = (int)shared;
    s.lds_wave_bytes = (int)wave;
    return shared + wg * wave + pad;
}
// The workgroup size and its staging, from the budgets of the occupancy the kernels are built for: two tiles if option pm1_wg
// allows them (simple materials only) and they fit `budget_wg2`; else one tile within `budget_wg1`; else -- over the budget of
// the kernel's occupancy, but the scene was admitted, so it runs -- one tile with nothing staged, up to `budget_max`.
struct Pm1Choice {
    Pm1Staging s;
    int wg = 1;
    size_t total = 0;
};
constexpr Pm1Choice pm1_choose(int meshes, int tri_slots, int n_lights, bool full, int stage, bool stage_bn, int lds_pad,
                                int pm1_wg, size_t budget_wg2, size_t budget_wg1, size_t budget_max) {
    Pm1Choice P;
    if (!full && pm1_wg != 1)
        P.total = pm1_stage(meshes, tri_slots, n_lights, full, stage, stage_bn, lds_pad, 2, budget_wg2, true, P.s);
    if (P.total) {
        P.wg = 2;
        return P;
    }
    P.total = pm1_stage(meshes, tri_slots, n_lights, full, stage, stage_bn, lds_pad, 1, budget_wg1, true, P.s);
    if (!P.total)
        P.total = pm1_stage(meshes, tri_slots, n_lights, full, stage, stage_bn, lds_pad, 1, budget_max, false, P.s);
    return P;
}

// ---- PMODE 2 in four-wave workgroups (option lds_nodes): mesh heads and the top levels of every BLAS are ONE copy per
// workgroup at the base of its LDS; behind them each wave has its own lists and stacks.
constexpr int NODES_WAVES = 4;
constexpr Layout nodes_layout(int meshes, int stack_entries, int top_nodes) {
    Layout L;
    size_t p = 0;
    put(L, p, MESHBOX, (size_t)meshes * HEAD_BYTES, 16);
    put(L, p, TOPNODES, (size_t)meshes * top_nodes * 64, 16);
    L.wave_off = (int)p;
    L.waves = NODES_WAVES;
    size_t w = 0;
    put_best(L, w, PLANE64, false);
    put(L, w, PAIRS, (size_t)meshes * PAIRS_PER_MESH, 4);
    put(L, w, OCC, PLANE32, 4);
    put(L, w, STACK, (size_t)stack_entries * PLANE64, 8);
    put_leaf_pairs(L, w);
    L.wave_bytes = (int)w;
    L.total = p + NODES_WAVES * w;
    return L;
}

// ---- PMODE 0: the lanes' lock-step stacks (the host passes no entries where every BLAS is one leaf)
constexpr Layout lockstep_layout(int stack_entries) {
    Layout L;
    size_t p = 0;
    put(L, p, STACK, (size_t)stack_entries * PLANE64, 8);
    L.total = p;
    return L;
}
// ---- the asynchronous-lane kernel: stacks, the ring of waiting pixels, the leaf phase's keys and owners
constexpr Layout async_layout(int stack_entries) {
    Layout L;
    size_t p = 0;
    put(L, p, STACK, (size_t)stack_entries * PLANE64, 8);
    put(L, p, RING, (size_t)AS_RING * 4, 4);
    put_leaf_pairs(L, p);
    L.total = p;
    return L;
}
// ---- the wavefront trace stage: four waves, each with its stacks and its ring
constexpr int WF_WAVES = 4;
constexpr Layout wavefront_layout(int stack_entries) {
    Layout L;
    size_t w = 0;
    put(L, w, STACK, (size_t)stack_entries * PLANE64, 8);
    put(L, w, RING, (size_t)WF_RING * 4, 4);
    L.wave_bytes = (int)w;
    L.waves = WF_WAVES;
    L.total = WF_WAVES * w;
    return L;
}

} // namespace lds
} // namespace pt
