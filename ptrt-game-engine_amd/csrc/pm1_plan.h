// pm1_plan.h -- PMODE 1, option "pm1_lane_groups": how the tail of a pair list (fewer than 64 pairs) is cut into sub-batches
// and how many lanes each of their pairs gets (closest_hit_pairs / any_hit_pairs, pt_render.hip.h).
// Plain C++, no HIP: the device library builds the table at upload, the host-only entry point ptrt_pm1_plan reads it back.
//
// With every staged leaf holding L triangles, a sub-batch gives each pair g lanes, g a divisor of L, and takes
// min(n, 64 / g) of the n pairs that are left; lane l serves pair l / g and tests triangles l mod g, l mod g + g, ...: L / g
// iterations of the full-leaf loop.  The plan for a tail of n pairs is the sequence that minimises the sum of
// (L / g) * PM1_BODY + PM1_HEADER wave-instructions; ties go to fewer sub-batches, then to the smaller g.  The present rule
// (one batch at 2^sh lanes per pair) is a candidate as well, at ceil(L / 2^sh) iterations: where 2^sh does not divide L it
// runs the guarded loop in ONE batch, which no sequence of divisor sub-batches need match (7 triangles, 10 pairs: two
// iterations against 1 + 1 and a second header).  Such a tail keeps the present rule: its entry has g = 0.
#pragma once
#include <cstdint>

namespace pt {

// The cost model, in VALU + LDS wave-instructions counted in the ISA of path_trace_kernel<0,false,1,1,true>:
// one test of the full-leaf closest-hit loop (42 + 3), and one sub-batch without its tests (45 + 9: lane / g, the pair read,
// meshtab, six ds_bpermute, the loop set-up, the triangle index and the merge with its division).  H = PM1_HEADER / PM1_BODY
// = 1.2 tests.
constexpr int PM1_BODY = 45, PM1_HEADER = 54;
constexpr int PM1_MAX_LEAF = 255;   // leaves above this keep the present rule (the entry's iteration count has 16 bits to spare; g never exceeds 64)
constexpr int PM1_DIV_SHIFT = 12;   // lane / g = (lane * (4096 / g + 1)) >> 12 for every lane < 64, g <= 64 (pm1_div_exact)

struct Pm1Entry {
    uint32_t w; // g | take << 8 | (L / g) << 16; g = 0: the present rule
    uint32_t m; // 4096 / g + 1
};
struct Pm1Plan {
    Pm1Entry e[64]; // by the tail n = 1 .. 63; e[0] (a full batch: one lane per pair) keeps the present rule
};

inline uint32_t pm1_div_mul(int g) { return (uint32_t)((1 << PM1_DIV_SHIFT) / g + 1); }
// the multiply-and-shift division is exact for this g over lanes 0 .. 63
inline bool pm1_div_exact(int g) {
    if (g < 1)
        return false;
    for (int lane = 0; lane < 64; ++lane)
        if ((int)(((uint32_t)lane * pm1_div_mul(g)) >> PM1_DIV_SHIFT) != lane / g)
            return false;
    return true;
}

// the present rule for n < 64 pairs: the shift, and through `iters` the iterations of its single batch
inline int pm1_present_shift(int L, int n, int *iters = nullptr) {
    int sh = 0;
    while ((n << (sh + 1)) <= 64 && (2 << sh) <= L)
        ++sh;
    if (iters)
        *iters = (L + (1 << sh) - 1) >> sh;
    return sh;
}

// Fills `plan` for leaves of L triangles; `cost` (may be null) receives the plan's cost per tail in wave-instructions.
// Returns false, with every entry at the present rule, when L is out of range.
inline bool pm1_build_plan(int L, Pm1Plan *plan, int *cost64 = nullptr) {
    int cost[64], count[64];
    cost[0] = count[0] = 0;
    plan->e[0] = Pm1Entry{0u, 0u};
    const bool ok = L >= 1 && L <= PM1_MAX_LEAF;
    for (int n = 1; n < 64; ++n) {
        plan->e[n] = Pm1Entry{(uint32_t)n << 8, 0u};
        int it;
        pm1_present_shift(ok ? L : 1, n, &it);
        cost[n] = it * PM1_BODY + PM1_HEADER; // the present rule's single batch
        count[n] = 1;
        for (int g = 1; ok && g <= L && g <= 64; ++g) {
            if (L % g || !pm1_div_exact(g))
                continue;
            const int cap = 64 / g, take = n < cap ? n : cap;
            const int cst = (L / g) * PM1_BODY + PM1_HEADER + cost[n - take], cnt = 1 + count[n - take];
            // (at equal cost and count a divisor sub-batch replaces the present rule,
            // whose guarded loop is the dearer one per test; among divisors the first, smallest, g stays)
            const bool present = (plan->e[n].w & 0xffu) == 0;
            if (cst < cost[n] || (cst == cost[n] && (cnt < count[n] || (cnt == count[n] && present)))) {
                cost[n] = cst;
                count[n] = cnt;
                plan->e[n] = Pm1Entry{(uint32_t)g | (uint32_t)take << 8 | (uint32_t)(L / g) << 16, pm1_div_mul(g)};
            }
        }
    }
    if (cost64)
        for (int n = 0; n < 64; ++n)
            cost64[n] = cost[n];
    return ok;
}

} // namespace pt
