// pt_atlas_filter.hip.h -- between scatter and dilation of a lightmap bake: one pass of the edge-aware a-trous filter of
// ptrt_atlas_filter over a baked atlas, src -> dst, float4 {r, g, b, valid} per texel, guided by the atlas's 32-byte records
// (world position, geometric normal, mesh: ptrt_atlas_texel).  One thread per texel, no traversal, no atomics: a pass reads
// only its source.
//
// The definition (include/ptrt.h has it in full) in fp32, -ffp-contract=off, `/` the compiler's IEEE quotient.  For the centre
// p = (i, j) with record G and colour C: G.mesh < 0 or C.valid == 0 copies C's 16 bytes.  Otherwise the 25 taps dy = -2..2
// outer, dx = -2..2 inner, q = (i + dx*step, j + dy*step); a tap outside the atlas, with Gq.mesh < 0 or with Cq.valid == 0 is
// skipped BY SELECTION (what it holds is loaded and never enters the arithmetic);
//     h  = K[|dx|] * K[|dy|]           K = {0.375, 0.25, 0.0625}
//     e  = Gq.position - G.position    d2 = (e.x*e.x + e.y*e.y) + e.z*e.z      x = 1 - d2 / rr      wd = x > 0 ? x : 0
//     pd = (G.n.x*e.x + G.n.y*e.y) + G.n.z*e.z                                 y = 1 - (pd*pd) / pp  wp = y > 0 ? y : 0
//     c  = (G.n.x*Gq.n.x + G.n.y*Gq.n.y) + G.n.z*Gq.n.z    c = c > 0 ? c : 0   then normal_power times c = c*c
//     w  = ((h * wd) * wp) * c         !(w > 0): skipped, else  num += w * Cq.rgb,  den += w
// den == 0 copies C; otherwise dst = {num / den, C.valid}.
//
// Two shapes of the same arithmetic (filter_tap), chosen per pass on the host (ptrt_atlas_filter, option "atlas_filter_tile"):
//   TILE_STEP 0: a workgroup of 64 x 4 texels, every tap three 16-byte global loads; at large steps the taps of a workgroup
//                are disjoint lattices that share little, and L2 serves them;
//   TILE_STEP 1, 2, 4 (== step): a workgroup of 16 x 16 texels stages its texels and a halo of 2*step -- (16 + 4*step)^2 records,
//                cut down to the 40 bytes a tap needs: position and a `usable` word, normal and red, green and blue -- in
//                static LDS (16 000, 23 040 and 40 960 bytes; step 8 would need 92 160), and the taps read that.  A record outside the atlas is staged as not
//                usable and no address outside the atlas is formed.
#pragma once
#include "pt_atlas.hip.h"

namespace pt {

constexpr int FILTER_TILE = 16;                       // the tiled shape's workgroup: FILTER_TILE^2 texels
constexpr int FILTER_ROW = 64, FILTER_ROWS = 4;       // the global shape's: a wave to a row of 64 texels
constexpr int filter_side(int step) { return FILTER_TILE + 4 * step; }

struct FilterSums {
    float r = 0.0f, g = 0.0f, b = 0.0f, den = 0.0f;
};

// One usable tap: its weight, and -- where the weight is above 0 -- its share of the sums.
__device__ __forceinline__ void filter_tap(FilterSums &s, float h, const float4 &gp, const float4 &gn, float qx, float qy, float qz, float qnx,
                                           float qny, float qnz, float qr, float qg, float qb, float rr, float pp, int normal_power) {
    const float ex = qx - gp.x, ey = qy - gp.y, ez = qz - gp.z;
    const float d2 = (ex * ex + ey * ey) + ez * ez;
    const float x = 1.0f - d2 / rr;
    const float wd = x > 0.0f ? x : 0.0f;
    const float pd = (gn.x * ex + gn.y * ey) + gn.z * ez;
    const float y = 1.0f - (pd * pd) / pp;
    const float wp = y > 0.0f ? y : 0.0f;
    float c = (gn.x * qnx + gn.y * qny) + gn.z * qnz;
    c = c > 0.0f ? c : 0.0f;
    for (int k = 0; k < normal_power; ++k) // (wave-uniform)
        c = c * c;
    const float w = ((h * wd) * wp) * c;
    if (w > 0.0f) {
        s.r = s.r + w * qr;
        s.g = s.g + w * qg;
        s.b = s.b + w * qb;
        s.den = s.den + w;
    }
}

__device__ __forceinline__ constexpr float filter_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

template <int TILE_STEP>
__global__ __launch_bounds__(256) void atlas_filter_kernel(const AtlasTexel *__restrict__ texels, const float4 *__restrict__ src,
                                                           float4 *__restrict__ dst, int aw, int ah, int step, float rr, float pp,
                                                           int normal_power, uint32_t tiles_x) {
    const float4 *__restrict__ guide = reinterpret_cast<const float4 *>(texels); // record t: guide[2t] position | face, guide[2t+1] normal | mesh
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    if constexpr (TILE_STEP == 0) {
        const int i = (int)(bx * FILTER_ROW + (threadIdx.x & (FILTER_ROW - 1))), j = (int)(by * FILTER_ROWS + threadIdx.x / FILTER_ROW);
        if (i >= aw || j >= ah)
            return;
        const size_t t = (size_t)j * (size_t)aw + (size_t)i;
        const float4 C = src[t];
        const float4 gp = guide[2 * t], gn = guide[2 * t + 1];
        if (__float_as_int(gn.w) < 0 || !(C.w != 0.0f)) {
            dst[t] = C;
            return;
        }
        FilterSums s;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int x = i + dx * step, y = j + dy * step; // |dx * step| <= 256, i < 2^28: no overflow
                if (x < 0 || y < 0 || x >= aw || y >= ah)
                    continue;
                const size_t q = (size_t)y * (size_t)aw + (size_t)x;
                const float4 qn = guide[2 * q + 1];
                const float4 qc = src[q];
                const float4 qp = guide[2 * q];
                if (__float_as_int(qn.w) < 0 || !(qc.w != 0.0f))
                    continue;
                filter_tap(s, filter_k(dx) * filter_k(dy), gp, gn, qp.x, qp.y, qp.z, qn.x, qn.y, qn.z, qc.x, qc.y, qc.z, rr, pp, normal_power);
            }
        }
        dst[t] = s.den == 0.0f ? C : make_float4(s.r / s.den, s.g / s.den, s.b / s.den, C.w);
    } else {
        constexpr int S = filter_side(TILE_STEP), H = 2 * TILE_STEP, N = S * S;
        static_assert(N * 40 <= 64 * 1024, "the tile and its halo fit a workgroup's LDS");
        __shared__ float4 l_pos[N]; // position | usable (in the atlas, mesh >= 0, valid != 0)
        __shared__ float4 l_nrm[N]; // normal | red
        __shared__ float2 l_gb[N];  // green, blue
        const int ox = (int)(bx * FILTER_TILE), oy = (int)(by * FILTER_TILE);
        for (int k = (int)threadIdx.x; k < N; k += 256) {
            const int ly = k / S, lx = k - ly * S;
            const int x = ox - H + lx, y = oy - H + ly;
            float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = p;
            float2 gb = make_float2(0.0f, 0.0f);
            if (x >= 0 && y >= 0 && x < aw && y < ah) {
                const size_t q = (size_t)y * (size_t)aw + (size_t)x;
                const float4 qp = guide[2 * q], qn = guide[2 * q + 1], qc = src[q];
                const bool usable = __float_as_int(qn.w) >= 0 && qc.w != 0.0f;
                p = make_float4(qp.x, qp.y, qp.z, __int_as_float(usable ? 1 : 0));
                n = make_float4(qn.x, qn.y, qn.z, qc.x);
                gb = make_float2(qc.y, qc.z);
            }
            l_pos[k] = p;
            l_nrm[k] = n;
            l_gb[k] = gb;
        }
        __syncthreads();
        const int tx = (int)(threadIdx.x & (FILTER_TILE - 1)), ty = (int)(threadIdx.x / FILTER_TILE);
        const int i = ox + tx, j = oy + ty;
        if (i >= aw || j >= ah)
            return;
        const size_t t = (size_t)j * (size_t)aw + (size_t)i;
        const float4 C = src[t];
        const int centre = (ty + H) * S + (tx + H);
        const float4 gp = l_pos[centre], gn = l_nrm[centre];
        if (__float_as_int(gp.w) == 0) { // G.mesh < 0 or C.valid == 0
            dst[t] = C;
            return;
        }
        FilterSums s;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int k = centre + dy * TILE_STEP * S + dx * TILE_STEP;
                const float4 qp = l_pos[k];
                const float4 qn = l_nrm[k];
                const float2 gb = l_gb[k];
                if (__float_as_int(qp.w) == 0)
                    continue;
                filter_tap(s, filter_k(dx) * filter_k(dy), gp, gn, qp.x, qp.y, qp.z, qn.x, qn.y, qn.z, qn.w, gb.x, gb.y, rr, pp, normal_power);
            }
        }
        dst[t] = s.den == 0.0f ? C : make_float4(s.r / s.den, s.g / s.den, s.b / s.den, C.w);
    }
}

} // namespace pt
