// pt_lightmap.hip.h -- the consumer of a lightmap bake: the baked atlas read back at ray hits.  lightmap_sample is the one
// definition (include/ptrt.h has it in full); atlas_sample_kernel applies it to ptrt_hit records that lie in device memory
// (ptrt_atlas_sample), lightmap_query_kernel to the hits of its own traversal (ptrt_query_lightmap) -- closest_chunk_loop
// (pt_query.hip.h), the one loop ray_query_kernel<GEOM, PMODE, QUERY_CLOSEST> is, with the 32-byte sample for a sink in place
// of the 64-byte hit record, so by construction the second equals the first over ptrt_query_rays' records.
//
// The definition in fp32, -ffp-contract=off (every operation rounds on its own), `/` the compiler's IEEE quotient.  For a hit
// on face f of mesh m at barycentrics (u, v) -- u belongs to corner v1, v to v2, as tri_test has them and as atlas_raster_kernel
// puts them through (v0 + b1*e1) + b2*e2:
//   a miss                                                       {0, 0, 0,  0,  0, 0,  -1, -1}
//   first = chart_first[m];  m outside the table, first < 0, f < 0 or first + f >= n_chart_faces (in 64 bits): no chart
//                                                                {0, 0, 0,  0,  0, 0,   f,  m}
//   (x0, y0, x1, y1, x2, y2) = charts[(first + f) * 6 ..]    b0 = (1 - u) - v
//   x = (b0*x0 + u*x1) + v*x2     y = (b0*y0 + u*y1) + v*y2      x or y not finite:   {0, 0, 0,  0,  x, y,   f,  m}
//   a tap (i, j) is usable iff 0 <= i < aw, 0 <= j < ah and image[j*aw + i].valid != 0.  Taps are skipped BY SELECTION: what an
//   unusable texel holds is loaded (its address clamped into the atlas where it lies outside) and never enters the arithmetic.
//   NEAREST   fi = floor(x), fj = floor(y); the tap (fi, fj), usable: rgb = its three words copied, weight = 1; else zeros.
//   BILINEAR  tx = x - 0.5, ty = y - 0.5; fi = floor(tx), fj = floor(ty); fx = tx - fi, fy = ty - fj; gx = 1 - fx, gy = 1 - fy;
//             taps (i0, j0) w = gx*gy, (i0+1, j0) fx*gy, (i0, j0+1) gx*fy, (i0+1, j0+1) fx*fy in that order; a usable tap with
//             w > 0: num += w * rgb per channel (the product rounded, then the sum), den += w.  den > 0: rgb = num / den,
//             weight = den; else zeros.
//   fi or fj outside [-1, 2^28], compared as floats before any conversion: no tap is usable (an atlas has at most 2^28 texels).
//   the record                                                   {rgb,  weight,  x, y,  f,  m}
//
// The additions to a traversal are one dependent chain: chart_first[m], then the chart's 24 bytes, then the image.  The four
// tap loads of the bilinear mode are issued together, each 16 bytes, and selected afterwards.
#pragma once
#include "pt_query.hip.h"

namespace pt {

constexpr int LIGHTMAP_NEAREST = 0, LIGHTMAP_BILINEAR = 1; // == PTRT_LIGHTMAP_* (include/ptrt.h)

struct LightmapSample { // mirrors ptrt_lightmap_sample, 32 bytes
    float rgb[3], weight, x, y;
    int face, mesh;
};

struct LightmapParams {
    const float *__restrict__ charts;     // n_chart_faces * 6 floats: ptrt_atlas_texels' d_uv, the meshes' charts concatenated
    const int *__restrict__ chart_first;  // per uploaded mesh the index in charts of its face 0, negative: no lightmap
    const float4 *__restrict__ image;     // aw * ah texels {r, g, b, valid}
    int n_chart_faces, n_meshes, aw, ah, mode;
};

// One tap: whether (i, j) lies in the atlas, and its texel -- the first texel of the atlas where it does not, so that the load
// can be issued before anything is known about the tap.
struct LightmapTap {
    float4 c;
    bool inside;
};
PT_DEV LightmapTap lightmap_tap(const LightmapParams &L, int i, int j, bool ok) {
    LightmapTap t;
    t.inside = ok && i >= 0 && j >= 0 && i < L.aw && j < L.ah;
    t.c = L.image[t.inside ? (size_t)j * (size_t)L.aw + (size_t)i : (size_t)0];
    return t;
}

// The definition.  o0 = {r, g, b, weight}, o1 = {x, y, face, mesh}: the record's two halves.
PT_DEV void lightmap_sample(const LightmapParams &L, bool hit, int m, int f, float u, float v, float4 &o0, float4 &o1) {
    o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o1 = make_float4(0.0f, 0.0f, __int_as_float(-1), __int_as_float(-1));
    if (!hit)
        return;
    o1.z = __int_as_float(f);
    o1.w = __int_as_float(m);
    if (m < 0 || m >= L.n_meshes)
        return;
    const int first = L.chart_first[m];
    if (first < 0 || f < 0 || (long long)first + (long long)f >= (long long)L.n_chart_faces)
        return;
    const float *c = L.charts + ((size_t)first + (size_t)f) * 6;
    const float x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5];
    const float b0 = (1.0f - u) - v;
    const float x = (b0 * x0 + u * x1) + v * x2;
    const float y = (b0 * y0 + u * y1) + v * y2;
    o1.x = x;
    o1.y = y;
    const float inf = __builtin_inff();
    if (!(__builtin_fabsf(x) < inf && __builtin_fabsf(y) < inf))
        return;
    const float LIMIT = 268435456.0f; // 2^28
    if (L.mode == LIGHTMAP_NEAREST) { // (wave-uniform)
        const float fi = __builtin_floorf(x), fj = __builtin_floorf(y);
        const bool ok = fi >= -1.0f && fi <= LIMIT && fj >= -1.0f && fj <= LIMIT;
        const LightmapTap t = lightmap_tap(L, ok ? (int)fi : -1, ok ? (int)fj : -1, ok);
        if (t.inside && t.c.w != 0.0f)
            o0 = make_float4(t.c.x, t.c.y, t.c.z, 1.0f);
        return;
    }
    const float tx = x - 0.5f, ty = y - 0.5f;
    const float fi = __builtin_floorf(tx), fj = __builtin_floorf(ty);
    const float fx = tx - fi, fy = ty - fj;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const bool ok = fi >= -1.0f && fi <= LIMIT && fj >= -1.0f && fj <= LIMIT;
    const int i0 = ok ? (int)fi : -1, j0 = ok ? (int)fj : -1; // -1 .. 2^28: i0 + 1 does not overflow
    const LightmapTap t00 = lightmap_tap(L, i0, j0, ok), t10 = lightmap_tap(L, i0 + 1, j0, ok);
    const LightmapTap t01 = lightmap_tap(L, i0, j0 + 1, ok), t11 = lightmap_tap(L, i0 + 1, j0 + 1, ok);
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
    const auto add = [&](const LightmapTap &t, float w) {
        if (t.inside && t.c.w != 0.0f && w > 0.0f) {
            nr = nr + w * t.c.x;
            ng = ng + w * t.c.y;
            nb = nb + w * t.c.z;
            den = den + w;
        }
    };
    add(t00, gx * gy);
    add(t10, fx * gy);
    add(t01, gx * fy);
    add(t11, fx * fy);
    if (den > 0.0f)
        o0 = make_float4(nr / den, ng / den, nb / den, den);
}

// ptrt_atlas_sample: one thread per 64-byte ptrt_hit record in device memory, read as 16-byte words -- {hit, t, point.xy},
// {mesh_index, front_face, u, v}, {face_index, local_point} --, the 32-byte sample written as two.
__global__ __launch_bounds__(256) void atlas_sample_kernel(const float4 *__restrict__ hits, size_t n, const LightmapParams L,
                                                           float4 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const float4 q0 = hits[i * 4 + 0], q2 = hits[i * 4 + 2], q3 = hits[i * 4 + 3];
    float4 o0, o1;
    lightmap_sample(L, __float_as_int(q0.x) != 0, __float_as_int(q2.x), __float_as_int(q3.x), q2.z, q2.w, o0, o1);
    out[i * 2 + 0] = o0;
    out[i * 2 + 1] = o1;
}

// ptrt_query_lightmap: closest_chunk_loop (pt_query.hip.h) -- the persistent grid of one-wave workgroups, the LDS carve and
// staging by PMODE, the closest-hit walk, winner_uv for the pair walks -- with, where ray_query_kernel forms the 64-byte HitOut,
// the face of the winning slot, its u and v, and the sample.  The hit point, the normal and the local point are not formed.
struct HitToLightmapSample {
    const KParams &K;
    const LightmapParams &L;
    float4 *out;
    PT_DEV void operator()(size_t i, const Hit &h, f3, f3) const {
        const bool hit = h.mesh >= 0;
        float4 o0, o1;
        lightmap_sample(L, hit, h.mesh, hit ? K.slot_face[h.slot].w : -1, hit ? h.u : 0.0f, hit ? h.v : 0.0f, o0, o1);
        out[i * 2 + 0] = o0;
        out[i * 2 + 1] = o1;
    }
};
template <int GEOM, int PMODE>
__global__ __launch_bounds__(64) void lightmap_query_kernel(const KParams K, const float *__restrict__ origins,
                                                            const float *__restrict__ dirs, size_t n, const LightmapParams L,
                                                            float4 *__restrict__ out) {
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    closest_chunk_loop<GEOM, PMODE>(K, PL, stk, cyc, lane, origins, dirs, n, HitToLightmapSample{K, L, out});
}

} // namespace pt
