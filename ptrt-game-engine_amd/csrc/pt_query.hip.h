// pt_query.hip.h -- ray_query_kernel: batched ray queries straight from device memory (ptrt_query_rays), and the frame that
// every device query shares with it: the prologue, the walks by PMODE, the chunk loop, the bakes' texel frame.
//
// Two questions, asked of the scene the next frame traces:
//   CLOSEST   traceRay (intersection.cuh:526-605) + the HitInfo fields of traceSingleRay (scene.cuh:1367-1391): one HitOut
//             (== ptrt_hit, 64 B) per ray -- the bits ptrt_trace_rays returns;
//   OCCLUDED  bvh_any_hit_tlas(ray, tmax[i]) (intersection.cuh:481-524), the reference's shadow query: one int32 per ray, 1 if
//             anything closer than tmax[i] blocks the ray.  Meshes with transmission > 0.5 do not block (their MeshHead flag).
//
// Two ways to walk, both the path kernel's own and both exact (the equivalences in pt_kernels.hip.h / pt_render.hip.h):
//   PMODE 0          one ray per lane, closest_hit<GEOM> / any_hit<GEOM> with the LDS stack of the lane;
//   PMODE 1, 2, 3    the wave-level (ray, mesh) pair traversal of phases [B] / [D] of path_trace_kernel, over the same LDS
//                    carve and staging (stage_pair_lds): PMODE 1 stages the triangle packets of a single-leaf scene, 2 the mesh
//                    heads of a single-leaf TLAS, 3 walks a real TLAS in rounds.
// The host picks the mode with pair_mode(c, geom, false) -- the path kernel's choice for the same scene and options.
//
// The grid is persistent: about one 64-thread workgroup per wave slot of the chip, each taking chunks of 64 rays with a
// grid-stride loop, so the staging above is paid once per workgroup.  Lanes past n in the last chunk take part in the wave's
// collectives as dead rays and write nothing.  Indices are size_t: i * 3 passes 2^31 at ~715 M rays.
#pragma once
#include "pt_render.hip.h"

namespace pt {

constexpr int QUERY_CLOSEST = 0, QUERY_OCCLUDED = 1; // == PTRT_QUERY_* (include/ptrt.h)

// the HitInfo record of a closest hit (trace_single_ray_kernel, scene_kernels.cuh; HitInfo() defaults on a miss)
PT_DEV HitOut hit_record(const KParams &K, const Hit &h, f3 o, f3 d) {
    HitOut r;
    if (h.mesh < 0) { // HitInfo() defaults (intersection.cuh:122-124)
        r.hit = 0;
        r.t = 1e30f;
        r.point[0] = r.point[1] = r.point[2] = 0.0f;
        r.normal[0] = r.normal[1] = r.normal[2] = 0.0f;
        r.mesh_index = -1;
        r.front_face = 1;
        r.u = r.v = 0.0f;
        r.face_index = -1;
        r.local_point[0] = r.local_point[1] = r.local_point[2] = 0.0f;
        return r;
    }
    f3 lp;
    int face;
    const Surface s = make_surface(K, h, o, d, &lp, &face);
    r.hit = 1;
    r.t = h.t;
    r.point[0] = s.point.x; r.point[1] = s.point.y; r.point[2] = s.point.z;
    r.normal[0] = s.normal.x; r.normal[1] = s.normal.y; r.normal[2] = s.normal.z;
    r.mesh_index = h.mesh;
    r.front_face = s.front_face ? 1 : 0;
    r.u = h.u;
    r.v = h.v;
    r.face_index = face;
    r.local_point[0] = lp.x; r.local_point[1] = lp.y; r.local_point[2] = lp.z;
    return r;
}

// The pair traversals return the winner's distance, mesh and slot but not its barycentrics (the path kernel has no use for
// them): one more triangle test of the winner, on the ray the traversal tested it with (local_ray for an instance), gives
// the u, v it computed -- tri_test's u and v depend on the packet and the ray only, not on the distance limit.
PT_DEV void winner_uv(const KParams &K, Hit &h, f3 o, f3 d) {
    if (h.mesh < 0)
        return;
    RayO r;
    r.o = o;
    r.d = d;
    if (__float_as_int(K.mesh_recs[h.mesh * MESH_REC_F4 + 1].w) & 1) {
        const float4 *rec = K.mesh_recs + h.mesh * MESH_REC_F4;
        r.o = xform_point(rec[2], rec[3], rec[4], o);
        r.d = normalize(xform_dir(rec[2], rec[3], rec[4], d));
    }
    const float4 p0 = K.tris[h.slot * 3 + 0], p1 = K.tris[h.slot * 3 + 1], p2 = K.tris[h.slot * 3 + 2];
    float t;
    tri_test(mk3(p0.x, p0.y, p0.z), mk3(p1.x, p1.y, p1.z), mk3(p2.x, p2.y, p2.z), r, T_FAR, t, h.u, h.v);
}

// ---- the frame every device query shares: inlined plain functions, so each kernel keeps its own allocation.

// The wave's prologue: the LDS carve and staging by PMODE, the stats build's hooks, the workgroup's one barrier.  A kernel holds
// `lane`, `stk` = {lds_raw + lane}, `cyc` and, behind this, a const PairLds.
template <int PMODE> PT_DEV PairLds query_stage(const KParams &K, uint2 *lds_raw, const int lane, CycleAcc &cyc) {
    PairLds PL = stage_pair_lds<PMODE>(K, lds_raw, lane);
    PL.cyc = &cyc;
    PL.stat_bounce = 0;
    __syncthreads();
    return PL;
}

// The closest hit and the any hit of the wave's 64 rays by PMODE; a lane that is not `alive` takes part in the collectives and
// hands the traversal whatever ray it holds (the callers: zeros).  Phases [B] and [D] of path_trace_kernel keep their own text.
template <int GEOM, int PMODE>
PT_DEV Hit walk_closest(const KParams &K, const PairLds &PL, const LdsStack stk, CycleAcc &cyc, const int lane, const bool alive,
                        const f3 o, const f3 d) {
    int order = 0; // (PMODE 1: the hit mesh's place in the leaf, which no query reads)
    return (PMODE == 1)   ? closest_hit_pairs(K, PL, lane, alive, o, d, order)
           : (PMODE == 2) ? closest_hit_pairs_dyn(K, PL, lane, alive, o, d)
           : (PMODE == 3) ? closest_hit_pairs_tlas(K, PL, lane, alive, o, d, cyc)
                          : closest_hit<GEOM>(K, alive, o, d, stk);
}
template <int GEOM, int PMODE>
PT_DEV bool walk_occluded(const KParams &K, const PairLds &PL, const LdsStack stk, CycleAcc &cyc, const int lane, const bool alive,
                          const f3 o, const f3 d, const float tmax) {
    return (PMODE == 1)   ? any_hit_pairs(K, PL, lane, alive, o, d, tmax)
           : (PMODE == 2) ? any_hit_pairs_dyn(K, PL, lane, alive, o, d, tmax)
           : (PMODE == 3) ? any_hit_pairs_tlas(K, PL, lane, alive, o, d, tmax, cyc)
                          : any_hit<GEOM>(K, alive, o, d, tmax, stk);
}

// Ray i of the caller's arrays for a chunk lane; a dead lane (i >= n) gets zeros.  (A loop that reads another word per ray -- the
// OCCLUDED loop its limit, radiance_query_kernel its generator state -- reads it in the same block as the ray and keeps that
// text: read behind this function it is a second round trip to memory per chunk, 3 to 6 % of the Cornell box's occlusion rate.)
struct ChunkRay {
    f3 o, d;
};
PT_DEV ChunkRay chunk_ray(const float *origins, const float *dirs, const size_t i, const bool live) {
    f3 o = mk3(0.0f), d = mk3(0.0f);
    if (live) {
        o = mk3(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]);
        d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
    }
    return ChunkRay{o, d};
}

// The closest-hit loop: the grid strides over chunks of 64 rays; per chunk one walk, the winner's u and v behind a pair walk
// (winner_uv), and sink(i, h, o, d) for every live lane.  ray_query_kernel<.., QUERY_CLOSEST>, lightmap_query_kernel
// (pt_lightmap.hip.h) and probe_light_query_kernel (pt_probe_sample.hip.h) are this loop with three sinks, so the latter two
// equal their samplers over ptrt_query_rays' records by construction.
template <int GEOM, int PMODE, class Sink>
PT_DEV void closest_chunk_loop(const KParams &K, const PairLds &PL, const LdsStack stk, CycleAcc &cyc, const int lane,
                               const float *origins, const float *dirs, const size_t n, const Sink sink) {
    const size_t chunks = (n + 63) / 64;
    for (size_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) { // (wave-uniform)
        const size_t i = ch * 64 + (size_t)lane;
        const bool live = i < n;
        const ChunkRay r = chunk_ray(origins, dirs, i, live);
        const f3 o = r.o, d = r.d;
        Hit h = walk_closest<GEOM, PMODE>(K, PL, stk, cyc, lane, live, o, d);
        if (live) {
            if (PMODE)
                winner_uv(K, h, o, d);
            sink(i, h, o, d);
        }
    }
}
struct HitToRecord { // the 64-byte HitOut of ptrt_query_rays
    const KParams &K;
    HitOut *out;
    PT_DEV void operator()(size_t i, const Hit &h, f3 o, f3 d) const { out[i] = hit_record(K, h, o, d); }
};

template <int GEOM, int PMODE, int KIND>
__global__ __launch_bounds__(64) void ray_query_kernel(const KParams K, const float *__restrict__ origins,
                                                       const float *__restrict__ dirs, const float *__restrict__ tmax,
                                                       size_t n, void *__restrict__ out) {
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    if (KIND == QUERY_CLOSEST) {
        closest_chunk_loop<GEOM, PMODE>(K, PL, stk, cyc, lane, origins, dirs, n, HitToRecord{K, (HitOut *)out});
        return;
    }
    const size_t chunks = (n + 63) / 64;
    for (size_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) { // (wave-uniform)
        const size_t i = ch * 64 + (size_t)lane;
        const bool live = i < n;
        f3 o = mk3(0.0f), d = mk3(0.0f);
        float tm = 0.0f;
        if (live) { // (the ray and its limit in one block: chunk_ray's comment)
            o = mk3(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]);
            d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
            tm = tmax[i];
        }
        const bool blocked = walk_occluded<GEOM, PMODE>(K, PL, stk, cyc, lane, live, o, d, tm);
        if (live)
            ((int *)out)[i] = blocked ? 1 : 0;
    }
}

// ---- the texel frame of the bakes (irradiance_query_kernel, direct_query_kernel, bounce_query_kernel): texels are many with
// few terms each, so the grid strides over GROUPS of texels.  With w = 1 << log2w the smallest power of two >= n_per (64
// beyond), a wave owns 64 / w consecutive texels, lane l being term l % w of texel slot l / w; beyond 64 terms a wave owns one
// texel and walks its ceil(n_per / 64) chunks.  Texel and group numbers fit 32 bits (n_texels + 63 < 2^32).  (wave-uniform)
struct TexelShape {
    int log2w, chunks;
    bool chunked;
    uint32_t groups;
};
__host__ PT_DEV TexelShape texel_shape(const int n_texels, const int n_per) {
    TexelShape S;
    S.log2w = 0;
    while (S.log2w < 6 && (1 << S.log2w) < n_per)
        ++S.log2w;
    S.chunked = n_per > 64;
    S.chunks = S.chunked ? (int)(((uint32_t)n_per + 63u) / 64u) : 1;
    S.groups = ((uint32_t)n_texels + (64u >> S.log2w) - 1u) >> (6 - S.log2w);
    return S;
}

// Lane l of group g in chunk c: term k of texel t.  The lane number goes through an empty asm, so that each use computes the
// pair afresh instead of holding it in registers.
struct TexelRay {
    uint32_t t, k;
};
PT_DEV TexelRay texel_ray(int lane, int log2w, uint32_t g, int c) {
    int me = lane;
    asm volatile("" : "+v"(me));
    return TexelRay{(g << (6 - log2w)) + (uint32_t)(me >> log2w), (uint32_t)c * 64u + (uint32_t)(me & ((1 << log2w) - 1))};
}

// v[j] + v[j ^ w/2], then ^ w/4, .. ^ 1 within segments of w lanes (w a power of two, wave-uniform), in every lane.  At w = 64
// it is the probes' fold over the wave: v[j] + v[j + 32], then + 16, 8, 4, 2, 1.
PT_DEV float segment_fold_sum(float v, int w) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        if (off < w) // (wave-uniform)
            v = v + __shfl_xor(v, off);
    return v;
}

} // namespace pt
