// pt_query.hip.h -- ray_query_kernel: batched ray queries straight from device memory (ptrt_query_rays).
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

template <int GEOM, int PMODE, int KIND>
__global__ __launch_bounds__(64) void ray_query_kernel(const KParams K, const float *__restrict__ origins,
                                                       const float *__restrict__ dirs, const float *__restrict__ tmax,
                                                       size_t n, void *__restrict__ out) {
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    PairLds PL = stage_pair_lds<PMODE>(K, lds_raw, lane);
    PL.cyc = &cyc;
    PL.stat_bounce = 0;
    __syncthreads();
    const size_t chunks = (n + 63) / 64;
    for (size_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) { // (wave-uniform)
        const size_t i = ch * 64 + (size_t)lane;
        const bool live = i < n;
        f3 o = mk3(0.0f), d = mk3(0.0f);
        float tm = 0.0f;
        if (live) {
            o = mk3(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]);
            d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
            if (KIND == QUERY_OCCLUDED)
                tm = tmax[i];
        }
        if (KIND == QUERY_CLOSEST) {
            int order;
            Hit h = (PMODE == 1)   ? closest_hit_pairs(K, PL, lane, live, o, d, order)
                    : (PMODE == 2) ? closest_hit_pairs_dyn(K, PL, lane, live, o, d)
                    : (PMODE == 3) ? closest_hit_pairs_tlas(K, PL, lane, live, o, d, cyc)
                                   : closest_hit<GEOM>(K, live, o, d, stk);
            if (live) {
                if (PMODE)
                    winner_uv(K, h, o, d);
                ((HitOut *)out)[i] = hit_record(K, h, o, d);
            }
        } else {
            const bool blocked = (PMODE == 1)   ? any_hit_pairs(K, PL, lane, live, o, d, tm)
                                 : (PMODE == 2) ? any_hit_pairs_dyn(K, PL, lane, live, o, d, tm)
                                 : (PMODE == 3) ? any_hit_pairs_tlas(K, PL, lane, live, o, d, tm, cyc)
                                                : any_hit<GEOM>(K, live, o, d, tm, stk);
            if (live)
                ((int *)out)[i] = blocked ? 1 : 0;
        }
    }
}

} // namespace pt
