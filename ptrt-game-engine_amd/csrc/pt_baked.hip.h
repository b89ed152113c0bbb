// pt_baked.hip.h -- the baked-light view (ptrt_render_baked): the scene lit by what was baked for it -- a lightmap atlas, a probe
// volume, both or neither -- as one frame in the RGB8 target every other view uses.  baked_view_kernel<GEOM, PMODE> is one launch:
// the primary ray, the closest hit, the two samplers, the albedo, the tonemap.  Every piece is a function another kernel already
// is: pixel_uv and pinhole_ray (pt_path.hip.h; camera_rays_kernel), query_stage, walk_closest, winner_uv and hit_record
// (pt_query.hip.h; ray_query_kernel), lightmap_sample (pt_lightmap.hip.h), probe_light (pt_probe_sample.hip.h), sample_sky,
// tonemap_pixel and rgb8_row (the path frame's).  So by construction a pixel equals what the chain ptrt_camera_rays ->
// ptrt_query_rays / ptrt_query_lightmap / ptrt_query_probe_light gives its ray, shaded as below; tests/baked_view_restatement.py
// states the shading in numpy over those rows.
//
// The definition in fp32, -ffp-contract=off (every operation rounds on its own), `/` the compiler's IEEE quotient.  For pixel
// (x, y) of the full W x H frame (a reduced render size plays no part), frame_index F:
//   1. (u, v) = pixel_uv(x, y, F);  (o, d) = pinhole_ray(u, v): the ray ptrt_camera_rays(F, 0) writes for the pixel.
//   2. the closest hit of ptrt_query_rays(PTRT_QUERY_CLOSEST) for (o, d).
//   3. a miss:  c = use_sky ? sample_sky(d) : 0.
//   4. a hit on face f of mesh m at (u, v):  E =
//        lightmap_sample's rgb                where a lightmap is given and its weight > 0;
//        probe_light's irradiance             otherwise, where a volume is given and its weight > 0 -- at hit_record's point and
//                                             face-forwarded normal, in the lanes the lightmap left empty only, BY SELECTION;
//        +0                                   otherwise (a NaN weight is not > 0).
//   5. c = (albedo_m * E) / 3.14159265f + emission_m, albedo_m = materials[m*6+0].xyz, emission_m = materials[m*6+2].xyz: the
//      product, the quotient, then the sum, per channel.
//   6. hdr[yl*W + x] = c;  normal / depth / object_id[yl*W + x] = hit_record's normal, t and mesh ({0,0,0}, 1e30f, -1 on a miss);
//      RGB8 = tonemap_pixel(c) at row rgb8_row(yl), bottom-up.  Each output is written where its pointer is given.
//
// Execution: the device queries' shape -- a persistent grid of one-wave workgroups, query_stage once per workgroup, then a stride
// over the 8x8 tiles of the context's rows in plain order; 64 lanes are one tile (tile_pixel), a lane outside the frame a dead ray
// that takes part in the wave's collectives and writes nothing.  Both samplers sit behind the walk: nothing of theirs is live
// across it.
#pragma once
#include "pt_lightmap.hip.h"
#include "pt_path.hip.h"
#include "pt_probe_sample.hip.h"

namespace pt {

struct BakedViewParams {   // ptrt_baked_view, vetted and copied into the launch
    LightmapParams L;      // L.image == nullptr: no lightmap
    ProbeVolumeParams V;   // V.probes == nullptr: no probes
    float *hdr, *normal, *depth; // each may be nullptr; rows * W pixels in PTRT_BUF_ACCUM's order
    int *object_id;
};

// Steps 3 to 6 for one live pixel.
PT_DEV void baked_pixel(const KParams &K, const BakedViewParams &B, const int x, const int yl, const Hit &h, const f3 o, const f3 d) {
    const bool hit = h.mesh >= 0;
    f3 c = mk3(0.0f);
    f3 gn = mk3(0.0f);
    float gt = 1e30f;
    int gm = -1;
    if (!hit) {
        if (K.use_sky)
            c = sample_sky(K, d);
    } else {
        float er = 0.0f, eg = 0.0f, eb = 0.0f;
        bool lit = false;
        if (B.L.image) { // (wave-uniform)
            float4 o0, o1;
            lightmap_sample(B.L, true, h.mesh, K.slot_face[h.slot].w, h.u, h.v, o0, o1);
            if (o0.w > 0.0f) {
                er = o0.x;
                eg = o0.y;
                eb = o0.z;
                lit = true;
            }
        }
        const bool want_probe = B.V.probes && !lit;
        if (want_probe || B.normal || B.depth || B.object_id) {
            const HitOut r = hit_record(K, h, o, d);
            gn = mk3(r.normal[0], r.normal[1], r.normal[2]);
            gt = r.t;
            gm = r.mesh_index;
            if (want_probe) {
                float4 o0, o1;
                probe_light(B.V, mk3(r.point[0], r.point[1], r.point[2]), gn, r.face_index, r.mesh_index, o0, o1);
                if (o0.w > 0.0f) {
                    er = o0.x;
                    eg = o0.y;
                    eb = o0.z;
                }
            }
        }
        const float4 m0 = K.materials[h.mesh * 6 + 0], m2 = K.materials[h.mesh * 6 + 2];
        c.x = (m0.x * er) / 3.14159265f + m2.x;
        c.y = (m0.y * eg) / 3.14159265f + m2.y;
        c.z = (m0.z * eb) / 3.14159265f + m2.z;
    }
    const size_t idx = (size_t)yl * (size_t)K.width + (size_t)x;
    if (B.hdr) {
        B.hdr[idx * 3 + 0] = c.x;
        B.hdr[idx * 3 + 1] = c.y;
        B.hdr[idx * 3 + 2] = c.z;
    }
    if (B.normal) {
        B.normal[idx * 3 + 0] = gn.x;
        B.normal[idx * 3 + 1] = gn.y;
        B.normal[idx * 3 + 2] = gn.z;
    }
    if (B.depth)
        B.depth[idx] = gt;
    if (B.object_id)
        B.object_id[idx] = gm;
    if (K.rgb8) {
        unsigned char r8, g8, b8;
        tonemap_pixel(c, r8, g8, b8);
        unsigned char *p = K.rgb8 + ((size_t)rgb8_row(K, yl) * (size_t)K.width + (size_t)x) * 3;
        p[0] = r8;
        p[1] = g8;
        p[2] = b8;
    }
}

// K: the context's parameters with width / height the FULL frame, rows / y0 the context's band, tiles_x the full frame's,
// frame_count the frame index, rgb8 / rgb8_frame the target (nullptr: none); the generator, accumulation and G-buffer pointers of
// the context are null -- this kernel writes none of them.
template <int GEOM, int PMODE>
__global__ __launch_bounds__(64) void baked_view_kernel(const KParams K, const BakedViewParams B) {
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    const int tiles = K.tiles_x * ((K.rows + 7) / 8);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (wave-uniform)
        int x, yl;
        tile_pixel(K.tiles_x, tile, lane, x, yl);
        const bool live = x < K.width && yl < K.rows;
        f3 o = mk3(0.0f), d = mk3(0.0f);
        if (live) {
            float u, v;
            pixel_uv(K, x, K.y0 + yl, K.frame_count, u, v); // (an interleaved context is refused by ptrt_render_baked)
            pinhole_ray(K.cam, u, v, o, d);
        }
        Hit h = walk_closest<GEOM, PMODE>(K, PL, stk, cyc, lane, live, o, d);
        if (live) {
            if (PMODE)
                winner_uv(K, h, o, d);
            baked_pixel(K, B, x, yl, h, o, d);
        }
    }
}

} // namespace pt
