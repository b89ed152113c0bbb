// pt_path.hip.h -- the primary ray and what starts and ends a pixel (scene_kernels.cuh:147-193), then one vertex of tracePath
// (path_logic.cuh:782-899), stated once for the loops that are not tuned by their ISA:
// wf_shade_path (pt_wavefront.hip.h), path_trace_async_kernel (pt_async.hip.h) and trace_chunk_samples (pt_radiance.hip.h: the
// radiance and probe queries).  path_trace_kernel (pt_render.hip.h, phases [C]-[E]) keeps its own text of the same statement:
// its instantiations are measured, and calling these helpers there moved their registers and scratch.
//
// The contract is the order of the floating-point operations and of the generator's draws; the build uses -ffp-contract=off, so
// a reordered product is a changed bit.  Every expression below is the one tests/shading_truth.py and tests/path_truth.py pin.
//
// The helpers take records that are already loaded (LightRec, Material, the two float4 of a material that [C] reads), so they
// do not care where a loop keeps them.  What differs between the loops stays in the loops: where the first hit goes, the
// counters, what carries the light sample to its shadow ray, and when its value is added.
#pragma once
#include "pt_kernels.hip.h"

namespace pt {

// ---- what starts and ends a pixel: phase [A] and the frame's per-pixel planes, stated once for wf_shade_path, the asynchronous
// lanes and camera_rays_kernel (pt_radiance.hip.h).  path_trace_kernel's [A] keeps its own text of the same statement, as its
// [C]-[E] do.  tests/frame_truth.py pins every expression.

// Position l of the 8x8 tile `tile` (tiles_x tiles per row): the pixel's column and its row within the context's rows.  A tile
// on the frame's edge has positions outside it.
PT_DEV void tile_pixel(const int tiles_x, const int tile, const int l, int &x, int &yl) {
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    x = tx * 8 + (l & 7);
    yl = ty * 8 + (l >> 3);
}

// Where pixel (x, y) of sample `frame` = frame_count + s looks through the image plane (scene_kernels.cuh:147-163): the TAA
// entry, the blue-noise entry, their sum, u and v.
PT_DEV void pixel_uv(const KParams &K, const int x, const int y, const int frame, float &u, float &v) {
    float tjx, tjy, bnx, bny;
    taa_jitter(frame, tjx, tjy);
    blue_noise_jitter(K.blue_noise, x, y, frame, bnx, bny);
    const float jitter_x = tjx + (bnx - 0.5f) * 0.25f;
    const float jitter_y = tjy + (bny - 0.5f) * 0.25f;
    u = ((float)x + 0.5f + jitter_x) / (float)K.width;
    v = 1.0f - ((float)y + 0.5f + jitter_y) / (float)K.height;
}

// Camera::get_ray with a generator (camera.cuh:156-166).  The pinhole (get_ray_simple, camera.cuh:201-205), and the thin lens
// (camera.cuh:160-165): a point of the unit disk by rejection, two draws per turn, `a` before `b`.
PT_DEV void pinhole_ray(const Camera &cam, const float u, const float v, f3 &ro, f3 &rd) {
    const f3 dir = cam.llc + u * cam.horizontal + v * cam.vertical - cam.origin;
    ro = cam.origin;
    rd = normalize(dir);
}
PT_DEV void camera_ray(const Camera &cam, const float u, const float v, Rng &rng, f3 &ro, f3 &rd) {
    if (cam.lens_radius <= 0) {
        pinhole_ray(cam, u, v, ro, rd);
    } else {
        f3 p;
        do {
            const float a = rng_uniform(rng);
            const float b = rng_uniform(rng);
            p = 2.0f * mk3(a, b, 0.0f) - mk3(1.0f, 1.0f, 0.0f);
        } while (dot(p, p) >= 1.0f);
        const f3 rdisk = cam.lens_radius * p;
        const f3 offset = cam.u * rdisk.x + cam.v * rdisk.y;
        const f3 dir = cam.llc + u * cam.horizontal + v * cam.vertical - cam.origin - offset;
        ro = cam.origin + offset;
        rd = normalize(dir);
    }
}

// A generator state in memory, six words in the canonical order {d, v0..v4}.  A ray's state in a caller's array (the queries):
// the words side by side.  A pixel's in the frame's six planes (K.rng, K.rng_plane words each): word k at idx + k * plane.
PT_DEV void load_rng_state(Rng &rng, const uint32_t *st) {
    rng.d = st[0];
    rng.v0 = st[1];
    rng.v1 = st[2];
    rng.v2 = st[3];
    rng.v3 = st[4];
    rng.v4 = st[5];
}
PT_DEV void store_rng_state(uint32_t *st, const Rng &rng) {
    st[0] = rng.d;
    st[1] = rng.v0;
    st[2] = rng.v1;
    st[3] = rng.v2;
    st[4] = rng.v3;
    st[5] = rng.v4;
}
PT_DEV void load_rng_planes(Rng &rng, const uint32_t *planes, const size_t plane, const size_t idx) {
    rng.d = planes[idx];
    rng.v0 = planes[plane + idx];
    rng.v1 = planes[2 * plane + idx];
    rng.v2 = planes[3 * plane + idx];
    rng.v3 = planes[4 * plane + idx];
    rng.v4 = planes[5 * plane + idx];
}
PT_DEV void store_rng_planes(uint32_t *planes, const size_t plane, const size_t idx, const Rng &rng) {
    planes[idx] = rng.d;
    planes[plane + idx] = rng.v0;
    planes[2 * plane + idx] = rng.v1;
    planes[3 * plane + idx] = rng.v2;
    planes[4 * plane + idx] = rng.v3;
    planes[5 * plane + idx] = rng.v4;
}

// Where the first hit of a pixel's sample 0 goes in a frame: NORMAL / DEPTH / OBJECT_ID at the pixel (scene_kernels.cuh:
// 179-193).  A miss stores the HitInfo() defaults: first(1e30f, mk3(0.0f), -1).  (The queries' sinks: FirstHitToRecord,
// pt_radiance.hip.h; FirstHitToRegs, pt_probe.hip.h.)
struct FirstHitToFrame {
    const KParams &K;
    size_t idx;
    PT_DEV void operator()(float depth, f3 normal, int object_id) const {
        K.normal[idx * 3 + 0] = normal.x;
        K.normal[idx * 3 + 1] = normal.y;
        K.normal[idx * 3 + 2] = normal.z;
        K.depth[idx] = depth;
        K.object_id[idx] = object_id;
    }
};

// ---- the vertex

// sampleSky (render_utils.cuh:115-137): the equirect map, or the gradient.  For a scene that has a sky (K.use_sky).
PT_DEV f3 sample_sky(const KParams &K, const f3 rd) {
    if (K.env) {
        const float phi = det_atan2(rd.z, rd.x);
        const float theta = det_acos(max_(-1.0f, min_(1.0f, rd.y)));
        const float u = (phi + PI_F) * (1.0f / TWO_PI_F);
        const float v = theta * (1.0f / PI_F);
        return tex2d_env(K.env, K.env_w, K.env_h, u, v);
    }
    const float t = 0.5f * (rd.y + 1.0f);
    return lerp(K.sky_bottom, K.sky_top, t);
}

// What a miss adds to the path's radiance (path_logic.cuh:795-800); without a sky the reference still adds its zero.
PT_DEV void add_miss_radiance(const KParams &K, const f3 rd, const f3 throughput, f3 &acc) {
    if (K.use_sky)
        acc = acc + throughput * sample_sky(K, rd);
    else
        acc = acc + throughput * mk3(0.0f);
}

// Beer-Lambert on back faces, then emission (path_logic.cuh:823-838).  m0, m2: float4 0 and 2 of the hit mesh's material
// record; first_or_behind_specular: bounce == 0 || prev_was_specular.
PT_DEV void absorb_and_emit(const float4 m0, const float4 m2, const Surface &hit, const bool first_or_behind_specular,
                            f3 &throughput, f3 &acc) {
    if (!hit.front_face) {
        const f3 T_unit = mk3(max_(1e-6f, m0.x), max_(1e-6f, m0.y), max_(1e-6f, m0.z));
        const f3 absorption = mk3(-det_log(T_unit.x), -det_log(T_unit.y), -det_log(T_unit.z));
        throughput = throughput * beerLambert(absorption, hit.t);
    }
    if (m2.x > 0.0f || m2.y > 0.0f || m2.z > 0.0f) {
        if (first_or_behind_specular)
            acc = acc + throughput * mk3(m2.x, m2.y, m2.z);
    }
}

// The light of next-event estimation (path_logic.cuh:305-312): one draw; the caller loads the record.  n_lights > 0.
PT_DEV int pick_light(Rng &rng, const int n_lights) {
    float r = rng_uniform(rng);
    r = min_(r, 0.99999994f);
    return (int)(r * (float)n_lights);
}

// The sample of the picked light seen from `hit` (path_logic.cuh:313-356, 840): direction L, its density, the light's radiance
// and the attenuation -- kept apart so that the caller's product is formed in the reference's order -- and the shadow ray's
// origin and length.  A light with a radius draws its cone sample here, from `rng`: the generator, or the two numbers a caller
// gives (GivenDraws: direct_sample, pt_direct.hip.h).
template <class Draws>
PT_DEV void sample_light(const LightRec &light, const float inv_n_lights, const Surface &hit, Draws &rng, f3 &L, float &pdf_sample,
                         f3 &light_scale, float &light_att, f3 &shadow_o, float &shadow_tmax) {
    const float pdf_pick = inv_n_lights; // 1.0f / (float)n_lights: KParams::inv_n_lights, the host's IEEE quotient
    float attenuation = 1.0f;
    float light_dist = 1e30f;
    const f3 light_radiance = light.color * light.intensity;
    if (light.type == 1) {
        L = -light.direction;
        pdf_sample = pdf_pick;
    } else {
        const f3 toLight = light.position - hit.point;
        const float light_dist_sq = dot(toLight, toLight);
        light_dist = sqrt_ieee(light_dist_sq);
        if (light.radius <= 0.0f) {
            L = toLight / light_dist;
            pdf_sample = pdf_pick;
        } else {
            float sin_theta_max_sq = (light.radius * light.radius) / light_dist_sq;
            sin_theta_max_sq = min_(sin_theta_max_sq, 0.9999f);
            const float cos_theta_max = sqrt_ieee(1.0f - sin_theta_max_sq);
            L = sample_cone_direction(rng, toLight / light_dist, cos_theta_max);
            const float solid_angle = TWO_PI_F * (1.0f - cos_theta_max);
            pdf_sample = (solid_angle > 1e-6f) ? (pdf_pick / solid_angle) : pdf_pick;
        }
        attenuation = attenuate(light_dist, light.range);
        if (light.type == 2) {
            const float theta = dot(L, -light.direction);
            const float epsilon = light.inner - light.outer;
            float spotIntensity;
            if (epsilon <= 1e-6f)
                spotIntensity = (theta >= light.outer) ? 1.0f : 0.0f;
            else
                spotIntensity = clampf((theta - light.outer) / epsilon, 0.0f, 1.0f);
            attenuation *= spotIntensity;
        }
    }
    const f3 shadow_offset = dot(hit.normal, L) > 0.0f ? hit.normal * 1e-4f : -hit.normal * 1e-4f;
    shadow_o = hit.point + shadow_offset;
    shadow_tmax = light_dist - 1e-3f;
    light_scale = light_radiance;
    light_att = attenuation;
}

// What the light sample adds if it is visible (path_logic.cuh:357-381, 840-867): bsdf * radiance * attenuation / pdf, soft-
// clamped, weighted against the BSDF's density, times the throughput.  False: it adds nothing either way (outside a spot's
// cone, BSDF zero below the horizon), and `value` is untouched.
template <bool FULL>
PT_DEV bool light_sample_value(const Surface &hit, const Material &mat, const f3 L, const f3 V, const float pdf_sample,
                               const f3 light_scale, const float light_att, const f3 throughput, f3 &value) {
    const f3 bsdf = evaluateBSDF<FULL>(hit, mat, L, V);
    if (pdf_sample > 0.0f) {
        f3 direct = bsdf * light_scale * light_att / pdf_sample;
        direct = clamp_vector_soft(direct, 500.0f);
        if (direct.x > 0.0f || direct.y > 0.0f || direct.z > 0.0f) {
            const float pdf_brdf = material_pdf<FULL>(hit, mat, V, L);
            const float wgt = mis_weight(pdf_sample, pdf_brdf);
            value = throughput * direct * wgt;
            return true;
        }
    }
    return false;
}

// The BSDF sample and what follows it (path_logic.cuh:843-896): scatter, Russian roulette from the third vertex, the
// throughput's clamp, the next ray from the offset origin, the depth limit.  True: the path goes on with (ro, rd) -- it ends
// where the material absorbs, the roulette kills, or `bounce` reaches max_depth (ray and throughput are then the last vertex's).
// `F`: hit.normal's tangent frame from the per-triangle table (KParams::tri_frames), for a loop that reads it; none of the
// loops this file serves does by default -- path_trace_kernel's PMODE 1 is the one measured to gain.
template <bool FULL>
PT_DEV bool scatter_and_continue(const Surface &hit, const Material &mat, Rng &rng, const int max_depth, f3 &ro, f3 &rd,
                                 f3 &throughput, int &bounce, bool &ray_spec, bool &prev_was_specular,
                                 const TangentFrame &F = no_frame()) {
    f3 scatter_dir = mk3(0.0f), att = mk3(0.0f);
    bool is_specular = false;
    if (!material_scatter<FULL>(hit, mat, rd, rng, scatter_dir, att, is_specular, false, F))
        return false;
    prev_was_specular = is_specular;
    if (bounce >= 2) { // Russian roulette (path_logic.cuh:871-880)
        const float p = max_(0.05f, min_(0.95f, max_(throughput.x, max_(throughput.y, throughput.z))));
        if (rng_uniform(rng) > p)
            return false;
        throughput = throughput / p;
    }
    throughput = throughput * att;
    throughput = clamp_vector_soft(throughput, 50.0f);
    const f3 off = hit.normal * 1e-4f;
    ro = (dot(scatter_dir, hit.normal) > 0.0f) ? (hit.point + off) : (hit.point - off);
    rd = scatter_dir;
    ray_spec = is_specular;
    ++bounce;
    return bounce < max_depth;
}

} // namespace pt
