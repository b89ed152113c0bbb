// pt_bounce.hip.h -- bounce_query_kernel: the analytic lights' one-bounce term at lightmap texels (ptrt_query_bounce), and
// bounce_terms_kernel, which writes the same terms out for hits the caller traced (ptrt_bounce_terms).
//
// The gather of ptrt_query_irradiance starts with ray_spec = true, so its rays take no light sample at their first hit, and
// ptrt_query_direct lights the texel itself: light that reaches the texel after exactly one reflection off the surface a gather
// ray hits first is in neither.  This is that term.  Ray (t, k) is irradiance_ray(t, k) (pt_irradiance.hip.h); its hit is the
// closest hit of the variant's traversal, made a Surface by make_surface -- the record ptrt_query_rays(PTRT_QUERY_CLOSEST)
// answers.  At the hit, term q = j * n_shadow + s of Q = light_count * n_shadow is the path tracer's own light sample
// (sample_light, pt_path.hip.h) of light light_first + j with one light in the pick and the two numbers of shadow2[s] (its second
// rotated by phases[t]) for the cone's draws, valued as a path vertex values it: evaluateBSDF<FULL>(hit, mat, L, -rd) * radiance
// * att / pdf, soft-clamped at 500, times the path's throughput -- (1, 1, 1), or the Beer-Lambert factor behind a back face.
// The reference's mis_weight is NOT applied: an analytic light has no geometry, no BSDF-sampled ray can reach it, and there is
// no second estimator to balance against (ptrt_query_direct applies none either).  The soft clamp is kept: it belongs to the
// BSDF product.  All of it is stated once, in bounce_sample, for both kernels.
//
// The frame is the queries' one and the bakes' texel frame (pt_query.hip.h: query_stage, walk_closest, walk_occluded,
// texel_shape, texel_ray, segment_fold_sum); the row store is the kernel's own.  A lane is gather ray (t, k):
// ONE closest-hit walk, then a wave-uniform loop over q in which every lane that hit forms its sample and ONE any-hit call runs with `walked` as its live mask, skipped by ballot when no lane walks; a lane adds its unblocked values in q
// order from +0.0f and counts its lit and blocked terms.  Behind the loop the six quantities -- B = sum / (float)n_shadow per
// channel, the two counts as floats, hit ? 1 : 0 -- are reduced over k exactly as the irradiance query reduces its six.  The
// lights are read from memory as in direct_query_kernel, the materials as in trace_chunk_samples.
#pragma once
#include "pt_direct.hip.h"

namespace pt {

struct BounceOut { // == ptrt_bounce (include/ptrt.h)
    float radiance[3];
    float lit_fraction, shadowed_fraction, hit_fraction;
    float reserved[2];
};

// The throughput a path carries to the light sample of its first vertex: the first half of absorb_and_emit (pt_path.hip.h) from
// (1, 1, 1), the emission discarded.  m0: float4 0 of the hit mesh's material record.
PT_DEV f3 bounce_throughput(const float4 m0, const Surface &hit) {
    f3 throughput = mk3(1.0f), unused = mk3(0.0f);
    absorb_and_emit(m0, make_float4(0.0f, 0.0f, 0.0f, 0.0f), hit, false, throughput, unused);
    return throughput;
}

// Term q at the hit of a gather ray of texel t: the one statement of it, for bounce_terms_kernel and bounce_query_kernel.
// `rd`: the gather ray's direction; `throughput`: bounce_throughput at the hit; `rotate`, `phase`: whether the texel has a
// phase, and phases[t].
struct BounceSample {
    f3 o, L, value;
    float tmax;
    bool walked;
};
template <bool FULL>
PT_DEV BounceSample bounce_sample(const float4 *__restrict__ lights, const float4 *__restrict__ materials, const Surface &hit,
                                  const int mesh, const f3 rd, const f3 throughput, const float *__restrict__ shadow2,
                                  const bool rotate, const float phase, const int n_shadow, const int light_first,
                                  const uint32_t q) {
    const uint32_t j = q / (uint32_t)n_shadow, s = q - j * (uint32_t)n_shadow;
    GivenDraws u{shadow2[2 * (size_t)s], shadow2[2 * (size_t)s + 1]};
    if (rotate) { // the texel's rotation about the cone's axis, as direct_sample's
        u.then = u.then + phase;
        if (u.then >= 1.0f)
            u.then = u.then - 1.0f;
    }
    const LightRec light = load_light(lights, light_first + (int)j);
    BounceSample r;
    f3 radiance;
    float pdf, att;
    sample_light(light, 1.0f, hit, u, r.L, pdf, radiance, att, r.o, r.tmax);
    const Material mat = load_material(materials, mesh);
    const f3 bsdf = evaluateBSDF<FULL>(hit, mat, r.L, -rd);
    const f3 direct = clamp_vector_soft(bsdf * radiance * att / pdf, 500.0f);
    r.value = throughput * direct;
    r.walked = pdf > 0.0f && (direct.x > 0.0f || direct.y > 0.0f || direct.z > 0.0f); // (false for a NaN)
    return r;
}

// Waves per SIMD the kernel is built for: RADIANCE_WAVES (168 VGPRs), at which eleven of the twelve variants keep the hit, the
// ray, the throughput, the sums and the sample across the shadow walk in registers.  The one-ray-per-lane walk of a real TLAS
// with the full material model (GEOM 2, PMODE 0: option pair_trace = 0, not a default path) spilled two registers, 16 bytes per
// lane of scratch, at that budget; it is built for two waves and takes the registers it needs.
constexpr int bounce_waves(int geom, bool full, int pmode) { return geom == 2 && pmode == 0 && full ? 2 : RADIANCE_WAVES; }
template <int GEOM, bool FULL, int PMODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(bounce_waves(GEOM, FULL, PMODE), 8))) void bounce_query_kernel(
    const KParams Kin, const float *__restrict__ positions, const float *__restrict__ normals, int n_texels,
    const float *__restrict__ samples2, int n_dirs, const float *__restrict__ phases, float offset,
    const float *__restrict__ shadow2, int n_shadow, int light_first, int n_terms, BounceOut *__restrict__ out) {
    (void)Kin; // (read through the kernarg segment, phase by phase: radiance_query_kernel)
    const kparams_ptr kp0 = (kparams_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const KParams &K = kparams(kp0); // staging
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    const TexelShape S = texel_shape(n_texels, n_dirs);
    const int log2w = S.log2w;
    const float f_dirs = (float)n_dirs, f_shadow = (float)n_shadow, f_all = (float)(n_dirs * n_terms); // (n_dirs * Q fits an int: the host)
    for (uint32_t g = blockIdx.x; g < S.groups; g += gridDim.x) { // (wave-uniform)
        float total = 0.0f; // beyond 64 directions, lane i: the running total of quantity i
        for (int c = 0; c < S.chunks; ++c) { // (wave-uniform)
            f3 ro = mk3(0.0f), rd = mk3(0.0f);
            float phase = 0.0f;
            bool live;
            {
                const TexelRay r = texel_ray(lane, log2w, g, c);
                live = r.t < (uint32_t)n_texels && r.k < (uint32_t)n_dirs;
                if (live) {
                    irradiance_ray(positions, normals, samples2, phases, offset, r.t, r.k, ro, rd);
                    if (phases)
                        phase = phases[r.t];
                }
            }
            // ---- the gather ray's closest hit, all live lanes together
            const KParams &KB = kparams(kp0);
            const Hit h = walk_closest<GEOM, PMODE>(KB, PL, stk, cyc, lane, live, ro, rd);
            const KParams &KC = kparams(kp0);
            const bool struck = live && h.mesh >= 0;
            Surface hit;
            hit.point = hit.normal = mk3(0.0f);
            hit.t = 0.0f;
            hit.front_face = true;
            f3 throughput = mk3(1.0f);
            if (struck) {
                hit = make_surface(KC, h, ro, rd, nullptr, nullptr);
                throughput = bounce_throughput(KC.materials[h.mesh * 6 + 0], hit);
            }
            // ---- the terms, q by q: a lane's sample, then one any-hit walk of the lanes whose sample can add something
            f3 sum = mk3(0.0f);
            int n_lit = 0, n_dark = 0;
            for (int q = 0; q < n_terms; ++q) { // (wave-uniform)
                const KParams &KQ = kparams(kp0);
                f3 o = mk3(0.0f), L = mk3(0.0f), value = mk3(0.0f);
                float tm = 0.0f;
                bool walked = false;
                if (struck) {
                    const BounceSample s = bounce_sample<FULL>(KQ.lights, KQ.materials, hit, h.mesh, rd, throughput, shadow2,
                                                               phases != nullptr, phase, n_shadow, light_first, (uint32_t)q);
                    if (s.walked) { // (a lane that is not walked hands the traversal a zero ray, as a dead lane of ray_query_kernel)
                        walked = true;
                        o = s.o;
                        L = s.L;
                        tm = s.tmax;
                        value = s.value;
                    }
                }
                if (__builtin_amdgcn_ballot_w64(walked)) { // (wave-uniform)
                    const KParams &KD = kparams(kp0);
                    const bool blocked = walk_occluded<GEOM, PMODE>(KD, PL, stk, cyc, lane, walked, o, L, tm);
                    if (walked && !blocked) {
                        sum = sum + value;
                        ++n_lit;
                    }
                    if (walked && blocked)
                        ++n_dark;
                }
            }
            // ---- the six quantities of the ray, a dead lane's selected to +0.0f, each folded within the segment (the ray's
            // numbers once more, from the lane number behind an empty asm: irradiance_query_kernel)
            const TexelRay r = texel_ray(lane, log2w, g, c);
            const int w = 1 << log2w;
            const float s_r = segment_fold_sum(struck ? sum.x / f_shadow : 0.0f, w);
            const float s_g = segment_fold_sum(struck ? sum.y / f_shadow : 0.0f, w);
            const float s_b = segment_fold_sum(struck ? sum.z / f_shadow : 0.0f, w);
            const float s_lit = segment_fold_sum((float)n_lit, w);
            const float s_dark = segment_fold_sum((float)n_dark, w);
            const float s_hit = segment_fold_sum(struck ? 1.0f : 0.0f, w);
            if (!S.chunked) {
                // one chunk: its sum added to a total that starts at +0.0f, divided, stored by the segment's first lane
                if (r.k == 0 && r.t < (uint32_t)n_texels) {
                    float *row = reinterpret_cast<float *>(out + r.t);
                    row[0] = (0.0f + s_r) / f_dirs;
                    row[1] = (0.0f + s_g) / f_dirs;
                    row[2] = (0.0f + s_b) / f_dirs;
                    row[3] = (0.0f + s_lit) / f_all;
                    row[4] = (0.0f + s_dark) / f_all;
                    row[5] = (0.0f + s_hit) / f_dirs;
                    row[6] = 0.0f;
                    row[7] = 0.0f;
                }
            } else { // (w is 64: the lane is the direction's number in its chunk)
                float mine = 0.0f;
                mine = lane == 0 ? s_r : mine;
                mine = lane == 1 ? s_g : mine;
                mine = lane == 2 ? s_b : mine;
                mine = lane == 3 ? s_lit : mine;
                mine = lane == 4 ? s_dark : mine;
                mine = lane == 5 ? s_hit : mine;
                total = total + mine; // chunk sums in chunk order, from +0.0f
            }
        }
        if (S.chunked && lane < 8) // the texel's 32-byte row (the group is the texel); reserved is 0.0f
            reinterpret_cast<float *>(out + g)[lane] = (lane == 3 || lane == 4) ? total / f_all : lane < 6 ? total / f_dirs : 0.0f;
    }
    cyc.flush(lane);
}

// The terms of a bake's one-bounce light, written out for hits the caller traced: row (t * n_dirs + k) * Q + q is (origin, L,
// tmax, value) of bounce_sample at hits[t * n_dirs + k] for the ray along dirs[t * n_dirs + k], as computed, walked or not; a
// miss, or a record whose mesh has no uploaded material, gives a row of zeros.  One thread per term.
template <bool FULL>
__global__ __launch_bounds__(256) void bounce_terms_kernel(const float4 *__restrict__ lights, const float4 *__restrict__ materials,
                                                           int n_materials, const HitOut *__restrict__ hits, const float *__restrict__ dirs, size_t n_rows,
                                                           int n_dirs, const float *__restrict__ shadow2, int n_shadow,
                                                           const float *__restrict__ phases, int light_first, int n_terms,
                                                           float *__restrict__ origins, float *__restrict__ Ls, float *__restrict__ tmax,
                                                           float *__restrict__ values) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows)
        return;
    const size_t ray = i / (size_t)n_terms;
    const HitOut rec = hits[ray];
    BounceSample s;
    s.o = s.L = s.value = mk3(0.0f);
    s.tmax = 0.0f;
    if (rec.hit && rec.mesh_index >= 0 && rec.mesh_index < n_materials) {
        Surface hit;
        hit.point = mk3(rec.point[0], rec.point[1], rec.point[2]);
        hit.normal = mk3(rec.normal[0], rec.normal[1], rec.normal[2]);
        hit.t = rec.t;
        hit.front_face = rec.front_face != 0;
        const f3 rd = mk3(dirs[ray * 3], dirs[ray * 3 + 1], dirs[ray * 3 + 2]);
        const f3 throughput = bounce_throughput(materials[rec.mesh_index * 6 + 0], hit);
        s = bounce_sample<FULL>(lights, materials, hit, rec.mesh_index, rd, throughput, shadow2, phases != nullptr,
                                phases ? phases[ray / (size_t)n_dirs] : 0.0f, n_shadow, light_first, (uint32_t)(i - ray * (size_t)n_terms));
    }
    origins[i * 3 + 0] = s.o.x;
    origins[i * 3 + 1] = s.o.y;
    origins[i * 3 + 2] = s.o.z;
    Ls[i * 3 + 0] = s.L.x;
    Ls[i * 3 + 1] = s.L.y;
    Ls[i * 3 + 2] = s.L.z;
    tmax[i] = s.tmax;
    values[i * 3 + 0] = s.value.x;
    values[i * 3 + 1] = s.value.y;
    values[i * 3 + 2] = s.value.z;
}

} // namespace pt
