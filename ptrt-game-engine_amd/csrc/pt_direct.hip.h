// pt_direct.hip.h -- direct_query_kernel: the analytic lights' direct term at lightmap texels (ptrt_query_direct), and
// direct_rays_kernel, which writes the same shadow rays and weights out (ptrt_direct_rays).
//
// Texel t has a position P and a normal N (used as given).  Term q = j * n_shadow + s of its Q = light_count * n_shadow terms is
// shadow sample s of light light_first + j: the path tracer's own light sample at a surface point (P, N) -- sample_light,
// pt_path.hip.h, with one light in the pick and the two numbers of samples2[s] (its second rotated by phases[t]) in place of the
// cone sample's two draws --, weighted by radiance * attenuation * dot(N, L) / pdf, stated once in direct_sample for both
// kernels.  A sample with a positive weight sends its shadow ray from P + offset * N along L to light_dist - 1e-3f through the
// any-hit traversal of ptrt_query_rays(PTRT_QUERY_OCCLUDED); an unblocked one adds its weight.  The texel keeps five sums over
// q: the three channels divided by (float)n_shadow -- the sum over the lights of each light's mean --, and the counts of
// unblocked and of blocked samples divided by (float)Q: one 32-byte DirectOut per texel.
//
// The frame is the queries' one (pt_query.hip.h: query_stage, walk_occluded): a persistent grid of one-wave workgroups, the LDS
// carve and staging by PMODE, six variants.  That frame stages no lights (the megakernel's PMODE 1 workgroup does, in a layout
// of its own), so the records are read from memory: at most light_count * 64 bytes that every lane of the grid shares.  The
// work shape is the bakes' texel frame (pt_query.hip.h: texel_shape, texel_ray, segment_fold_sum) with Q terms per texel.  Per
// chunk every lane forms its sample, ONE any-hit call runs with `walked` as its live mask -- a lane whose sample adds nothing
// either way never enters the traversal --, and the five terms are reduced within each segment.  Dead lanes -- q >= Q, or a
// texel past the end -- take part in the collectives and contribute +0.0f.  Up to 64 terms a segment's first lane adds the sum
// to +0.0f, divides and stores the record; beyond, lane i adds the chunk's sum of quantity i to its running total and lanes 0-7
// divide and store at the end.  The sum order is part of the contract (include/ptrt.h, tests/direct_restatement.py).
#pragma once
#include "pt_irradiance.hip.h"

namespace pt {

struct DirectOut { // == ptrt_direct (include/ptrt.h)
    float irradiance[3];
    float lit_fraction, shadowed_fraction;
    float reserved[3];
};

// Term (t, q) of a bake's direct light: the one statement of it, for direct_rays_kernel and direct_query_kernel.  The light
// arithmetic is sample_light's, its `hit` the texel and its draws u1, u2; the shadow origin is the texel's own.
struct DirectSample {
    f3 o, L, weight;
    float tmax;
    bool walked;
};
PT_DEV DirectSample direct_sample(const float4 *__restrict__ lights, const float *__restrict__ positions,
                                  const float *__restrict__ normals, const float *__restrict__ samples2,
                                  const float *__restrict__ phases, float offset, int n_shadow, int light_first, size_t t, uint32_t q) {
    const uint32_t j = q / (uint32_t)n_shadow, s = q - j * (uint32_t)n_shadow;
    GivenDraws u{samples2[2 * (size_t)s], samples2[2 * (size_t)s + 1]};
    if (phases) { // the texel's rotation about the cone's axis
        u.then = u.then + phases[t];
        if (u.then >= 1.0f)
            u.then = u.then - 1.0f;
    }
    Surface hit{};
    hit.point = mk3(positions[t * 3], positions[t * 3 + 1], positions[t * 3 + 2]);
    hit.normal = mk3(normals[t * 3], normals[t * 3 + 1], normals[t * 3 + 2]);
    const LightRec light = load_light(lights, light_first + (int)j);
    DirectSample r;
    f3 radiance, path_o;
    float pdf, att;
    sample_light(light, 1.0f, hit, u, r.L, pdf, radiance, att, path_o, r.tmax);
    const float c = dot(hit.normal, r.L);
    r.weight = mk3(0.0f);
    if (c > 0.0f && pdf > 0.0f)
        r.weight = mk3(radiance.x * att * c / pdf, radiance.y * att * c / pdf, radiance.z * att * c / pdf);
    r.walked = r.weight.x > 0.0f || r.weight.y > 0.0f || r.weight.z > 0.0f; // (false for a NaN weight)
    r.o = mk3(hit.point.x + offset * hit.normal.x, hit.point.y + offset * hit.normal.y, hit.point.z + offset * hit.normal.z);
    return r;
}

template <int GEOM, int PMODE>
__global__ __launch_bounds__(64) void direct_query_kernel(const KParams K, const float *__restrict__ positions,
                                                          const float *__restrict__ normals, int n_texels,
                                                          const float *__restrict__ samples2, int n_shadow,
                                                          const float *__restrict__ phases, float offset, int light_first,
                                                          int n_terms, DirectOut *__restrict__ out) {
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    const TexelShape S = texel_shape(n_texels, n_terms);
    const int log2w = S.log2w, w = 1 << log2w;
    const float f_shadow = (float)n_shadow, f_terms = (float)n_terms;
    for (uint32_t g = blockIdx.x; g < S.groups; g += gridDim.x) { // (wave-uniform)
        float total = 0.0f; // beyond 64 terms, lane i: the running total of quantity i
        for (int c = 0; c < S.chunks; ++c) { // (wave-uniform)
            const TexelRay r = texel_ray(lane, log2w, g, c); // (r.k: the term q)
            const bool live = r.t < (uint32_t)n_texels && r.k < (uint32_t)n_terms;
            f3 o = mk3(0.0f), d = mk3(0.0f), weight = mk3(0.0f);
            float tm = 0.0f;
            bool walked = false;
            if (live) {
                const DirectSample s = direct_sample(K.lights, positions, normals, samples2, phases, offset, n_shadow, light_first, r.t, r.k);
                if (s.walked) { // (a lane that is not walked hands the traversal a zero ray, as a dead lane of ray_query_kernel)
                    walked = true;
                    o = s.o;
                    d = s.L;
                    tm = s.tmax;
                    weight = s.weight;
                }
            }
            bool blocked = false;
            if (__builtin_amdgcn_ballot_w64(walked)) // (wave-uniform; a wave none of whose samples can add anything walks nothing, as phase [D] of the path loop)
                blocked = walk_occluded<GEOM, PMODE>(K, PL, stk, cyc, lane, walked, o, d, tm);
            // the five terms, selected to +0.0f where the sample adds nothing, each folded within the segment
            const bool lit = walked && !blocked, dark = walked && blocked;
            const float s_r = segment_fold_sum(lit ? weight.x : 0.0f, w);
            const float s_g = segment_fold_sum(lit ? weight.y : 0.0f, w);
            const float s_b = segment_fold_sum(lit ? weight.z : 0.0f, w);
            const float s_lit = segment_fold_sum(lit ? 1.0f : 0.0f, w);
            const float s_dark = segment_fold_sum(dark ? 1.0f : 0.0f, w);
            if (!S.chunked) {
                // one chunk: its sum added to a total that starts at +0.0f, divided, stored by the segment's first lane
                if (r.k == 0 && r.t < (uint32_t)n_texels) {
                    float *row = reinterpret_cast<float *>(out + r.t);
                    row[0] = (0.0f + s_r) / f_shadow;
                    row[1] = (0.0f + s_g) / f_shadow;
                    row[2] = (0.0f + s_b) / f_shadow;
                    row[3] = (0.0f + s_lit) / f_terms;
                    row[4] = (0.0f + s_dark) / f_terms;
                    row[5] = 0.0f;
                    row[6] = 0.0f;
                    row[7] = 0.0f;
                }
            } else { // (w is 64: the lane is the term's number in its chunk)
                float mine = 0.0f;
                mine = lane == 0 ? s_r : mine;
                mine = lane == 1 ? s_g : mine;
                mine = lane == 2 ? s_b : mine;
                mine = lane == 3 ? s_lit : mine;
                mine = lane == 4 ? s_dark : mine;
                total = total + mine; // chunk sums in chunk order, from +0.0f
            }
        }
        if (S.chunked && lane < 8) // the texel's 32-byte row (the group is the texel); reserved is 0.0f
            reinterpret_cast<float *>(out + g)[lane] = lane < 3 ? total / f_shadow : lane < 5 ? total / f_terms : 0.0f;
    }
    cyc.flush(lane);
}

// The terms of a bake, written out: ray t * Q + q is (origin, L, tmax, weight) of direct_sample(t, q) as computed, walked or
// not; one thread per ray.
__global__ __launch_bounds__(256) void direct_rays_kernel(const float4 *__restrict__ lights, const float *__restrict__ positions,
                                                          const float *__restrict__ normals, size_t n_rays,
                                                          const float *__restrict__ samples2, int n_shadow,
                                                          const float *__restrict__ phases, float offset, int light_first, int n_terms,
                                                          float *__restrict__ origins, float *__restrict__ dirs,
                                                          float *__restrict__ tmax, float *__restrict__ weights) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays)
        return;
    const size_t t = i / (size_t)n_terms;
    const DirectSample s = direct_sample(lights, positions, normals, samples2, phases, offset, n_shadow, light_first, t,
                                         (uint32_t)(i - t * (size_t)n_terms));
    origins[i * 3 + 0] = s.o.x;
    origins[i * 3 + 1] = s.o.y;
    origins[i * 3 + 2] = s.o.z;
    dirs[i * 3 + 0] = s.L.x;
    dirs[i * 3 + 1] = s.L.y;
    dirs[i * 3 + 2] = s.L.z;
    tmax[i] = s.tmax;
    weights[i * 3 + 0] = s.weight.x;
    weights[i * 3 + 1] = s.weight.y;
    weights[i * 3 + 2] = s.weight.z;
}

} // namespace pt
