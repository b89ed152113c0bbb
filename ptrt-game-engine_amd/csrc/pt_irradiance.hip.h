// pt_irradiance.hip.h -- irradiance_query_kernel: lightmap texels filled by the path tracer (ptrt_query_irradiance), and
// irradiance_rays_kernel, which writes the same rays out (ptrt_irradiance_rays).
//
// Texel t gathers n_dirs rays from positions[t] + offset * normals[t], ray (t, k) along the cosine-distributed direction that
// the k-th point of samples2 (ONE set in [0,1)^2 for all texels, its second coordinate rotated by phases[t]) maps to about
// normals[t] -- sample_cosine_hemisphere's arithmetic and to_world (pt_device.hip.h), stated once in irradiance_ray for both
// kernels -- with generator state t * n_dirs + k.  Each ray's radiance, first-hit depth and object id are what
// ptrt_query_radiance puts into ptrt_radiance for that ray and state -- the path loop is that kernel's own
// (trace_chunk_samples, pt_radiance.hip.h) -- and the texel keeps six means over k: radiance, min(depth, max_distance), its
// square, and the fraction of rays that hit: one 32-byte IrradianceOut per texel.
//
// The frame is probe_query_kernel's: a persistent grid of one-wave workgroups, the LDS carve and staging by PMODE, three waves
// per SIMD, the parameters through the kernarg pointer.  The work shape is the bakes' texel frame (pt_query.hip.h: texel_shape,
// texel_ray, segment_fold_sum: groups of 64 / w texels, or one texel in chunks beyond 64 directions); the row store is the
// kernel's own.  Both shapes are one loop around one call of the path loop, told apart by wave-uniform values.  After a chunk's
// paths have ended the six terms are reduced within each segment of w lanes by segment_fold_sum (for w = 64 the probes' order).
// Dead lanes -- k >= n_dirs, or a texel past the end -- take part in the collectives and contribute +0.0f.  Up to 64 directions
// a segment's first lane adds the sum to +0.0f, divides by (float)n_dirs and stores the record; nothing but the lane's own ray
// lives across the path loop -- its texel and direction numbers are formed again behind it (texel_ray).  Beyond, lane q adds
// the chunk's sum of quantity q to its running total, the one register kept across the path loop, and lanes 0-7 divide and
// store at the end.  The sum order is part of the contract (include/ptrt.h, tests/irradiance_restatement.py).
#pragma once
#include "pt_probe.hip.h"

namespace pt {

struct IrradianceOut { // == ptrt_irradiance (include/ptrt.h)
    float radiance[3];
    float mean_distance, mean_distance_sq, hit_fraction;
    float reserved[2];
};

// Ray (t, k) of a bake: the one statement of it, for irradiance_rays_kernel and irradiance_query_kernel.  u1, u2 take the place
// of sample_cosine_hemisphere's two draws; the normal is used as given.
PT_DEV void irradiance_ray(const float *__restrict__ positions, const float *__restrict__ normals, const float *__restrict__ samples2,
                           const float *__restrict__ phases, float offset, size_t t, size_t k, f3 &o, f3 &d) {
    const float u1 = samples2[2 * k];
    float u2 = samples2[2 * k + 1];
    if (phases) { // the texel's rotation about its normal
        u2 = u2 + phases[t];
        if (u2 >= 1.0f)
            u2 = u2 - 1.0f;
    }
    const float r = sqrt_ieee(u1);
    const float phi = TWO_PI_F * u2;
    float sp, cp;
    det_sincos(phi, sp, cp);
    const f3 local = mk3(r * cp, r * sp, sqrt_ieee(max_(0.0f, 1.0f - u1)));
    const f3 N = mk3(normals[t * 3], normals[t * 3 + 1], normals[t * 3 + 2]);
    const f3 P = mk3(positions[t * 3], positions[t * 3 + 1], positions[t * 3 + 2]);
    d = to_world(local, N);
    o = mk3(P.x + offset * N.x, P.y + offset * N.y, P.z + offset * N.z);
}

template <int GEOM, bool FULL, int PMODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RADIANCE_WAVES, 8))) void irradiance_query_kernel(
    const KParams Kin, const float *__restrict__ positions, const float *__restrict__ normals, int n_texels,
    const float *__restrict__ samples2, int n_dirs, const float *__restrict__ phases, float offset,
    uint32_t *__restrict__ rng_states, float max_distance, IrradianceOut *__restrict__ out) {
    (void)Kin; // (read through the kernarg segment, phase by phase: radiance_query_kernel)
    const kparams_ptr kp0 = (kparams_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const KParams &K = kparams(kp0); // staging
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    // (query_stage's text, pt_query.hip.h, and not a call of it: behind the call this kernel's allocation moved and the Cornell
    // bake was 0.6 to 1.0 % slower in every run; with the text here all twelve variants are the ISA they were -- DESIGN 3.33)
    LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    PairLds PL = stage_pair_lds<PMODE>(K, lds_raw, lane);
    PL.cyc = &cyc;
    PL.stat_bounce = 0;
    __syncthreads();
    const TexelShape S = texel_shape(n_texels, n_dirs); // (the state index does not fit 32 bits; texel and group numbers do)
    const int log2w = S.log2w;
    for (uint32_t g = blockIdx.x; g < S.groups; g += gridDim.x) { // (wave-uniform)
        float total = 0.0f; // beyond 64 directions, lane q: the running total of quantity q
        for (int c = 0; c < S.chunks; ++c) { // (wave-uniform)
            f3 o0 = mk3(0.0f), d0 = mk3(0.0f);
            Rng rng = {0, 0, 0, 0, 0, 0};
            bool live;
            {
                const TexelRay r = texel_ray(lane, log2w, g, c);
                live = r.t < (uint32_t)n_texels && r.k < (uint32_t)n_dirs;
                if (live) {
                    irradiance_ray(positions, normals, samples2, phases, offset, r.t, r.k, o0, d0);
                    load_rng_state(rng, rng_states + ((size_t)r.t * (size_t)n_dirs + r.k) * 6);
                }
            }
            float depth = 1e30f;
            int object_id = -1;
            const FirstHitToRegs first{&depth, &object_id};
            const f3 sum = trace_chunk_samples<GEOM, FULL, PMODE>(kp0, PL, stk, cyc, lane, live, o0, d0, rng, first);
            // (the ray's numbers once more, from the lane number behind an empty asm: held across the path loop they cost
            // registers the loop needs; so do compares of `lane` itself and (float)n_dirs, invariants the compiler hoists)
            const TexelRay r = texel_ray(lane, log2w, g, c);
            int nd = n_dirs;
            asm volatile("" : "+s"(nd));
            f3 mean = mk3(0.0f);
            if (live) {
                store_rng_state(rng_states + ((size_t)r.t * (size_t)nd + r.k) * 6, rng);
                mean = sum / (float)kparams(kp0).spp; // ptrt_radiance.radiance of this ray
            }
            // the six terms, a dead lane's selected to +0.0f, each folded within the segment
            const int w = 1 << log2w;
            const float dist = min_(depth, max_distance);
            const float s_r = segment_fold_sum(live ? mean.x : 0.0f, w);
            const float s_g = segment_fold_sum(live ? mean.y : 0.0f, w);
            const float s_b = segment_fold_sum(live ? mean.z : 0.0f, w);
            const float s_dist = segment_fold_sum(live ? dist : 0.0f, w);
            const float s_dist2 = segment_fold_sum(live ? dist * dist : 0.0f, w);
            const float s_hit = segment_fold_sum(live && object_id >= 0 ? 1.0f : 0.0f, w);
            if (!S.chunked) {
                // one chunk: its sum added to a total that starts at +0.0f, divided, stored by the segment's first lane
                if (r.k == 0 && r.t < (uint32_t)n_texels) {
                    const float fn = (float)nd;
                    float *row = reinterpret_cast<float *>(out + r.t);
                    row[0] = (0.0f + s_r) / fn;
                    row[1] = (0.0f + s_g) / fn;
                    row[2] = (0.0f + s_b) / fn;
                    row[3] = (0.0f + s_dist) / fn;
                    row[4] = (0.0f + s_dist2) / fn;
                    row[5] = (0.0f + s_hit) / fn;
                    row[6] = 0.0f;
                    row[7] = 0.0f;
                }
            } else { // (w is 64: r.k - c * 64 is the lane)
                const uint32_t me = r.k - (uint32_t)c * 64u;
                float mine = 0.0f;
                mine = me == 0 ? s_r : mine;
                mine = me == 1 ? s_g : mine;
                mine = me == 2 ? s_b : mine;
                mine = me == 3 ? s_dist : mine;
                mine = me == 4 ? s_dist2 : mine;
                mine = me == 5 ? s_hit : mine;
                total = total + mine; // chunk sums in chunk order, from +0.0f
            }
        }
        if (S.chunked) { // the texel's 32-byte row (the group is the texel); reserved is 0.0f
            int me = lane, nd = n_dirs;
            asm volatile("" : "+v"(me), "+s"(nd));
            if (me < 8)
                reinterpret_cast<float *>(out + g)[me] = me < 6 ? total / (float)nd : 0.0f;
        }
    }
    cyc.flush(lane);
}

// The rays of a bake, written out: ray t * n_dirs + k is (origin, direction) of irradiance_ray(t, k), one thread per ray.
__global__ __launch_bounds__(256) void irradiance_rays_kernel(const float *__restrict__ positions, const float *__restrict__ normals,
                                                              size_t n_rays, const float *__restrict__ samples2, int n_dirs,
                                                              const float *__restrict__ phases, float offset,
                                                              float *__restrict__ origins, float *__restrict__ dirs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays)
        return;
    f3 o, d;
    irradiance_ray(positions, normals, samples2, phases, offset, i / (size_t)n_dirs, i % (size_t)n_dirs, o, d);
    origins[i * 3 + 0] = o.x;
    origins[i * 3 + 1] = o.y;
    origins[i * 3 + 2] = o.z;
    dirs[i * 3 + 0] = d.x;
    dirs[i * 3 + 1] = d.y;
    dirs[i * 3 + 2] = d.z;
}

} // namespace pt
