// pt_probe.hip.h -- probe_query_kernel: light probes filled by the path tracer (ptrt_query_probes).
//
// Probe p sends n_dirs rays from positions[p], ray (p, k) along directions[k] (one set for all probes, used as given) with
// generator state p * n_dirs + k.  Each ray's radiance, first-hit depth and object id are what ptrt_query_radiance puts into
// ptrt_radiance for that ray and state -- the path loop is that kernel's own (trace_chunk_samples, pt_radiance.hip.h) -- and the
// probe keeps their projection onto the nine real spherical harmonics of bands 0-2, the mean of min(depth, max_distance), of
// its square, and the fraction of rays that hit: one 128-byte ProbeOut per probe instead of 32 bytes per ray.
//
// The frame is radiance_query_kernel's: a persistent grid of one-wave workgroups, the LDS carve and staging by PMODE, three
// waves per SIMD, the parameters through the kernarg pointer.  The grid strides over PROBES: a wave owns a probe and walks its
// ceil(n_dirs / 64) chunks of 64 consecutive k in order.  After a chunk's paths have ended each lane holds its ray's mean
// radiance; the 30 terms are formed one at a time, each reduced over the wave by segment_fold_sum at w = 64 (pt_query.hip.h),
// the butterfly v[j] + v[j ^ 32], ^ 16, .. ^ 1 -- float addition is commutative, so every lane ends with the bits of the
// fold v[j] + v[j + 32], then 16, 8, 4, 2, 1 -- and lane q adds the chunk's sum of quantity q to its running total,
// the one register the projection keeps across the path loop.
// Dead lanes of the tail chunk take part in the collectives and contribute +0.0f.  At the end lanes 0-31 divide by
// (float)n_dirs and store the probe's row.  The sum order is part of the contract (include/ptrt.h, tests/probe_restatement.py).
#pragma once
#include "pt_radiance.hip.h"

namespace pt {

struct ProbeOut { // == ptrt_probe (include/ptrt.h)
    float sh[9][3];
    float mean_distance, mean_distance_sq, hit_fraction;
    float reserved[2];
};

// The first hit of sample 0 for a probe's ray: its depth and what it hit, in two registers.
struct FirstHitToRegs {
    float *depth;
    int *object_id;
    PT_DEV void operator()(float d, f3, int id) const {
        *depth = d;
        *object_id = id;
    }
};

// Y_i of the direction as given (not normalised), in the operation order include/ptrt.h states
PT_DEV float sh9_basis(int i, f3 d) {
    switch (i) {
    case 0: return 0.282095f;
    case 1: return 0.488603f * d.y;
    case 2: return 0.488603f * d.z;
    case 3: return 0.488603f * d.x;
    case 4: return 1.092548f * (d.x * d.y);
    case 5: return 1.092548f * (d.y * d.z);
    case 6: return 0.315392f * (3.0f * (d.z * d.z) - 1.0f);
    case 7: return 1.092548f * (d.x * d.z);
    default: return 0.546274f * (d.x * d.x - d.y * d.y);
    }
}

template <int GEOM, bool FULL, int PMODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RADIANCE_WAVES, 8))) void probe_query_kernel(
    const KParams Kin, const float *__restrict__ positions, int n_probes, const float *__restrict__ dirs, int n_dirs,
    uint32_t *__restrict__ rng_states, float max_distance, ProbeOut *__restrict__ out) {
    (void)Kin; // (read through the kernarg segment, phase by phase: radiance_query_kernel)
    const kparams_ptr kp0 = (kparams_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const KParams &K = kparams(kp0); // staging
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    for (int p = blockIdx.x; p < n_probes; p += gridDim.x) { // (wave-uniform)
        const f3 o0 = mk3(positions[(size_t)p * 3], positions[(size_t)p * 3 + 1], positions[(size_t)p * 3 + 2]);
        float total = 0.0f; // lane q: the running total of quantity q
        const int chunks = (int)(((size_t)n_dirs + 63) / 64);
        for (int c = 0; c < chunks; ++c) { // (wave-uniform)
            const size_t k = (size_t)c * 64 + (size_t)lane;
            const bool live = k < (size_t)n_dirs;
            const size_t i = (size_t)p * (size_t)n_dirs + k; // the ray's generator state
            f3 d0 = mk3(0.0f);
            Rng rng = {0, 0, 0, 0, 0, 0};
            if (live) {
                d0 = mk3(dirs[k * 3], dirs[k * 3 + 1], dirs[k * 3 + 2]);
                load_rng_state(rng, rng_states + i * 6);
            }
            float depth = 1e30f;
            int object_id = -1;
            const FirstHitToRegs first{&depth, &object_id};
            const f3 sum = trace_chunk_samples<GEOM, FULL, PMODE>(kp0, PL, stk, cyc, lane, live, o0, d0, rng, first);
            f3 mean = mk3(0.0f);
            if (live) {
                store_rng_state(rng_states + i * 6, rng);
                mean = sum / (float)kparams(kp0).spp; // ptrt_radiance.radiance of this ray
            }
            // the chunk's 30 terms, one quantity at a time; lane q picks up the chunk's sum of quantity q
            const float dist = min_(depth, max_distance);
            float mine = 0.0f;
            // (the lane number behind an empty asm: compares of `lane` itself are loop invariants, and the compiler hoists all 30
            // masks out of the path loop and holds them in 60 SGPRs across it)
            int me = lane;
            asm volatile("" : "+v"(me));
#pragma unroll
            for (int b = 0; b < 9; ++b) {
                const float y = sh9_basis(b, d0);
                const float sx = segment_fold_sum(live ? y * mean.x : 0.0f, 64);
                mine = me == 3 * b ? sx : mine;
                const float sy = segment_fold_sum(live ? y * mean.y : 0.0f, 64);
                mine = me == 3 * b + 1 ? sy : mine;
                const float sz = segment_fold_sum(live ? y * mean.z : 0.0f, 64);
                mine = me == 3 * b + 2 ? sz : mine;
            }
            const float s_dist = segment_fold_sum(live ? dist : 0.0f, 64);
            mine = me == 27 ? s_dist : mine;
            const float s_dist2 = segment_fold_sum(live ? dist * dist : 0.0f, 64);
            mine = me == 28 ? s_dist2 : mine;
            const float s_hit = segment_fold_sum(live && object_id >= 0 ? 1.0f : 0.0f, 64);
            mine = me == 29 ? s_hit : mine;
            total = total + mine; // chunk sums in chunk order, from +0.0f
        }
        // the probe's 128-byte row; reserved is 0.0f.  (The opaque lane number again: the row's per-lane address without the probe is
        // an invariant of the probe loop, and held across it, it was the one value the simple-materials PMODE 3 variant spilled.)
        // (and the direction count: converted before the loop, (float)n_dirs was the full-materials PMODE 3 variant's one spill)
        int me = lane, nd = n_dirs;
        asm volatile("" : "+v"(me), "+s"(nd));
        if (me < 32)
            reinterpret_cast<float *>(out + p)[me] = me < 30 ? total / (float)nd : 0.0f;
    }
    cyc.flush(lane);
}

} // namespace pt
