// pt_radiance.hip.h -- radiance_query_kernel: the path tracer asked about rays the caller chooses (ptrt_query_radiance), and
// the two small kernels that let a caller start where a frame starts: camera_rays_kernel (ptrt_camera_rays) and
// rng_states_kernel (ptrt_init_rng_states).
//
// Ray i with generator state i: for s < samples, tracePath(ray, state, max_depth) (path_logic.cuh:782-899), each sample soft-
// clamped and added in order to a sum that starts at zero, the sum divided by (float)samples -- what path_trace_kernel
// (scene_kernels.cuh:122-194) leaves in ACCUM for a pixel -- and the first hit of sample 0 as NORMAL / DEPTH / OBJECT_ID hold it
// (scene_kernels.cuh:179-193).  Past the primary ray tracePath reads nothing of the pixel -- no blue noise, no frame count -- so a
// query fed a pinhole frame's own primary rays and generator states reproduces that frame bit for bit, states included
// (tests/test_radiance_query_gpu.py).
//
// The frame is the queries' one (pt_query.hip.h: query_stage, walk_closest, walk_occluded): a persistent grid of one-wave
// workgroups, a grid-stride loop over chunks of 64 rays, dead lanes of the tail chunk taking part in the wave's collectives,
// size_t indices, the LDS carve and staging and the traversal by PMODE.  Per chunk the 64 lanes run the path loop in lock
// step -- closest hit, the vertex of tracePath through the functions of pt_path.hip.h in the phases [C], [C2], [D], [E] of
// path_trace_kernel, the light sample's shadow ray between its value and its addition, the scatter -- until no lane has a path
// left, then the next sample.  No lane refill, no staged shading inputs, no counters: a lane whose path has ended idles until
// the chunk's longest path is done.
#pragma once
#include "pt_path.hip.h"
#include "pt_query.hip.h"

namespace pt {

struct RadianceOut { // == ptrt_radiance (include/ptrt.h)
    float radiance[3];
    float depth;
    float normal[3];
    int object_id;
};

// Where the first hit of sample 0 goes, as DEPTH / NORMAL / OBJECT_ID hold it (a miss: 1e30f, zeros, -1): the query writes it
// straight into the ray's record, while the path is still running, so nothing of it stays in registers across the loop.
struct FirstHitToRecord {
    RadianceOut *out;
    size_t i;
    PT_DEV void operator()(float depth, f3 normal, int object_id) const {
        RadianceOut *r = out + i;
        r->depth = depth;
        r->normal[0] = normal.x;
        r->normal[1] = normal.y;
        r->normal[2] = normal.z;
        r->object_id = object_id;
    }
};

// The samples of one chunk: the 64 lanes' rays (o0, d0; `live` lanes only) through phases [B]-[E] in lock step, K.spp times,
// each lane's generator advanced in `rng`; returns the lane's sum of soft-clamped samples (avg_color of path_trace_kernel,
// scene_kernels.cuh:171-176, before its division).  `first` takes the first hit of sample 0.  radiance_query_kernel and
// probe_query_kernel (pt_probe.hip.h) are this loop in two frames; inlined, so each kernel keeps its own register allocation.
template <int GEOM, bool FULL, int PMODE, class FirstHit>
PT_DEV f3 trace_chunk_samples(const kparams_ptr kp0, const PairLds &PL, const LdsStack stk, CycleAcc &cyc, const int lane,
                              const bool live, const f3 o0, const f3 d0, Rng &rng, const FirstHit first) {
    f3 sum = mk3(0.0f); // avg_color of path_trace_kernel (scene_kernels.cuh:171-176)
    for (int s = 0; s < kparams(kp0).spp; ++s) { // (wave-uniform)
        // the sample's own copy of the ray: tracePath starts every sample from the caller's ray
        f3 ro = o0, rd = d0;
        bool ray_spec = true, prev_was_specular = true;
        f3 throughput = mk3(1.0f), acc = mk3(0.0f);
        int bounce = 0;
        bool act = live;
        while (__builtin_amdgcn_ballot_w64(act)) {
            // ---- [B] closest hit, all lanes that have a path together
            const KParams &KB = kparams(kp0);
            // (walk_closest's text, pt_query.hip.h, and not a call of it: one more level of inlining around the closest-hit walk
            // schedules the pair walk's stack push differently, and the PMODE 2 radiance and probe queries were 0.8 to 1.5 %
            // slower in every run -- DESIGN 3.33; a change there is a change here)
            int h_order = 0;
            const Hit h = (PMODE == 1)   ? closest_hit_pairs(KB, PL, lane, act, ro, rd, h_order)
                          : (PMODE == 2) ? closest_hit_pairs_dyn(KB, PL, lane, act, ro, rd)
                          : (PMODE == 3) ? closest_hit_pairs_tlas(KB, PL, lane, act, ro, rd, cyc)
                                         : closest_hit<GEOM>(KB, act, ro, rd, stk);
            // ---- [C] first half of the shading
            const KParams &KC = kparams(kp0);
            bool end_path = false, shaded = false, want_shadow = false;
            Surface hit;
            hit.point = hit.normal = mk3(0.0f);
            hit.t = 0.0f;
            hit.front_face = true;
            f3 L = mk3(0.0f), light_scale = mk3(0.0f), shadow_o = mk3(0.0f);
            float pdf_sample = 1.0f, shadow_tmax = 0.0f, light_att = 1.0f;
            if (act) {
                if (h.mesh < 0) {
                    if (s == 0 && bounce == 0) // first hit of the first sample (scene_kernels.cuh:181-193): HitInfo() defaults
                        first(1e30f, mk3(0.0f), -1);
                    add_miss_radiance(KC, rd, throughput, acc);
                    end_path = true;
                } else {
                    shaded = true;
                    hit = make_surface(KC, h, ro, rd, nullptr, nullptr);
                    if (s == 0 && bounce == 0)
                        first(hit.t, hit.normal, h.mesh);
                    const float4 m0 = KC.materials[h.mesh * 6 + 0], m2 = KC.materials[h.mesh * 6 + 2];
                    absorb_and_emit(m0, m2, hit, bounce == 0 || prev_was_specular, throughput, acc);
                    // light sample of next-event estimation (path_logic.cuh:305-382, 840)
                    if (!ray_spec && KC.n_lights > 0) {
                        const LightRec light = load_light(KC.lights, pick_light(rng, KC.n_lights));
                        sample_light(light, KC.inv_n_lights, hit, rng, L, pdf_sample, light_scale, light_att, shadow_o, shadow_tmax);
                        want_shadow = true;
                    }
                }
            }
            // ---- [C2] the light sample's value, before its visibility is known (path_logic.cuh:840-867): what a visible
            // sample adds to `acc`, formed from the same operands in the same order as in the reference.  A sample that adds
            // nothing either way (outside a spot cone, BSDF zero below the horizon) is not walked; the frame does not walk it.
            const KParams &KC2 = kparams(kp0);
            bool lit = false;
            f3 lit_now = mk3(0.0f);
            if (want_shadow) {
                const Material mat = load_material(KC2.materials, h.mesh);
                lit = light_sample_value<FULL>(hit, mat, L, -rd, pdf_sample, light_scale, light_att, throughput, lit_now);
            }
            // ---- [D] shadow rays, all lanes that have one together (bvh_any_hit_tlas); the contribution is added once its
            // visibility is known and before anything else touches the path's radiance
            const KParams &KD = kparams(kp0);
            if (__builtin_amdgcn_ballot_w64(lit)) {
                const bool in_shadow = walk_occluded<GEOM, PMODE>(KD, PL, stk, cyc, lane, lit, shadow_o, L, shadow_tmax);
                if (lit && !in_shadow)
                    acc = acc + lit_now;
            }
            // ---- [E] second half of the shading
            const KParams &KE = kparams(kp0);
            if (shaded) {
                const Material mat = load_material(KE.materials, h.mesh);
                if (!scatter_and_continue<FULL>(hit, mat, rng, KE.max_depth, ro, rd, throughput, bounce, ray_spec, prev_was_specular))
                    end_path = true;
            }
            if (act && end_path) { // the sample is complete (scene_kernels.cuh:170-171)
                acc = clamp_vector_soft(acc, 100.0f);
                sum = sum + acc;
                act = false;
            }
        }
    }
    return sum;
}

// (A ray's generator state in the caller's array is read before the ray's paths and written back advanced behind them:
// load_rng_state / store_rng_state, pt_path.hip.h.)

// Waves per SIMD the kernel is built for (its register budget: 512 / waves, in steps of 8): the most at which the pair variants
// keep a lane's whole path state -- ray, throughput, radiance, sum, generator, hit and light sample across the shadow walk -- in
// registers.  At four (128 VGPRs, path_trace_kernel's budget, which parks part of that state in LDS and recomputes the rest)
// every variant but PMODE 1 with the simple materials spilled 16 to 112 bytes per lane into scratch; at three none does.
constexpr int RADIANCE_WAVES = 3;
template <int GEOM, bool FULL, int PMODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RADIANCE_WAVES, 8))) void radiance_query_kernel(
    const KParams Kin, const float *__restrict__ origins, const float *__restrict__ dirs, uint32_t *__restrict__ rng_states, size_t n,
    RadianceOut *__restrict__ out) {
    // The parameters are read where they are used, through the kernarg segment (scalar loads that hit the constant cache), and
    // each phase of the loop gets its own opaque copy of the pointer, as in path_trace_kernel: held in SGPRs across the loop, the
    // ~110 dwords of the by-value copy are spilled into VGPR lanes, and from there into scratch.
    (void)Kin;
    const kparams_ptr kp0 = (kparams_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const KParams &K = kparams(kp0); // staging
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    const size_t chunks = (n + 63) / 64;
    for (size_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) { // (wave-uniform)
        const size_t i = ch * 64 + (size_t)lane;
        const bool live = i < n;
        f3 o0 = mk3(0.0f), d0 = mk3(0.0f);
        Rng rng = {0, 0, 0, 0, 0, 0};
        if (live) { // (the ray and its generator state in one block: chunk_ray's comment, pt_query.hip.h)
            o0 = mk3(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]);
            d0 = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
            load_rng_state(rng, rng_states + i * 6);
        }
        const FirstHitToRecord first{out, i};
        const f3 sum = trace_chunk_samples<GEOM, FULL, PMODE>(kp0, PL, stk, cyc, lane, live, o0, d0, rng, first);
        if (live) {
            store_rng_state(rng_states + i * 6, rng);
            const f3 mean = sum / (float)kparams(kp0).spp;
            RadianceOut *r = out + i;
            r->radiance[0] = mean.x;
            r->radiance[1] = mean.y;
            r->radiance[2] = mean.z;
        }
    }
    cyc.flush(lane);
}

// The primary rays ptrt_render(frame, ..) gives sample `sample` of every pixel of the context's rows, pinhole camera: phase [A]
// (scene_kernels.cuh:147-167, get_ray_simple) as pt_path.hip.h states it -- pixel_uv, pinhole_ray --, one thread per pixel,
// ray yl * width + x.  K.frame_count = frame + sample.
__global__ __launch_bounds__(256) void camera_rays_kernel(const KParams K, float *__restrict__ origins, float *__restrict__ dirs) {
    const size_t npix = (size_t)K.rows * K.width;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix)
        return;
    const int yl = (int)(i / (size_t)K.width), x = (int)(i % (size_t)K.width);
    const int y = global_row(yl, K.y0, K.il_period, K.il_phase);
    float u, v;
    pixel_uv(K, x, y, K.frame_count, u, v);
    f3 ro, rd;
    pinhole_ray(K.cam, u, v, ro, rd);
    origins[i * 3 + 0] = ro.x;
    origins[i * 3 + 1] = ro.y;
    origins[i * 3 + 2] = ro.z;
    dirs[i * 3 + 0] = rd.x;
    dirs[i * 3 + 1] = rd.y;
    dirs[i * 3 + 2] = rd.z;
}

// n generator states in canonical order {d, v0..v4}, state(seed) advanced by first, first + 1, .. subsequences of 2^67 draws:
// xorwow_init_kernel's arithmetic (the jump matrices selected by the bits of the subsequence number) for a number the caller
// chooses instead of the pixel's.
__global__ __launch_bounds__(256) void rng_states_kernel(uint32_t *__restrict__ states, size_t n, unsigned long long first,
                                                         uint32_t d0, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3,
                                                         uint32_t s4, const uint32_t *__restrict__ jump, int n_jump) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    unsigned long long sub = first + (unsigned long long)i;
    uint32_t v[5] = {s0, s1, s2, s3, s4};
    for (int k = 0; k < n_jump && sub; ++k, sub >>= 1) {
        if (!(sub & 1ull))
            continue;
        const uint32_t *M = jump + (size_t)k * 800;
        uint32_t a[5] = {0, 0, 0, 0, 0};
        for (int w = 0; w < 5; ++w) {
            uint32_t bits = v[w];
            while (bits) {
                const int b = __builtin_ctz(bits);
                bits &= bits - 1;
                const uint32_t *c = M + (w * 32 + b) * 5;
                a[0] ^= c[0];
                a[1] ^= c[1];
                a[2] ^= c[2];
                a[3] ^= c[3];
                a[4] ^= c[4];
            }
        }
        for (int w = 0; w < 5; ++w)
            v[w] = a[w];
    }
    states[i * 6 + 0] = d0;
    states[i * 6 + 1] = v[0];
    states[i * 6 + 2] = v[1];
    states[i * 6 + 3] = v[2];
    states[i * 6 + 4] = v[3];
    states[i * 6 + 5] = v[4];
}

} // namespace pt
