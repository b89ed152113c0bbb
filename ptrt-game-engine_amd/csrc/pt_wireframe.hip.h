// pt_wireframe.hip.h -- the wireframe view of Scene::render_to_device_wireframe (scene.cuh:1211-1245):
// render_kernel_wireframe (scene_kernels.cuh:53-117) with wireframeMode == true, its only caller.
//
//   wireframe_kernel<GEOM>  one primary ray per pixel through the RNG-free Camera::get_ray(s, t), one closest hit,
//        an edge test on the hit's barycentrics, the sky elsewhere, Reinhard + gamma, RGB8.  No generator state,
//        no accumulation, no G-buffer: the kernel reads the scene and writes the caller's image, nothing else.
//
// Execution: one 8x8 tile per 64-lane workgroup (the reference's 8x8 block), tiles in plain order; the traversal stack
// in LDS as in trace_rays_kernel.  Every helper is the path kernel's own (closest_hit, normalize, det_*, tex2d_env), so
// the arithmetic is the one tests/wireframe_restatement.py restates on the CPU.
#pragma once
#include "pt_kernels.hip.h"
#include "pt_path.hip.h"

namespace pt {

// Camera::random_in_unit_disk_hash (camera.cuh:55-70): an integer hash of (x, y), then a point of the unit disk
PT_DEV f3 lens_disk_hash(uint32_t x, uint32_t y) {
    uint32_t seed = (x * 1973u) ^ (y * 9277u) ^ 0x9e3779b9u;
    seed ^= seed >> 17;
    seed *= 0xed5ad4bbu;
    seed ^= seed >> 11;
    seed *= 0xac4c1b51u;
    seed ^= seed >> 15;
    seed *= 0x31848babu;
    seed ^= seed >> 14;
    const float r1 = ((float)(seed & 0xFFFFu) + 0.5f) / 65536.0f;
    const float r2 = ((float)((seed * 0x343fdu + 0xc0f5u) & 0xFFFFu) + 0.5f) / 65536.0f;
    const float r = sqrt_ieee(r1);
    const float phi = 6.2831853f * r2;
    return mk3(r * det_cos(phi), r * det_sin(phi), 0.0f);
}

// powf(c, 1 / 2.2) of the kernel's gamma step.  det_pow is defined for c > 0 only; Reinhard gives exactly 0 where the
// colour is 0 (the sky switched off) and powf(0, y) is 0.  (c < 0 -- a negative sky colour -- is NaN in powf, which the
// clamp that follows turns into 0 as well.)
PT_DEV float wire_gamma(float c) { return c > 0.0f ? det_pow(c, 1.0f / 2.2f) : 0.0f; }

// Waves per SIMD GEOM 2 is compiled for (a real TLAS: closest_hit keeps its TLAS stack in registers).  Left alone it takes
// 131 VGPRs, three waves per SIMD; at four it fits 128 with no scratch: `many` 1080p 221 -> 194 us per frame.  GEOM 0 / 1
// are left alone (7 - 8 waves): bounding them to four cost the showcase frame 170 -> 180 us.
#ifndef PT_WIRE_WAVES
#define PT_WIRE_WAVES 4
#endif

// K: the context's parameters with width / height the FULL frame, rows / y0 the context's band, rgb8 / rgb8_frame the
// target (see rgb8_row); the generator, accumulation and G-buffer pointers are null -- this kernel writes none of them.
template <int GEOM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GEOM == 2 ? PT_WIRE_WAVES : 1, 8))) void wireframe_kernel(const KParams K, float thickness) {
    extern __shared__ uint2 lds_stack[];
    LdsStack stk{lds_stack + threadIdx.x};
    const int lane = threadIdx.x;
    const int x = blockIdx.x * 8 + (lane & 7), yl = blockIdx.y * 8 + (lane >> 3);
    const bool live = x < K.width && yl < K.rows;
    const int y = K.y0 + yl; // (an interleaved context is refused by ptrt_render_wireframe)
    const float s = ((float)x + 0.5f) / (float)K.width;
    const float t = 1.0f - ((float)y + 0.5f) / (float)K.height;
    // Camera::get_ray(s, t), device branch (camera.cuh:173-199)
    f3 ro = K.cam.origin, rd;
    if (K.cam.lens_radius <= 0) {
        rd = normalize(K.cam.llc + s * K.cam.horizontal + t * K.cam.vertical - K.cam.origin);
    } else {
        const uint32_t hx = (uint32_t)(s * 10000.0f) + (uint32_t)(t * 5000.0f);
        const uint32_t hy = (uint32_t)(t * 10000.0f) + (uint32_t)(s * 5000.0f);
        const f3 rdisk = K.cam.lens_radius * lens_disk_hash(hx, hy);
        const f3 offset = K.cam.u * rdisk.x + K.cam.v * rdisk.y;
        rd = normalize(K.cam.llc + s * K.cam.horizontal + t * K.cam.vertical - K.cam.origin - offset);
        ro = K.cam.origin + offset;
    }
    const Hit h = closest_hit<GEOM>(K, live, ro, rd, stk);
    if (!live)
        return;
    f3 c = mk3(0.0f);
    bool edge = false;
    if (h.mesh >= 0) {
        const float w = 1.0f - h.u - h.v;
        if (h.u < thickness || h.v < thickness || w < thickness) {
            edge = true;
            const float4 m2 = K.materials[h.mesh * 6 + 2]; // emission, as the path kernel reads it at a hit
            c = m2.x > 0.0f ? mk3(m2.x, m2.y, m2.z) : mk3(1.0f);
        }
    }
    if (!edge && K.use_sky) { // sampleSky (render_utils.cuh:115-137), as the path kernel restates it at a miss
        c = sample_sky(K, rd);
    }
    c = c / (c + mk3(1.0f));
    const f3 rgb = clampv(mk3(wire_gamma(c.x), wire_gamma(c.y), wire_gamma(c.z)), 0.0f, 1.0f) * 255.99f;
    unsigned char *o = K.rgb8 + ((size_t)rgb8_row(K, yl) * K.width + x) * 3;
    o[0] = (unsigned char)rgb.x;
    o[1] = (unsigned char)rgb.y;
    o[2] = (unsigned char)rgb.z;
}

} // namespace pt
