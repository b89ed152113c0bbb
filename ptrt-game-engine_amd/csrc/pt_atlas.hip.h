// pt_atlas.hip.h -- the front and the tail of a lightmap bake: a mesh's UV charts rasterised to atlas texels (world position,
// geometric normal, owning face: ptrt_atlas_texels) and the dilation of a baked atlas over its empty and invalid texels
// (ptrt_atlas_dilate).  No traversal: the rasteriser reads the triangle packets, slot_face and the mesh record an upload keeps.
//
// Coverage and barycentrics are ONE written definition in fp32 (-ffp-contract=off: every operation rounds on its own; `/` is
// the compiler's IEEE quotient), for the texel centre p = ((float)i + 0.5f, (float)j + 0.5f) and the face's corners 0, 1, 2:
//   d1 = (x1 - x0, y1 - y0)   d2 = (x2 - x0, y2 - y0)   q = (px - x0, py - y0)
//   A  = d1x * d2y - d1y * d2x
//   b1 = (qx * d2y - qy * d2x) / A     b2 = (d1x * qy - d1y * qx) / A     b0 = (1 - b1) - b2
//   covered  <=>  b0 >= 0 && b1 >= 0 && b2 >= 0                     (edges inclusive, both windings, a NaN fails)
// A face with a non-finite corner, A == 0 or A NaN covers nothing and is dropped before any float-to-int conversion.  The texels
// tested for a face are those of its SCAN RANGE: columns max(floor(min x) - 1, 0) .. min(ceil(max x), w - 1), rows likewise,
// clamped in float first (corners at +-1e30 are legal).  The range holds every centre inside the triangle's bounds with a
// texel to spare; it is part of the definition (tests/atlas_restatement.py walks the same one).
//
// Ownership: the LOWEST face index that covers a centre owns it, whatever the leaf order, the grid or the lanes per triangle:
// pass 1 takes the minimum with a device-scope atomicMin on the record's `face` word (empty records primed to INT32_MAX,
// records an earlier call owns -- mesh >= 0 -- left alone), pass 2 is a launch of its own -- the kernel boundary makes the
// atomics of every XCD visible -- and runs the same loop: the lane whose face is the winner writes the record.  A face held by
// several leaf slots computes the same record in each, so it does not matter which of them writes last.
#pragma once
#include "pt_kernels.hip.h"

namespace pt {

struct AtlasTexel { // mirrors ptrt_atlas_texel, 32 bytes
    float px, py, pz;
    int face;
    float nx, ny, nz;
    int mesh;
};
constexpr int ATLAS_NO_FACE = 0x7fffffff;

// Before pass 1: with `clear` every record becomes the empty one {0, 0, 0, INT32_MAX, 0, 0, 0, -1}; without, the records no
// earlier call owns get their face word primed and keep the rest.  One thread per record.
__global__ __launch_bounds__(256) void atlas_prime_kernel(AtlasTexel *__restrict__ texels, uint32_t n, int clear) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n)
        return;
    int4 *r = reinterpret_cast<int4 *>(texels + t);
    if (clear) {
        r[0] = make_int4(0, 0, 0, ATLAS_NO_FACE);
        r[1] = make_int4(0, 0, 0, -1);
    } else if (texels[t].mesh < 0) {
        texels[t].face = ATLAS_NO_FACE;
    }
}

// PASS 1: atomicMin of the face index into every covered, unowned record.  PASS 2: the winner's record.  A persistent grid of
// one-wave workgroups strides over units of 64 >> log2g leaf slots of the mesh; the 1 << log2g lanes of a slot walk its scan
// range row-major, lane l the texels l, l + g, ...
template <int PASS>
__global__ __launch_bounds__(64) void atlas_raster_kernel(const float4 *__restrict__ tris, const int4 *__restrict__ slot_face,
                                                          const float4 *__restrict__ rec, int slot_base, int slot_count, int mesh,
                                                          const float *__restrict__ uv, int aw, int ah, int log2g,
                                                          AtlasTexel *__restrict__ texels) {
    const int lane = threadIdx.x;
    const int g = 1 << log2g, per = 64 >> log2g;
    const int sub = lane >> log2g, li = lane & (g - 1);
    const uint32_t units = ((uint32_t)slot_count + (uint32_t)per - 1u) / (uint32_t)per;
    const float inf = __builtin_inff();
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) { // (wave-uniform)
        const uint32_t k = u * (uint32_t)per + (uint32_t)sub;
        if (k >= (uint32_t)slot_count)
            continue;
        const int s = slot_base + (int)k;
        const int f = slot_face[s].w;
        const float *c = uv + (size_t)f * 6;
        const float x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5];
        const bool finite = __builtin_fabsf(x0) < inf && __builtin_fabsf(y0) < inf && __builtin_fabsf(x1) < inf &&
                            __builtin_fabsf(y1) < inf && __builtin_fabsf(x2) < inf && __builtin_fabsf(y2) < inf;
        if (!finite)
            continue;
        const float d1x = x1 - x0, d1y = y1 - y0, d2x = x2 - x0, d2y = y2 - y0;
        const float A = d1x * d2y - d1y * d2x;
        if (A == 0.0f || A != A)
            continue;
        // the scan range, clamped to the atlas as floats (all finite), then as ints: (float)(aw - 1) may have rounded up
        const float fi0 = __builtin_fmaxf(__builtin_floorf(__builtin_fminf(x0, __builtin_fminf(x1, x2))) - 1.0f, 0.0f);
        const float fj0 = __builtin_fmaxf(__builtin_floorf(__builtin_fminf(y0, __builtin_fminf(y1, y2))) - 1.0f, 0.0f);
        const float fi1 = __builtin_fminf(__builtin_ceilf(__builtin_fmaxf(x0, __builtin_fmaxf(x1, x2))), (float)(aw - 1));
        const float fj1 = __builtin_fminf(__builtin_ceilf(__builtin_fmaxf(y0, __builtin_fmaxf(y1, y2))), (float)(ah - 1));
        if (fi0 > fi1 || fj0 > fj1)
            continue;
        const int i0 = (int)fi0, j0 = (int)fj0, i1 = min((int)fi1, aw - 1), j1 = min((int)fj1, ah - 1);
        if (i0 > i1 || j0 > j1)
            continue;
        const int wr = i1 - i0 + 1;
        const uint32_t total = (uint32_t)wr * (uint32_t)(j1 - j0 + 1); // at most aw * ah <= 2^28

        f3 v0 = mk3(0.0f), e1 = mk3(0.0f), e2 = mk3(0.0f), n = mk3(0.0f);
        bool inst = false;
        if (PASS == 2) {
            const float4 p0 = tris[s * 3 + 0], p1 = tris[s * 3 + 1], p2 = tris[s * 3 + 2];
            v0 = mk3(p0.x, p0.y, p0.z);
            e1 = mk3(p1.x, p1.y, p1.z);
            e2 = mk3(p2.x, p2.y, p2.z);
            n = mk3(p0.w, p1.w, p2.w); // the packet's geometric normal: the side cross(e1, e2) points to
            inst = (__float_as_int(rec[1].w) & 1) != 0;
            if (inst) // as make_surface_of has it for a front-face hit
                n = normalize(xform_dir(rec[8], rec[9], rec[10], n));
        }

        int j = li / wr, i = li - j * wr;
        const int gj = g / wr, gi = g - gj * wr;
        for (uint32_t q = (uint32_t)li; q < total; q += (uint32_t)g) {
            const int ti = i0 + i, tj = j0 + j; // in 0 .. aw - 1, 0 .. ah - 1
            const float qx = ((float)ti + 0.5f) - x0, qy = ((float)tj + 0.5f) - y0;
            const float b1 = (qx * d2y - qy * d2x) / A;
            const float b2 = (d1x * qy - d1y * qx) / A;
            const float b0 = (1.0f - b1) - b2;
            if (b0 >= 0.0f && b1 >= 0.0f && b2 >= 0.0f) {
                AtlasTexel *r = texels + ((size_t)tj * (size_t)aw + (size_t)ti);
                if (PASS == 1) {
                    if (r->mesh < 0)
                        atomicMin(&r->face, f);
                } else if (r->mesh < 0 && r->face == f) {
                    f3 p = mk3((v0.x + b1 * e1.x) + b2 * e2.x, (v0.y + b1 * e1.y) + b2 * e2.y, (v0.z + b1 * e1.z) + b2 * e2.z);
                    if (inst)
                        p = xform_point(rec[5], rec[6], rec[7], p);
                    float4 *o = reinterpret_cast<float4 *>(r);
                    o[0] = make_float4(p.x, p.y, p.z, __int_as_float(f));
                    o[1] = make_float4(n.x, n.y, n.z, __int_as_float(mesh));
                }
            }
            i += gi;
            j += gj;
            if (i >= wr) {
                i -= wr;
                ++j;
            }
        }
    }
}

// One dilation pass, src -> dst, float4 {r, g, b, valid} per texel, one thread per texel: a valid texel (valid != 0) is
// copied; an invalid one with n > 0 valid 8-neighbours inside the atlas becomes their rgb sum -- from 0.0f, in the order
// (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) -- divided by (float)n, valid = 1; with none it is copied as it is.
__global__ __launch_bounds__(256) void atlas_dilate_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, int aw, int ah) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)aw * (uint32_t)ah)
        return;
    const int j = (int)(t / (uint32_t)aw), i = (int)(t - (uint32_t)j * (uint32_t)aw);
    float4 v = src[t];
    if (!(v.w != 0.0f)) {
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
        int n = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int dx = (k < 3 ? k : k < 5 ? (k - 3) * 2 : k - 5) - 1, dy = k < 3 ? -1 : k < 5 ? 0 : 1;
            const int x = i + dx, y = j + dy;
            if (x < 0 || y < 0 || x >= aw || y >= ah)
                continue;
            const float4 a = src[(size_t)y * (size_t)aw + (size_t)x];
            if (a.w != 0.0f) {
                sr = sr + a.x;
                sg = sg + a.y;
                sb = sb + a.z;
                ++n;
            }
        }
        if (n > 0) {
            const float fn = (float)n;
            v = make_float4(sr / fn, sg / fn, sb / fn, 1.0f);
        }
    }
    dst[t] = v;
}

} // namespace pt
