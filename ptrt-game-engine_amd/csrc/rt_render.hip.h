// rt_render.hip.h -- the one-bounce ray tracer of src/raytracer/ (RTscene.cuh, RTmesh.cuh, RTcamera.cuh) on gfx950.
//
//   rt_render_kernel  render_kernel (RTscene.cuh:1240-1293): per pixel the lens-free Camera::get_ray(u, v)
//        (RTcamera.cuh:135-157, device branch), traceRay over every mesh's own binary BVH in that mesh's rotated frame
//        (518-529), calculatePBRLightingCore (537-736) with one shadow ray per light, and for glass at the primary hit
//        a reflection and a refraction ray shaded without glass (shadeOneBounce, 749-761); then Reinhard, gamma 1/2.2,
//        clamp, * 255.0, truncation, row H-1-y.
//
// Execution: one 8x8 tile per 64-lane workgroup (the reference's 8x8 block).  The reference's recursion has a fixed depth
// (primary -> at most two secondary rays, which never recurse), so it is flattened into one loop of three segments: the
// primary ray, the reflection ray and the refraction ray, each a closest hit followed by the direct-lighting part of
// calculatePBRLightingCore.  Lanes whose pixel is not glass sit out segments 1 and 2.  Both traversals keep their
// 32-entry stacks in LDS (8 KB per workgroup), so nothing is indexed per lane in registers and the kernel has no scratch.
// Meshes and lights are looped over in order, so their descriptors are read wave-uniformly (scalar loads).
//
// Arithmetic: the project's numerics contract.  dot / cross are the fused forms of pt_device.hip.h,
// every other product and sum is rounded on its own (-ffp-contract=off), divisions and square roots are IEEE, __powf /
// __sincosf / __cosf are det_pow / det_sincos / det_cos.  tests/rt_restatement.py restates every line on the CPU.
#pragma once
#include "pt_device.hip.h"

namespace rt {
using pt::clamp01;
using pt::clampf;
using pt::clampv;
using pt::cross;
using pt::det_cos;
using pt::det_pow;
using pt::det_sincos;
using pt::dot;
using pt::f3;
using pt::length;
using pt::lerp;
using pt::max_;
using pt::min_;
using pt::mk3;
using pt::normalize;
using pt::rcp_ieee;
using pt::reflectVec;
using pt::sqrt_ieee;
using pt::operator+;
using pt::operator-;
using pt::operator*;
using pt::operator/;

constexpr int RT_STACK = 32; // bvh_trace / bvh_any_hit: pushes beyond 32 entries are dropped
constexpr float RT_PI = 3.14159265358979323846f, RT_TWO_PI = 6.28318530717958647692f, RT_INV_PI = 0.31830988618379067154f;
enum { RT_LIGHT_POINT = 0, RT_LIGHT_DIRECTIONAL = 1, RT_LIGHT_SPOT = 2 };

struct Mat { // Material (RTscene.cuh:21-61), 27 floats
    f3 albedo, specular;
    float metallic, roughness;
    f3 emission;
    float ior, transmission, transmission_roughness, clearcoat, clearcoat_roughness;
    f3 subsurface_color;
    float subsurface_radius, anisotropy, sheen;
    f3 sheen_tint;
    float iridescence, iridescence_thickness;
};

// One mesh as the kernel reads it (DeviceMesh, RTscene.cuh:84-102, re-laid out):
//   tris  3 float4 per face, in face order: (v0, 0), (v1 - v0, 0), (v2 - v0, 0) -- the edges subtracted in float32 on
//         the host, the same bits as intersect_triangle_mt's own subtraction
//   nodes 2 float4 per node: (bmin, a), (bmax, b) with a / b int bits: leaf (count > 0) a = start, b = ~count;
//         inner node a = left, b = right (-1: none)
struct MeshDev {
    const float4 *tris;
    const float4 *nodes;
    const int *prims;
    int face_count, node_count;
    float translation[3];
    float rot[9], inv[9]; // row-major mat3
    Mat mat;
};

struct LightDev { // Light (RTscene.cuh:64-80); cones already cosines
    int type;
    f3 position, direction, color;
    float intensity, range, inner_cone, outer_cone;
};

struct Params {
    const MeshDev *meshes;
    const LightDev *lights;
    int n_meshes, n_lights;
    f3 cam_origin, cam_cmo, cam_horizontal, cam_vertical; // Camera: origin, corner_minus_origin, horizontal, vertical
    f3 ambient, sky_top, sky_bottom;
    int use_sky;
    unsigned char *out;
    int width, height;
};

struct RayL { // RayOpt (RTmesh.cuh:18-50)
    f3 o, d, inv;
};

PT_DEV float safe_inv(float d) { return (__builtin_fabsf(d) > 1e-8f) ? rcp_ieee(d) : ((d >= 0.0f) ? 1e30f : -1e30f); }
PT_DEV RayL rt_ray(f3 o, f3 d) { return RayL{o, d, mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z))}; }

// m * v of mat3 (matrix.cuh operator*), row by row, each a rounded product and sum
PT_DEV f3 mat_mul(const float *m, f3 v) {
    return mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z);
}

PT_DEV RayL to_local(const MeshDev &M, f3 o, f3 d) {
    const f3 t = mk3(M.translation[0], M.translation[1], M.translation[2]);
    return rt_ray(mat_mul(M.inv, o - t), mat_mul(M.inv, d));
}

// AABB::hit_fast (RTmesh.cuh:58-80)
PT_DEV bool hit_fast(float4 lo, float4 hi, const RayL &r, float tmax_in, float &tmin_out) {
    const float tx1 = (lo.x - r.o.x) * r.inv.x, tx2 = (hi.x - r.o.x) * r.inv.x;
    float tmin = min_(tx1, tx2), tmax = max_(tx1, tx2);
    const float ty1 = (lo.y - r.o.y) * r.inv.y, ty2 = (hi.y - r.o.y) * r.inv.y;
    tmin = max_(tmin, min_(ty1, ty2));
    tmax = min_(tmax, max_(ty1, ty2));
    const float tz1 = (lo.z - r.o.z) * r.inv.z, tz2 = (hi.z - r.o.z) * r.inv.z;
    tmin = max_(tmin, min_(tz1, tz2));
    tmax = min_(tmax, max_(tz1, tz2));
    tmin = max_(tmin, 1e-4f);
    tmin_out = tmin;
    return tmax >= tmin && tmin < tmax_in;
}

// intersect_triangle_mt (RTmesh.cuh:245-285) on a (v0, e1, e2) record; t > 1e-4 on success
PT_DEV bool tri_hit(const float4 *rec, const RayL &r, float &t_out) {
    const float4 a0 = rec[0], a1 = rec[1], a2 = rec[2];
    const f3 v0 = mk3(a0.x, a0.y, a0.z), e1 = mk3(a1.x, a1.y, a1.z), e2 = mk3(a2.x, a2.y, a2.z);
    const f3 h = cross(r.d, e2);
    const float a = dot(e1, h);
    if (__builtin_fabsf(a) < 1e-8f)
        return false;
    const float f = rcp_ieee(a);
    const f3 s = r.o - v0;
    const float u = f * dot(s, h);
    if (u < 0.0f || u > 1.0f)
        return false;
    const f3 q = cross(s, e1);
    const float v = f * dot(r.d, q);
    if (v < 0.0f || u + v > 1.0f)
        return false;
    const float t = f * dot(e2, q);
    t_out = t;
    return t > 1e-4f;
}

struct Hit {
    bool hit;
    float t;
    int mesh, face;
};

// traceRay (RTscene.cuh:518-529) over bvh_trace (415-510): per mesh a fresh best t of 1e30, near child first, pushes
// dropped when the stack is full; across meshes a strictly smaller t wins (a tie keeps the lower mesh index).
PT_DEV Hit trace_closest(const Params &P, f3 o, f3 d, bool active, int *stk) {
    Hit best{false, 1e30f, -1, -1};
    for (int m = 0; m < P.n_meshes; ++m) {
        const MeshDev &M = P.meshes[m];
        if (M.node_count <= 0 || M.face_count <= 0 || !active)
            continue;
        const RayL r = to_local(M, o, d);
        float mt = 1e30f;
        int mface = -1;
        int sp = 0, ni = 0;
        while (true) {
            const float4 lo = M.nodes[2 * ni], hi = M.nodes[2 * ni + 1];
            float te;
            bool pop = false;
            if (!hit_fast(lo, hi, r, mt, te)) {
                pop = true;
            } else if (__float_as_int(hi.w) < -1) { // leaf
                const int start = __float_as_int(lo.w), count = ~__float_as_int(hi.w);
                for (int i = 0; i < count; ++i) {
                    const int f = M.prims[start + i];
                    float th;
                    if (tri_hit(M.tris + 3 * f, r, th) && th < mt) {
                        mt = th;
                        mface = f;
                    }
                }
                pop = true;
            } else {
                const int L = __float_as_int(lo.w), R = __float_as_int(hi.w);
                float tL = 1e30f, tR = 1e30f;
                const bool hL = L >= 0 && hit_fast(M.nodes[2 * L], M.nodes[2 * L + 1], r, mt, tL);
                const bool hR = R >= 0 && hit_fast(M.nodes[2 * R], M.nodes[2 * R + 1], r, mt, tR);
                if (hL && hR) {
                    const bool lfirst = tL <= tR;
                    if (sp < RT_STACK)
                        stk[(sp++) * 64] = lfirst ? R : L;
                    ni = lfirst ? L : R;
                } else if (hL || hR) {
                    ni = hL ? L : R;
                } else {
                    pop = true;
                }
            }
            if (pop) {
                if (sp == 0)
                    break;
                ni = stk[(--sp) * 64];
            }
        }
        if (mface >= 0 && mt < best.t) {
            best.hit = true;
            best.t = mt;
            best.mesh = m;
            best.face = mface;
        }
    }
    return best;
}

// bvh_any_hit (RTscene.cuh:362-413): both children pushed, left first, pushes dropped when full
PT_DEV bool any_hit(const MeshDev &M, const RayL &r, float tmax, int *stk) {
    int sp = 0;
    stk[(sp++) * 64] = 0;
    while (sp > 0) {
        const int ni = stk[(--sp) * 64];
        const float4 lo = M.nodes[2 * ni], hi = M.nodes[2 * ni + 1];
        float te;
        if (!hit_fast(lo, hi, r, tmax, te))
            continue;
        if (__float_as_int(hi.w) < -1) {
            const int start = __float_as_int(lo.w), count = ~__float_as_int(hi.w);
            for (int i = 0; i < count; ++i) {
                float th;
                if (tri_hit(M.tris + 3 * M.prims[start + i], r, th) && th < tmax)
                    return true;
            }
        } else {
            const int L = __float_as_int(lo.w), R = __float_as_int(hi.w);
            if (L >= 0 && sp < RT_STACK)
                stk[(sp++) * 64] = L;
            if (R >= 0 && sp < RT_STACK)
                stk[(sp++) * 64] = R;
        }
    }
    return false;
}

// ------------------------------------------------------------ shading helpers (RTscene.cuh:125-354)
PT_DEV float rt_attenuate(float distance, float range) {
    const float att = range / (range + distance);
    return att * att;
}
PT_DEV f3 fresnel(float cosTheta, f3 F0) { // fresnelSchlick: no clamp of cosTheta
    const float x = 1.0f - cosTheta;
    const float x2 = x * x;
    const float x5 = x2 * x2 * x;
    return F0 + (mk3(1.0f) - F0) * x5;
}
PT_DEV f3 fresnel_rough(float cosTheta, f3 F0, float roughness) {
    const float x = max_(1.0f - cosTheta, 0.0f);
    const float x2 = x * x;
    const float x5 = x2 * x2 * x;
    const float m = 1.0f - roughness;
    const f3 maxRefl = mk3(max_(m, F0.x), max_(m, F0.y), max_(m, F0.z));
    return F0 + (maxRefl - F0) * x5;
}
PT_DEV float ggx_d(f3 N, f3 H, float roughness) {
    const float a = roughness * roughness;
    const float a2 = a * a;
    const float NdotH = max_(dot(N, H), 0.0f);
    const float NdotH2 = NdotH * NdotH;
    float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
    denom = RT_PI * denom * denom;
    return a2 / max_(denom, 0.001f);
}
PT_DEV float ggx_g1(float NdotV, float roughness) {
    const float r = roughness + 1.0f;
    const float k = (r * r) * 0.125f;
    return NdotV / (NdotV * (1.0f - k) + k + 0.001f);
}
PT_DEV float ggx_g(f3 N, f3 V, f3 L, float roughness) {
    const float NdotV = max_(dot(N, V), 0.0f);
    const float NdotL = max_(dot(N, L), 0.0f);
    return ggx_g1(NdotV, roughness) * ggx_g1(NdotL, roughness);
}
PT_DEV void tangent_frame(f3 N, f3 &T, f3 &B) {
    T = (__builtin_fabsf(N.z) < 0.9999f) ? normalize(cross(mk3(0.0f, 0.0f, 1.0f), N)) : normalize(cross(mk3(1.0f, 0.0f, 0.0f), N));
    B = cross(N, T);
}
PT_DEV float ggx_d_aniso(f3 N, f3 H, f3 T, f3 B, float ax, float ay) {
    const float NdotH = dot(N, H);
    if (NdotH <= 0.0f)
        return 0.0f;
    const float TdotH = dot(T, H), BdotH = dot(B, H);
    const float ax2 = ax * ax, ay2 = ay * ay;
    float denom = (TdotH * TdotH / ax2) + (BdotH * BdotH / ay2) + (NdotH * NdotH);
    denom = RT_PI * ax * ay * denom * denom;
    return 1.0f / max_(denom, 0.001f);
}
PT_DEV float ggx_g1_aniso(float NdotV, float TdotV, float BdotV, float ax, float ay) {
    const float ax2 = ax * ax, ay2 = ay * ay;
    const float lambda = sqrt_ieee(ax2 * TdotV * TdotV + ay2 * BdotV * BdotV + NdotV * NdotV);
    return 2.0f * NdotV / (NdotV + lambda + 0.001f);
}
PT_DEV f3 iridescence(float thickness, float cosTheta) { // calculateIridescence, filmIOR 1.3, baseIOR 1.5
    cosTheta = clamp01(cosTheta);
    const float sinTheta = sqrt_ieee(1.0f - cosTheta * cosTheta);
    const float sinThetaFilm = sinTheta / 1.3f;
    if (sinThetaFilm * sinThetaFilm > 1.0f)
        return mk3(1.0f);
    const float cosThetaFilm = sqrt_ieee(1.0f - sinThetaFilm * sinThetaFilm);
    const float OPD = 2.0f * 1.3f * thickness * cosThetaFilm;
    float Ra = (1.0f - 1.3f) / (1.0f + 1.3f);
    Ra *= Ra;
    float Rb = (1.3f - 1.5f) / (1.3f + 1.5f);
    Rb *= Rb;
    const float sqrtR1R2 = sqrt_ieee(Ra * Rb);
    float R_max = sqrt_ieee(Ra) + sqrt_ieee(Rb);
    R_max *= R_max;
    const float den = R_max + 1e-6f;
    const float r0 = Ra + Rb + 2.0f * sqrtR1R2 * det_cos(RT_TWO_PI * OPD / 650.0f);
    const float r1 = Ra + Rb + 2.0f * sqrtR1R2 * det_cos(RT_TWO_PI * OPD / 550.0f);
    const float r2 = Ra + Rb + 2.0f * sqrtR1R2 * det_cos(RT_TWO_PI * OPD / 450.0f);
    return mk3(clamp01(r0 / den), clamp01(r1 / den), clamp01(r2 / den));
}
// perturbDirectionGGX (RTscene.cuh:246-277); callers only reach it with roughness > 0.02
PT_DEV f3 perturb_ggx(f3 dir, float roughness, uint32_t &seed) {
    seed = seed * 747796405u + 2891336453u;
    const float u1 = (float)seed * 2.3283064365386963e-10f;
    seed = seed * 747796405u + 2891336453u;
    const float u2 = (float)seed * 2.3283064365386963e-10f;
    const float a = roughness * roughness;
    const float phi = RT_TWO_PI * u1;
    const float cosTheta = sqrt_ieee((1.0f - u2) / (1.0f + (a * a - 1.0f) * u2));
    const float sinTheta = sqrt_ieee(1.0f - cosTheta * cosTheta);
    f3 T, B;
    tangent_frame(dir, T, B);
    float sinPhi, cosPhi;
    det_sincos(phi, sinPhi, cosPhi);
    return normalize(T * (cosPhi * sinTheta) + B * (sinPhi * sinTheta) + dir * cosTheta);
}
// __powf(x, y) of beerLambert and of the gamma step: det_pow is defined for x > 0 only.  x == 0 gives 0 (powf(0, y) = 0
// for the y > 0 both callers pass: a thickness is > 1e-4 or 1, the gamma 0.4545...); x < 0 or NaN cannot reach
// beerLambert (its input is clamped to [0, 1]) and would be NaN in gamma, which the final clamp makes 0 -- so 0 as well.
PT_DEV float pos_pow(float x, float y) { return x > 0.0f ? det_pow(x, y) : 0.0f; }

PT_DEV f3 sky(const Params &P, f3 d) { // sampleSky (RTscene.cuh:354-360) and render_kernel's miss colour
    if (!P.use_sky)
        return mk3(0.0f);
    return lerp(P.sky_bottom, P.sky_top, 0.5f * (d.y + 1.0f));
}

// The direct part of calculatePBRLightingCore (RTscene.cuh:537-684): emission, ambient and one shadow-tested term per
// light.  `active`: the lane has a hit to shade (its shadow rays are traced); other lanes compute nothing useful.
PT_DEV f3 shade_direct(const Params &P, const Mat &mat, f3 point, f3 Ng, float t, f3 dir, bool allowSpecTransmission,
                       bool active, int *stk) {
    const f3 V = mk3(-dir.x, -dir.y, -dir.z);
    const float rough = min_(max_(mat.roughness, 0.02f), 1.0f);
    const float metal = min_(max_(mat.metallic, 0.0f), 1.0f);
    const bool isGlass = (mat.transmission > 0.0f) && (metal < 0.1f);
    const f3 F0 = lerp(mat.specular, mat.albedo, metal);
    f3 color = mk3(0.0f) + mat.emission;
    const float NdotV = max_(dot(Ng, V), 0.0f);
    const f3 F_ambient = fresnel_rough(NdotV, F0, rough);
    f3 kD_ambient = (mk3(1.0f) - F_ambient) * (1.0f - metal);
    if (isGlass)
        kD_ambient = mk3(0.0f);
    color = color + kD_ambient * mat.albedo * P.ambient;
    const float eps = 1e-3f * max_(1.0f, t);
    const f3 so = point + Ng * eps;
    for (int i = 0; i < P.n_lights; ++i) {
        const LightDev &light = P.lights[i];
        f3 L;
        float attenuation = 1.0f, lightDistance = 1e30f;
        if (light.type == RT_LIGHT_DIRECTIONAL) {
            L = -light.direction;
        } else {
            const f3 toLight = light.position - point;
            const float distance = length(toLight);
            L = toLight / max_(distance, 1e-6f);
            float att = rt_attenuate(distance, light.range);
            if (light.type == RT_LIGHT_SPOT) {
                const float theta = dot(L, -light.direction);
                const float epsilon = light.inner_cone - light.outer_cone;
                const float spot = clampf((theta - light.outer_cone) / epsilon, 0.0f, 1.0f);
                att *= spot;
            }
            attenuation = att;
            lightDistance = distance;
        }
        // shadow ray: meshes with transmission > 0 cast none
        bool inShadow = false;
        for (int m = 0; m < P.n_meshes; ++m) {
            const MeshDev &M = P.meshes[m];
            if (M.mat.transmission > 0.0f || M.node_count <= 0 || M.face_count <= 0)
                continue;
            if (active && !inShadow)
                inShadow = any_hit(M, to_local(M, so, L), lightDistance, stk);
        }
        if (inShadow)
            continue;
        const f3 H = normalize(L + V);
        const float NdotL = max_(dot(Ng, L), 0.0f);
        const float VdotH = max_(dot(V, H), 0.0f);
        float D, G;
        if (__builtin_fabsf(mat.anisotropy) > 0.01f) {
            f3 T, B;
            tangent_frame(Ng, T, B);
            const float r2 = rough * rough;
            const float aspect = sqrt_ieee(1.0f - 0.9f * __builtin_fabsf(mat.anisotropy));
            float ax, ay;
            if (mat.anisotropy >= 0.0f) {
                ax = r2 / aspect;
                ay = r2 * aspect;
            } else {
                ax = r2 * aspect;
                ay = r2 / aspect;
            }
            ax = max_(ax, 0.001f);
            ay = max_(ay, 0.001f);
            D = ggx_d_aniso(Ng, H, T, B, ax, ay);
            const float nv = max_(dot(Ng, V), 0.0f), nl = max_(dot(Ng, L), 0.0f);
            G = ggx_g1_aniso(nv, dot(T, V), dot(B, V), ax, ay) * ggx_g1_aniso(nl, dot(T, L), dot(B, L), ax, ay);
        } else {
            D = ggx_d(Ng, H, rough);
            G = ggx_g(Ng, V, L, rough);
        }
        f3 F = fresnel(VdotH, F0);
        if (mat.iridescence > 0.0f) {
            const f3 irid = iridescence(mat.iridescence_thickness, VdotH);
            F = lerp(F, F * irid, mat.iridescence);
        }
        const f3 specular = (D * G * F) / (4.0f * max_(dot(Ng, V), 0.0f) * NdotL + 0.001f);
        f3 kD = (mk3(1.0f) - F) * (1.0f - metal);
        f3 diffuse = mat.albedo * RT_INV_PI;
        if (mat.sheen > 0.0f) {
            const float x = 1.0f - VdotH;
            const float x2 = x * x;
            const float FH = x2 * x2 * x;
            const f3 sheenColor = lerp(mk3(1.0f), mat.sheen_tint, FH);
            kD = kD + sheenColor * mat.sheen * (1.0f - metal);
        }
        if (mat.subsurface_radius > 0.0f) {
            float sss = max_(dot(V, -L), 0.0f);
            sss = sss * sss * mat.subsurface_radius;
            diffuse = lerp(diffuse, mat.subsurface_color * RT_INV_PI, sss);
        }
        f3 thinTrans = mk3(0.0f);
        if (isGlass && !allowSpecTransmission) {
            kD = mk3(0.0f);
            thinTrans = (mk3(1.0f) - F) * mat.transmission;
        }
        f3 Lo = (kD * diffuse + specular + thinTrans) * light.color * light.intensity * 20.0f * NdotL * attenuation;
        if (mat.clearcoat > 0.0f) {
            const float ccD = ggx_d(Ng, H, mat.clearcoat_roughness);
            const float ccG = ggx_g(Ng, V, L, mat.clearcoat_roughness);
            const f3 ccF = fresnel(VdotH, mk3(0.04f));
            const f3 ccBRDF = (ccD * ccG * ccF) / (4.0f * max_(dot(Ng, V), 0.0f) * NdotL + 0.001f);
            Lo = Lo * (mk3(1.0f) - mat.clearcoat * ccF) +
                 ccBRDF * light.color * light.intensity * 20.0f * NdotL * attenuation * mat.clearcoat;
        }
        color = color + Lo;
    }
    return color;
}

PT_DEV Mat load_mat(const MeshDev &M) { return M.mat; }

__global__ __launch_bounds__(64) void rt_render_kernel(const Params P) {
    __shared__ int stack_lds[RT_STACK * 64];
    const int lane = threadIdx.x;
    int *stk = stack_lds + lane;
    const int x = blockIdx.x * 8 + (lane & 7), y = blockIdx.y * 8 + (lane >> 3);
    const bool live = x < P.width && y < P.height;
    const float u = ((float)x + 0.5f) * (1.0f / (float)P.width);
    const float v = 1.0f - ((float)y + 0.5f) * (1.0f / (float)P.height);
    const f3 rd0 = normalize(P.cam_cmo + u * P.cam_horizontal + v * P.cam_vertical);

    // segment 0: the primary ray; 1: glass reflection; 2: glass refraction
    f3 color = mk3(0.0f), Rcol = mk3(0.0f), Tcol = mk3(0.0f), Fr = mk3(0.0f), Rdir = rd0, Tdir = rd0, gP = mk3(0.0f),
       gNf = mk3(0.0f), albedo = mk3(0.0f);
    float geps = 0.0f, transmission = 0.0f;
    bool glass = false, refrOk = false;
    for (int seg = 0; seg < 3; ++seg) {
        const bool active = seg == 0 ? live : (glass && (seg == 1 || refrOk));
        if (__builtin_amdgcn_ballot_w64(active) == 0ull)
            continue;
        const f3 ro = seg == 0 ? P.cam_origin : (seg == 1 ? gP + gNf * geps : gP - gNf * geps);
        const f3 rd = seg == 0 ? rd0 : (seg == 1 ? Rdir : Tdir);
        const Hit h = trace_closest(P, ro, rd, active, stk);
        f3 c;
        Mat mat{};
        f3 point = mk3(0.0f), Ng = mk3(0.0f);
        if (h.hit) {
            const MeshDev &M = P.meshes[h.mesh];
            mat = load_mat(M);
            point = mk3(ro.x + h.t * rd.x, ro.y + h.t * rd.y, ro.z + h.t * rd.z);
            const float4 *rec = M.tris + 3 * h.face;
            const float4 a1 = rec[1], a2 = rec[2];
            const f3 nl = normalize(cross(mk3(a1.x, a1.y, a1.z), mk3(a2.x, a2.y, a2.z)));
            Ng = normalize(mat_mul(M.rot, nl));
        }
        c = shade_direct(P, mat, point, Ng, h.t, rd, seg == 0, active && h.hit, stk);
        if (!h.hit)
            c = sky(P, rd);
        if (seg == 0) {
            color = c;
            const float metal = min_(max_(mat.metallic, 0.0f), 1.0f);
            glass = live && h.hit && mat.transmission > 0.0f && metal < 0.1f;
            if (glass) { // RTscene.cuh:686-733
                const f3 I = rd;
                const float NgI = dot(Ng, I);
                const f3 Nf = (NgI < 0.0f) ? Ng : -Ng;
                float n1 = 1.0f, n2 = mat.ior;
                if (NgI > 0.0f) {
                    n1 = mat.ior;
                    n2 = 1.0f;
                }
                const float eta = n1 / n2;
                float F0s = (n2 - n1) / (n2 + n1);
                F0s = F0s * F0s;
                const float cosTheta = max_(dot(-I, Nf), 0.0f);
                Fr = fresnel(cosTheta, mk3(F0s));
                geps = 1e-3f * max_(1.0f, h.t);
                gP = point;
                gNf = Nf;
                transmission = mat.transmission;
                albedo = mat.albedo;
                uint32_t seed = __float_as_uint(point.x * 12.9898f + point.y * 78.233f + point.z * 45.164f);
                seed = seed * 747796405u + 2891336453u;
                Rdir = normalize(reflectVec(I, Nf));
                const float reflRough = max_(mat.roughness, mat.transmission_roughness);
                if (reflRough > 0.02f)
                    Rdir = perturb_ggx(Rdir, reflRough, seed);
                // refractVec (RTscene.cuh:333-341)
                const float NdotI = dot(Nf, I);
                const float k = 1.0f - eta * eta * (1.0f - NdotI * NdotI);
                refrOk = !(k < 0.0f);
                if (refrOk) {
                    Tdir = normalize(eta * I - (eta * NdotI + sqrt_ieee(k)) * Nf);
                    if (mat.transmission_roughness > 0.02f)
                        Tdir = perturb_ggx(Tdir, mat.transmission_roughness, seed);
                }
            }
        } else if (seg == 1) {
            Rcol = c;
        } else if (active) {
            const float thickness = h.hit ? h.t : 1.0f;
            const f3 a = clampv(albedo, 0.0f, 1.0f);
            const f3 absorb = mk3(pos_pow(a.x, thickness), pos_pow(a.y, thickness), pos_pow(a.z, thickness));
            Tcol = absorb * c;
        }
    }
    if (!live)
        return;
    if (glass) {
        if (!refrOk) {
            Fr = mk3(1.0f);
            Tcol = mk3(0.0f);
        }
        color = color + Fr * Rcol + (mk3(1.0f) - Fr) * transmission * Tcol;
    }
    // Reinhard, gamma, clamp, * 255.0, truncation; a NaN channel (inner == outer spot cones, 0 / 0 edge cases) ends as 0
    color = color / (color + mk3(1.0f));
    const f3 g = mk3(pos_pow(color.x, 0.4545454545f), pos_pow(color.y, 0.4545454545f), pos_pow(color.z, 0.4545454545f));
    const f3 rgb = clampv(g, 0.0f, 1.0f) * 255.0f;
    unsigned char *o = P.out + ((size_t)(P.height - 1 - y) * P.width + x) * 3;
    o[0] = (unsigned char)rgb.x;
    o[1] = (unsigned char)rgb.y;
    o[2] = (unsigned char)rgb.z;
}

} // namespace rt
