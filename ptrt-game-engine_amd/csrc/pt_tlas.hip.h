// pt_tlas.hip.h -- GPU refit of a TLAS with inner nodes over the topology that was uploaded: instances and
// meshes move without a host round trip (ptrt_set_instance_transforms, ptrt_refit_tlas).
//
// The reference rebuilds its TLAS on the CPU whenever a mesh moved (Scene::buildAndUploadTLAS,
// scene.cuh:458-594); it has no refit.  Here the child pairs, leaf ranges and mesh indices of the upload
// stay, and everything that depends on boxes and matrices is derived again on the context's stream:
//   1. scatter_xforms_kernel  the flag bit and nine matrix rows of the meshes a caller moved, from staging
//                             into the mesh records (root boxes untouched); or compose_poses_kernel, which derives
//                             them on the device from the nine floats of the reference's Transform3D (below)
//   2. refit_tlas_kernel      ONE workgroup, barriers between its phases:
//        a. per TLAS index: the mesh's world box (Transform3D::transformAABB, transform.cuh:399-416, the
//           arithmetic of tlas_root_box) into scratch, and the instance's first-pass box
//        b. per TLAS leaf: union of its members' world boxes, stored into its parent's child slot
//           (or the TLAS root box)
//        c. the inner levels, deepest first, as refit_top_levels_kernel walks a BLAS
//      A TLAS has at most mesh-count nodes; every phase strides over its items, so any mesh count is
//      covered.  Beyond TLAS_WIDE meshes phase a runs as a launch of its own over the whole device.
// min / max are exact, so the boxes equal a host refit of the same topology bit for bit (Scene::refitTLAS).
//
// Re-order (ptrt_reorder_tlas), in front of the refit.  The reference's TLAS builder splits n > leafMax entries into
// n/2 | n - n/2 whatever the boxes are (scene.cuh:497-548), so a TLAS of a given mesh count has ONE shape; what a rebuild
// changes is which mesh sits at which TLAS index.  As ptrt_build_bvh does for the faces of a mesh (pt_build.hip.h), the
// meshes are re-dealt to the indices in Morton order of their world boxes' centres:
//   3. reorder_tlas_kernel    ONE workgroup, up to TLAS_WIDE meshes; item i is MESH i, so the result does not depend on the
//                             order it replaces:
//        a. centre of the mesh's world box (mesh_world_box; AABB::center(), transform.cuh:97: (bmin + bmax) * 0.5f)
//        b. min / max of the centres: wave shuffles, then one LDS slot per wave (no atomics)
//        c. 30-bit Morton code (morton30 of pt_build.hip.h), key = code << 32 | mesh
//        d. bitonic sort of the keys in LDS, padded to a power of two with all-ones keys (32 KB at most)
//        e. tlas_mesh_ids[j] = the mesh ranked j
//      Beyond TLAS_WIDE meshes: tlas_centres_kernel (ordered-int atomics, as centroid_bounds_kernel), morton_kernel and the
//      radix passes of pt_build.hip.h over (code, mesh) seeded in ascending mesh order -- the sort is stable, so equal codes
//      keep that order, which is what the mesh in the key's low half gives -- and tlas_take_order_kernel.
// The builder emits its leaves depth first and each appends its members to the index array (build_bvh_range: prims.push_back;
// upload_tlas keeps those ranges in tlas_leaves), so the leaves' index ranges are consecutive and in tree order, left subtree
// before right: rank j -> index j puts the lower half of the curve under every node's left child, i.e. an object-median split
// along the Z-order curve.  (A TLAS uploaded through the C ABI with other ranges is still re-ordered validly -- any
// permutation is a valid TLAS under the refit that follows -- only without that reading.)
#pragma once
#include "pt_build.hip.h"
#include "pt_refit.hip.h"

namespace pt {

constexpr int XFORM_F = 40;       // floats per staged record: {flag, -, -, -}, inverse rows, world rows, normal rows
// where scatter_xforms_kernel finds a record's fields, in floats: the staged records above, or a caller's ptrt_instance_xform
// array read in place (ptrt_set_instance_transforms_device).  `flag`: a word that is non-zero for has_transform.
struct XformLayout {
    int stride, flag, inverse, world, normal;
};
constexpr XformLayout XFORM_STAGED{XFORM_F, 0, 4, 16, 28};
constexpr int TLAS_BLOCK = 256;   // threads of the one workgroup (the fp64 first-pass bound wants registers, not lanes)
constexpr int TLAS_WIDE = 4096;   // more TLAS indices than this: world boxes in a launch of their own

__global__ void scatter_xforms_kernel(const float *__restrict__ xf, XformLayout L, float4 *mesh_recs, int first, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * 37)
        return;
    const int r = i / 37, k = i - r * 37; // k == 0: the flags word, k >= 1: float k - 1 of the nine rows
    float *rec = reinterpret_cast<float *>(mesh_recs + (size_t)(first + r) * MESH_REC_F4);
    const float *src = xf + (size_t)r * L.stride;
    if (k == 0) {
        const int flags = (__float_as_int(rec[7]) & ~1) | (__float_as_int(src[L.flag]) != 0 ? 1 : 0); // (bit 1 belongs to the materials)
        rec[7] = __int_as_float(flags);
    } else {
        const int b = (k - 1) / 12, j = (k - 1) - b * 12; // matrix b (inverse, world, normal), float j of its first three rows
        const int off = b == 0 ? L.inverse : (b == 1 ? L.world : L.normal);
        rec[8 + k - 1] = (b == 2 && (j & 3) == 3) ? 0.0f : src[off + j]; // (a normal row's fourth word is 0 in the records)
    }
}

// ---- poses -> mesh records (ptrt_set_instance_poses_device) ----------------------------------------------------------------
// The reference keeps nine floats per mesh -- Transform3D::position, rotation (Euler radians), scale -- and derives the three
// matrices and the has_transform bit from them on the HOST (Transform3D::updateMatrices, transform.cuh:260-306; the descriptor
// loop, scene.cuh:718-721).  compose_poses_kernel is that derivation, one instance per thread, with this arithmetic contract:
//   * every product and sum is a rounded multiply followed by a rounded add, in the order the reference's expressions are
//     written: nothing is fused (no fma_ here, unlike dot and cross; the translation unit is built with -ffp-contract=off);
//   * sinf / cosf of the three angles are det_sincos, the project's one sine and cosine (dm_sincos of oracle/detmath.h bit
//     for bit): whichever libm the reference's caller links is not reproducible;
//   * the rotation matrix as transform.cuh:270-288; world = rot * diag(scale) through mat4::operator* (mat4.cuh:280-323) with
//     its typo in r.m[3] (b.m[11] where b.m[1] belongs).  With these operands the typo only ever multiplies zeros, but the
//     zero terms are added (they decide the sign of a zero and carry a NaN), so the four-term sums stay; then position goes
//     into m[3], m[7], m[11];
//   * inverse = mat4::inverse (mat4.cuh:211-262): the eighteen 2x2 determinants, det, the identity when fabsf(det) < 1e-10f,
//     otherwise invDet = 1.0f / det correctly rounded (rcp_ieee) and every entry invDet * (+-(...)), negations as written;
//   * normal = the inverse's transpose (the records keep its 3x3 part);
//   * has_transform = position.length() > 0.001f || rotation.length() > 0.001f || fabsf(scale.x - 1.0f) > 0.001f with
//     length = sqrtf(x*x + y*y + z*z), left to right, the root correctly rounded (sqrt_ieee).  Only scale.x is looked at:
//     a mesh scaled in y alone at the origin is NOT an instance, as in the reference;
//   * a NaN or an infinity in a pose propagates as that arithmetic propagates it: no special case but the determinant test.
// Only rows 0-2 of each matrix reach the records, so what feeds row 3 alone is not computed.
// Mapping: a thread composes one instance into LDS (37 words, an odd stride: no bank conflicts), then the workgroup copies
// its instances' 37-word runs -- flags word and nine rows are contiguous in a record -- with consecutive lanes on consecutive
// words: a thread storing its own record would put every lane of a store on another cache line.  Bit 1 of the flags word
// belongs to the materials and is kept; the root box is not touched.
constexpr int POSE_F = 9;         // floats per pose: position, rotation, scale
constexpr int POSE_BLOCK = 256;   // instances (= threads) per workgroup
constexpr int POSE_OUT = 37;      // words per instance: the flags word and the nine rows (floats 7 .. 43 of a mesh record)

struct PoseMat4 {
    float m[16];
};
// mat4::operator* as the reference writes it (column-major product; r.m[3] takes b.m[11] for b.m[1])
__device__ __forceinline__ PoseMat4 pose_mul(const PoseMat4 &a, const PoseMat4 &b) {
    PoseMat4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float b1 = (c == 0 && k == 3) ? b.m[11] : b.m[c * 4 + 1];
            r.m[c * 4 + k] = a.m[k] * b.m[c * 4] + a.m[4 + k] * b1 + a.m[8 + k] * b.m[c * 4 + 2] + a.m[12 + k] * b.m[c * 4 + 3];
        }
    return r;
}
__device__ __forceinline__ float pose_length(float x, float y, float z) { return sqrt_ieee(x * x + y * y + z * z); }

__global__ __launch_bounds__(POSE_BLOCK) void compose_poses_kernel(const float *__restrict__ poses, float4 *mesh_recs, int first,
                                                                   int count) {
    __shared__ float out[POSE_BLOCK * POSE_OUT];
    const int base = blockIdx.x * POSE_BLOCK, t = threadIdx.x;
    const int here = min(POSE_BLOCK, count - base); // instances of this workgroup (the grid covers `count`: here >= 1)
    if (t < here) {
        const float *p = poses + (size_t)(base + t) * POSE_F;
        const float px = p[0], py = p[1], pz = p[2], rx = p[3], ry = p[4], rz = p[5], scx = p[6], scy = p[7], scz = p[8];
        float sx, cx, sy, cy, sz, cz;
        det_sincos(rx, sx, cx);
        det_sincos(ry, sy, cy);
        det_sincos(rz, sz, cz);
        PoseMat4 rot, w;
        rot.m[0] = cy * cz;
        rot.m[1] = cz * sx * sy - cx * sz;
        rot.m[2] = cx * cz * sy + sx * sz;
        rot.m[3] = 0.0f;
        rot.m[4] = cy * sz;
        rot.m[5] = cx * cz + sx * sy * sz;
        rot.m[6] = cx * sy * sz - cz * sx;
        rot.m[7] = 0.0f;
        rot.m[8] = -sy;
        rot.m[9] = cy * sx;
        rot.m[10] = cx * cy;
        rot.m[11] = 0.0f;
        rot.m[12] = rot.m[13] = rot.m[14] = 0.0f;
        rot.m[15] = 1.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            w.m[k] = (k % 5 == 0) ? 1.0f : 0.0f;
        w.m[0] = scx;
        w.m[5] = scy;
        w.m[10] = scz;
        w = pose_mul(rot, w);
        w.m[3] = px;
        w.m[7] = py;
        w.m[11] = pz;
        const float *m = w.m;
        const float A2323 = m[10] * m[15] - m[11] * m[14], A1323 = m[9] * m[15] - m[11] * m[13];
        const float A1223 = m[9] * m[14] - m[10] * m[13], A0323 = m[8] * m[15] - m[11] * m[12];
        const float A0223 = m[8] * m[14] - m[10] * m[12], A0123 = m[8] * m[13] - m[9] * m[12];
        const float A2313 = m[6] * m[15] - m[7] * m[14], A1313 = m[5] * m[15] - m[7] * m[13];
        const float A1213 = m[5] * m[14] - m[6] * m[13], A0313 = m[4] * m[15] - m[7] * m[12];
        const float A0113 = m[4] * m[13] - m[5] * m[12]; // (A0213 and A0212 feed row 3 of the inverse alone)
        const float A2312 = m[6] * m[11] - m[7] * m[10], A1312 = m[5] * m[11] - m[7] * m[9];
        const float A1212 = m[5] * m[10] - m[6] * m[9], A0312 = m[4] * m[11] - m[7] * m[8];
        const float A0112 = m[4] * m[9] - m[5] * m[8];
        const float det = m[0] * (m[5] * A2323 - m[6] * A1323 + m[7] * A1223) - m[1] * (m[4] * A2323 - m[6] * A0323 + m[7] * A0223) +
                          m[2] * (m[4] * A1323 - m[5] * A0323 + m[7] * A0123) - m[3] * (m[4] * A1223 - m[5] * A0223 + m[6] * A0123);
        float inv[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f}; // (rows 0-2 of the identity)
        if (!(__builtin_fabsf(det) < 1e-10f)) {
            const float invDet = rcp_ieee(det);
            inv[0] = invDet * (m[5] * A2323 - m[6] * A1323 + m[7] * A1223);
            inv[1] = invDet * -(m[1] * A2323 - m[2] * A1323 + m[3] * A1223);
            inv[2] = invDet * (m[1] * A2313 - m[2] * A1313 + m[3] * A1213);
            inv[3] = invDet * -(m[1] * A2312 - m[2] * A1312 + m[3] * A1212);
            inv[4] = invDet * -(m[4] * A2323 - m[6] * A0323 + m[7] * A0223);
            inv[5] = invDet * (m[0] * A2323 - m[2] * A0323 + m[3] * A0223);
            inv[6] = invDet * -(m[0] * A2313 - m[2] * A0313 + m[3] * A0113);
            inv[7] = invDet * (m[0] * A2312 - m[2] * A0312 + m[3] * A0112);
            inv[8] = invDet * (m[4] * A1323 - m[5] * A0323 + m[7] * A0123);
            inv[9] = invDet * -(m[0] * A1323 - m[1] * A0323 + m[3] * A0123);
            inv[10] = invDet * (m[0] * A1313 - m[1] * A0313 + m[3] * A0113);
            inv[11] = invDet * -(m[0] * A1312 - m[1] * A0312 + m[3] * A0112);
        }
        const bool has = pose_length(px, py, pz) > 0.001f || pose_length(rx, ry, rz) > 0.001f || __builtin_fabsf(scx - 1.0f) > 0.001f;
        float *o = out + t * POSE_OUT;
        o[0] = __int_as_float(has ? 1 : 0);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            o[1 + j] = inv[j];
            o[13 + j] = m[j];
            o[25 + j] = (j & 3) == 3 ? 0.0f : inv[(j & 3) * 4 + (j >> 2)]; // (a normal row's fourth word is 0 in the records)
        }
    }
    __syncthreads();
    float *dst = reinterpret_cast<float *>(mesh_recs + (size_t)(first + base) * MESH_REC_F4) + 7;
    for (int i = t; i < here * POSE_OUT; i += POSE_BLOCK) {
        const int r = i / POSE_OUT, k = i - r * POSE_OUT; // word k of this workgroup's instance r
        float *word = dst + (size_t)r * (MESH_REC_F4 * 4) + k;
        float v = out[i];
        if (k == 0)
            v = __int_as_float((__float_as_int(*word) & ~1) | __float_as_int(v)); // (bit 1 belongs to the materials)
        *word = v;
    }
}

// box -> its storage: dst >= 0: child slot (dst & 1) of TLAS inner node (dst >> 1); dst < 0: the TLAS root box
__device__ __forceinline__ void store_tlas_box(float4 *tlas_nodes, float4 *root_box, int dst, float3 lo, float3 hi) {
    if (dst >= 0) {
        float *n = reinterpret_cast<float *>(tlas_nodes + (size_t)(dst >> 1) * 4) + ((dst & 1) ? 6 : 0);
        n[0] = lo.x; n[1] = lo.y; n[2] = lo.z;
        n[3] = hi.x; n[4] = hi.y; n[5] = hi.z;
    } else {
        root_box[0] = make_float4(lo.x, lo.y, lo.z, 0.0f);
        root_box[1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
    }
}

// World-space first-pass box of instance `rec` (PMODE 3): upload_instance_pretests (ptrt_capi.hip) restated for
// the device, same bound, same fp64 (gfx950 has it; this runs once per mesh and refit).  `c2_cap`: the growth
// factor the host hands the trace kernels; an instance whose own factor exceeds it gets the infinite box.
__device__ inline void instance_pretest(const float4 *rec, double c2_cap, float4 *pre) {
    const float big = 3.0e38f;
    float4 p0 = make_float4(-big, -big, -big, 0.0f), p1 = make_float4(big, big, big, 0.0f);
    const float4 h0 = rec[0], h1 = rec[1];
    if (__float_as_int(h1.w) & 1) {
        const double Kc = 1e-4, BIG = 3.0e38;
        const float4 r0 = rec[2], r1 = rec[3], r2 = rec[4];
        const double A[3][3] = {{r0.x, r0.y, r0.z}, {r1.x, r1.y, r1.z}, {r2.x, r2.y, r2.z}};
        const double t[3] = {r0.w, r1.w, r2.w};
        const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
        bool ok = isfinite(det) && fabs(det) > 1e-30;
        const double id = ok ? 1.0 / det : 0.0; // (the host divides each cofactor; the difference is ulps of fp64 under a 1e-4 margin)
        const double I[3][3] = {{(A[1][1] * A[2][2] - A[1][2] * A[2][1]) * id, (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * id,
                                 (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * id},
                                {(A[1][2] * A[2][0] - A[1][0] * A[2][2]) * id, (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * id,
                                 (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * id},
                                {(A[1][0] * A[2][1] - A[1][1] * A[2][0]) * id, (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * id,
                                 (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * id}};
        double nA = 0.0, nI = 0.0;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) {
                nA += A[r][k] * A[r][k];
                nI += I[r][k] * I[r][k];
            }
        nA = sqrt(nA);
        nI = sqrt(nI);
        const double lo[3] = {h0.x, h0.y, h0.z}, hi[3] = {h1.x, h1.y, h1.z};
        double wmin[3] = {BIG, BIG, BIG}, wmax[3] = {-BIG, -BIG, -BIG}, boxn = 0.0, tn = 0.0, wn = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double a = fmax(fabs(lo[k]), fabs(hi[k]));
            boxn += a * a;
            tn += t[k] * t[k];
        }
        boxn = sqrt(boxn);
        tn = sqrt(tn);
        for (int corner = 0; corner < 8; ++corner) {
            const double p[3] = {((corner & 1) ? hi[0] : lo[0]) - t[0], ((corner & 2) ? hi[1] : lo[1]) - t[1],
                                 ((corner & 4) ? hi[2] : lo[2]) - t[2]};
            for (int r = 0; r < 3; ++r) {
                const double x = I[r][0] * p[0] + I[r][1] * p[1] + I[r][2] * p[2];
                ok = ok && isfinite(x);
                wmin[r] = fmin(wmin[r], x);
                wmax[r] = fmax(wmax[r], x);
                wn = fmax(wn, fabs(x));
            }
        }
        const double C1 = Kc * (nI * (tn + boxn) + wn) + 1e-6, C2 = Kc * (nI * nA + 1.0);
        ok = ok && isfinite(C1) && isfinite(C2) && C1 < 1e30 && C2 < 1e3 && C2 <= c2_cap && wn < 1e30;
        if (ok) { // (outward rounding of the double results to float, as on the host)
            p0 = make_float4(nextafterf((float)(wmin[0] - C1), -INFINITY), nextafterf((float)(wmin[1] - C1), -INFINITY),
                             nextafterf((float)(wmin[2] - C1), -INFINITY), 0.0f);
            p1 = make_float4(nextafterf((float)(wmax[0] + C1), INFINITY), nextafterf((float)(wmax[1] + C1), INFINITY),
                             nextafterf((float)(wmax[2] + C1), INFINITY), 0.0f);
        }
    }
    pre[0] = p0;
    pre[1] = p1;
}

// world box of the mesh behind `rec`: its root box as the device holds it through its world rows
__device__ inline void mesh_world_box(const float4 *rec, float3 &lo, float3 &hi) {
    const float4 b0 = rec[0], b1 = rec[1], w0 = rec[5], w1 = rec[6], w2 = rec[7];
    lo = make_float3(1e30f, 1e30f, 1e30f);
    hi = make_float3(-1e30f, -1e30f, -1e30f);
    for (int k = 0; k < 8; ++k) { // the 8 corners through the world matrix, as tlas_root_box and the host do
        const float x = (k & 1) ? b1.x : b0.x, y = (k & 2) ? b1.y : b0.y, z = (k & 4) ? b1.z : b0.z;
        const float px = w0.x * x + w0.y * y + w0.z * z + w0.w;
        const float py = w1.x * x + w1.y * y + w1.z * z + w1.w;
        const float pz = w2.x * x + w2.y * y + w2.z * z + w2.w;
        lo.x = fminf(lo.x, px); lo.y = fminf(lo.y, py); lo.z = fminf(lo.z, pz);
        hi.x = fmaxf(hi.x, px); hi.y = fmaxf(hi.y, py); hi.z = fmaxf(hi.z, pz);
    }
}

// phase a for TLAS index j: world box of its mesh into world[2j..2j+1], first-pass box into pre[2m..2m+1]
__device__ inline void tlas_world_box(const float4 *mesh_recs, const int *tlas_mesh_ids, int j, double c2_cap, float4 *world,
                                      float4 *pre) {
    const int m = tlas_mesh_ids[j];
    const float4 *rec = mesh_recs + (size_t)m * MESH_REC_F4;
    float3 lo, hi;
    mesh_world_box(rec, lo, hi);
    world[2 * j] = make_float4(lo.x, lo.y, lo.z, 0.0f);
    world[2 * j + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
    instance_pretest(rec, c2_cap, pre + 2 * (size_t)m);
}

__global__ __launch_bounds__(TLAS_BLOCK) void tlas_world_boxes_kernel(const float4 *__restrict__ mesh_recs,
                                                                      const int *__restrict__ tlas_mesh_ids, int n_index,
                                                                      float c2_cap, float4 *world, float4 *pre) {
    const int j = blockIdx.x * TLAS_BLOCK + threadIdx.x;
    if (j < n_index)
        tlas_world_box(mesh_recs, tlas_mesh_ids, j, (double)c2_cap, world, pre);
}

// `world`, `tlas_nodes` and `root_box` are written and read again inside the launch: no __restrict__ / const on them, so
// that the reads stay vector loads behind the barrier's workgroup-scope release / acquire (one CU, one L1), as in
// refit_top_levels_kernel.
__global__ __launch_bounds__(TLAS_BLOCK) void refit_tlas_kernel(const float4 *__restrict__ mesh_recs,
                                                                const int *__restrict__ tlas_mesh_ids, int n_index,
                                                                const int2 *__restrict__ tlas_leaves,
                                                                const int *__restrict__ leaf_dst, int n_leaves,
                                                                const int *__restrict__ level_nodes, TopLevels T,
                                                                const int *__restrict__ node_dst, float c2_cap, int do_world,
                                                                float4 *world, float4 *pre, float4 *tlas_nodes, float4 *root_box) {
    if (do_world) {
        for (int j = threadIdx.x; j < n_index; j += TLAS_BLOCK)
            tlas_world_box(mesh_recs, tlas_mesh_ids, j, (double)c2_cap, world, pre);
        __syncthreads();
    }
    for (int l = threadIdx.x; l < n_leaves; l += TLAS_BLOCK) {
        const int2 lf = tlas_leaves[l];
        if (lf.y <= 0)
            continue; // placeholder for an absent child: its box stays unhittable
        float3 lo = make_float3(1e30f, 1e30f, 1e30f), hi = make_float3(-1e30f, -1e30f, -1e30f);
        for (int i = 0; i < lf.y; ++i) {
            const float4 a = world[2 * (lf.x + i)], b = world[2 * (lf.x + i) + 1];
            lo.x = fminf(lo.x, a.x); lo.y = fminf(lo.y, a.y); lo.z = fminf(lo.z, a.z);
            hi.x = fmaxf(hi.x, b.x); hi.y = fmaxf(hi.y, b.y); hi.z = fmaxf(hi.z, b.z);
        }
        store_tlas_box(tlas_nodes, root_box, leaf_dst[l], lo, hi);
    }
    for (int l = 0; l < T.n; ++l) {
        __syncthreads();
        for (int i = threadIdx.x; i < T.count[l]; i += TLAS_BLOCK) {
            const int n = level_nodes[T.begin[l] + i];
            const float4 a = tlas_nodes[(size_t)n * 4 + 0], b = tlas_nodes[(size_t)n * 4 + 1], c = tlas_nodes[(size_t)n * 4 + 2];
            const float3 lo = make_float3(fminf(a.x, b.z), fminf(a.y, b.w), fminf(a.z, c.x));
            const float3 hi = make_float3(fmaxf(a.w, c.y), fmaxf(b.x, c.z), fmaxf(b.y, c.w));
            store_tlas_box(tlas_nodes, root_box, node_dst[n], lo, hi);
        }
    }
}

// ---- re-order (see the head of the file) -------------------------------------------------------------------------------
// centre of mesh m's world box into centres[3m..3m+2], folded into the caller's running bounds (ordered bits)
__device__ inline void tlas_mesh_centre(const float4 *mesh_recs, int m, float *centres, uint32_t tmn[3], uint32_t tmx[3]) {
    float3 lo, hi;
    mesh_world_box(mesh_recs + (size_t)m * MESH_REC_F4, lo, hi);
    const float c[3] = {(lo.x + hi.x) * 0.5f, (lo.y + hi.y) * 0.5f, (lo.z + hi.z) * 0.5f};
    for (int k = 0; k < 3; ++k) {
        centres[(size_t)m * 3 + k] = c[k];
        const uint32_t o = ordered_bits(c[k]);
        tmn[k] = o < tmn[k] ? o : tmn[k];
        tmx[k] = o > tmx[k] ? o : tmx[k];
    }
}

// n_meshes <= TLAS_WIDE (the host launches it for nothing else; a larger count returns at once: `keys` holds TLAS_WIDE).
// `centres` (3 floats per mesh) is written in phase a and read in phase c by the same thread.
__global__ __launch_bounds__(TLAS_BLOCK) void reorder_tlas_kernel(const float4 *__restrict__ mesh_recs, int n_meshes,
                                                                  float *centres, int *__restrict__ tlas_mesh_ids) {
    __shared__ unsigned long long keys[TLAS_WIDE];
    __shared__ uint32_t wave_bounds[TLAS_BLOCK / 64][6];
    if (n_meshes > TLAS_WIDE)
        return;
    uint32_t tmn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, tmx[3] = {0u, 0u, 0u};
    for (int m = threadIdx.x; m < n_meshes; m += TLAS_BLOCK)
        tlas_mesh_centre(mesh_recs, m, centres, tmn, tmx);
    for (int k = 0; k < 3; ++k) {
        uint32_t mn = tmn[k], mx = tmx[k];
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((threadIdx.x & 63) == 0) {
            wave_bounds[threadIdx.x >> 6][k] = mn;
            wave_bounds[threadIdx.x >> 6][3 + k] = mx;
        }
    }
    __syncthreads();
    uint32_t cb[6];
    for (int k = 0; k < 3; ++k) {
        uint32_t mn = wave_bounds[0][k], mx = wave_bounds[0][3 + k];
        for (int w = 1; w < TLAS_BLOCK / 64; ++w) {
            mn = wave_bounds[w][k] < mn ? wave_bounds[w][k] : mn;
            mx = wave_bounds[w][3 + k] > mx ? wave_bounds[w][3 + k] : mx;
        }
        cb[k] = mn;
        cb[3 + k] = mx;
    }
    float lo[3];
    const float ext = bounds_scale(cb, lo);
    int padded = 1;
    while (padded < n_meshes)
        padded <<= 1;
    for (int i = threadIdx.x; i < padded; i += TLAS_BLOCK)
        keys[i] = i < n_meshes ? ((unsigned long long)morton30(centres + (size_t)i * 3, lo, ext) << 32) | (unsigned)i : ~0ull;
    for (int k = 2; k <= padded; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (padded >> 1); t += TLAS_BLOCK) { // pair t of this step: (i, i | j), bit j of i clear
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0)) {
                    keys[i] = b;
                    keys[l] = a;
                }
            }
        }
    __syncthreads();
    for (int j = threadIdx.x; j < n_meshes; j += TLAS_BLOCK)
        tlas_mesh_ids[j] = (int)(uint32_t)keys[j];
}

// beyond TLAS_WIDE meshes: phases a and b as a launch of their own over few workgroups (cbounds as centroid_bounds_kernel's)
__global__ __launch_bounds__(256) void tlas_centres_kernel(const float4 *__restrict__ mesh_recs, int n_meshes,
                                                           float *__restrict__ centres, uint32_t *cbounds) {
    uint32_t tmn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, tmx[3] = {0u, 0u, 0u};
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < n_meshes; m += gridDim.x * blockDim.x)
        tlas_mesh_centre(mesh_recs, m, centres, tmn, tmx);
    block_bounds_to_global(tmn, tmx, cbounds);
}

// ... and phase e: TLAS index j <- the mesh ranked j by the radix sort; cbounds made ready for the next re-order
__global__ __launch_bounds__(256) void tlas_take_order_kernel(const uint32_t *__restrict__ order, int n_meshes,
                                                              int *__restrict__ tlas_mesh_ids, uint32_t *cbounds) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < 6)
        cbounds[j] = j < 3 ? 0xffffffffu : 0u;
    if (j < n_meshes)
        tlas_mesh_ids[j] = (int)order[j];
}

} // namespace pt
