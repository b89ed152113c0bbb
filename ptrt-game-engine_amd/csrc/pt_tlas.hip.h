// pt_tlas.hip.h -- GPU refit of a TLAS with inner nodes over the topology that was uploaded: instances and
// meshes move without a host round trip (ptrt_set_instance_transforms, ptrt_refit_tlas).
//
// The reference rebuilds its TLAS on the CPU whenever a mesh moved (Scene::buildAndUploadTLAS,
// scene.cuh:458-594); it has no refit.  Here the child pairs, leaf ranges and mesh indices of the upload
// stay, and everything that depends on boxes and matrices is derived again on the context's stream:
//   1. scatter_xforms_kernel  the flag bit and nine matrix rows of the meshes a caller moved, from staging
//                             into the mesh records (root boxes untouched)
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
