// pt_probe_sample.hip.h -- the consumer of a probe bake: a regular grid of ptrt_probe records (ptrt_query_probes' output, laid
// out as ptrt_amd.probes.probe_grid orders them) read back at surface points.  probe_light is the one definition (include/ptrt.h
// has it in full); probe_sample_kernel applies it to points and normals that lie in device memory (ptrt_probe_sample),
// probe_light_query_kernel to the hits of its own traversal (ptrt_query_probe_light) -- closest_chunk_loop
// (pt_query.hip.h), the one loop ray_query_kernel<GEOM, PMODE, QUERY_CLOSEST> is, with hit_record's point and normal put
// through probe_light and the 32-byte ProbeLight for a sink in place of the 64-byte hit record, so by construction the second
// equals the first over ptrt_query_rays' records.
//
// The definition in fp32, -ffp-contract=off (every operation rounds on its own), `/` and sqrt the compiler's IEEE ones.  For a
// point P with normal N (used as given), the hit's face f and mesh m:
//   a miss                                                  {0, 0, 0,  0,  -1, 0,  -1, -1}
//   P has a non-finite component                            {0, 0, 0,  0,  -1, 0,   f,  m}     (nothing is loaded)
//   per axis a   g = (P[a] - origin[a]) / spacing[a];  g = min(max(g, 0), (float)(counts[a] - 1));  i0 = (int)floor(g);
//                i1 = min(i0 + 1, counts[a] - 1);  f = g - (float)i0           cell = i0x + nx * (i0y + ny * i0z)
//   B_i = K_i * Y_i(N): Y_i as sh9_basis (pt_probe.hip.h), K_0 = 39.478418f, K_1..3 = 26.318945f, K_4..8 = 9.869604f
//   corner c = 0..7 in order, bit 0 of c: i1 on x, bit 1: on y, bit 2: on z;  wt = (wx*wy)*wz, each factor f or 1 - f.
//     wt <= 0: skipped BY SELECTION and its row is never loaded.
//     TRILINEAR   w = wt
//     VISIBILITY  Q = origin + (float)idx * spacing;  Pb = P + bias * N;  V = Q - Pb;  r2 = (Vx*Vx + Vy*Vy) + Vz*Vz;  r = sqrt(r2);
//                 D = r > 0 ? V / r : 0;  c = ((Dx*Nx + Dy*Ny) + Dz*Nz + 1) * 0.5f;  wf = c*c + 0.2f;
//                 var = |mean_sq - mean*mean|;  wv = r <= mean ? 1 : (ch*ch)*ch with ch = var / (var + d*d), d = r - mean;
//                 w = wf * wv;  w < 0.2f: w = w * ((w*w) / 0.04f);  w = w * wt
//     w not > 0 (a NaN included): skipped by selection.  Otherwise per channel E = (((+0 + B_0*sh[0]) + B_1*sh[1]) .. + B_8*sh[8]),
//     num += w * E, den += w, bit c of `used` set.
//   den > 0: irradiance = num / den with a channel < 0 replaced by +0, weight = den; else zeros.
//   the record                                              {irradiance,  weight,  cell, used,  f,  m}
//
// Memory safety depends on P alone: every row index is formed from i0 and i1, which are conversions of a value already clamped
// into [0, counts - 1]; a non-finite P returns before any index is formed, and the spans were vetted on the host.
//
// A probe row is one 128-byte line of which 29 words are read: seven 16-byte loads (sh, mean_distance) and one word
// (mean_distance_sq).  Eight rows held live at once would be about 240 VGPRs, so the corners go in groups of PROBE_GROUP: the
// loads of a group are issued together, then each row is reduced to E_rgb, mean and mean_sq and the next group follows.
// Groups of 1 -- one row's eight loads in flight -- are the default: groups of 2 cost 24 to 29 VGPRs and a wave per SIMD in four
// of the seven kernels and were no faster anywhere, groups of 4 leave 2 waves (DESIGN.md 3.32 has the listing and the times).
#pragma once
#include "pt_probe.hip.h"
#include "pt_query.hip.h"

namespace pt {

constexpr int PROBES_TRILINEAR = 0, PROBES_VISIBILITY = 1; // == PTRT_PROBES_* (include/ptrt.h)
#ifndef PT_PROBE_GROUP
#define PT_PROBE_GROUP 1
#endif
constexpr int PROBE_GROUP = PT_PROBE_GROUP; // corners whose rows are in flight together: 1, 2, 4 or 8
static_assert(8 % PROBE_GROUP == 0, "the eight corners go in whole groups");

struct ProbeLight { // mirrors ptrt_probe_light, 32 bytes
    float irradiance[3], weight;
    int cell, used, face, mesh;
};

struct ProbeVolumeParams {                // ptrt_probe_volume and the call's scalars, copied into the launch
    const float4 *__restrict__ probes;    // nx * ny * nz rows of 8 float4 (ptrt_probe, 128 bytes)
    float origin[3], spacing[3];
    int counts[3];
    int mode;
    float bias;
};

// The definition.  o0 = {irradiance, weight}, o1 = {cell, used, face, mesh}: the record's two halves.
PT_DEV void probe_light(const ProbeVolumeParams &V, f3 P, f3 N, int face, int mesh, float4 &o0, float4 &o1) {
    o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o1 = make_float4(__int_as_float(-1), __int_as_float(0), __int_as_float(face), __int_as_float(mesh));
    const float inf = __builtin_inff();
    if (!(__builtin_fabsf(P.x) < inf && __builtin_fabsf(P.y) < inf && __builtin_fabsf(P.z) < inf))
        return;
    const float p[3] = {P.x, P.y, P.z};
    int i0[3], i1[3];
    float fr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float top = (float)(V.counts[a] - 1);
        float g = (p[a] - V.origin[a]) / V.spacing[a];
        g = __builtin_fminf(__builtin_fmaxf(g, 0.0f), top); // g is never a NaN: P, origin finite, spacing positive and finite
        const float fl = __builtin_floorf(g);
        i0[a] = (int)fl;                                     // 0 .. counts - 1
        i1[a] = i0[a] + 1 < V.counts[a] - 1 ? i0[a] + 1 : V.counts[a] - 1;
        fr[a] = g - (float)i0[a];
    }
    const int nx = V.counts[0], ny = V.counts[1];
    o1.x = __int_as_float(i0[0] + nx * (i0[1] + ny * i0[2]));

    float B[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
        B[i] = (i == 0 ? 39.478418f : i < 4 ? 26.318945f : 9.869604f) * sh9_basis(i, N);

    const bool vis = V.mode == PROBES_VISIBILITY; // (wave-uniform)
    const f3 Pb = mk3(P.x + V.bias * N.x, P.y + V.bias * N.y, P.z + V.bias * N.z);
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
    int used = 0;
#pragma unroll
    for (int c0 = 0; c0 < 8; c0 += PROBE_GROUP) {
        float4 q[PROBE_GROUP][7];
        float msq[PROBE_GROUP], wt[PROBE_GROUP];
        int ix[PROBE_GROUP], iy[PROBE_GROUP], iz[PROBE_GROUP];
#pragma unroll
        for (int k = 0; k < PROBE_GROUP; ++k) { // the group's loads, issued together
            const int c = c0 + k;
            ix[k] = (c & 1) ? i1[0] : i0[0];
            iy[k] = (c & 2) ? i1[1] : i0[1];
            iz[k] = (c & 4) ? i1[2] : i0[2];
            const float wx = (c & 1) ? fr[0] : 1.0f - fr[0];
            const float wy = (c & 2) ? fr[1] : 1.0f - fr[1];
            const float wz = (c & 4) ? fr[2] : 1.0f - fr[2];
            wt[k] = (wx * wy) * wz;
            msq[k] = 0.0f;
#pragma unroll
            for (int j = 0; j < 7; ++j)
                q[k][j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (wt[k] > 0.0f) {
                const float4 *row = V.probes + (size_t)(ix[k] + nx * (iy[k] + ny * iz[k])) * 8;
#pragma unroll
                for (int j = 0; j < 7; ++j)
                    q[k][j] = row[j];
                if (vis)
                    msq[k] = reinterpret_cast<const float *>(row)[28];
            }
        }
#pragma unroll
        for (int k = 0; k < PROBE_GROUP; ++k) {
            if (!(wt[k] > 0.0f))
                continue;
            float w = wt[k];
            if (vis) {
                const float mean = q[k][6].w;
                const float qx = V.origin[0] + (float)ix[k] * V.spacing[0];
                const float qy = V.origin[1] + (float)iy[k] * V.spacing[1];
                const float qz = V.origin[2] + (float)iz[k] * V.spacing[2];
                const float vx = qx - Pb.x, vy = qy - Pb.y, vz = qz - Pb.z;
                const float r2 = (vx * vx + vy * vy) + vz * vz;
                const float r = __builtin_sqrtf(r2);
                const bool apart = r > 0.0f;
                const float dx = apart ? vx / r : 0.0f, dy = apart ? vy / r : 0.0f, dz = apart ? vz / r : 0.0f;
                const float cs = (((dx * N.x + dy * N.y) + dz * N.z) + 1.0f) * 0.5f;
                const float wf = cs * cs + 0.2f;
                const float var = __builtin_fabsf(msq[k] - mean * mean);
                float wv = 1.0f;
                if (!(r <= mean)) {
                    const float d = r - mean;
                    const float ch = var / (var + d * d);
                    wv = (ch * ch) * ch;
                }
                w = wf * wv;
                if (w < 0.2f)
                    w = w * ((w * w) / 0.04f);
                w = w * wt[k];
            }
            if (!(w > 0.0f))
                continue;
            const float s[28] = {q[k][0].x, q[k][0].y, q[k][0].z, q[k][0].w, q[k][1].x, q[k][1].y, q[k][1].z, q[k][1].w,
                                 q[k][2].x, q[k][2].y, q[k][2].z, q[k][2].w, q[k][3].x, q[k][3].y, q[k][3].z, q[k][3].w,
                                 q[k][4].x, q[k][4].y, q[k][4].z, q[k][4].w, q[k][5].x, q[k][5].y, q[k][5].z, q[k][5].w,
                                 q[k][6].x, q[k][6].y, q[k][6].z, q[k][6].w};
            float er = 0.0f, eg = 0.0f, eb = 0.0f;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                er = er + B[i] * s[i * 3 + 0];
                eg = eg + B[i] * s[i * 3 + 1];
                eb = eb + B[i] * s[i * 3 + 2];
            }
            nr = nr + w * er;
            ng = ng + w * eg;
            nb = nb + w * eb;
            den = den + w;
            used |= 1 << (c0 + k);
        }
    }
    o1.y = __int_as_float(used);
    if (den > 0.0f) {
        const float r = nr / den, g = ng / den, b = nb / den;
        o0 = make_float4(r < 0.0f ? 0.0f : r, g < 0.0f ? 0.0f : g, b < 0.0f ? 0.0f : b, den);
    }
}

// ptrt_probe_sample: one thread per point, the 32-byte record written as two 16-byte words; face and mesh are -1.
__global__ __launch_bounds__(256) void probe_sample_kernel(const float *__restrict__ positions, const float *__restrict__ normals,
                                                           size_t n, const ProbeVolumeParams V, float4 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const f3 P = mk3(positions[i * 3], positions[i * 3 + 1], positions[i * 3 + 2]);
    const f3 N = mk3(normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2]);
    float4 o0, o1;
    probe_light(V, P, N, -1, -1, o0, o1);
    out[i * 2 + 0] = o0;
    out[i * 2 + 1] = o1;
}

// ptrt_query_probe_light: closest_chunk_loop (pt_query.hip.h) -- the persistent grid of one-wave workgroups, the LDS carve and
// staging by PMODE, the closest-hit walk, winner_uv for the pair walks -- with hit_record, of which the point, the face-forwarded
// normal, the face and the mesh are kept, and probe_light for a sink.
struct HitToProbeLight {
    const KParams &K;
    const ProbeVolumeParams &V;
    float4 *out;
    PT_DEV void operator()(size_t i, const Hit &h, f3 o, f3 d) const {
        const HitOut r = hit_record(K, h, o, d);
        float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 o1 = make_float4(__int_as_float(-1), __int_as_float(0), __int_as_float(-1), __int_as_float(-1));
        if (r.hit)
            probe_light(V, mk3(r.point[0], r.point[1], r.point[2]), mk3(r.normal[0], r.normal[1], r.normal[2]), r.face_index,
                        r.mesh_index, o0, o1);
        out[i * 2 + 0] = o0;
        out[i * 2 + 1] = o1;
    }
};
template <int GEOM, int PMODE>
__global__ __launch_bounds__(64) void probe_light_query_kernel(const KParams K, const float *__restrict__ origins,
                                                               const float *__restrict__ dirs, size_t n, const ProbeVolumeParams V,
                                                               float4 *__restrict__ out) {
    extern __shared__ uint2 lds_raw[];
    const int lane = threadIdx.x;
    const LdsStack stk{lds_raw + lane};
    CycleAcc cyc;
    const PairLds PL = query_stage<PMODE>(K, lds_raw, lane, cyc);
    closest_chunk_loop<GEOM, PMODE>(K, PL, stk, cyc, lane, origins, dirs, n, HitToProbeLight{K, V, out});
}

} // namespace pt
