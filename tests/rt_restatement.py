"""CPU restatement of the one-bounce ray tracer (render_kernel of the reference's src/raytracer/RTscene.cuh:1240-1293,
as csrc/rt_render.hip.h runs it) for the exact comparisons of tests/test_rt_gpu.py.

Input is `Scene.snapshot()` of ptrt_amd.rt: the vertices, faces, trees, descriptors, lights and view the GPU was
given.  numpy float32 in the reference's operation order: every product and sum is one rounded float32 operation, as
in the kernel's -ffp-contract=off build; dot and cross are the fused forms of the numerics contract (`fma32`, from
wireframe_restatement); divisions and square roots are IEEE float32; __powf, __sincosf and __cosf are the oracle's
det_pow / det_sin / det_cos (oracle.detmath ops 4, 0, 1), which equal the device's bit for bit.  fmaxf / fminf are
NaN-ignoring (`mx`, `mn`), like the kernel's max_ / min_.

Decisions shared with the kernel (documented in DESIGN.md 3.14): powf(x, y) for x <= 0 or NaN is 0 (Beer-Lambert of a
zero albedo channel, gamma of black or of a NaN), and a NaN colour channel ends as 0 in the final clamp.

The traversal is the reference's, per mesh, vectorised over rays: bvh_trace's near-first walk with a fresh best t of
1e30 per mesh and pushes dropped when the 32-entry stack is full; bvh_any_hit's unordered walk with the same rule.
"""
import numpy as np

from wireframe_restatement import fma32

f32 = np.float32
PI = f32(3.14159265358979323846)
TWO_PI = f32(6.28318530717958647692)
INV_PI = f32(0.31830988618379067154)
STACK = 32
GAMMA = f32(0.4545454545)


def mx(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.where((a > b) | (b != b), a, b).astype(f32)


def mn(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.where((a < b) | (b != b), a, b).astype(f32)


def V(x):
    return np.asarray(x, dtype=f32)


def dot(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross(a, b):
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                     fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1).astype(f32)


def length(v):
    return np.sqrt(dot(v, v)).astype(f32)


def normalize(v):
    ln = length(v)
    ok = ln > 0
    safe = np.where(ok, ln, f32(1))[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok[..., None], v / safe, f32(0)).astype(f32)


def lerp(a, b, t):
    t = V(t)
    if t.ndim == 1:
        t = t[:, None]
    return ((f32(1.0) - t) * a + t * b).astype(f32)


def mat_mul(m, v):
    """m (3, 3) row-major times v (n, 3), each row ((m0 x + m1 y) + m2 z) with rounded products."""
    return np.stack([(m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]) + m[i, 2] * v[:, 2] for i in range(3)], axis=1).astype(f32)


def safe_inv(d):
    with np.errstate(divide="ignore"):
        return np.where(np.abs(d) > f32(1e-8), f32(1.0) / np.where(d == 0, f32(1), d),
                        np.where(d >= 0, f32(1e30), f32(-1e30))).astype(f32)


class MeshData:
    def __init__(self, m):
        v, f = V(m["vertices"]), np.asarray(m["faces"], np.int64)
        self.face_count, self.node_count = len(f), len(m["left"])
        self.ok = self.face_count > 0 and self.node_count > 0
        if len(f):
            self.v0 = v[f[:, 0]]
            self.e1 = (v[f[:, 1]] - self.v0).astype(f32)
            self.e2 = (v[f[:, 2]] - self.v0).astype(f32)
        self.bmin, self.bmax = V(m["bmin"]), V(m["bmax"])
        self.left, self.right = np.asarray(m["left"], np.int64), np.asarray(m["right"], np.int64)
        self.start, self.count = np.asarray(m["start"], np.int64), np.asarray(m["count"], np.int64)
        self.prims = np.asarray(m["prims"], np.int64)
        self.T, self.R, self.Ri = V(m["translation"]), V(m["rotation"]), V(m["inv_rotation"])
        self.mat = m["material"]
        self.transmission = f32(self.mat.transmission)

    def local(self, o, d):
        lo = mat_mul(self.Ri, (o - self.T).astype(f32))
        ld = mat_mul(self.Ri, d)
        return lo, ld, np.stack([safe_inv(ld[:, k]) for k in range(3)], axis=1)

    def box(self, node, o, inv, tmax):
        """AABB::hit_fast for rays (o, inv) against nodes `node`: (hit, tmin)."""
        lo, hi = self.bmin[node], self.bmax[node]
        t1 = (lo - o) * inv
        t2 = (hi - o) * inv
        tmin, tmax_ = mn(t1[:, 0], t2[:, 0]), mx(t1[:, 0], t2[:, 0])
        for k in (1, 2):
            tmin = mx(tmin, mn(t1[:, k], t2[:, k]))
            tmax_ = mn(tmax_, mx(t1[:, k], t2[:, k]))
        tmin = mx(tmin, f32(1e-4))
        return (tmax_ >= tmin) & (tmin < tmax), tmin

    def tri(self, face, o, d):
        """intersect_triangle_mt: (ok, t) with ok requiring t > 1e-4."""
        v0, e1, e2 = self.v0[face], self.e1[face], self.e2[face]
        with np.errstate(all="ignore"):
            h = cross(d, e2)
            a = dot(e1, h)
            ok = ~(np.abs(a) < f32(1e-8))
            f = (f32(1.0) / a).astype(f32)
            s = (o - v0).astype(f32)
            u = f * dot(s, h)
            ok &= ~((u < 0) | (u > 1))
            q = cross(s, e1)
            v = f * dot(d, q)
            ok &= ~((v < 0) | (u + v > 1))
            t = (f * dot(e2, q)).astype(f32)
        return ok & (t > f32(1e-4)), t


def closest(M, o, d):
    """bvh_trace of one mesh for rays (o, d): (t, face) with face -1 where nothing was hit."""
    n = o.shape[0]
    lo, ld, inv = M.local(o, d)
    mt = np.full(n, f32(1e30), f32)
    mface = np.full(n, -1, np.int64)
    ni = np.zeros(n, np.int64)
    sp = np.zeros(n, np.int64)
    stack = np.zeros((n, STACK), np.int64)
    alive = np.ones(n, bool)
    while alive.any():
        s = np.nonzero(alive)[0]
        node = ni[s]
        hit, _ = M.box(node, lo[s], inv[s], mt[s])
        leaf = M.count[node] > 0
        pop = ~hit
        L = hit & leaf
        if L.any():
            r = s[L]
            nd = node[L]
            cnt, st = M.count[nd], M.start[nd]
            for k in range(int(cnt.max())):
                kk = k < cnt
                rr = r[kk]
                face = M.prims[st[kk] + k]
                ok, t = M.tri(face, lo[rr], ld[rr])
                better = ok & (t < mt[rr])
                mt[rr[better]] = t[better]
                mface[rr[better]] = face[better]
            pop |= L
        I = hit & ~leaf
        if I.any():
            r = s[I]
            nd = node[I]
            Lc, Rc = M.left[nd], M.right[nd]
            hL = np.zeros(len(r), bool)
            hR = np.zeros(len(r), bool)
            tL = np.full(len(r), f32(1e30), f32)
            tR = np.full(len(r), f32(1e30), f32)
            for c, hh, tt in ((Lc, hL, tL), (Rc, hR, tR)):
                g = c >= 0
                if g.any():
                    h2, t2 = M.box(c[g], lo[r[g]], inv[r[g]], mt[r[g]])
                    hh[g] = h2
                    tt[g] = t2
            both = hL & hR
            lfirst = tL <= tR
            push = both & (sp[r] < STACK)
            pr = r[push]
            stack[pr, sp[pr]] = np.where(lfirst[push], Rc[push], Lc[push])
            sp[pr] += 1
            nxt = np.where(both, np.where(lfirst, Lc, Rc), np.where(hL, Lc, Rc))
            ni[r] = nxt
            none = ~hL & ~hR
            popI = np.zeros(len(s), bool)
            popI[np.nonzero(I)[0][none]] = True
            pop |= popI
        ps = s[pop]
        empty = sp[ps] == 0
        alive[ps[empty]] = False
        q = ps[~empty]
        sp[q] -= 1
        ni[q] = stack[q, sp[q]]
    return mt, mface


def any_hit(M, o, d, tmax):
    """bvh_any_hit of one mesh: bool per ray."""
    n = o.shape[0]
    lo, ld, inv = M.local(o, d)
    found = np.zeros(n, bool)
    sp = np.ones(n, np.int64)
    stack = np.zeros((n, STACK), np.int64)
    alive = np.ones(n, bool)
    while alive.any():
        s = np.nonzero(alive)[0]
        sp[s] -= 1
        node = stack[s, sp[s]]
        hit, _ = M.box(node, lo[s], inv[s], tmax[s])
        leaf = M.count[node] > 0
        L = hit & leaf
        if L.any():
            r = s[L]
            nd = node[L]
            cnt, st = M.count[nd], M.start[nd]
            got = np.zeros(len(r), bool)
            for k in range(int(cnt.max())):
                kk = (k < cnt) & ~got
                if not kk.any():
                    continue
                rr = r[kk]
                ok, t = M.tri(M.prims[st[kk] + k], lo[rr], ld[rr])
                g = ok & (t < tmax[rr])
                idx = np.nonzero(kk)[0][g]
                got[idx] = True
            found[r[got]] = True
            alive[r[got]] = False
        I = hit & ~leaf
        if I.any():
            r = s[I]
            nd = node[I]
            for c in (M.left[nd], M.right[nd]):
                g = (c >= 0) & (sp[r] < STACK)
                rr = r[g]
                stack[rr, sp[rr]] = c[g]
                sp[rr] += 1
        done = s[alive[s] & (sp[s] == 0)]
        alive[done] = False
    return found


def trace(meshes, o, d):
    """traceRay: (hit, t, mesh, face); a strictly smaller t replaces the best."""
    n = o.shape[0]
    bt = np.full(n, f32(1e30), f32)
    bm = np.full(n, -1, np.int64)
    bf = np.full(n, -1, np.int64)
    for mi, M in enumerate(meshes):
        if not M.ok or n == 0:
            continue
        t, face = closest(M, o, d)
        better = (face >= 0) & (t < bt)
        bt[better], bm[better], bf[better] = t[better], mi, face[better]
    return bm >= 0, bt, bm, bf


def pos_pow(x, y, O):
    x = V(x)
    out = np.zeros_like(x)
    p = x > 0
    if p.any():
        yy = np.broadcast_to(V(y), x.shape)[p]
        out[p] = O.detmath(4, x[p], np.ascontiguousarray(yy))
    return out


def fresnel(c, F0):
    x = f32(1.0) - c
    x2 = x * x
    x5 = x2 * x2 * x
    return (F0 + (f32(1.0) - F0) * x5[:, None]).astype(f32)


def ggx_d(N, H, r):
    a = r * r
    a2 = a * a
    NdotH = mx(dot(N, H), f32(0))
    denom = NdotH * NdotH * (a2 - f32(1)) + f32(1)
    denom = PI * denom * denom
    return (a2 / mx(denom, f32(0.001))).astype(f32)


def ggx_g1(NdotV, r):
    rr = r + f32(1)
    k = (rr * rr) * f32(0.125)
    return (NdotV / (NdotV * (f32(1) - k) + k + f32(0.001))).astype(f32)


def ggx_g(N, Vv, L, r):
    return ggx_g1(mx(dot(N, Vv), f32(0)), r) * ggx_g1(mx(dot(N, L), f32(0)), r)


def tangent_frame(N):
    z = np.zeros_like(N)
    z[:, 2] = 1
    x = np.zeros_like(N)
    x[:, 0] = 1
    T = np.where((np.abs(N[:, 2]) < f32(0.9999))[:, None], normalize(cross(z, N)), normalize(cross(x, N)))
    return T, cross(N, T)


def iridescence(thick, c, O):
    c = mn(mx(c, f32(0)), f32(1))
    sinT = np.sqrt(f32(1) - c * c)
    sf = sinT / f32(1.3)
    out = np.ones((len(c), 3), f32)
    ok = ~(sf * sf > 1)
    cf = np.sqrt(np.where(ok, f32(1) - sf * sf, f32(0))).astype(f32)
    OPD = f32(2.0) * f32(1.3) * thick * cf
    Ra = (f32(1) - f32(1.3)) / (f32(1) + f32(1.3))
    Ra = Ra * Ra
    Rb = (f32(1.3) - f32(1.5)) / (f32(1.3) + f32(1.5))
    Rb = Rb * Rb
    s12 = np.sqrt(Ra * Rb)
    Rmax = np.sqrt(Ra) + np.sqrt(Rb)
    Rmax = Rmax * Rmax
    den = Rmax + f32(1e-6)
    for i, lam in enumerate((f32(650), f32(550), f32(450))):
        delta = (TWO_PI * OPD / lam).astype(f32)
        r = Ra + Rb + f32(2) * s12 * O.detmath(1, delta)
        out[:, i] = np.where(ok, mn(mx(r / den, f32(0)), f32(1)), f32(1))
    return out


def perturb(dirs, rough, seed, O):
    with np.errstate(over="ignore"):
        seed = seed * np.uint32(747796405) + np.uint32(2891336453)
        u1 = seed.astype(f32) * f32(2.3283064365386963e-10)
        seed = seed * np.uint32(747796405) + np.uint32(2891336453)
        u2 = seed.astype(f32) * f32(2.3283064365386963e-10)
    a = rough * rough
    phi = TWO_PI * u1
    cosT = np.sqrt((f32(1) - u2) / (f32(1) + (a * a - f32(1)) * u2)).astype(f32)
    sinT = np.sqrt(f32(1) - cosT * cosT).astype(f32)
    T, B = tangent_frame(dirs)
    sp, cp = O.detmath(0, phi), O.detmath(1, phi)
    v = T * (cp * sinT)[:, None] + B * (sp * sinT)[:, None] + dirs * cosT[:, None]
    return normalize(v.astype(f32)), seed


def mat_arrays(meshes, idx):
    """Material fields of meshes[idx] as arrays."""
    def g(name, vec):
        vals = [getattr(M.mat, name) for M in meshes]
        a = V(vals)
        return a[idx].reshape(len(idx), 3) if vec else a[idx]
    names = {"albedo": 1, "specular": 1, "metallic": 0, "roughness": 0, "emission": 1, "ior": 0, "transmission": 0,
             "transmission_roughness": 0, "clearcoat": 0, "clearcoat_roughness": 0, "subsurface_color": 1,
             "subsurface_radius": 0, "anisotropy": 0, "sheen": 0, "sheen_tint": 1, "iridescence": 0,
             "iridescence_thickness": 0}
    return {k: g(k, v) for k, v in names.items()}


def shade_direct(meshes, lights, ambient, m, P, Ng, t, d, allow, O, detail=None):
    """The direct part of calculatePBRLightingCore for hits with material arrays m.  `detail` (a dict) receives what is
    computed on the way: "amb" (the ambient term) and, per light, "Lo" (zero where shadowed), "shadow", and the terms of Lo
    whether shadowed or not: "D", "G", "Fs" (Fresnel after the iridescence blend), "kD", "dif" (the diffuse colour) and
    "ccB" (the clearcoat BRDF, zero without clearcoat)."""
    n = len(t)
    Vv = -d
    rough = mn(mx(m["roughness"], f32(0.02)), f32(1))
    metal = mn(mx(m["metallic"], f32(0)), f32(1))
    glass = (m["transmission"] > 0) & (metal < f32(0.1))
    F0 = lerp(m["specular"], m["albedo"], metal)
    color = (f32(0) + m["emission"]).astype(f32)
    NdotV = mx(dot(Ng, Vv), f32(0))
    x = mx(f32(1) - NdotV, f32(0))
    x2 = x * x
    x5 = x2 * x2 * x
    mr = (f32(1) - rough)[:, None]
    maxRefl = mx(np.broadcast_to(mr, F0.shape), F0)
    Famb = (F0 + (maxRefl - F0) * x5[:, None]).astype(f32)
    kDa = ((f32(1) - Famb) * (f32(1) - metal)[:, None]).astype(f32)
    kDa[glass] = 0
    color = (color + kDa * m["albedo"] * V(ambient)).astype(f32)
    if detail is not None:
        detail.update(amb=(kDa * m["albedo"] * V(ambient)).astype(f32), Lo=np.zeros((n, len(lights), 3), f32),
                      shadow=np.zeros((n, len(lights)), bool), D=np.zeros((n, len(lights)), f32),
                      G=np.zeros((n, len(lights)), f32), Fs=np.zeros((n, len(lights), 3), f32),
                      kD=np.zeros((n, len(lights), 3), f32), dif=np.zeros((n, len(lights), 3), f32),
                      ccB=np.zeros((n, len(lights), 3), f32))
    eps = f32(1e-3) * mx(f32(1), t)
    so = (P + Ng * eps[:, None]).astype(f32)
    for li, lt in enumerate(lights):
        ltype = lt.type
        lpos = V([lt.position.x, lt.position.y, lt.position.z])
        ldir = V([lt.direction.x, lt.direction.y, lt.direction.z])
        lcol = V([lt.color.x, lt.color.y, lt.color.z])
        if ltype == 1:
            L = np.broadcast_to(-ldir, (n, 3)).astype(f32)
            att = np.ones(n, f32)
            ldist = np.full(n, f32(1e30), f32)
        else:
            toL = (lpos - P).astype(f32)
            dist = length(toL)
            L = (toL / mx(dist, f32(1e-6))[:, None]).astype(f32)
            r = f32(lt.range)
            a = r / (r + dist)
            att = (a * a).astype(f32)
            if ltype == 2:
                theta = dot(L, np.broadcast_to(-ldir, (n, 3)))
                e = f32(lt.inner_cone) - f32(lt.outer_cone)
                with np.errstate(all="ignore"):
                    sp = mn(mx((theta - f32(lt.outer_cone)) / e, f32(0)), f32(1))
                att = (att * sp).astype(f32)
            ldist = dist
        shadow = np.zeros(n, bool)
        for M in meshes:
            if M.transmission > 0 or not M.ok:
                continue
            q = np.nonzero(~shadow)[0]
            if len(q):
                shadow[q] = any_hit(M, so[q], L[q], ldist[q])
        lit = ~shadow
        with np.errstate(all="ignore"):
            H = normalize((L + Vv).astype(f32))
            NdotL = mx(dot(Ng, L), f32(0))
            VdotH = mx(dot(Vv, H), f32(0))
            D = ggx_d(Ng, H, rough)
            G = ggx_g(Ng, Vv, L, rough)
            an = np.abs(m["anisotropy"]) > f32(0.01)
            if an.any():
                T, B = tangent_frame(Ng)
                r2 = rough * rough
                aspect = np.sqrt(f32(1) - f32(0.9) * np.abs(m["anisotropy"])).astype(f32)
                pos = m["anisotropy"] >= 0
                ax = mx(np.where(pos, r2 / aspect, r2 * aspect), f32(0.001))
                ay = mx(np.where(pos, r2 * aspect, r2 / aspect), f32(0.001))
                NdotH = dot(Ng, H)
                TdotH, BdotH = dot(T, H), dot(B, H)
                ax2, ay2 = ax * ax, ay * ay
                den = (TdotH * TdotH / ax2) + (BdotH * BdotH / ay2) + (NdotH * NdotH)
                den = PI * ax * ay * den * den
                Da = np.where(NdotH <= 0, f32(0), f32(1) / mx(den, f32(0.001)))

                def g1(nv, tv, bv):
                    lam = np.sqrt(ax2 * tv * tv + ay2 * bv * bv + nv * nv)
                    return f32(2) * nv / (nv + lam + f32(0.001))
                nv, nl = mx(dot(Ng, Vv), f32(0)), mx(dot(Ng, L), f32(0))
                Ga = g1(nv, dot(T, Vv), dot(B, Vv)) * g1(nl, dot(T, L), dot(B, L))
                D = np.where(an, Da, D).astype(f32)
                G = np.where(an, Ga, G).astype(f32)
            F = fresnel(VdotH, F0)
            ir = m["iridescence"] > 0
            if ir.any():
                irc = iridescence(m["iridescence_thickness"], VdotH, O)
                F = np.where(ir[:, None], lerp(F, F * irc, m["iridescence"]), F).astype(f32)
            spec = ((D * G)[:, None] * F / ((f32(4) * mx(dot(Ng, Vv), f32(0)) * NdotL + f32(0.001))[:, None])).astype(f32)
            kD = ((f32(1) - F) * (f32(1) - metal)[:, None]).astype(f32)
            diffuse = (m["albedo"] * INV_PI).astype(f32)
            sh = m["sheen"] > 0
            if sh.any():
                xx = f32(1) - VdotH
                xx2 = xx * xx
                FH = xx2 * xx2 * xx
                sc = lerp(np.ones_like(F), m["sheen_tint"], FH)
                kD = np.where(sh[:, None], kD + sc * m["sheen"][:, None] * (f32(1) - metal)[:, None], kD).astype(f32)
            ss = m["subsurface_radius"] > 0
            if ss.any():
                sss = mx(dot(Vv, -L), f32(0))
                sss = sss * sss * m["subsurface_radius"]
                diffuse = np.where(ss[:, None], lerp(diffuse, m["subsurface_color"] * INV_PI, sss), diffuse).astype(f32)
            thin = np.zeros_like(F)
            if not allow:
                kD[glass] = 0
                thin = np.where(glass[:, None], (f32(1) - F) * m["transmission"][:, None], thin).astype(f32)
            Lo = ((((((kD * diffuse + spec) + thin) * lcol) * f32(lt.intensity)) * f32(20)) * NdotL[:, None]) * att[:, None]
            Lo = Lo.astype(f32)
            if detail is not None:
                for k, v in (("D", D), ("G", G), ("Fs", F), ("kD", kD), ("dif", diffuse)):
                    detail[k][:, li] = v
            cc = m["clearcoat"] > 0
            if cc.any():
                ccr = m["clearcoat_roughness"]
                ccD = ggx_d(Ng, H, ccr)
                ccG = ggx_g(Ng, Vv, L, ccr)
                ccF = fresnel(VdotH, np.full_like(F, f32(0.04)))
                ccB = ((ccD * ccG)[:, None] * ccF / ((f32(4) * mx(dot(Ng, Vv), f32(0)) * NdotL + f32(0.001))[:, None]))
                ccw = m["clearcoat"][:, None]
                Lcc = Lo * (f32(1) - ccw * ccF) + (((((ccB * lcol) * f32(lt.intensity)) * f32(20)) * NdotL[:, None]) *
                                                    att[:, None]) * ccw
                Lo = np.where(cc[:, None], Lcc, Lo).astype(f32)
                if detail is not None:
                    detail["ccB"][:, li] = np.where(cc[:, None], ccB, f32(0))
        color = np.where(lit[:, None], color + Lo, color).astype(f32)
        if detail is not None:
            detail["Lo"][:, li] = np.where(lit[:, None], Lo, f32(0))
            detail["shadow"][:, li] = shadow
    return color


def sky(view, d):
    if not view.use_sky:
        return np.zeros((len(d), 3), f32)
    top = V([view.sky_top.x, view.sky_top.y, view.sky_top.z])
    bot = V([view.sky_bottom.x, view.sky_bottom.y, view.sky_bottom.z])
    return lerp(bot[None, :], top[None, :], f32(0.5) * (d[:, 1] + f32(1)))


def shade_segment(meshes, lights, view, o, d, allow, O, counts=None, detail=None):
    """closest hit + direct shading (or the sky): (colour, hit, t, material arrays, point, normal).  `detail` (a dict)
    receives the segment's records over all its rays: hit, t, mesh, face, point, normal, linear, and shade_direct's
    amb, Lo, shadow, D, G, Fs, kD, dif, ccB."""
    hit, t, mi, face = trace(meshes, o, d)
    c = sky(view, d)
    h = np.nonzero(hit)[0]
    if counts is not None:
        counts["shadow"] += len(h) * len(lights)
    P = Ng = m = None
    if len(h):
        th = t[h]
        P = (o[h] + th[:, None] * d[h]).astype(f32)
        Ng = np.zeros((len(h), 3), f32)
        for k in np.unique(mi[h]):
            sel = mi[h] == k
            M = meshes[k]
            fc = face[h][sel]
            nl = normalize(cross(M.e1[fc], M.e2[fc]))
            Ng[sel] = normalize(mat_mul(M.R, nl))
        m = mat_arrays(meshes, mi[h])
        amb = V([view.ambient.x, view.ambient.y, view.ambient.z])
        dd = None if detail is None else {}
        c[h] = shade_direct(meshes, lights, amb, m, P, Ng, th, d[h], allow, O, dd)
    if detail is not None:
        n, nl = len(t), len(lights)
        detail.update(hit=hit, t=np.where(hit, t, f32(0)), mesh=np.where(hit, mi, -1), face=np.where(hit, face, -1),
                      point=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32), linear=c.copy(),
                      amb=np.zeros((n, 3), f32), Lo=np.zeros((n, nl, 3), f32), shadow=np.zeros((n, nl), bool),
                      D=np.zeros((n, nl), f32), G=np.zeros((n, nl), f32), Fs=np.zeros((n, nl, 3), f32),
                      kD=np.zeros((n, nl, 3), f32), dif=np.zeros((n, nl, 3), f32), ccB=np.zeros((n, nl, 3), f32))
        if len(h):
            detail["point"][h], detail["normal"][h] = P, Ng
            for k in ("amb", "Lo", "shadow", "D", "G", "Fs", "kD", "dif", "ccB"):
                detail[k][h] = dd[k]
    return c, hit, t, h, m, P, Ng


def render(snap, W, H, O, counts=None, detail=None):
    """The image of rt_render_kernel for `snap` (Scene.snapshot()) as (H, W, 3) uint8 in the buffer's bottom-up order.
    `counts` (a dict) receives the rays the frame traces: "primary" (one per pixel), "shadow" (one per light at every
    shaded hit, whatever the light's contribution), "reflection" and "refraction" (glass pixels; no refraction ray
    under total internal reflection).  `detail` (a dict) receives what the frame computes on the way, per pixel in the
    order y * W + x of the kernel's threads: "dir", the segments' records "0", "R", "T" (see shade_segment; R and T over
    "glass" pixels, T over those with "refr_ok"), "Fr", "Rdir", "Tdir", "thickness", "seed" (before the first draw),
    "linear" (before Reinhard) and "final" (after gamma, before the clamp)."""
    if counts is not None:
        counts.update(primary=W * H, shadow=0, reflection=0, refraction=0)
    meshes = [MeshData(m) for m in snap["meshes"]]
    lights, view = snap["lights"], snap["view"]
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    x, y = xs.reshape(-1), ys.reshape(-1)
    u = (x.astype(f32) + f32(0.5)) * (f32(1) / f32(W))
    v = f32(1) - (y.astype(f32) + f32(0.5)) * (f32(1) / f32(H))
    cmo = V([view.corner_minus_origin.x, view.corner_minus_origin.y, view.corner_minus_origin.z])
    hor = V([view.horizontal.x, view.horizontal.y, view.horizontal.z])
    ver = V([view.vertical.x, view.vertical.y, view.vertical.z])
    org = V([view.origin.x, view.origin.y, view.origin.z])
    d = normalize(((cmo + u[:, None] * hor) + v[:, None] * ver).astype(f32))
    o = np.broadcast_to(org, d.shape).astype(f32)
    want = detail is not None
    d0 = {} if want else None
    color, hit, t, h, m, P, Ng = shade_segment(meshes, lights, view, o, d, True, O, counts, d0)
    if want:
        n = W * H
        detail.update({"dir": d, "0": d0, "glass": np.zeros(n, bool), "refr_ok": np.zeros(n, bool),
                       "Fr": np.zeros((n, 3), f32), "Rdir": np.zeros((n, 3), f32), "Tdir": np.zeros((n, 3), f32),
                       "thickness": np.zeros(n, f32), "seed": np.zeros(n, np.uint32), "R": None, "T": None})
    if len(h):
        metal = mn(mx(m["metallic"], f32(0)), f32(1))
        gl = (m["transmission"] > 0) & (metal < f32(0.1))
        if gl.any():
            g = h[gl]
            I = d[g]
            Ngg, Pg = Ng[gl], P[gl]
            ior = m["ior"][gl]
            NgI = dot(Ngg, I)
            Nf = np.where((NgI < 0)[:, None], Ngg, -Ngg).astype(f32)
            n1 = np.where(NgI > 0, ior, f32(1))
            n2 = np.where(NgI > 0, f32(1), ior)
            eta = (n1 / n2).astype(f32)
            F0s = (n2 - n1) / (n2 + n1)
            F0s = F0s * F0s
            cosT = mx(dot(-I, Nf), f32(0))
            Fr = fresnel(cosT, np.repeat(F0s[:, None], 3, axis=1))
            eps = f32(1e-3) * mx(f32(1), t[g])
            seed = (Pg[:, 0] * f32(12.9898) + Pg[:, 1] * f32(78.233) + Pg[:, 2] * f32(45.164)).astype(f32).view(np.uint32)
            with np.errstate(over="ignore"):
                seed = seed * np.uint32(747796405) + np.uint32(2891336453)
            if want:
                detail["seed"][g] = seed
            Rdir = normalize((I - (f32(2) * dot(I, Nf))[:, None] * Nf).astype(f32))
            rr = mx(m["roughness"][gl], m["transmission_roughness"][gl])
            pr = rr > f32(0.02)
            if pr.any():
                nd, ns = perturb(Rdir[pr], rr[pr], seed[pr], O)
                Rdir[pr], seed[pr] = nd, ns
            NdotI = dot(Nf, I)
            k = f32(1) - eta * eta * (f32(1) - NdotI * NdotI)
            ok = ~(k < 0)
            Tdir = np.zeros_like(I)
            with np.errstate(invalid="ignore"):
                Traw = (eta[:, None] * I - (eta * NdotI + np.sqrt(np.where(ok, k, f32(0))))[:, None] * Nf).astype(f32)
            Tdir[ok] = normalize(Traw[ok])
            tr = m["transmission_roughness"][gl]
            pt = ok & (tr > f32(0.02))
            if pt.any():
                Tdir[pt], _ = perturb(Tdir[pt], tr[pt], seed[pt], O)
            if counts is not None:
                counts["reflection"] += len(g)
                counts["refraction"] += int(ok.sum())
            dR = {} if want else None
            Rcol, *_ = shade_segment(meshes, lights, view, (Pg + Nf * eps[:, None]).astype(f32), Rdir, False, O, counts, dR)
            Tcol = np.zeros_like(Rcol)
            if ok.any():
                oo = (Pg[ok] - Nf[ok] * eps[ok][:, None]).astype(f32)
                dT = {} if want else None
                beh, h2, t2, *_ = shade_segment(meshes, lights, view, oo, Tdir[ok], False, O, counts, dT)
                thick = np.where(h2, t2, f32(1)).astype(f32)
                if want:
                    detail["T"] = dT
                    detail["thickness"][g[ok]] = thick
                a = mn(mx(m["albedo"][gl][ok], f32(0)), f32(1))
                absorb = np.stack([pos_pow(a[:, c], thick, O) for c in range(3)], axis=1)
                Tcol[ok] = (absorb * beh).astype(f32)
            Fr[~ok] = 1
            if want:
                detail["glass"][g], detail["refr_ok"][g], detail["R"] = True, ok, dR
                detail["Fr"][g], detail["Rdir"][g], detail["Tdir"][g] = Fr, Rdir, Tdir
            tm = m["transmission"][gl]
            color[g] = ((color[g] + Fr * Rcol) + ((f32(1) - Fr) * tm[:, None]) * Tcol).astype(f32)
    with np.errstate(all="ignore"):
        c = (color / (color + f32(1))).astype(f32)
    gch = np.stack([pos_pow(c[:, k], GAMMA, O) for k in range(3)], axis=1)
    rgb = (mn(mx(gch, f32(0)), f32(1)) * f32(255.0)).astype(f32)
    if want:
        detail.update(linear=color, final=gch, rgb=rgb)
    img = np.zeros((H, W, 3), np.uint8)
    img[H - 1 - y, x] = rgb.astype(np.int32).astype(np.uint8)
    return img

