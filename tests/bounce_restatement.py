"""ptrt_query_bounce restated in numpy (include/ptrt.h).  `restate` takes what ptrt_bounce_terms writes for the texels'
n * n_dirs gather rays -- term q of ray i in row i * Q + q, Q = light_count * n_shadow --, the flags
ptrt_query_rays(PTRT_QUERY_OCCLUDED) gives the walked terms and the rays' hit records to the (n, 8) float32 rows the kernel must
write, bit for bit: a ray's sum over q runs in q order from +0.0f, the reduction over k is irradiance_restatement's fold.
`walked` is read off the value (some channel above zero): the device decides it on `direct`, the value before the throughput,
and the two agree unless a Beer-Lambert factor underflows to zero in every channel that is lit.  `restate64` and `magnitudes64`
are the float64 twins the float32 order is bounded against (tests/test_bounce.py).

`value32` composes a term's value in float32 from its pieces -- BSDF, radiance, attenuation, density, throughput --, and
`light_pieces32` restates the three that come from the light record, operation by operation, the fused multiply-adds of the
device's dot products formed exactly and rounded once; `throughput32` restates the Beer-Lambert factor behind a back face
(tests/test_bounce_gpu.py feeds value32 the device's own BSDF).

`statement64` states the term in float64 on path_truth.light_sample (one light in the pick) and path_truth.light_value
(shading_truth.evaluateBSDF, the soft clamp; no MIS weight), `margins` bounds the float32 term against it rounding by rounding,
the way direct_restatement.margins does, with the BSDF's own conditioning from shading_truth."""
from fractions import Fraction

import numpy as np

import direct_restatement as D
import irradiance_restatement as R
import path_truth as PT
import shading_truth as T
from shading_truth import _col, _dot

F = np.float32
QUANTITIES = 6  # radiance[3], lit_fraction, shadowed_fraction, hit_fraction
U = D.U
MAX_UNDECIDED = 0.02  # the cap tests/test_direct.py uses


def walked32(values):
    """value.x > 0 || value.y > 0 || value.z > 0: false for a NaN"""
    return D.walked32(values)


def _hit_mask(hits, rays):
    h = np.asarray(hits)
    if h.dtype.names:
        h = (h["hit"] != 0) & (h["mesh_index"] >= 0)
    h = h.reshape(-1) != 0
    assert h.shape == (rays,)
    return h


def ray_terms32(values, flags, hits, n_shadow, count):
    """(rays, 6) float32: B[3] = (the sum over q, in q order from +0.0f, of the unblocked values) / (float)n_shadow, the counts
    of lit and of blocked terms as floats, and hit ? 1 : 0; a miss is a row of +0.0f"""
    Q = n_shadow * count
    v = np.ascontiguousarray(values, F).reshape(-1, Q, 3)
    r = v.shape[0]
    hit = _hit_mask(hits, r)
    walked = walked32(values).reshape(r, Q)
    dark = walked & (np.asarray(flags).reshape(r, Q) != 0)
    lit = walked & ~dark
    out = np.zeros((r, QUANTITIES), F)
    s = np.zeros((r, 3), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(Q):
            s = s + np.where(lit[:, q, None], v[:, q], F(0.0))
        out[:, :3] = s / F(n_shadow)
    assert s.dtype == F
    out[:, 3] = lit.sum(axis=1).astype(F)
    out[:, 4] = dark.sum(axis=1).astype(F)
    out[:, 5] = np.where(hit, F(1.0), F(0.0))
    out[~hit] = F(0.0)
    return out


def restate(values, flags, hits, n_dirs, n_shadow, count):
    """(n, 8) float32 rows of ptrt_bounce"""
    Q = n_shadow * count
    assert Q >= 1 and n_dirs >= 1  # (light_count == 0 is rows of zero bytes: nothing to restate)
    t = ray_terms32(values, flags, hits, n_shadow, count).reshape(-1, n_dirs, QUANTITIES)
    n = t.shape[0]
    w = R.width(n_dirs)
    chunks = (n_dirs + w - 1) // w
    assert chunks == 1 or w == 64
    padded = np.zeros((n, chunks * w, QUANTITIES), F)  # +0.0f for absent k
    padded[:, :n_dirs] = t
    total = np.zeros((n, QUANTITIES), F)               # starts at +0.0f
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(chunks):
            total = total + R.fold(padded[:, c * w:(c + 1) * w])
        out = np.zeros((n, 8), F)                      # reserved: 0.0f
        out[:, :3] = total[:, :3] / F(n_dirs)
        out[:, 3:5] = total[:, 3:5] / F(n_dirs * Q)
        out[:, 5] = total[:, 5] / F(n_dirs)
    assert total.dtype == F
    return out


def restate64(values, flags, hits, n_dirs, n_shadow, count):
    """(n, 6) float64: the same quantities from the same float32 inputs, every operation in float64 with plain sums"""
    Q = n_shadow * count
    v = np.ascontiguousarray(values, F).reshape(-1, Q, 3).astype(np.float64)
    r = v.shape[0]
    hit = _hit_mask(hits, r)
    walked = walked32(values).reshape(r, Q) & hit[:, None]
    dark = walked & (np.asarray(flags).reshape(r, Q) != 0)
    lit = walked & ~dark
    per_ray = np.zeros((r, QUANTITIES))
    per_ray[:, :3] = np.where(lit[:, :, None], v, 0.0).sum(axis=1) / n_shadow
    per_ray[:, 3], per_ray[:, 4], per_ray[:, 5] = lit.sum(axis=1), dark.sum(axis=1), hit
    out = per_ray.reshape(-1, n_dirs, QUANTITIES).sum(axis=1)
    out[:, :3] /= n_dirs
    out[:, 3:5] /= n_dirs * Q
    out[:, 5] /= n_dirs
    return out


def magnitudes64(values, flags, hits, n_dirs, n_shadow, count):
    """(n, 6) float64: M_i, every quantity's sum of absolute terms under its divisors"""
    with np.errstate(invalid="ignore"):
        return restate64(np.abs(np.ascontiguousarray(values, F)), flags, hits, n_dirs, n_shadow, count)


# ---- a term's value in float32 ---------------------------------------------------------------------------------------------------
def clamp32(v, max_lum=500.0):
    """clamp_vector_soft: lum = (0.2126f x + 0.7152f y) + 0.0722f z; above max_lum (and zero) the vector times max_lum / lum"""
    v = np.ascontiguousarray(v, F)
    with np.errstate(all="ignore"):
        lum = F(0.2126) * v[:, 0] + F(0.7152) * v[:, 1] + F(0.0722) * v[:, 2]
        on = (lum > F(max_lum)) & (lum > F(0.0))
        out = np.where(on[:, None], v * (F(max_lum) / np.where(on, lum, F(1.0)))[:, None], v)
    assert out.dtype == F
    return out


def value32(bsdf, radiance, att, pdf, throughput):
    """(rows, 3) float32: throughput * clamp(((bsdf * radiance) * att) / pdf, 500), every operation rounded on its own"""
    f, rad, thr = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (bsdf, radiance, throughput))
    a, p = (np.ascontiguousarray(x, F).reshape(-1, 1) for x in (att, pdf))
    with np.errstate(all="ignore"):
        direct = ((f * rad) * a) / p
        out = thr * clamp32(direct)
    assert out.dtype == F
    return out


def throughput32(O, albedo, t, front_face):
    """(rows, 3) float32: (1, 1, 1) in front of a face; behind one exp(-max(-log(max(1e-6f, albedo)), 0) * t) per channel, the
    path's Beer-Lambert factor, its logarithm and exponential the library's deterministic ones (oracle.detmath 3 and 2)"""
    a = np.maximum(F(1e-6), np.ascontiguousarray(albedo, F).reshape(-1, 3))
    coeff = np.maximum(-O.detmath(3, np.ascontiguousarray(a.reshape(-1))).astype(F), F(0.0))
    x = (-coeff).reshape(-1, 3) * np.ascontiguousarray(t, F).reshape(-1, 1)
    assert x.dtype == F
    thr = O.detmath(2, np.ascontiguousarray(x.reshape(-1))).astype(F).reshape(-1, 3)
    return np.where(np.asarray(front_face).reshape(-1, 1) != 0, F(1.0), thr)


def _round32(x):
    """the float32 nearest the Fraction x, ties to even (x finite and inside float32's range)"""
    r = F(float(x))  # (float(x) is the nearest double; its float32 is x's nearest or next to it)
    fr = Fraction(float(r))
    if fr == x:
        return r
    lo, hi = (np.nextafter(r, F(-np.inf)), r) if fr > x else (r, np.nextafter(r, F(np.inf)))
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    if x != mid:
        return lo if x < mid else hi
    return lo if (np.array(lo).view(np.uint32) & 1) == 0 else hi


def dot32(a, b):
    """the device's dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), each fused multiply-add exact and rounded once"""
    ax, ay, az = (Fraction(float(x)) for x in a)
    bx, by, bz = (Fraction(float(x)) for x in b)
    s = F(a[0]) * F(b[0])
    s = _round32(ay * by + Fraction(float(s)))
    return _round32(az * bz + Fraction(float(s)))


def light_pieces32(lights, j, point, L):
    """(radiance (3,), att, pdf, tmax) in float32 of light j (path_truth.lights64's fields) seen from `point` along the sampled
    direction L, as sample_light computes them with one light in the pick"""
    g = {k: v[j] for k, v in lights.items()}
    col, pos, direction = (np.asarray(g[k], F) for k in ("color", "position", "direction"))
    intensity, rng, inner, outer, radius = (F(g[k]) for k in ("intensity", "range", "inner", "outer", "radius"))
    radiance = col * intensity
    if g["type"] == PT.LIGHT_DIRECTIONAL:
        return radiance, F(1.0), F(1.0), F(1e30) - F(1e-3)
    to = pos - np.asarray(point, F)
    d2 = dot32(to, to)
    dist = np.sqrt(d2)
    pdf = F(1.0)
    if not radius <= F(0.0):
        sin2 = min((radius * radius) / d2, F(0.9999))
        cos_max = np.sqrt(F(1.0) - sin2)
        solid = F(R.TWO_PI_F) * (F(1.0) - cos_max)
        pdf = F(1.0) / solid if solid > F(1e-6) else F(1.0)
    att = rng / (rng + dist)
    att = att * att
    if g["type"] == PT.LIGHT_SPOT:
        theta = dot32(np.asarray(L, F), -direction)
        eps = inner - outer
        if eps <= F(1e-6):
            spot = F(1.0) if theta >= outer else F(0.0)
        else:
            spot = min(max((theta - outer) / eps, F(0.0)), F(1.0))
        att = att * spot
    for x in (d2, dist, pdf, att):
        assert type(x) is F
    return radiance, att, pdf, dist - F(1e-3)


# ---- the term in float64 ---------------------------------------------------------------------------------------------------------
def statement64(hits, directions, lights, materials, light_first, light_count, shadow2, phases, n_dirs, n_shadow):
    """Every term (i, q) of the rays that hit, in float64.  `hits`: HIT_DTYPE records of the n * n_dirs gather rays, `directions`
    their directions; `lights`: path_truth.lights64 of the uploaded set; `materials`: shading_truth.load_materials of the
    scene.  The hit's point, normal, distance and side and the ray's direction are the float32 inputs of the term as they
    stand; the pair (u1, u2) is the float32 pair the header forms.  Behind them: path_truth.light_sample with one light in the
    pick, path_truth.light_value (evaluateBSDF at V = -rd, times radiance * att / pdf, the soft clamp; no MIS weight), times
    path_truth.absorption behind a back face.
    -> (dict(rows, L, origin, tmax, direct, value, walked, ...), decided): `rows` the indices i * Q + q of the terms stated (those
    of rays that hit), `decided` per stated term -- no cosine, cone edge, clamp threshold or walked test within its margin of a
    branch (margins() gives the clamp's and the walked test's)."""
    h = np.asarray(hits)
    rays = len(h)
    n, Q = rays // n_dirs, light_count * n_shadow
    assert n * n_dirs == rays
    u1, u2 = R.samples32(shadow2, phases, n)                          # (m,), (n, m) float32
    struck = np.flatnonzero((h["hit"] != 0) & (h["mesh_index"] >= 0))
    i = np.repeat(struck, Q)                                          # the ray of a stated term
    q = np.tile(np.arange(Q), len(struck))
    j, s = q // n_shadow + light_first, q % n_shadow
    point, N = h["point"][i].astype(np.float64), h["normal"][i].astype(np.float64)
    ff = h["front_face"][i] != 0
    V = -np.asarray(directions, np.float64).reshape(-1, 3)[i]
    M = T.gather(materials, h["mesh_index"][i])
    Lt = {f: v[j] for f, v in lights.items()}
    U1 = u1[s].astype(np.float64)
    U2 = u2[i // n_dirs, s].astype(np.float64)
    smp = PT.light_sample(point, N, Lt, np.zeros(len(i)), U1, U2, n_lights=1)
    direct, dec_f = PT.light_value(smp, V, N, ff, M, np.zeros(len(i), bool))
    thr = PT.absorption(M["albedo"], h["t"][i].astype(np.float64), ~ff)
    with np.errstate(all="ignore"):
        unclamped = T.evaluateBSDF(M, N, V, smp["L"], ff)[0] * smp["radatt"] / _col(smp["pdf_sample"])
        walked = (smp["pdf_sample"] > 0.0) & (direct > 0.0).any(axis=1)
    st = dict(rows=i * Q + q, ray=i, L=smp["L"], origin=smp["shadow_origin"], tmax=smp["shadow_tmax"], direct=direct,
              unclamped=unclamped, value=thr * direct, throughput=thr, walked=walked, sample=smp, Lt=Lt, u1=U1, N=N, V=V, ff=ff, M=M,
              t=h["t"][i].astype(np.float64), cos=_dot(N, smp["L"]), weight=np.zeros((len(i), 3)))
    E = margins(st)
    lum = PT.F(0.2126) * unclamped[:, 0] + PT.F(0.7152) * unclamped[:, 1] + PT.F(0.0722) * unclamped[:, 2]
    with np.errstate(all="ignore"):
        clamp_far = np.abs(lum - 500.0) > E["lum"]
        top = unclamped.max(axis=1)
        walked_far = (top <= 0.0) | (top > E["unclamped"].max(axis=1))
    decided = smp["decided"] & dec_f & clamp_far & walked_far & np.isfinite(unclamped).all(axis=1)
    st["E"] = E
    return st, decided


# what the deterministic exponential and logarithm lose (tests/test_detmath.py): 2 ulp; the logarithm next to 1 an absolute bound
EXP_REL = 4 * U
LOG_ABS, LOG_REL = 2e-8, 2.4e-7


def margins(st):
    """Per stated term, the bounds on |float32 - statement64|: dict(L (n,), tmax (n,), unclamped (n, 3), lum (n,), value (n, 3)).
    Every rounding counted at U = 2^-24 relative, first order, times 1.01 for the second-order terms.
      L, tmax        direct_restatement.margins', with the hit's point in the texel's place: E_L, E_tmax.
      bsdf           the device's evaluateBSDF against shading_truth's at the same inputs: shading_truth.TOL["f"] units of
                     EPS32 x conditioning (|f| + sum |x df/dx| over N, V, L and the material's fields: tests/shading_truth.py).
                     L is not the same input on both sides: it is off by E_L per component, which moves f by |df/dL_c| E_L,
                     summed over c -- central differences with an absolute step of 1e-6.
      radiance       colour x intensity: U.
      att, pdf       as direct_restatement.margins counts them: 12 U on the squared range factor, 2 U and (sqrt(3) E_L + 4 U) /
                     eps absolute with a soft cone, (E_c + U) / (1 - cos_max) + 2 U on a sphere light's density.
      unclamped      f x radiance x att / pdf: three more roundings.  Together
                     E_u = |radiance att / pdf| E_f + |unclamped| (1 + 12 (+ 2) + 3) U + pdf's share + the soft cone's.
      lum            three products, two sums of terms taken absolute, and the channels' own errors under the same weights.
      clamp          below the threshold the vector passes.  Above, v x (500 / lum): E_u scale + |v| scale (E_lum / lum) + 2 U.
      throughput     1 exactly in front of a face.  Behind one exp(-c t), c = -log(max(1e-6, albedo)): the logarithm to
                     LOG_ABS + LOG_REL |c|, the product with t one rounding, the exponential 2 ulp:
                     relative t (LOG_ABS + LOG_REL c) + (c t + 4) U.  The product with the clamped value one rounding more."""
    smp, Lt, M = st["sample"], st["Lt"], st["M"]
    E_L, E_t, _ = D.margins(st)
    E_L, E_t = E_L / 1.01, E_t / 1.01
    N, V, L, ff = st["N"], st["V"], smp["L"], st["ff"]

    def f_only(M_, N_, V_, L_, ff_):
        return T.evaluateBSDF(M_, N_, V_, L_, ff_)[0]

    with np.errstate(all="ignore"):
        cond = T.conditioning(f_only, M, [N, V, L], (ff,))
        E_f = T.TOL["f"] * T.EPS32 * cond
        h = 1e-6
        for c in range(3):
            step = np.zeros(3)
            step[c] = h
            slope = np.abs(f_only(M, N, V, L + step, ff) - f_only(M, N, V, L - step, ff)) / (2 * h)
            E_f = E_f + slope * _col(E_L)
        # the density's and the soft cone's shares, as direct_restatement.margins forms them
        cos_max = 1.0 - smp["solid_angle"] / (2.0 * np.pi)
        sin2 = 1.0 - cos_max * cos_max
        E_c = (7 * U * sin2 + U) / (2.0 * cos_max) + U
        pdf_rel = np.where(smp["sphere"] & (smp["solid_angle"] > F(1e-6)), (E_c + U) / (1.0 - cos_max) + 2 * U, 0.0)
        directional = Lt["type"] == PT.LIGHT_DIRECTIONAL
        spot = ~directional & (Lt["type"] == PT.LIGHT_SPOT)
        eps = (Lt["inner"].astype(np.float32) - Lt["outer"].astype(np.float32)).astype(np.float64)
        soft = spot & ~(eps <= F(1e-6))
        E_spot = np.where(soft, (np.sqrt(3.0) * E_L + 4 * U) / np.where(soft, eps, 1.0), 0.0)
        att0 = np.where(directional, 1.0, PT.attenuate(smp["light_dist"], Lt["range"]))
        f = f_only(M, N, V, L, ff)
        per_f = smp["radatt"] / _col(smp["pdf_sample"])
        per_spot = f * smp["radiance"] * _col(att0 / smp["pdf_sample"])
        u = st["unclamped"]
        rel = (1 + 12 + 3) * U + np.where(soft, 2 * U, 0.0) + pdf_rel
        E_u = np.abs(per_f) * E_f + np.abs(u) * _col(rel) + np.abs(per_spot) * _col(E_spot)
        w = np.array([PT.F(0.2126), PT.F(0.7152), PT.F(0.0722)])
        lum = (np.abs(u) * w).sum(axis=1)
        E_lum = (E_u * w).sum(axis=1) + 5 * U * lum
        on = lum > 500.0
        scale = np.where(on, 500.0 / np.where(on, lum, 1.0), 1.0)
        E_d = np.where(_col(on), E_u * _col(scale) + np.abs(u) * _col(scale * (E_lum / np.where(on, lum, 1.0) + 2 * U)), E_u)
        coeff = np.maximum(-np.log(np.maximum(F(1e-6), M["albedo"])), 0.0)
        t = _col(st["t"])
        thr_rel = np.where(_col(ff), 0.0, t * (LOG_ABS + LOG_REL * coeff) + (coeff * t + 4) * U)
        E_v = st["throughput"] * E_d + np.abs(st["value"]) * (thr_rel + U)
    return dict(L=1.01 * E_L, tmax=1.01 * E_t, unclamped=1.01 * E_u, lum=1.01 * E_lum, value=1.01 * E_v)


# ---- the inputs of the comparison with statement64 ---------------------------------------------------------------------------------
STATEMENT_TEXELS, STATEMENT_DIRS, STATEMENT_SHADOW = 35, 4, 2


def statement_rays(P, positions, normals):
    """(samples2, shadow2, phases, origins, directions): the float32 gather rays of STATEMENT_DIRS Hammersley points per texel,
    built on the CPU -- irradiance_restatement.rays64 rounded to float32 (the device's own rays differ from these in the last
    bits; either set is a set of rays to state terms at)"""
    n = len(positions)
    s2 = P.lightmap.hammersley2(STATEMENT_DIRS)
    sh2 = np.array([[0.375, 0.5], [np.nextafter(F(1.0), F(0.0)), 0.75]], F)[:STATEMENT_SHADOW]
    ph = P.lightmap.texel_phases(n, 7)
    d = R.rays64(normals, s2, ph).astype(F)
    o = R.origins32(positions, normals, F(1e-4), STATEMENT_DIRS)
    return s2, sh2, ph, np.ascontiguousarray(o), np.ascontiguousarray(d)
