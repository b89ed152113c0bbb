"""ptrt_query_direct restated in numpy (include/ptrt.h).  `restate` takes what ptrt_direct_rays writes for the texels' n * Q
rays -- ray (t, q) in row t * Q + q, Q = light_count * n_shadow -- and the flags ptrt_query_rays(PTRT_QUERY_OCCLUDED) gives
those rays to the (n, 8) float32 rows the kernel must write, bit for bit: the fold functions are irradiance_restatement's.
`restate64` is the same in float64 with plain sums, the twin the float32 order is bounded against (tests/test_direct.py).
`statement64` states the sample itself -- L, tmax, weight -- in float64 on path_truth.light_sample, and `margins` the bound of
the float32 sample against it, rounding by rounding (tests/test_direct_gpu.py)."""

import numpy as np

import irradiance_restatement as R
import path_truth as PT
from shading_truth import _col, _dot

F = np.float32
QUANTITIES = 5  # irradiance[3], lit_fraction, shadowed_fraction
U = 2.0 ** -24  # a float32 operation returns its exact result times (1 + e), |e| <= U


def walked32(weights):
    """weight.x > 0 || weight.y > 0 || weight.z > 0: false for a NaN weight"""
    w = np.ascontiguousarray(weights, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (w[:, 0] > 0) | (w[:, 1] > 0) | (w[:, 2] > 0)


def terms32(weights, blocked, n_shadow, light_count):
    """(n, Q, 5) float32: every sample's term of every quantity"""
    Q = n_shadow * light_count
    w = np.ascontiguousarray(weights, F).reshape(-1, Q, 3)
    n = w.shape[0]
    walked = walked32(weights).reshape(n, Q)
    dark = walked & (np.asarray(blocked).reshape(n, Q) != 0)
    lit = walked & ~dark
    t = np.zeros((n, Q, QUANTITIES), F)
    t[:, :, :3] = np.where(lit[:, :, None], w, F(0.0))
    t[:, :, 3] = np.where(lit, F(1.0), F(0.0))
    t[:, :, 4] = np.where(dark, F(1.0), F(0.0))
    return t


def restate(weights, blocked, n_shadow, light_count):
    """(n, 8) float32 rows of ptrt_direct"""
    Q = n_shadow * light_count
    assert Q >= 1  # (light_count == 0 is rows of zero bytes, whatever n: nothing to restate)
    t = terms32(weights, blocked, n_shadow, light_count)
    n = t.shape[0]
    w = R.width(Q)
    chunks = (Q + w - 1) // w
    assert chunks == 1 or w == 64
    padded = np.zeros((n, chunks * w, QUANTITIES), F)  # +0.0f for absent q
    padded[:, :Q] = t
    total = np.zeros((n, QUANTITIES), F)               # starts at +0.0f
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(chunks):
            total = total + R.fold(padded[:, c * w:(c + 1) * w])
        out = np.zeros((n, 8), F)                      # reserved: 0.0f
        out[:, :3] = total[:, :3] / F(n_shadow)
        out[:, 3:5] = total[:, 3:5] / F(Q)
    assert total.dtype == F
    return out


def restate64(weights, blocked, n_shadow, light_count):
    """(n, 5) float64: the same quantities from the same float32 inputs, every operation in float64"""
    t = terms32(weights, blocked, n_shadow, light_count).astype(np.float64)
    out = t.sum(axis=1)
    out[:, :3] /= n_shadow
    out[:, 3:] /= n_shadow * light_count
    return out


def magnitudes64(weights, blocked, n_shadow, light_count):
    """(n, 5) float64: M_i, every quantity's sum of absolute terms under its divisor"""
    t = np.abs(terms32(weights, blocked, n_shadow, light_count).astype(np.float64))
    out = t.sum(axis=1)
    out[:, :3] /= n_shadow
    out[:, 3:] /= n_shadow * light_count
    return out


# ---- the sample --------------------------------------------------------------------------------------------------------------
def origins32(positions, normals, offset, Q):
    """(n * Q, 3) float32: positions[t] + offset * normals[t], the product rounded, then the sum"""
    return R.origins32(positions, normals, offset, Q)


def statement64(positions, normals, lights, light_first, light_count, samples2, phases, n_shadow):
    """The sample of every ray (t, q) in float64.  `lights`: path_truth.lights64 of the uploaded set.  The pair (u1, u2) is the
    float32 pair the header forms (the phase added in float32); everything behind it is path_truth.light_sample with one light
    in the pick, then cos = dot(N, L) and weight = radiance * att * cos / pdf where cos > 0 and pdf > 0.
    -> (dict(L, tmax, weight, walked, and the fields of light_sample under "sample"), decided)"""
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    n, Q = len(p), light_count * n_shadow
    u1, u2 = R.samples32(samples2, phases, n)               # (k,), (n, k) float32
    j = np.repeat(np.arange(light_count), n_shadow) + light_first   # light of term q
    s = np.tile(np.arange(n_shadow), light_count)                  # shadow sample of term q
    point = np.repeat(p, Q, axis=0)
    N = np.repeat(nrm, Q, axis=0)
    jj = np.tile(j, n)
    Lt = {f: v[jj] for f, v in lights.items()}
    U1 = np.tile(u1[s].astype(np.float64), n)
    U2 = u2[:, s].astype(np.float64).reshape(-1)
    smp = PT.light_sample(point, N, Lt, np.zeros(n * Q), U1, U2, n_lights=1)
    cos = _dot(N, smp["L"])
    with np.errstate(all="ignore"):
        on = (cos > 0.0) & (smp["pdf_sample"] > 0.0)
        weight = np.where(_col(on), smp["radiance"] * _col(smp["attenuation"] * cos / smp["pdf_sample"]), 0.0)
    walked = (weight > 0).any(axis=1)
    return dict(L=smp["L"], tmax=smp["shadow_tmax"], weight=weight, walked=walked, cos=cos, sample=smp, N=N, Lt=Lt,
                u1=U1), smp["decided"]


def margins(st):
    """Per ray, the bound on |float32 - statement64| of a component of L, of tmax, and of a channel of the weight, for unit
    normals and texels away from the lights: every rounding counted, U = 2^-24 relative each, first order, times 1.01 for the
    second-order terms.
      toLight, dist   a component of toLight: 1 rounding, U relative to it.  d2 = dot: the inputs' 2 U (squared) and the
                      FMA chain's 3; the root halves that and adds its own: dist to 3.5 U relative.
      L, no radius    toLight / dist: 1 + 3.5 + 1 = 5.5 U relative to a component that is at most 1.  A directional light's L
                      is an input negated: exact.
      tmax            dist - 1e-3f: 3.5 U and one rounding, relative to dist: 4.5 U dist (1e30f for a directional light).
      cone            sin2 = r * r / d2: 1 + 5 + 1 = 7 U relative; cos_max = sqrt(1 - sin2): (7 U sin2 + U) / (2 cos_max) + U
                      absolute -- E_c.  1 - cos_max then carries E_c + U: the cancellation path_truth names, and what the
                      density's relative error is made of, (E_c + U) / (1 - cos_max) + 2 U (the product with 2 pi, the
                      division).  cos_theta = 1 - u1 (1 - cos_max): E_c + 3 U absolute -- E_t; s2 = 1 - cos_theta^2: 2 E_t
                      + 2 U absolute, the second cancellation: sin_theta to sqrt(s2 + 2 E_t + 2 U) - sqrt(s2) + U.  phi =
                      2 pi u2 in float32 is off by 2 pi U from the statement's float64 product, and det_sincos by
                      SINCOS_ABS, both times sin_theta <= 1.  The basis about the axis and the three products and two
                      sums to the world are irradiance_restatement.ray_margin()'s count (which holds SINCOS_ABS twice
                      already), the axis itself is off by 5.5 U.
      cos             dot(N, L) with |N| = 1: sqrt(3) E_L + 3 U absolute -- E_cos.
      att             range / (range + dist): 3.5 + 1 + 1 = 5.5 U; squared 12 U.  The soft spot factor (theta - outer) / eps,
                      clamped: theta = dot(L, -dir) to sqrt(3) E_L + 3 U, the difference 1 more, over eps (formed in float32
                      on both sides); the quotient's and the product's roundings 2 U relative: E_f = (sqrt(3) E_L + 4 U) /
                      eps absolute on the factor.  A hard edge is decided or left out.
      weight          radiance: 1 U; att: 12 (+ 2 with a soft factor); two products and the division: 3; the density's share
                      above.  |weight| times that sum, plus (radiance att / pdf) E_cos, plus (radiance att0 cos / pdf) E_f."""
    smp, Lt = st["sample"], st["Lt"]
    n = len(st["tmax"])
    directional = Lt["type"] == PT.LIGHT_DIRECTIONAL
    sphere = smp["sphere"]
    with np.errstate(all="ignore"):
        cos_max = 1.0 - smp["solid_angle"] / (2.0 * np.pi)
        sin2 = 1.0 - cos_max * cos_max
        E_c = (7 * U * sin2 + U) / (2.0 * cos_max) + U
        E_t = E_c + 3 * U
        cos_theta = 1.0 - st["u1"] * (1.0 - cos_max)
        s2 = np.maximum(0.0, 1.0 - cos_theta * cos_theta)
        sin_err = np.sqrt(s2 + 2 * E_t + 2 * U) - np.sqrt(s2) + U
        E_cone = R.ray_margin() + 5.5 * U + 2.0 * np.pi * U + sin_err + E_t
        # (below the reference's 1e-6 threshold -- a decided comparison -- the density is the literal 1)
        pdf_rel = np.where(sphere & (smp["solid_angle"] > F(1e-6)), (E_c + U) / (1.0 - cos_max) + 2 * U, 0.0)
    E_L = np.where(directional, 0.0, np.where(sphere, E_cone, 5.5 * U))
    E_tmax = 4.5 * U * np.abs(smp["light_dist"])
    E_cos = np.sqrt(3.0) * E_L + 3 * U
    spot = ~directional & (Lt["type"] == PT.LIGHT_SPOT)
    eps = (Lt["inner"].astype(np.float32) - Lt["outer"].astype(np.float32)).astype(np.float64)
    soft = spot & ~(eps <= F(1e-6))
    E_f = np.where(soft, (np.sqrt(3.0) * E_L + 4 * U) / np.where(soft, eps, 1.0), 0.0)
    with np.errstate(all="ignore"):
        att0 = np.where(directional, 1.0, PT.attenuate(smp["light_dist"], Lt["range"]))
        on = (st["cos"] > 0.0) & (smp["pdf_sample"] > 0.0)
        per_cos = np.where(_col(on), smp["radiance"] * _col(smp["attenuation"] / smp["pdf_sample"]), 0.0)
        per_f = np.where(_col(on), smp["radiance"] * _col(att0 * st["cos"] / smp["pdf_sample"]), 0.0)
    rel = (1 + 12 + 3) * U + np.where(soft, 2 * U, 0.0) + pdf_rel
    E_w = np.abs(st["weight"]) * _col(rel) + np.abs(per_cos) * _col(E_cos) + np.abs(per_f) * _col(E_f)
    assert E_L.shape == E_tmax.shape == (n,) and E_w.shape == (n, 3)
    return 1.01 * E_L, 1.01 * E_tmax, 1.01 * E_w


# ---- the inputs of the comparison with statement64 ------------------------------------------------------------------------------
STATEMENT_LIGHTS = [
    dict(type=0, position=(0.0, 4.5, -5.0), color=(1.0, 0.9, 0.8), intensity=3.0, range=20.0),                        # a hard point
    dict(type=0, position=(2.0, 3.0, -4.0), color=(0.8, 0.8, 1.0), intensity=5.0, range=15.0, radius=0.3),            # a sphere
    dict(type=2, position=(-3.0, 4.0, -6.0), direction=(0.3, -1.0, 0.1), color=(1.0, 1.0, 1.0), intensity=12.0, range=30.0,
         inner=0.6, outer=0.6),                                                                                      # a hard cone
    dict(type=2, position=(1.0, 4.5, -7.0), direction=(0.0, -1.0, 0.0), color=(1.0, 0.7, 0.4), intensity=15.0, range=25.0,
         inner=0.9, outer=0.5, radius=0.2),                                                                          # a soft cone, with a radius
    dict(type=1, direction=(-0.4, -1.0, -0.3), color=(1.0, 0.96, 0.9), intensity=3.0),                                # the sun
    dict(type=0, position=(-2.0, 2.5, -3.0), color=(0.5, 1.0, 0.5), intensity=4.0, range=10.0, radius=1e-4),          # below 1e-6 sr
]
STATEMENT_TEXELS, STATEMENT_SHADOW = 41, 4


def statement_inputs(P):
    """(lights (ctypes array), positions, normals, samples2, phases): 41 texels at least 3.5 below the lowest light with unit
    normals, most of them facing up; four shadow samples, the first on the cone's axis (u1 = 0, where sin_theta cancels most)
    and the last on its rim."""
    rs = np.random.RandomState(20261020)
    n = STATEMENT_TEXELS
    pos = np.stack([rs.uniform(-4, 4, n), rs.uniform(-4.5, -1.0, n), rs.uniform(-9, -1, n)], axis=1).astype(F)
    nrm = rs.normal(size=(n, 3))
    nrm[:, 1] = np.abs(nrm[:, 1]) + 0.5
    nrm[::7, 1] *= -1.0                                     # every seventh faces away from most lights
    nrm[:3] = [[0, 1, 0], [1, 0, 0], [0, 0, -1]]
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    s2 = np.array([[0.0, 0.3], [0.375, 0.5], [0.625, 0.25], [np.nextafter(F(1.0), F(0.0)), 0.75]], F)
    ph = rs.random_sample(n).astype(F)
    ph[:2] = [0.0, 0.999999]
    return PT.make_lights(P, STATEMENT_LIGHTS), np.ascontiguousarray(pos), np.ascontiguousarray(nrm), s2, np.ascontiguousarray(ph)
