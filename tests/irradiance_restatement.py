"""ptrt_query_irradiance restated in numpy float32, operation by operation (include/ptrt.h): the records ptrt_query_radiance
gives the texels' n * n_dirs rays -- ray (t, k) in row t * n_dirs + k --, n_dirs and max_distance go to the (n, 8) float32 rows
the irradiance kernel must write, bit for bit.  `restate64` is the same statement in float64 with plain sums: the twin the
float32 order is bounded against (tests/test_irradiance.py).  `rays64` states the rays themselves in float64: the cosine map
and the basis about the normal (tests/test_irradiance_gpu.py)."""

import numpy as np

F = np.float32
QUANTITIES = 6  # radiance[3], mean_distance, mean_distance_sq, hit_fraction


def width(n_dirs):
    """w: the smallest power of two >= n_dirs up to 64 directions, 64 beyond"""
    w = 1
    while w < 64 and w < n_dirs:
        w *= 2
    return w


def terms32(radiance, depth, object_id, n_dirs, max_distance):
    """(n, n_dirs, 6) float32: every ray's term of every quantity"""
    L = np.ascontiguousarray(radiance, F).reshape(-1, n_dirs, 3)
    n = L.shape[0]
    t = np.empty((n, n_dirs, QUANTITIES), F)
    t[:, :, :3] = L
    dist = np.minimum(np.ascontiguousarray(depth, F).reshape(n, n_dirs), F(max_distance))
    t[:, :, 3] = dist
    with np.errstate(over="ignore"):  # (a miss under the default max_distance of 1e30: the square is +inf, on the device too)
        t[:, :, 4] = dist * dist
    t[:, :, 5] = np.where(np.asarray(object_id).reshape(n, n_dirs) >= 0, F(1.0), F(0.0))
    return t


def fold(v):
    """v[j] + v[j + w/2], then w/4, .. 1 along axis 1 (of length w, a power of two)"""
    w = v.shape[1]
    assert w & (w - 1) == 0 and 1 <= w <= 64 and v.dtype == F
    h = w // 2
    while h >= 1:
        v = v[:, :h] + v[:, h:2 * h]
        h //= 2
    return v[:, 0]


def restate(radiance, depth, object_id, n_dirs, max_distance):
    """(n, 8) float32 rows of ptrt_irradiance"""
    t = terms32(radiance, depth, object_id, n_dirs, max_distance)
    n = t.shape[0]
    w = width(n_dirs)
    chunks = (n_dirs + w - 1) // w
    assert chunks == 1 or w == 64
    padded = np.zeros((n, chunks * w, QUANTITIES), F)  # +0.0f for absent k
    padded[:, :n_dirs] = t
    total = np.zeros((n, QUANTITIES), F)               # starts at +0.0f
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(chunks):
            total = total + fold(padded[:, c * w:(c + 1) * w])
        out = np.zeros((n, 8), F)                      # reserved: 0.0f
        out[:, :QUANTITIES] = total / F(n_dirs)
    assert total.dtype == F
    return out


def restate64(radiance, depth, object_id, n_dirs, max_distance):
    """(n, 6) float64: the same quantities from the same float32 inputs, every operation in float64"""
    L = np.asarray(radiance, np.float64).reshape(-1, n_dirs, 3)
    n = L.shape[0]
    out = np.empty((n, QUANTITIES))
    out[:, :3] = L.sum(axis=1) / n_dirs
    dist = np.minimum(np.asarray(depth, np.float64).reshape(n, n_dirs), float(F(max_distance)))
    out[:, 3] = dist.sum(axis=1) / n_dirs
    out[:, 4] = (dist * dist).sum(axis=1) / n_dirs
    out[:, 5] = (np.asarray(object_id).reshape(n, n_dirs) >= 0).sum(axis=1) / n_dirs
    return out


def magnitudes64(radiance, depth, n_dirs, max_distance):
    """(n, 6) float64: M_i, the mean of every quantity's terms taken absolute -- |L|, dist, dist^2 and 1"""
    L = np.abs(np.asarray(radiance, np.float64).reshape(-1, n_dirs, 3))
    n = L.shape[0]
    out = np.empty((n, QUANTITIES))
    out[:, :3] = L.sum(axis=1) / n_dirs
    dist = np.abs(np.minimum(np.asarray(depth, np.float64).reshape(n, n_dirs), float(F(max_distance))))
    out[:, 3] = dist.sum(axis=1) / n_dirs
    out[:, 4] = (dist * dist).sum(axis=1) / n_dirs
    out[:, 5] = 1.0
    return out


# ---- the rays ---------------------------------------------------------------------------------------------------------------
TWO_PI_F = F(6.28318530717958647692)


def samples32(samples2, phases, n):
    """(u1 (k,), u2 (n, k)) float32: the sample pair of every ray, the texel's phase added as the header states"""
    s = np.ascontiguousarray(samples2, F).reshape(-1, 2)
    u1 = s[:, 0]
    u2 = np.repeat(s[None, :, 1], n, axis=0)
    if phases is not None:
        u2 = u2 + np.ascontiguousarray(phases, F).reshape(n, 1)
        u2 = np.where(u2 >= F(1.0), u2 - F(1.0), u2)
    assert u2.dtype == F
    return u1, u2


def origins32(positions, normals, offset, n_dirs):
    """(n * n_dirs, 3) float32: positions[t] + offset * normals[t], the product rounded, then the sum"""
    p, nrm = np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(normals, F).reshape(-1, 3)
    o = p + F(offset) * nrm
    assert o.dtype == F
    return np.repeat(o, n_dirs, axis=0)


def rays64(normals, samples2, phases):
    """(n * k, 3) float64 directions: the cosine map of the float32 pair (u1, u2) -- (sqrt(u1) cos(phi), sqrt(u1) sin(phi),
    sqrt(1 - u1)) with phi the FLOAT32 product 2 pi * u2, as the device forms it -- taken to the world by the basis of
    createOrthoNormalBasis about the unit normal (Frisvad's, with the sign of n.z): T = (1 + s a x^2, s b, -s x),
    B = n x T, a = -1 / (s + z), b = x y a; a degenerate normal (|n|^2 < 1e-20) takes the reference's fixed T = (1, 0, 0),
    B = (0, 1, 0).  Everything past phi in float64."""
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    n = nrm.shape[0]
    u1, u2 = samples32(samples2, phases, n)
    phi = (TWO_PI_F * u2).astype(np.float64)
    assert (TWO_PI_F * u2).dtype == F
    r = np.sqrt(u1.astype(np.float64))[None, :]
    lx, ly, lz = r * np.cos(phi), r * np.sin(phi), np.repeat(np.sqrt(np.maximum(0.0, 1.0 - u1.astype(np.float64)))[None, :], n, axis=0)
    len2 = (nrm * nrm).sum(axis=1, keepdims=True)
    flat = len2[:, 0] < 1e-20
    nn = np.where(flat[:, None], [0.0, 0.0, 1.0], nrm) / np.sqrt(np.where(flat[:, None], 1.0, len2))
    x, y, z = nn[:, 0], nn[:, 1], nn[:, 2]
    s = np.copysign(1.0, z)
    a = -1.0 / (s + z)
    b = x * y * a
    T = np.stack([1.0 + s * x * x * a, s * b, -s * x], axis=1)
    B = np.cross(nn, T)
    T[flat], B[flat] = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    d = lx[:, :, None] * T[:, None, :] + ly[:, :, None] * B[:, None, :] + lz[:, :, None] * nrm[:, None, :]
    return d.reshape(-1, 3)


# det_sincos's absolute error on [0, 2 pi], as tests/test_detmath.py states it (test_sincos_on_sampling_range)
SINCOS_ABS = 1.5e-7
ULP = 2.0 ** -23  # one ulp of a float32 number below 2 in magnitude: every intermediate of the ray is one


def ray_margin():
    """The bound on |float32 direction component - rays64| for unit normals: det_sincos's bound plus one ulp per further
    rounding, counted.  Every factor an error is multiplied by on its way to the result is at most 1 in magnitude (local and
    basis components, |a| = 1 / (1 + |z|)), so the errors add.
      basis      dot(N, N) 5, its root 1, the reciprocal 1, three scalings 3, s + z 1, the division 1, x * y * a 2, T.x 3
                 (s * x is exact, as are T.y = s * b and T.z = -s * x): 17 roundings behind T; a component of B = Nn x T two
                 products and a difference more: 20.  T and B enter a world component times local.x and local.y, and
                 |local.x| + |local.y| <= sqrt(2): at most 2 * 20 ulp.
      local      x and y: the cosine or sine (SINCOS_ABS), sqrt(u1) 1, the product 1; z: 1 - u1 1, the root 1.  Times basis
                 components <= 1: 2 * SINCOS_ABS + 6 ulp.
      world      three products, two sums: 5 ulp.
    phi is the same float32 number on both sides and adds nothing."""
    return 2.0 * SINCOS_ABS + (2 * 20 + 6 + 5) * ULP
