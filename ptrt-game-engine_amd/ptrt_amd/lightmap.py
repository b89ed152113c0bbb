"""Around Scene.query_irradiance: the sample set the texels share, per-texel phases, the texels of a planar quad and what to do
with the (n, 8) rows.  Plain numpy, no device code -- the arrays go to the device with torch.from_numpy(..).cuda() and the rows
come back with .cpu().numpy() (torch tensors on the host are accepted where rows are).

A texel's rays are cosine-distributed about its normal, so the mean of their radiance times pi is the irradiance; a texel whose
rays mostly end close by -- inside a wall, under a carpet -- is one a baker fills from its neighbours (`invalid_texels`).

Scene.query_direct adds what the gather cannot see, the analytic lights at the texel itself: `direct_irradiance`,
`penumbra_texels` and `total_irradiance` read its rows."""
import math

import numpy as np


def _radical_inverse2(i):
    """van der Corput in base 2 of the uint32 array i: the bits mirrored about the binary point, exact in float64"""
    i = np.asarray(i, np.uint32).copy()
    i = (i << np.uint32(16)) | (i >> np.uint32(16))
    i = ((i & np.uint32(0x00ff00ff)) << np.uint32(8)) | ((i & np.uint32(0xff00ff00)) >> np.uint32(8))
    i = ((i & np.uint32(0x0f0f0f0f)) << np.uint32(4)) | ((i & np.uint32(0xf0f0f0f0)) >> np.uint32(4))
    i = ((i & np.uint32(0x33333333)) << np.uint32(2)) | ((i & np.uint32(0xcccccccc)) >> np.uint32(2))
    i = ((i & np.uint32(0x55555555)) << np.uint32(1)) | ((i & np.uint32(0xaaaaaaaa)) >> np.uint32(1))
    return i.astype(np.float64) * 2.0 ** -32


def hammersley2(n):
    """(n, 2) float32 points in [0,1)^2: the Hammersley set ((i + 0.5) / n, radical inverse of i in base 2).  The first
    coordinate picks the ring of the cosine map (u1), the second the azimuth (u2).  n up to 2^24: the radical inverse of such an
    i has at most 24 bits and is exact in float32, so no two points are equal."""
    n = int(n)
    if n < 1 or n > 1 << 24:
        raise ValueError(f"hammersley2: {n} points (1 .. 2^24)")
    i = np.arange(n, dtype=np.uint32)
    p = np.stack([(i.astype(np.float64) + 0.5) / n, _radical_inverse2(i)], axis=1).astype(np.float32)
    # (a first coordinate that rounds up to 1.0f: the largest float32 below it instead)
    return np.ascontiguousarray(np.minimum(p, np.nextafter(np.float32(1.0), np.float32(0.0))))


def texel_phases(n, seed=0):
    """(n,) float32 in [0,1): one rotation of the shared sample set per texel, from numpy's generator seeded with `seed`"""
    n = int(n)
    if n < 0:
        raise ValueError(f"texel_phases: {n} texels")
    p = np.random.default_rng(seed).random(n, dtype=np.float32)
    return np.ascontiguousarray(np.minimum(p, np.nextafter(np.float32(1.0), np.float32(0.0))))


def quad_texels(origin, eu, ev, nu, nv):
    """(positions (nu * nv, 3), normals (nu * nv, 3)), float32: the texel centres origin + (i + 0.5) / nu * eu +
    (j + 0.5) / nv * ev of the planar quad spanned by the edges eu and ev from `origin`, i running fastest, and the quad's unit
    normal eu x ev / |eu x ev| repeated for every texel.  Computed in float64, rounded once."""
    o, eu, ev = (np.asarray(a, np.float64).reshape(3) for a in (origin, eu, ev))
    nu, nv = int(nu), int(nv)
    if nu < 1 or nv < 1:
        raise ValueError(f"quad_texels: {nu} x {nv} texels")
    n = np.cross(eu, ev)
    length = math.sqrt(float(n @ n))
    if not length > 0.0:
        raise ValueError("quad_texels: the edges are parallel")
    n /= length
    a = (np.arange(nu) + 0.5) / nu
    b = (np.arange(nv) + 0.5) / nv
    pos = o[None, None, :] + b[:, None, None] * ev[None, None, :] + a[None, :, None] * eu[None, None, :]
    return (np.ascontiguousarray(pos.reshape(-1, 3).astype(np.float32)),
            np.ascontiguousarray(np.repeat(n[None, :], nu * nv, axis=0).astype(np.float32)))


def _rows(records):
    r = records.cpu().numpy() if hasattr(records, "cpu") else np.asarray(records)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"lightmap: rows of shape {r.shape}, expected (n, 8)")
    return r


def irradiance(records):
    """(n, 3) float32: pi times the mean radiance of query_irradiance's (n, 8) rows (one float32 product per value)"""
    return np.float32(math.pi) * _rows(records)[:, 0:3].astype(np.float32)


def invalid_texels(records, threshold):
    """(n,) bool: texels whose rays all hit something and on average within `threshold` -- hit_fraction == 1 and
    mean_distance < threshold: the texel lies inside or right under geometry, and a baker dilates its neighbours over it."""
    r = _rows(records)
    return (r[:, 5] >= np.float32(1.0)) & (r[:, 3] < np.float32(threshold))


def direct_irradiance(rows):
    """(n, 3) float32: the irradiance columns of query_direct's (n, 8) rows -- already an irradiance (the lights' radiance times
    attenuation times the cosine, over the sample's density), no factor of pi"""
    return np.ascontiguousarray(_rows(rows)[:, 0:3].astype(np.float32))


def penumbra_texels(rows):
    """(n,) bool: texels of query_direct's rows that some shadow samples reached and some did not -- lit_fraction > 0 and
    shadowed_fraction > 0: a sphere light's penumbra, or a texel lit by some lights of the range and shadowed from others.
    These are the texels that gain from more shadow samples."""
    r = _rows(rows)
    return (r[:, 3] > np.float32(0.0)) & (r[:, 4] > np.float32(0.0))


def total_irradiance(direct_rows, gather_rows):
    """(n, 3) float32: direct_irradiance(direct_rows) + irradiance(gather_rows), the direct term of the analytic lights at the
    texel plus pi times the gather's mean radiance (one float32 product and one sum per value).

    What this sum still LACKS: a gather ray takes no light sample at its first hit (the quirk of a caller's ray, include/ptrt.h),
    so the analytic lights' one-bounce term -- light that reaches the texel after exactly one diffuse reflection off the surface
    a gather ray hits first -- is absent; emissive meshes, the sky and every later bounce are in the gather.  A lit first vertex
    for the gather is not built."""
    d, g = direct_irradiance(direct_rows), irradiance(gather_rows)
    if d.shape != g.shape:
        raise ValueError(f"total_irradiance: {d.shape[0]} direct rows, {g.shape[0]} gather rows")
    return d + g
