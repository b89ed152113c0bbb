"""Around Scene.query_probes: direction sets, probe grids and what to do with the nine coefficients.  Plain numpy, no device
code -- the arrays go to the device with torch.from_numpy(..).cuda() and the (n, 32) rows come back with .cpu().numpy().

A probe-lit view of a scene: bake `ProbeVolume.positions()` with Scene.query_probes, then Scene.camera_rays, then
Scene.query_probe_light, then `shade_probe_light`.  Scene.probe_sample lights points that are no ray hits (moving objects).

The basis is the real spherical harmonics of bands 0-2 in the order of `ptrt_probe.sh` (include/ptrt.h), z the polar axis:
1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2, each with its normalisation.  The kernel multiplies by six-digit float32
constants; `sh9_basis` uses the exact ones in float64."""
import math

import numpy as np

# cosine-lobe factors per coefficient: A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4 (Ramamoorthi and Hanrahan 2001)
COSINE_LOBE = np.array([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5)


def fibonacci_sphere(k):
    """(k, 3) float32 unit directions spread evenly over the sphere: the spherical Fibonacci lattice, z descending from
    1 - 1/k in equal steps, the azimuth advancing by the golden angle.  Normalised in float64, rounded once."""
    k = int(k)
    if k < 1:
        raise ValueError(f"fibonacci_sphere: {k} directions")
    i = np.arange(k, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / k
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(d.astype(np.float32))


def probe_grid(lo, hi, counts):
    """(nx * ny * nz, 3) float32 positions of a regular grid from corner `lo` to corner `hi`, both included, `counts` =
    (nx, ny, nz) probes per axis (an axis with one probe sits at its middle); x runs fastest, then y, then z."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    counts = [int(c) for c in counts]
    if len(counts) != 3 or min(counts) < 1:
        raise ValueError(f"probe_grid: counts {counts}")
    axes = [np.linspace(lo[a], hi[a], counts[a]) if counts[a] > 1 else np.array([0.5 * (lo[a] + hi[a])]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32))


def sh9_basis(dirs):
    """(n, 9) float64: the nine basis functions at the (n, 3) directions, which are used as given (unit vectors expected)."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0 = 0.5 * math.sqrt(1.0 / math.pi)
    c1 = math.sqrt(3.0 / (4.0 * math.pi))
    c2 = 0.5 * math.sqrt(15.0 / math.pi)
    c6 = 0.25 * math.sqrt(5.0 / math.pi)
    c8 = 0.25 * math.sqrt(15.0 / math.pi)
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c6 * (3.0 * (z * z) - 1.0),
                     c2 * (x * z), c8 * (x * x - y * y)], axis=1)


def sh9_irradiance(coeffs, normals):
    """Irradiance at surface normals from a probe's coefficients.  `coeffs`: (9, C) or (n, 9, C), the MEANS query_probes
    returns for directions uniform on the sphere (probe_fields(..)["sh"]); they are multiplied by 4 pi to become the
    projection integrals, then by the cosine lobe's factors pi, 2 pi / 3, pi / 4 per band, and summed against the basis at
    `normals` (m, 3).  Returns float64 (m, C) or (n, m, C).  Exact for radiance of bands 0-2; a band-limited estimate
    otherwise."""
    c = np.asarray(coeffs, np.float64)
    if c.ndim not in (2, 3) or c.shape[-2] != 9:
        raise ValueError(f"sh9_irradiance: coefficients of shape {c.shape}, expected (9, C) or (n, 9, C)")
    w = sh9_basis(normals) * (4.0 * math.pi * COSINE_LOBE)[None, :]
    return np.einsum("mi,...ic->...mc", w, c)


class ProbeVolume:
    """A regular grid of probes as Scene.probe_sample / query_probe_light read it (ptrt_probe_volume): probe (i, j, k) stands at
    origin + (i, j, k) * spacing and is row i + nx * (j + ny * k) of the probe records -- `probe_grid`'s order.  origin and
    spacing are kept as float32, the numbers the device gets."""

    def __init__(self, origin, spacing, counts):
        self.origin = np.asarray(origin, np.float32).reshape(3).copy()
        self.spacing = np.asarray(spacing, np.float32).reshape(3).copy()
        counts = [int(c) for c in counts]
        if len(counts) != 3 or min(counts) < 1 or counts[0] * counts[1] * counts[2] > 2 ** 24:
            raise ValueError(f"ProbeVolume: counts {counts} (three, each >= 1, at most 2^24 probes)")
        if not (np.isfinite(self.spacing).all() and (self.spacing > 0).all() and np.isfinite(self.origin).all()):
            raise ValueError(f"ProbeVolume: spacing {self.spacing.tolist()} (positive and finite), origin {self.origin.tolist()} (finite)")
        self.counts = tuple(counts)

    @classmethod
    def from_corners(cls, lo, hi, counts):
        """The volume whose probes run from corner `lo` to corner `hi`: spacing (hi - lo) / (count - 1) formed in float64 and
        rounded once; an axis with one probe sits at lo and gets the spacing hi - lo (or 1 where that is 0), which only scales
        a coordinate that is clamped to 0 anyway."""
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        counts = [int(c) for c in counts]
        if len(counts) != 3 or min(counts) < 1:
            raise ValueError(f"ProbeVolume.from_corners: counts {counts}")
        ext = hi - lo
        spacing = [ext[a] / (counts[a] - 1) if counts[a] > 1 else (ext[a] if ext[a] > 0 else 1.0) for a in range(3)]
        return cls(lo, spacing, counts)

    @property
    def rows(self):
        return self.counts[0] * self.counts[1] * self.counts[2]

    def corners(self):
        """(lo, hi): the first and the last probe's positions, float32 (3,) each"""
        top = np.asarray(self.counts, np.float32) - np.float32(1.0)
        return self.origin.copy(), (self.origin + top * self.spacing).astype(np.float32)

    def positions(self):
        """(nx * ny * nz, 3) float32, x fastest: origin + float32(i) * spacing in float32, the product rounded, then the sum --
        the sampler's own Q, so probes baked here sit exactly where it assumes."""
        ax = [(self.origin[a] + np.arange(self.counts[a], dtype=np.float32) * self.spacing[a]).astype(np.float32) for a in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))

    def __repr__(self):
        return f"ProbeVolume(origin={self.origin.tolist()}, spacing={self.spacing.tolist()}, counts={self.counts})"


# columns of the (n, 8) int32 rows of Scene.probe_sample / query_probe_light: the fields of ptrt_probe_light
PROBE_LIGHT_COLUMNS = dict(irradiance=(0, 3, True), weight=(3, 4, True), cell=(4, 5, False), used=(5, 6, False), face=(6, 7, False),
                           mesh=(7, 8, False))


def _light_rows(rows):
    if getattr(rows, "ndim", None) != 2 or rows.shape[1] != 8 or "int32" not in str(rows.dtype):
        raise ValueError(f"probe light rows: expected (n, 8) int32, got {getattr(rows, 'shape', None)} of {getattr(rows, 'dtype', type(rows).__name__)}")
    return rows


def probe_light_fields(rows):
    """Named views of probe_sample's and query_probe_light's (n, 8) int32 rows (a tensor or an array): irradiance (n, 3) and
    weight (n,) reinterpreted as float32; cell, used, face and mesh int32, (n,)."""
    from . import _flagged, _named_columns
    return _named_columns(_light_rows(rows), PROBE_LIGHT_COLUMNS, ("float32", _flagged(PROBE_LIGHT_COLUMNS, True)))


def shade_probe_light(rows, albedo, background=(0.0, 0.0, 0.0)):
    """(n, 3) float32, the Lambertian view of a probe-lit surface: (albedo * irradiance) / pi, each step one float32 operation
    -- the product, then the quotient by float32(pi).  `albedo`: (M, 3), one row per uploaded mesh, looked up by the rows' mesh
    column, with `background` on a miss (mesh < 0); or (3,), one albedo for every row (probe_sample's rows carry no mesh).  Arrays or tensors, answered in the kind of `rows`; the counterpart of lightmap.shade_samples.

    A probe-lit view of a scene is Scene.camera_rays, then Scene.query_probe_light, then this."""
    rows = _light_rows(rows)
    f = probe_light_fields(rows)
    n = rows.shape[0]
    if hasattr(rows, "cpu"):
        import torch
        a = torch.as_tensor(albedo, dtype=torch.float32, device=rows.device)
        bg = torch.as_tensor(background, dtype=torch.float32, device=rows.device)
        mesh = f["mesh"].to(torch.int64)
        pi, where, clamp = torch.tensor(math.pi, dtype=torch.float32, device=rows.device), torch.where, lambda m: m.clamp(min=0)
    else:
        a = np.asarray(albedo.cpu() if hasattr(albedo, "cpu") else albedo, np.float32)
        bg = np.asarray(background, np.float32)
        mesh = f["mesh"].astype(np.int64)
        pi, where, clamp = np.float32(math.pi), np.where, lambda m: np.maximum(m, 0)
    if tuple(bg.shape) != (3,):
        raise ValueError(f"shade_probe_light: background {tuple(bg.shape)}, expected (3,)")
    if tuple(a.shape) == (3,):
        return (a * f["irradiance"]) / pi
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"shade_probe_light: albedo {tuple(a.shape)}, expected (M, 3) or (3,)")
    if n and int(mesh.max()) >= a.shape[0]:
        raise ValueError(f"shade_probe_light: a row of mesh {int(mesh.max())}, albedo has {a.shape[0]} rows")
    lit = (a[clamp(mesh)] * f["irradiance"]) / pi
    return where((mesh >= 0)[:, None], lit, bg[None, :].expand(n, 3) if hasattr(rows, "cpu") else np.broadcast_to(bg, (n, 3)))
