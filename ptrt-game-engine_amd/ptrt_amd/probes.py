"""Around Scene.query_probes: direction sets, probe grids and what to do with the nine coefficients.  Plain numpy, no device
code -- the arrays go to the device with torch.from_numpy(..).cuda() and the (n, 32) rows come back with .cpu().numpy().

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
