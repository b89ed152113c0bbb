"""ptrt_query_probes restated in numpy float32, operation by operation (include/ptrt.h): the records ptrt_query_radiance gives
the probes' n * n_dirs rays -- ray (p, k) in row p * n_dirs + k -- the direction set, n_dirs and max_distance go to the (n, 32)
float32 rows the probe kernel must write, bit for bit.  `restate64` is the same statement in float64 with plain sums: the twin
the float32 order is bounded against (tests/test_probes.py)."""
import numpy as np

F = np.float32
C0, C1, C2, C6, C8 = F(0.282095), F(0.488603), F(1.092548), F(0.315392), F(0.546274)
QUANTITIES = 30  # sh[9][3], mean_distance, mean_distance_sq, hit_fraction


def basis32(directions):
    """(k, 9) float32: Y_i of the directions as given, in the header's operation order"""
    d = np.ascontiguousarray(directions, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    out = np.stack([np.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C6 * (F(3.0) * (z * z) - F(1.0)),
                    C2 * (x * z), C8 * (x * x - y * y)], axis=1)
    assert out.dtype == F
    return out


def terms32(radiance, depth, object_id, directions, n_dirs, max_distance):
    """(n, n_dirs, 30) float32: every ray's term of every quantity"""
    L = np.ascontiguousarray(radiance, F).reshape(-1, n_dirs, 3)
    n = L.shape[0]
    Y = basis32(directions)
    assert Y.shape == (n_dirs, 9)
    t = np.empty((n, n_dirs, QUANTITIES), F)
    t[:, :, :27] = (Y[None, :, :, None] * L[:, :, None, :]).reshape(n, n_dirs, 27)  # sh[i][c] in column 3 * i + c
    dist = np.minimum(np.ascontiguousarray(depth, F).reshape(n, n_dirs), F(max_distance))
    t[:, :, 27] = dist
    with np.errstate(over="ignore"):  # (a miss under the default max_distance of 1e30: the square is +inf, on the device too)
        t[:, :, 28] = dist * dist
    t[:, :, 29] = np.where(np.asarray(object_id).reshape(n, n_dirs) >= 0, F(1.0), F(0.0))
    return t


def fold64(v):
    """v[j] + v[j + 32], then 16, 8, 4, 2, 1 along axis 1 (of length 64)"""
    assert v.shape[1] == 64 and v.dtype == F
    for h in (32, 16, 8, 4, 2, 1):
        v = v[:, :h] + v[:, h:2 * h]
    return v[:, 0]


def restate(radiance, depth, object_id, directions, n_dirs, max_distance):
    """(n, 32) float32 rows of ptrt_probe"""
    t = terms32(radiance, depth, object_id, directions, n_dirs, max_distance)
    n = t.shape[0]
    chunks = (n_dirs + 63) // 64
    padded = np.zeros((n, chunks * 64, QUANTITIES), F)  # +0.0f for absent k
    padded[:, :n_dirs] = t
    total = np.zeros((n, QUANTITIES), F)                 # starts at +0.0f
    for c in range(chunks):
        total = total + fold64(padded[:, c * 64:(c + 1) * 64])
    out = np.zeros((n, 32), F)                            # reserved: 0.0f
    out[:, :QUANTITIES] = total / F(n_dirs)
    assert total.dtype == F
    return out


def restate64(radiance, depth, object_id, directions, n_dirs, max_distance):
    """(n, 30) float64: the same quantities from the same float32 inputs and constants, every operation in float64"""
    L = np.asarray(radiance, np.float64).reshape(-1, n_dirs, 3)
    n = L.shape[0]
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c6, c8 = (float(c) for c in (C0, C1, C2, C6, C8))
    Y = np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c6 * (3.0 * (z * z) - 1.0),
                  c2 * (x * z), c8 * (x * x - y * y)], axis=1)
    out = np.empty((n, QUANTITIES))
    out[:, :27] = (Y[None, :, :, None] * L[:, :, None, :]).reshape(n, n_dirs, 27).sum(axis=1) / n_dirs
    dist = np.minimum(np.asarray(depth, np.float64).reshape(n, n_dirs), float(F(max_distance)))
    out[:, 27] = dist.sum(axis=1) / n_dirs
    out[:, 28] = (dist * dist).sum(axis=1) / n_dirs
    out[:, 29] = (np.asarray(object_id).reshape(n, n_dirs) >= 0).sum(axis=1) / n_dirs
    return out


def magnitudes64(radiance, depth, directions, n_dirs, max_distance):
    """(n, 30) float64: M_i, the mean of every term with each of its own terms taken absolute -- A_i(d_k) * |L_k| for the
    coefficients (A_6 = c6 * (3 z^2 + 1), A_8 = c8 * (x^2 + y^2)), dist, dist^2 and 1 for the rest"""
    L = np.abs(np.asarray(radiance, np.float64).reshape(-1, n_dirs, 3))
    n = L.shape[0]
    d = np.abs(np.asarray(directions, np.float64).reshape(-1, 3))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c6, c8 = (float(c) for c in (C0, C1, C2, C6, C8))
    A = np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c6 * (3.0 * (z * z) + 1.0),
                  c2 * (x * z), c8 * (x * x + y * y)], axis=1)
    out = np.empty((n, QUANTITIES))
    out[:, :27] = (A[None, :, :, None] * L[:, :, None, :]).reshape(n, n_dirs, 27).sum(axis=1) / n_dirs
    dist = np.minimum(np.asarray(depth, np.float64).reshape(n, n_dirs), float(F(max_distance)))
    out[:, 27] = dist.sum(axis=1) / n_dirs
    out[:, 28] = (dist * dist).sum(axis=1) / n_dirs
    out[:, 29] = 1.0
    return out
