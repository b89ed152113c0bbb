"""What pt::compose_poses_kernel computes (ptrt_set_instance_poses_device), restated in numpy float32 operation by operation from
the reference's text: Transform3D::updateMatrices (transform.cuh:260-306), mat4::inverse and mat4::operator* (mat4.cuh:211-262,
280-323), the has_transform rule (scene.cuh:718-721) and vec3::length (vec3.cuh:99-101).  Every product and every sum is a numpy
operation of its own on float32 arrays, so each is rounded once, in the order the expressions are written; nothing is fused.
No GPU, no library call in the restatement itself: sine and cosine come in through `sincos`."""
import numpy as np

F = np.float32


def detmath_sincos(O):
    """sine and cosine as the device computes them: dm_sin / dm_cos of oracle/detmath.h"""
    return lambda x: (O.detmath(0, x), O.detmath(1, x))


def libm_sincos(x):
    """float64 sine and cosine rounded to float32: some libm's, for nothing in particular"""
    x = np.asarray(x, np.float32).astype(np.float64)
    return np.sin(x).astype(np.float32), np.cos(x).astype(np.float32)


def _mul(a, b):
    """mat4::operator*, the typo in r.m[3] included (b.m[11] where b.m[1] belongs); a, b: lists of 16 float32 arrays"""
    r = [None] * 16
    for c in range(4):
        for k in range(4):
            b1 = b[11] if (c == 0 and k == 3) else b[c * 4 + 1]
            r[c * 4 + k] = ((a[k] * b[c * 4] + a[4 + k] * b1) + a[8 + k] * b[c * 4 + 2]) + a[12 + k] * b[c * 4 + 3]
    return r


def _length(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def compose(position, rotation, scale, sincos):
    """(world rows, inverse rows, normal rows, has_transform): (n, 3, 4) float32 each -- a normal row's fourth word is 0, as
    in the mesh records -- and (n,) int32.  position, rotation, scale: (n, 3); sincos(x) -> (sin x, cos x) as float32."""
    p = np.ascontiguousarray(position, np.float32).reshape(-1, 3)
    r = np.ascontiguousarray(rotation, np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(scale, np.float32).reshape(-1, 3)
    n = len(p)
    zero, one = np.zeros(n, F), np.ones(n, F)
    with np.errstate(all="ignore"):
        (sx, cx), (sy, cy), (sz, cz) = (tuple(np.asarray(v, F) for v in sincos(np.ascontiguousarray(r[:, k]))) for k in range(3))
        rot = [cy * cz, cz * sx * sy - cx * sz, cx * cz * sy + sx * sz, zero,
               cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx, zero,
               -sy, cy * sx, cx * cy, zero,
               zero, zero, zero, one]
        w = [zero] * 16
        w[0], w[5], w[10], w[15] = s[:, 0], s[:, 1], s[:, 2], one
        m = _mul(rot, w)
        m[3], m[7], m[11] = p[:, 0], p[:, 1], p[:, 2]
        A2323 = m[10] * m[15] - m[11] * m[14]
        A1323 = m[9] * m[15] - m[11] * m[13]
        A1223 = m[9] * m[14] - m[10] * m[13]
        A0323 = m[8] * m[15] - m[11] * m[12]
        A0223 = m[8] * m[14] - m[10] * m[12]
        A0123 = m[8] * m[13] - m[9] * m[12]
        A2313 = m[6] * m[15] - m[7] * m[14]
        A1313 = m[5] * m[15] - m[7] * m[13]
        A1213 = m[5] * m[14] - m[6] * m[13]
        A0313 = m[4] * m[15] - m[7] * m[12]
        A0213 = m[4] * m[14] - m[6] * m[12]
        A0113 = m[4] * m[13] - m[5] * m[12]
        A2312 = m[6] * m[11] - m[7] * m[10]
        A1312 = m[5] * m[11] - m[7] * m[9]
        A1212 = m[5] * m[10] - m[6] * m[9]
        A0312 = m[4] * m[11] - m[7] * m[8]
        A0212 = m[4] * m[10] - m[6] * m[8]
        A0112 = m[4] * m[9] - m[5] * m[8]
        det = (m[0] * (m[5] * A2323 - m[6] * A1323 + m[7] * A1223) - m[1] * (m[4] * A2323 - m[6] * A0323 + m[7] * A0223) +
               m[2] * (m[4] * A1323 - m[5] * A0323 + m[7] * A0123) - m[3] * (m[4] * A1223 - m[5] * A0223 + m[6] * A0123))
        invDet = F(1.0) / det
        inv = [invDet * (m[5] * A2323 - m[6] * A1323 + m[7] * A1223),
               invDet * -(m[1] * A2323 - m[2] * A1323 + m[3] * A1223),
               invDet * (m[1] * A2313 - m[2] * A1313 + m[3] * A1213),
               invDet * -(m[1] * A2312 - m[2] * A1312 + m[3] * A1212),
               invDet * -(m[4] * A2323 - m[6] * A0323 + m[7] * A0223),
               invDet * (m[0] * A2323 - m[2] * A0323 + m[3] * A0223),
               invDet * -(m[0] * A2313 - m[2] * A0313 + m[3] * A0113),
               invDet * (m[0] * A2312 - m[2] * A0312 + m[3] * A0112),
               invDet * (m[4] * A1323 - m[5] * A0323 + m[7] * A0123),
               invDet * -(m[0] * A1323 - m[1] * A0323 + m[3] * A0123),
               invDet * (m[0] * A1313 - m[1] * A0313 + m[3] * A0113),
               invDet * -(m[0] * A1312 - m[1] * A0312 + m[3] * A0112),
               invDet * -(m[4] * A1223 - m[5] * A0223 + m[6] * A0123),
               invDet * (m[0] * A1223 - m[1] * A0223 + m[2] * A0123),
               invDet * -(m[0] * A1213 - m[1] * A0213 + m[2] * A0113),
               invDet * (m[0] * A1212 - m[1] * A0212 + m[2] * A0112)]
        singular = np.abs(det) < F(1e-10)                     # (false for a NaN determinant, as in C)
        eye = [one if k % 5 == 0 else zero for k in range(16)]
        inv = [np.where(singular, eye[k], inv[k]).astype(F) for k in range(16)]
        has = (_length(p) > F(0.001)) | (_length(r) > F(0.001)) | (np.abs(s[:, 0] - F(1.0)) > F(0.001))
    for a in m + inv + [det]:
        assert a.dtype == np.float32
    world = np.stack(m[:12], axis=1).reshape(n, 3, 4)
    inverse = np.stack(inv[:12], axis=1).reshape(n, 3, 4)
    normal = np.stack([zero if c == 3 else inv[c * 4 + row] for row in range(3) for c in range(4)], axis=1).reshape(n, 3, 4)
    return world, inverse, normal, has.astype(np.int32)
