"""CPU restatement of the lightmap atlas kernels (csrc/pt_atlas.hip.h: ptrt_atlas_texels, ptrt_atlas_dilate) for the exact
comparisons of tests/test_atlas_gpu.py.  numpy float32, operation by operation as the kernels' -ffp-contract=off build has
them: every product, sum and quotient is one rounded float32 operation; dot and cross are the fused forms of the numerics
contract (rt_restatement, on wireframe_restatement's fma32); normalize is rt_restatement's (IEEE square root and quotients,
which the device's guarded cores equal bit for bit).

Coverage (include/ptrt.h), for the centre p = (i + 0.5, j + 0.5) of texel (i, j) and the corners 0, 1, 2 of a face:
    d1 = (x1-x0, y1-y0)   d2 = (x2-x0, y2-y0)   q = (px-x0, py-y0)        A = d1x*d2y - d1y*d2x
    b1 = (qx*d2y - qy*d2x) / A      b2 = (d1x*qy - d1y*qx) / A      b0 = (1 - b1) - b2
    covered  <=>  b0 >= 0 && b1 >= 0 && b2 >= 0
over the face's scan range -- columns max(floor(min x) - 1, 0) .. min(ceil(max x), w - 1), rows alike --; a face with a
non-finite corner, A == 0 or A NaN covers nothing.  The lowest covering face owns a texel; with clear == 0 a texel that has
mesh >= 0 is kept whole.  Records are (n, 8) int32 rows: position bits 0:3, face 3, normal bits 4:7, mesh 7; the empty record
is {0, 0, 0, INT32_MAX, 0, 0, 0, -1} (its face word is unspecified by the contract: `comparable` masks it)."""
import numpy as np

from rt_restatement import cross, normalize

f32 = np.float32
NO_FACE = np.int32(0x7fffffff)


def empty_records(w, h):
    r = np.zeros((w * h, 8), np.int32)
    r[:, 3] = NO_FACE
    r[:, 7] = -1
    return r


def comparable(records):
    """a copy with the face word of the empty records (unspecified) set to 0"""
    r = np.array(records, np.int32, copy=True)
    r[r[:, 7] < 0, 3] = 0
    return r


def scan_range(c, w, h):
    """(i0, i1, j0, j1) of the face with corners c = (x0, y0, x1, y1, x2, y2) float32, or None where it covers nothing"""
    c = np.asarray(c, f32)
    if not np.isfinite(c).all():
        return None
    xs, ys = c[0::2], c[1::2]
    fi0 = max(f32(np.floor(xs.min()) - f32(1.0)), f32(0.0))
    fj0 = max(f32(np.floor(ys.min()) - f32(1.0)), f32(0.0))
    fi1 = min(f32(np.ceil(xs.max())), f32(w - 1))
    fj1 = min(f32(np.ceil(ys.max())), f32(h - 1))
    if fi0 > fi1 or fj0 > fj1:
        return None
    i0, j0, i1, j1 = int(fi0), int(fj0), min(int(fi1), w - 1), min(int(fj1), h - 1)
    if i0 > i1 or j0 > j1:
        return None
    return i0, i1, j0, j1


def face_coverage(c, w, h):
    """(texel indices, b1, b2) of the centres the face covers, float32 barycentrics as the kernel computes them"""
    none = (np.zeros(0, np.int64), np.zeros(0, f32), np.zeros(0, f32))
    c = np.asarray(c, f32)
    rng = scan_range(c, w, h)
    if rng is None:
        return none
    with np.errstate(all="ignore"):
        x0, y0, x1, y1, x2, y2 = c
        d1x, d1y, d2x, d2y = f32(x1 - x0), f32(y1 - y0), f32(x2 - x0), f32(y2 - y0)
        A = f32(f32(d1x * d2y) - f32(d1y * d2x))
        if A == 0 or A != A:
            return none
        i0, i1, j0, j1 = rng
        ii, jj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1))
        qx = ((ii.astype(f32) + f32(0.5)) - x0).astype(f32)
        qy = ((jj.astype(f32) + f32(0.5)) - y0).astype(f32)
        b1 = (((qx * d2y).astype(f32) - (qy * d2x).astype(f32)).astype(f32) / A).astype(f32)
        b2 = (((d1x * qy).astype(f32) - (d1y * qx).astype(f32)).astype(f32) / A).astype(f32)
        b0 = ((f32(1.0) - b1).astype(f32) - b2).astype(f32)
        ok = (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
    return (jj[ok].astype(np.int64) * w + ii[ok]), b1[ok], b2[ok]


def atlas_texels(verts, faces, uv, w, h, mesh, world=None, normal=None, has_transform=False, clear=True, records=None,
                 in_slots=None):
    """The records ptrt_atlas_texels leaves.  verts (V, 3) float32 and faces (F, 3): the mesh as uploaded (or as last refitted);
    uv (F, 6) float32; world, normal: the mesh's 16-float row-major matrices, read when has_transform; records: what an earlier
    call left (clear False); in_slots: (F,) bool, the faces some leaf slot holds (None: all)."""
    verts = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, f32).reshape(-1, 6)
    assert len(uv) == len(faces)
    out = empty_records(w, h) if clear else np.array(records, np.int32, copy=True)
    assert out.shape == (w * h, 8)
    owned = out[:, 7] >= 0  # by an earlier call
    out[~owned, 3] = NO_FACE
    best = np.full(w * h, NO_FACE, np.int64)
    bary = {}
    for f in range(len(faces)):
        if in_slots is not None and not in_slots[f]:
            continue
        idx, b1, b2 = face_coverage(uv[f], w, h)
        take = ~owned[idx] & (f < best[idx])  # ascending f: the first face to cover a texel keeps it
        best[idx[take]] = f
        bary[f] = (idx[take], b1[take], b2[take])
    W = None if not has_transform else np.asarray(world, f32).reshape(4, 4)
    N = None if not has_transform else np.asarray(normal, f32).reshape(4, 4)
    for f, (idx, b1, b2) in bary.items():
        if len(idx) == 0:
            continue
        v0 = verts[faces[f, 0]]
        e1 = (verts[faces[f, 1]] - v0).astype(f32)  # the upload's own subtractions
        e2 = (verts[faces[f, 2]] - v0).astype(f32)
        gn = normalize(cross(e1[None, :], e2[None, :]))[0]
        p = ((v0[None, :] + (b1[:, None] * e1[None, :]).astype(f32)).astype(f32) + (b2[:, None] * e2[None, :]).astype(f32)).astype(f32)
        n = gn
        if has_transform:
            p = np.stack([((((W[r, 0] * p[:, 0]).astype(f32) + (W[r, 1] * p[:, 1]).astype(f32)).astype(f32)
                            + (W[r, 2] * p[:, 2]).astype(f32)).astype(f32) + W[r, 3]).astype(f32) for r in range(3)], axis=1)
            d = np.array([f32(f32(f32(N[r, 0] * gn[0]) + f32(N[r, 1] * gn[1])) + f32(N[r, 2] * gn[2])) for r in range(3)], f32)
            n = normalize(d[None, :])[0]
        rows = np.zeros((len(idx), 8), np.int32)
        rows[:, 0:3] = p.view(np.int32)
        rows[:, 3] = f
        rows[:, 4:7] = np.asarray(n, f32).view(np.int32)[None, :]
        rows[:, 7] = mesh
        out[idx] = rows
    return out


NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def dilate_pass(img):
    """one pass of ptrt_atlas_dilate over img (h, w, 4) float32: a new array"""
    img = np.asarray(img, f32)
    h, w, _ = img.shape
    valid = img[:, :, 3] != 0
    s = np.zeros((h, w, 3), f32)
    n = np.zeros((h, w), np.int32)
    with np.errstate(all="ignore"):
        for dx, dy in NEIGHBOURS:
            src = np.zeros((h, w, 3), f32)
            ok = np.zeros((h, w), bool)
            ys, yd = (slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0)))
            xs, xd = (slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0)))
            src[yd, xd] = img[ys, xs, 0:3]
            ok[yd, xd] = valid[ys, xs]
            s = np.where(ok[:, :, None], (s + src).astype(f32), s)  # a neighbour that is not valid is not added, not added as 0
            n += ok
        out = img.copy()
        fill = ~valid & (n > 0)
        out[fill, 0:3] = (s[fill] / n[fill].astype(f32)[:, None]).astype(f32)
        out[fill, 3] = f32(1.0)
    return out


def dilate(img, passes):
    for _ in range(passes):
        img = dilate_pass(img)
    return img
