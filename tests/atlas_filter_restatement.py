"""CPU restatement of ptrt_atlas_filter (csrc/pt_atlas_filter.hip.h) for the exact comparisons of tests/test_atlas_filter_gpu.py:
numpy float32, operation by operation as include/ptrt.h states the pass and as the kernel's -ffp-contract=off build has it --
every product, sum, difference and quotient is one rounded float32 operation.  Vectorised over texels; a Python loop over the
25 taps and the passes.

For texel p = (i, j), G = texels[p], C = src[p]:  G.mesh < 0 or C.valid == 0 copies C.  Otherwise, over the taps dy = -2..2
(outer), dx = -2..2 (inner) at q = (i + dx*step, j + dy*step), skipping -- by selection -- those outside the atlas, with
Gq.mesh < 0 or with Cq.valid == 0:
    h  = K[|dx|] * K[|dy|]                     K = {0.375, 0.25, 0.0625}
    e  = Gq.position - G.position
    d2 = (e.x*e.x + e.y*e.y) + e.z*e.z         x = 1 - d2 / rr          wd = x > 0 ? x : 0
    pd = (G.n.x*e.x + G.n.y*e.y) + G.n.z*e.z   y = 1 - (pd*pd) / pp     wp = y > 0 ? y : 0
    c  = (G.n.x*Gq.n.x + G.n.y*Gq.n.y) + G.n.z*Gq.n.z     c = c > 0 ? c : 0     normal_power times c = c*c
    w  = ((h * wd) * wp) * c                   !(w > 0): skipped, else  num += w * Cq.rgb,  den += w
with rr = (sigma_distance * step)^2 and pp = sigma_plane^2 formed in the working precision.  den == 0 copies C; otherwise
dst = {num / den, C.valid}.  Pass s has step 1 << s.

`filter` is that in float32; `filter64` is the same definition with every operation in float64 (the float32 inputs widened,
the result left in float64), for the bound of tests/test_atlas_filter.py."""
import numpy as np

K = (0.375, 0.25, 0.0625)
TAPS = tuple((dx, dy) for dy in range(-2, 3) for dx in range(-2, 3))


def _guides(texels, h, w, T):
    r = np.ascontiguousarray(np.asarray(texels, np.int32).reshape(h * w, 8))
    pos = np.ascontiguousarray(r[:, 0:3]).view(np.float32).reshape(h, w, 3).astype(T)
    nrm = np.ascontiguousarray(r[:, 4:7]).view(np.float32).reshape(h, w, 3).astype(T)
    return pos, nrm, r[:, 7].reshape(h, w) >= 0


def _shifted(a, dx, dy, fill):
    """b[j, i] = a[j + dy, i + dx] where that is inside, `fill` elsewhere"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    if abs(dx) < w and abs(dy) < h:
        b[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)] = a[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)]
    return b


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def filter_pass(pos, nrm, meshed, src, step, rr, pp, normal_power, T):
    """one pass over src (h, w, 4) of dtype T; rr, pp of dtype T; a new array"""
    usable = meshed & (src[:, :, 3] != 0)
    num = np.zeros(src.shape[:2] + (3,), T)
    den = np.zeros(src.shape[:2], T)
    one, zero = T(1.0), T(0.0)
    with np.errstate(all="ignore"):
        for dx, dy in TAPS:
            ok = _shifted(usable, dx * step, dy * step, False)
            if not ok.any():
                continue
            qp, qn = _shifted(pos, dx * step, dy * step, 0), _shifted(nrm, dx * step, dy * step, 0)
            qc = _shifted(src[:, :, 0:3], dx * step, dy * step, 0)
            hk = T(K[abs(dx)]) * T(K[abs(dy)])
            e = qp - pos
            d2 = _dot(e, e)
            x = one - d2 / rr
            wd = np.where(x > 0, x, zero)
            pd = _dot(nrm, e)
            y = one - (pd * pd) / pp
            wp = np.where(y > 0, y, zero)
            c = _dot(nrm, qn)
            c = np.where(c > 0, c, zero)
            for _ in range(normal_power):
                c = c * c
            wgt = ((hk * wd) * wp) * c
            take = ok & (wgt > 0)  # selection: what a skipped tap holds, NaN included, enters nothing
            num = np.where(take[:, :, None], num + wgt[:, :, None] * qc, num)
            den = np.where(take, den + wgt, den)
        out = src.copy()
        done = usable & (den != 0)
        out[done, 0:3] = num[done] / den[done][:, None]
    assert out.dtype == T
    return out


def _run(texels, image, passes, sigma_distance, sigma_plane, normal_power, T):
    image = np.asarray(image, np.float32)
    h, w, _ = image.shape
    pos, nrm, meshed = _guides(texels, h, w, T)
    img = image.astype(T)
    with np.errstate(all="ignore"):
        pp = T(sigma_plane) * T(sigma_plane)
        for s in range(passes):
            r = T(sigma_distance) * T(1 << s)
            img = filter_pass(pos, nrm, meshed, img, 1 << s, r * r, pp, normal_power, T)
    return img


def filter(texels, image, passes, sigma_distance, sigma_plane, normal_power):  # noqa: A001 (the issue's name)
    """ptrt_atlas_filter's result, float32 (h, w, 4): texels (h * w, 8) int32 rows, image (h, w, 4) float32"""
    return _run(texels, image, passes, np.float32(sigma_distance), np.float32(sigma_plane), normal_power, np.float32)


def filter64(texels, image, passes, sigma_distance, sigma_plane, normal_power):
    """the same definition in float64 from the same float32 inputs (the sigmas as float32, as the entry point takes them)"""
    return _run(texels, image, passes, np.float32(sigma_distance), np.float32(sigma_plane), normal_power, np.float64)


def records(pos, nrm, mesh, face=None):
    """(n, 8) int32 rows from positions (n, 3), normals (n, 3), mesh (n,) and face (n,)"""
    pos, nrm = np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 3)
    r = np.zeros((len(pos), 8), np.int32)
    r[:, 0:3], r[:, 4:7] = pos.view(np.int32), nrm.view(np.int32)
    r[:, 3] = 0 if face is None else face
    r[:, 7] = mesh
    return r
