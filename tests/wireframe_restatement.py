"""CPU restatement of the wireframe view (render_kernel_wireframe, scene_kernels.cuh:53-117, wireframeMode true) for
the exact comparison of tests/test_wireframe_gpu.py.

numpy float32, in the reference's operation order: every product and sum is one rounded float32 operation, as in the
kernels' -ffp-contract=off build.  The one fused operation is the one the source spells: dot() is
fma(z, z, fma(y, y, x * x)) (vec3.cuh, see the arithmetic contract of oracle/ptrt_oracle.cpp), restated by `fma32`.
sqrt and the quotients are IEEE float32 (what sqrt_ieee / normalize / the kernel's divisions compute); sin, cos, atan2,
acos and pow are the oracle's deterministic versions (oracle.detmath ops 0, 1, 5, 6, 4), which equal the device ones
bit for bit.  Closest hits come from the oracle's traceRay (oracle.trace_rays).
"""
import ctypes as C

import numpy as np

f32 = np.float32
PI_F = f32(3.14159265358979323846)
TWO_PI_F = f32(6.28318530717958647692)
GAMMA = f32(1.0) / f32(2.2)


def fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded: a*b is exact in float64, the float64 sum's error is exact (TwoSum), and the
    only case where rounding that sum to float32 differs from rounding the exact value is a sum that lands on a float32
    midpoint while the error is not zero -- there the error's sign picks the neighbour."""
    a, b, c = (np.asarray(v, dtype=f32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    with np.errstate(over="ignore"):
        r = s.astype(f32)
        n = np.nextafter(r, np.where(s > r.astype(np.float64), f32(np.inf), f32(-np.inf)).astype(f32))
    mid = (r.astype(np.float64) + n.astype(np.float64)) * 0.5
    tie = (s == mid) & (e != 0) & (r.astype(np.float64) != s)
    lo, hi = np.minimum(r, n), np.maximum(r, n)
    return np.where(tie, np.where(e > 0, hi, lo), r).astype(f32)


def dot(a, b):
    return fma32(a[2], b[2], fma32(a[1], b[1], a[0] * b[0]))


def normalize(v):
    """vec3::normalized (vec3.cuh:107-110): v / |v| component by component, 0 for a zero vector."""
    ln = np.sqrt(dot(v, v))
    safe = np.where(ln > 0, ln, f32(1))
    return [np.where(ln > 0, c / safe, f32(0)).astype(f32) for c in v]


def disk_hash(x, y, O):
    """Camera::random_in_unit_disk_hash(x, y) (camera.cuh:55-70) for uint32 arrays: (px, py); pz is 0."""
    x = np.asarray(x, dtype=np.uint32)
    y = np.asarray(y, dtype=np.uint32)
    with np.errstate(over="ignore"):
        seed = (x * np.uint32(1973)) ^ (y * np.uint32(9277)) ^ np.uint32(0x9e3779b9)
        seed ^= seed >> np.uint32(17)
        seed *= np.uint32(0xed5ad4bb)
        seed ^= seed >> np.uint32(11)
        seed *= np.uint32(0xac4c1b51)
        seed ^= seed >> np.uint32(15)
        seed *= np.uint32(0x31848bab)
        seed ^= seed >> np.uint32(14)
        r1 = ((seed & np.uint32(0xFFFF)).astype(f32) + f32(0.5)) / f32(65536.0)
        r2 = (((seed * np.uint32(0x343fd) + np.uint32(0xc0f5)) & np.uint32(0xFFFF)).astype(f32) + f32(0.5)) / f32(65536.0)
    r = np.sqrt(r1)
    phi = f32(6.2831853) * r2
    return r * O.detmath(1, phi), r * O.detmath(0, phi)


def gamma(c, O):
    """powf(c, 1 / 2.2): 0 where c <= 0 (powf(0, y) = 0; a negative c is NaN, which the clamp makes 0)."""
    c = np.asarray(c, dtype=f32)
    pos = c > 0
    out = np.zeros_like(c)
    if pos.any():
        out[pos] = O.detmath(4, c[pos], np.full(int(pos.sum()), GAMMA, dtype=f32))
    return out


def edge_colour(emission):
    """Colour of an edge pixel: its mesh's emission if emission.x > 0 -- only .x is tested -- and white otherwise."""
    e = np.asarray(emission, dtype=f32).reshape(-1, 3)
    return np.where((e[:, 0] > 0)[:, None], e, f32(1.0)).astype(f32)


def reinhard_gamma_rgb8(c, O):
    """c / (c + 1), powf(c, 1 / 2.2), clamp to [0, 1], * 255.99, truncated to uint8 (scene_kernels.cuh:106-116)."""
    c = np.asarray(c, dtype=f32)
    c = c / (c + f32(1.0))
    g = np.minimum(np.maximum(gamma(c, O), f32(0)), f32(1)) * f32(255.99)
    return g.astype(np.int32).astype(np.uint8)


def tex2d_env(env, u, v):
    """pt_device.hip.h tex2d_env: tex2D<float4> of Scene::loadHDRI's texture (normalised coordinates, wrap in u, clamp
    in v, linear filter with 8-bit weights).  env: (h, w, 4) float32."""
    h, w = env.shape[0], env.shape[1]
    uw = u - np.floor(u)
    vmax = f32(1.0) - f32(1.0) / f32(h)
    vc = np.where(v < 0, f32(0), np.where(v >= f32(1), vmax, v)).astype(f32)
    xB = uw * f32(w) - f32(0.5)
    yB = vc * f32(h) - f32(0.5)
    fi, fj = np.floor(xB), np.floor(yB)
    a = np.rint((xB - fi) * f32(256.0)) * f32(1.0 / 256.0)
    b = np.rint((yB - fj) * f32(256.0)) * f32(1.0 / 256.0)
    i, j = fi.astype(np.int64), fj.astype(np.int64)

    def texel(ii, jj):
        return env[np.clip(jj, 0, h - 1), np.mod(ii, w), :3]

    w00 = (f32(1) - a) * (f32(1) - b)
    w10 = a * (f32(1) - b)
    w01 = (f32(1) - a) * b
    w11 = a * b
    t00, t10, t01, t11 = texel(i, j), texel(i + 1, j), texel(i, j + 1), texel(i + 1, j + 1)
    return ((t00 * w00[:, None] + t10 * w10[:, None]) + t01 * w01[:, None]) + t11 * w11[:, None]


def _v(p):
    return np.array([p.x, p.y, p.z], dtype=f32)


def primary_rays(cam, W, H, y0, rows, O):
    """Camera::get_ray(s, t), device branch (camera.cuh:173-199), for the pixels of rows y0 .. y0 + rows - 1:
    (origins, directions) as (rows * W, 3) float32, row-major from row y0."""
    xs, ys = np.meshgrid(np.arange(W), np.arange(y0, y0 + rows))
    s = (xs.reshape(-1).astype(f32) + f32(0.5)) / f32(W)
    t = f32(1.0) - (ys.reshape(-1).astype(f32) + f32(0.5)) / f32(H)
    llc, hor, ver, org = _v(cam.lower_left_corner), _v(cam.horizontal), _v(cam.vertical), _v(cam.origin)
    d = [((llc[k] + s * hor[k]) + t * ver[k]) - org[k] for k in range(3)]
    o = [np.full_like(s, org[k]) for k in range(3)]
    lr = f32(cam.lens_radius)
    if not lr <= 0:
        with np.errstate(over="ignore", invalid="ignore"):
            hx = (s * f32(10000.0)).astype(np.uint32) + (t * f32(5000.0)).astype(np.uint32)
            hy = (t * f32(10000.0)).astype(np.uint32) + (s * f32(5000.0)).astype(np.uint32)
        px, py = disk_hash(hx, hy, O)
        rx, ry = lr * px, lr * py
        cu, cv = _v(cam.u), _v(cam.v)
        off = [cu[k] * rx + cv[k] * ry for k in range(3)]
        d = [d[k] - off[k] for k in range(3)]
        o = [org[k] + off[k] for k in range(3)]
    d = normalize(d)
    return np.stack(o, axis=1).astype(f32), np.stack(d, axis=1).astype(f32)


def sky(desc, d, O):
    """sampleSky (render_utils.cuh:115-137) for unit directions d (n, 3)."""
    n = d.shape[0]
    if not desc.use_sky:
        return np.zeros((n, 3), dtype=f32)
    if desc.env_rgba and desc.env_width > 0 and desc.env_height > 0:
        h, w = desc.env_height, desc.env_width
        env = np.ctypeslib.as_array(C.cast(desc.env_rgba, C.POINTER(C.c_float)), (h * w * 4,)).reshape(h, w, 4).copy()
        phi = O.detmath(5, d[:, 2], d[:, 0])
        theta = O.detmath(6, np.maximum(f32(-1.0), np.minimum(f32(1.0), d[:, 1])))
        u = (phi + PI_F) * (f32(1.0) / TWO_PI_F)
        v = theta * (f32(1.0) / PI_F)
        return tex2d_env(env, u, v).astype(f32)
    t = f32(0.5) * (d[:, 1] + f32(1.0))
    top, bottom = _v(desc.sky_top), _v(desc.sky_bottom)
    return ((f32(1.0) - t)[:, None] * bottom[None, :] + t[:, None] * top[None, :]).astype(f32)


def render(P, O, scene, thickness):
    """The wireframe image of `scene`'s rows (tile_y0 .. tile_y0 + tile_rows - 1) of the width x height frame, as
    (tile_rows, width, 3) uint8 in the buffer's bottom-up order -- what Scene.render_wireframe_to_host returns."""
    desc = C.cast(scene.flatten(), C.POINTER(P.SceneDesc)).contents
    W, H, y0, rows = scene.width, scene.height, scene.tile_y0, scene.tile_rows
    o, d = primary_rays(desc.camera, W, H, y0, rows, O)
    hits = O.trace_rays(scene.flatten(), o, d)
    th = f32(thickness)
    u, v = hits["u"].astype(f32), hits["v"].astype(f32)
    edge = (hits["hit"] != 0) & ((u < th) | (v < th) | (((f32(1.0) - u) - v) < th))
    c = sky(desc, d, O)
    if edge.any():
        m = desc.materials
        em = np.ctypeslib.as_array(C.cast(m.emission, C.POINTER(C.c_float)), (m.count * 3,)).reshape(m.count, 3)
        c[edge] = edge_colour(em[hits["mesh_index"][edge]])
    rgb = reinhard_gamma_rgb8(c, O).reshape(rows, W, 3)
    return np.ascontiguousarray(rgb[::-1])
