"""The host camera, the primary ray of a pixel's sample (phase [A] of every frame kernel) and what path_trace_kernel keeps of a
sample, stated once more in float64 numpy.

TEST INFRASTRUCTURE.  The five device copies of [A] (pt_render's staged and unstaged variants, pt_async, pt_wavefront,
pt_radiance's camera_rays_kernel), oracle/ptrt_oracle.cpp and the host mirror's Camera (host/ptrt/scene.hpp) are ONE reading of
the reference, held to each other at tolerance 0.  This module is a second reading, made from the reference's text alone
(file:line beside each function, relative to the reference's src/pathtracer; mat4.cuh and bluenoise.cuh are ../common).  It
reuses three things that are pinned elsewhere and nothing else: `brute_force.closest` for the first hit (rays rounded to float32
before use, as path_truth does), `oracle.xorwow_draw` for the uniforms of a generator state, and the committed blue-noise table
(tests/test_ref_probe.py pins it); the sky of a miss is path_truth's `sample_sky`.  It imports nothing of the oracle's camera or
frame code and none of ptrt_amd.scenes.  Literals are the float32 values the text spells; everything else is float64.

THE TEXT'S ODDITIES, kept as written:
  * taa.cuh:35: entry 15 of the Halton table repeats x = 0.0625 (entry 7's; base 2 would give 0.03125).
  * mat4.cuh:289: operator*'s m[3] term reads b.m[11] where b.m[1] belongs; proj.m[7] = 0 makes it harmless for proj x view.
  * camera.cuh:26: the two curand_uniform calls are arguments of one constructor; this statement, like the oracle, takes the
    first draw for x (the order of evaluation is the compiler's; clang and nvcc go left to right).  Part of what stays
    parity-unpinned with cuRAND's seed constants: a generator-order matter, not a camera matter.

WHAT A FRAME KEEPS (scene_kernels.cuh:142-193, path_logic.cuh:795-815): normal, depth and object id of sample 0's first hit,
0 / 1e30 / -1 on a miss, and the mean of the samples' colours.  The lab's walls are opaque dielectrics (metallic 0,
transmission 0, no coat) that emit, there are no lights and max_depth is 1, so a sample's colour is the emission of the wall it
meets (throughput 1, front faces only, far below the soft clamp at 100: path_logic.cuh:831-836, :895) or sample_sky(d), and a
sample that HITS draws three uniforms in material_scatter (path_logic.cuh:699-714: one for the lobe, two for the direction;
with metallic 0 the diffuse branch's guard 1 - max_fresnel > 1e-6 holds off grazing) before the loop ends.  A lens draws two
per turn of its rejection loop before that (camera.cuh:23-30).

DECIDED.  Discontinuous decisions and their margins; a sample is decided when every decision on it is, a pixel when its samples
are:
    M_WRAP = 1e-6    val + shift against 1 in next_blue_noise (the sum rounds by 2^-24)
    M_DISK = 1e-5    dot(p, p) against 1 in random_in_unit_disk (p = 2 u - 1 carries 2^-24 twice, squared and summed)
    the (uint) casts and the 24-bit masks of the shifts are integer arithmetic, and a 24-bit integer times 2^-24 is exact in
    float32: no margin needed, the statement does them in integers
    brute_force's DELTA / GAP for which wall a ray meets, reused unchanged; only front faces are judged
`lens_radius <= 0` compares a float32 input with a literal and needs none.  At most MAX_UNDECIDED = 2 % of the pixels of any
case may be undecided (asserted in tests/test_frame_truth.py from this module alone).

THE LAB (`lab_walls`, `build_lab`).  A room of 6 x 4 x 8 around the origin, turned about three axes so that no wall is
perpendicular to any view used here (depth on a frontal wall does not see sideways jitter).  Each wall is its own mesh of four
triangles -- a shallow pyramid whose apex lies 0.4 outside the room, so no two faces are coplanar -- wound to face inwards,
with its own emission: object_id names the wall and accum the emission.  24 triangles closed, 20 with the +x side opened to a
gradient sky; the frame cases use the open room, so every case has hits, misses and sky.  SENSITIVITY (asserted from the module
alone): 1/256 pixel of jitter_x, of jitter_y, and 1/256 lens_radius along u and along v each move the predicted depth by at
least 8 units at >= 90 % of the decided hit pixels of every case.  That needs every face in view to slope by some 10 degrees
along BOTH image axes at every pixel, which a wide view of several walls cannot give (along some line of the image a face turns
frontal to one axis): the two cameras look along the -y wall's pyramid with a vertical field of 35 degrees, rolled by a good 25
degrees, and see that wall's faces, a little of the +y wall and the sky -- found by a random search over poses in the room, one
orientation serving both axes (the measured shares are 100 %, the median movement 34 units and more).

TOLERANCES.  shading_truth's convention: unit(q) = EPS32 x (|q| + sum_i |x_i dq/dx_i|), EPS32 = 2^-23, x_i over the float32
inputs -- the camera's vectors (the statement's own construction, rounded to float32 as a Camera stores them), the blue-noise
entry, the accepted pair of uniforms and, for depth and normal, the corners of the wall's triangle -- by central differences with
a relative step of 2^-23, branches held; vectors count by their norm.  For the camera's construction the inputs are the
arguments of the calls (and aspect = (float)W / H).  Cancelling expressions that lose more than the inputs' rounding explains are
NAMED and add a term of their own:
  * `x + 0.5f + jitter_x` (scene_kernels.cuh:164, and :165 for y): the jitter rounds at its own size, up to 0.6, which the
    blue-noise entry's share (a quarter of the entry) does not explain where the sum nearly cancels (x = 0, jitter -0.44):
                   unit(u) += EPS32 x |jitter_x| / W, unit(v) += EPS32 x |jitter_y| / H.
  * `1.0f - (y + 0.5f + jitter_y) / height` (scene_kernels.cuh:165): the quotient rounds at its own size before it is taken
    from 1:        unit(v) += EPS32 x |quotient|; |horizontal| and |vertical| / |unnormalised direction| of u's and v's
    terms go on to the direction.
  * `lower_left_corner + s * horizontal + t * vertical - origin` (camera.cuh:163, :203): the two partial sums round at the
    size of the corner -- the camera's distance from the world's origin -- before the origin is taken away:
                   unit(direction) += EPS32 x (|llc + s h| + |llc + s h + t v|) / |unnormalised direction|.
  Both reach the depth as t x (the direction's term) / cos(ray, normal) and the normal not at all.  Without the terms
  (NAMED_TERMS = False) the oracle's u reads 13.2 units and its v 62.1 (WITHOUT_TERMS, re-measured by the test); the third term
  is sized for a camera far from the world's origin and in the lab's views about doubles the direction's unit (without it the
  direction reads 0.68 and the depth 1.01 where the table has 0.36 and 0.59).
MEASURED below is the oracle's (and, for the camera, the host mirror's) largest deviation in those units over CASES and
HOST_CAMERAS, on the CPU; `python tests/frame_truth.py` prints it and tests/test_frame_truth.py re-measures it.
TOL = 4 x MEASURED, the siblings' margin; the device is judged against TOL (tests/test_frame_truth_gpu.py).  Discrete
quantities (object_id, the miss values, uniforms drawn, generator states) are exact on decided pixels.
"""
import ctypes as C

import numpy as np

import brute_force as bf
from path_truth import Sky, sample_sky

EPS32 = 2.0 ** -23
FD_STEP = EPS32
M_WRAP, M_DISK = 1e-6, 1e-5
MAX_UNDECIDED = 0.02
SEED = 20261021
TURNS = 12                                             # rejection turns provided for per sample ((1 - pi/4)^12 = 1e-8)
SCATTER_DRAWS = 3                                      # rendering/path_logic.cuh:699-714, opaque lobes


def F(x):
    return float(np.float32(x))


PI = F(3.14159265358979323846)                         # math/mathutils.cuh:13
DEG = F(np.float32(PI) / np.float32(180.0))            # `PI / 180.0f`, folded in float
MISS_DEPTH = F(1e30)

MISREADINGS = ("v_unflipped", "no_pixel_centre", "bn_unscaled", "bn_uncentred", "bn_transposed", "bn_no_wrap", "frame_not_plus_s",
               "halton15_fixed", "height_for_u", "aperture_unhalved", "lens_dir_unshifted", "lens_uv_swapped", "lens_one_draw",
               "gbuffer_last_sample", "sum_not_mean", "fov_full_angle", "vertical_from_vup")

RAY_QUANTITIES = ("jitter", "u", "v", "origin", "direction")
# quantity -> (case that attains it, largest deviation in units); tests/test_frame_truth.py re-measures
MEASURED = dict(camera=("move-look-move", 0.2826), view_proj=("move-look-move", 1.255), jitter=("pinhole-96x48-whole-f1000003-s2", 0.6542),
                u=("pinhole-70x33-whole-f14-s3", 0.9165), v=("pinhole-70x33-whole-f15-s1", 0.6687), origin=("lens-96x48-whole-f14-s3", 0.183),
                direction=("lens-70x33-whole-f14-s3", 0.3596), depth=("pinhole-70x33-whole-f14-s3", 0.5891),
                normal=("pinhole-96x48-whole-f0-s1", 0.1555), accum=("far_pinhole-70x33-whole-f14-s3", 0.539))
TOL = {q: 4 * v for q, (_, v) in MEASURED.items()}
NAMED_TERMS = True                                     # False: the units without the named terms, which then read:
WITHOUT_TERMS = {("pinhole-70x33-whole-f15-s1", "u"): 13.22, ("pinhole-96x48-whole-f1000003-s2", "v"): 62.12}


def _v(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _unit(a):
    return a / _norm(a)[..., None]


def _s(a):
    return np.asarray(a, np.float64)[..., None]


# ------------------------------------------------------------------------------------------------------------ mat4
def look_at_matrix(eye, center, up):                   # ../common/mat4.cuh:143-163
    f = _unit(center - eye)
    s = _unit(np.cross(f, up))
    u = np.cross(s, f)
    m = np.zeros(f.shape[:-1] + (16,))
    m[..., 0], m[..., 4], m[..., 8] = s[..., 0], s[..., 1], s[..., 2]
    m[..., 1], m[..., 5], m[..., 9] = u[..., 0], u[..., 1], u[..., 2]
    m[..., 2], m[..., 6], m[..., 10] = -f[..., 0], -f[..., 1], -f[..., 2]
    m[..., 12], m[..., 13], m[..., 14] = -_dot(s, eye), -_dot(u, eye), _dot(f, eye)
    m[..., 15] = 1.0
    return m


def perspective(fov_y_radians, aspect, znear, zfar):   # ../common/mat4.cuh:168-195
    t = np.tan(np.asarray(fov_y_radians, np.float64) / 2.0)
    m = np.zeros(t.shape + (16,))
    m[..., 0] = 1.0 / (aspect * t)
    m[..., 5] = 1.0 / t
    m[..., 10] = -(zfar + znear) / (zfar - znear)
    m[..., 11] = -1.0
    m[..., 14] = -(2.0 * zfar * znear) / (zfar - znear)
    return m


def mat_mul(a, b):                                     # ../common/mat4.cuh:280-322, term by term
    r = np.zeros(np.broadcast(a, b).shape)
    for c in range(4):
        for k in range(4):
            b1 = b[..., 11] if (c == 0 and k == 3) else b[..., c * 4 + 1]          # :289 reads b.m[11]
            r[..., c * 4 + k] = a[..., k] * b[..., c * 4] + a[..., 4 + k] * b1 + a[..., 8 + k] * b[..., c * 4 + 2] + \
                a[..., 12 + k] * b[..., c * 4 + 3]
    return r


# ------------------------------------------------------------------------------------------------------------ the camera
CAMERA_VECTORS = ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")


def _frame_of(cam, lookat, vup, focus_dist, mis=None):
    """The lines the lookfrom / lookat constructor, set_position and look_at each write out (camera.cuh:99-120, :277-293,
    :308-323): w, u, v, the viewport, the corner and the matrices, from the camera's origin, fov and aspect."""
    origin = cam["origin"]
    theta = cam["fov"] * DEG
    h = np.tan(theta if mis == "fov_full_angle" else theta / 2.0)
    viewport_height = 2.0 * h
    viewport_width = cam["aspect"] * viewport_height
    w = _unit(origin - lookat)
    u = _unit(np.cross(vup, w))
    v = vup if mis == "vertical_from_vup" else np.cross(w, u)
    horizontal = _s(focus_dist * viewport_width) * u
    vertical = _s(focus_dist * viewport_height) * v
    llc = origin - horizontal * 0.5 - vertical * 0.5 - _s(focus_dist) * w
    out = dict(cam, u=u, v=v, w=w, horizontal=horizontal, vertical=vertical, lower_left_corner=llc)
    out["view"] = look_at_matrix(origin, lookat, vup)                               # :80-87 update_matrices
    out["proj"] = perspective(cam["fov"] * DEG, cam["aspect"], cam["near"], cam["far"])
    return out


def camera(lookfrom, lookat, vup, vfov, aspect, aperture=0.0, focus_dist=1.0, znear=0.1, zfar=1000.0, mis=None):   # scene/camera.cuh:95-121
    a = np.asarray
    cam = dict(origin=a(lookfrom, np.float64), fov=a(vfov, np.float64), aspect=a(aspect, np.float64), near=F(znear), far=F(zfar))
    cam = _frame_of(cam, a(lookat, np.float64), a(vup, np.float64), a(focus_dist, np.float64), mis)
    cam["lens_radius"] = a(aperture, np.float64) / (1.0 if mis == "aperture_unhalved" else 2.0)
    return cam


def camera_simple(aspect, viewport_height=2.0, focal_length=1.0):                  # scene/camera.cuh:128-149
    aspect = np.asarray(aspect, np.float64)
    z = np.zeros(aspect.shape + (3,))
    ex, ey, ez = z + [1.0, 0.0, 0.0], z + [0.0, 1.0, 0.0], z + [0.0, 0.0, 1.0]
    viewport_width = viewport_height * aspect
    horizontal, vertical = _s(viewport_width) * ex, _s(viewport_height) * ey
    llc = z - horizontal * 0.5 - vertical * 0.5 - _s(focal_length) * ez
    cam = dict(origin=z, lower_left_corner=llc, horizontal=horizontal, vertical=vertical, u=ex, v=ey, w=ez,
               lens_radius=np.zeros(aspect.shape), fov=np.asarray(90.0), aspect=aspect, near=F(0.1), far=F(100.0))
    cam["view"] = look_at_matrix(z, -ez, ey)
    cam["proj"] = perspective(cam["fov"] * DEG, aspect, cam["near"], cam["far"])
    return cam


def set_position(cam, pos):                            # scene/camera.cuh:268-294
    old_center = cam["lower_left_corner"] + 0.5 * cam["horizontal"] + 0.5 * cam["vertical"]
    focus_dist = _norm(cam["origin"] - old_center)
    lookat = cam["origin"] - cam["w"] * _s(focus_dist)
    vup = cam["v"]
    moved = dict(cam, origin=np.asarray(pos, np.float64) + 0.0 * cam["origin"])
    return _frame_of(moved, lookat, vup, _norm(moved["origin"] - lookat))


def look_at(cam, target, vup=(0.0, 1.0, 0.0)):          # scene/camera.cuh:301-324
    target = np.asarray(target, np.float64)
    return _frame_of(cam, target, np.asarray(vup, np.float64) + 0.0 * cam["origin"], _norm(cam["origin"] - target))


def view_proj(cam):                                    # scene/camera.cuh:259-261: 16 floats, column-major as mat4 stores them
    return mat_mul(cam["proj"], cam["view"])


def stored(cam):
    """The ray-generation state as a Camera holds it: every vector and the lens radius rounded to float32."""
    out = {k: _v(cam[k]) for k in CAMERA_VECTORS}
    out["lens_radius"] = float(np.float32(cam["lens_radius"]))
    return out


def camera_of_desc(desc):
    """ptrt_camera of a flattened scene as the same dict (float64 of the floats it holds): what is COMPARED with `camera`."""
    c = desc.contents.camera
    out = {k: np.array([getattr(c, k).x, getattr(c, k).y, getattr(c, k).z], np.float64) for k in CAMERA_VECTORS}
    out["lens_radius"] = float(c.lens_radius)
    return out


# ------------------------------------------------------------------------------------------------------------ jitter
HALTON = _v([[0.500000, 0.333333], [0.250000, 0.666667], [0.750000, 0.111111], [0.125000, 0.444444], [0.625000, 0.777778],
             [0.375000, 0.222222], [0.875000, 0.555556], [0.062500, 0.888889], [0.562500, 0.037037], [0.312500, 0.370370],
             [0.812500, 0.703704], [0.187500, 0.148148], [0.687500, 0.481481], [0.437500, 0.814815], [0.937500, 0.259259],
             [0.062500, 0.592593]])                    # rendering/taa.cuh:19-36, entry 15 as written


def taa_jitter(i, mis=None):                           # rendering/taa.cuh:41-61
    h = HALTON[int(i) % 16].copy()
    if mis == "halton15_fixed" and int(i) % 16 == 15:
        h[0] = 0.03125
    return h - 0.5


def blue_noise_shift(frame):                           # math/sampling.cuh:22-32
    m = 0xFFFFFFFF
    h = (int(frame) * 0x9e3779b9) & m
    h ^= h >> 15
    h = (h * 0x85ebca6b) & m
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & m
    h ^= h >> 16
    sx = (h & 0xFFFFFF) / 16777216.0
    h = (h * 0x85ebca6b) & m
    return np.array([sx, (h & 0xFFFFFF) / 16777216.0])


def blue_noise(table, x, y, frame, mis=None):          # math/sampling.cuh:15-43
    """-> dict(value (n, 2), val (the table's entry), shift (2,), wrap (n, 2), decided (n,))"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    t = _v(table).reshape(64 * 64, 2)
    idx = (x & 63) * 64 + (y & 63) if mis == "bn_transposed" else (y & 63) * 64 + (x & 63)
    val = t[idx]
    shift = blue_noise_shift(frame)
    s = val + shift[None, :]
    wrap = (s >= 1.0) & (mis != "bn_no_wrap")
    return dict(value=np.where(wrap, s - 1.0, s), val=val, shift=shift, wrap=wrap, decided=(np.abs(s - 1.0) > M_WRAP).all(axis=1))


# ------------------------------------------------------------------------------------------------------------ pixel to ray
def _ray_fn(X, held):
    """The arithmetic of scene_kernels.cuh:152-167 and Camera::get_ray (camera.cuh:156-166, :201-205) with every branch held,
    and, where `held` names the triangle a ray met, the hit on that triangle's plane and the sample's colour."""
    mis = held.get("mis")
    x, y, W, H = held["x"], held["y"], held["W"], held["H"]
    s = X["val"] + held["shift"][None, :]
    bn = np.where(held["wrap"], s - 1.0, s)
    centre = 0.0 if mis == "bn_uncentred" else 0.5
    scale = 1.0 if mis == "bn_unscaled" else 0.25
    jitter = held["taa"][None, :] + (bn - centre) * scale
    if "nudge_jitter" in held:
        jitter = jitter + np.asarray(held["nudge_jitter"])[None, :]
    half = 0.0 if mis == "no_pixel_centre" else 0.5
    u = (x + half + jitter[:, 0]) / (H if mis == "height_for_u" else W)
    quotient = (y + half + jitter[:, 1]) / H
    v = quotient if mis == "v_unflipped" else 1.0 - quotient
    p1 = X["lower_left_corner"] + _s(u) * X["horizontal"]
    p2 = p1 + _s(v) * X["vertical"]
    through = p2 - X["origin"]
    if held["lens"]:
        p = 2.0 * X["acc"] - 1.0                                                   # camera.cuh:26-27
        if "nudge_lens" in held:
            p = p + np.asarray(held["nudge_lens"])[None, :]
        rd = _s(X["lens_radius"]) * p
        a, b = (rd[:, 1], rd[:, 0]) if mis == "lens_uv_swapped" else (rd[:, 0], rd[:, 1])
        offset = X["u"] * _s(a) + X["v"] * _s(b)
        dirv = through if mis == "lens_dir_unshifted" else through - offset
        origin = X["origin"] + offset
    else:
        dirv, origin = through, X["origin"] + 0.0
    length = _norm(dirv)
    d = dirv / _s(length)
    term_u = EPS32 * np.abs(jitter[:, 0]) / W
    term_v = EPS32 * np.abs(jitter[:, 1]) / H + (0.0 if mis == "v_unflipped" else EPS32 * np.abs(quotient))
    term_d = (EPS32 * (_norm(p1) + _norm(p2)) + term_u * _norm(X["horizontal"]) + term_v * _norm(X["vertical"])) / length
    out = dict(jitter=jitter, u=u, v=v, origin=origin, direction=d, term_u=term_u, term_v=term_v, term_direction=term_d)
    if "hit" in held:
        hit = held["hit"]
        tri = X["tri"].reshape(-1, 3, 3)
        g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        with np.errstate(all="ignore"):
            g = g / _s(_norm(g))
            dn = _dot(d, g)
            t = _dot(tri[:, 0] - origin, g) / dn
        out["depth"] = np.where(hit, t, MISS_DEPTH)
        out["normal"] = np.where(_s(hit), g, 0.0)                                   # wound inwards: the front face's own normal
        out["term_depth"] = np.where(hit, np.abs(t) * term_d / np.maximum(np.abs(dn), 1e-300), 0.0)
        sky, _ = sample_sky(d, held["sky"])
        out["radiance"] = np.where(_s(hit), held["emission"], sky)
    return out


def _mag(a):
    return _norm(a) if a.ndim == 2 else np.abs(a)


def condition(fn, X, outputs, entrywise=()):
    """|q| + sum_i |x_i dq/dx_i| of every named output of fn(X) over every column of every array of X, by central differences
    with a relative step of 2^-23.  Vector outputs count by their norm, those named in `entrywise` entry by entry."""
    def mag(q, a):
        return np.abs(a) if q in entrywise else _mag(a)
    q0 = fn(X)
    cond = {q: mag(q, q0[q]) for q in outputs}
    for k, a in X.items():
        a = np.asarray(a, np.float64)
        for c in (range(a.shape[1]) if a.ndim == 2 else [None]):
            if not np.any(a[:, c] if c is not None else a):
                continue
            res = []
            for sgn in (1.0, -1.0):
                w = a.copy()
                if c is None:
                    w *= 1.0 + sgn * FD_STEP
                else:
                    w[:, c] *= 1.0 + sgn * FD_STEP
                res.append(fn(dict(X, **{k: w})))
            with np.errstate(all="ignore"):
                for q in outputs:
                    cond[q] = cond[q] + np.nan_to_num(mag(q, res[0][q] - res[1][q])) / (2.0 * FD_STEP)
    return cond, q0


def primary_ray_detail(cam, x, y, W, H, frame, s, uniforms, table, mis=None):
    """Sample s of frame `frame` at pixels (x, y) of a W x H frame, `uniforms` (n, k) the next uniforms of each pixel's
    generator.  -> dict: origin, direction, jitter, u, v, draws, decided, and X / held for `_ray_fn`."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    n = len(x)
    index = frame if mis == "frame_not_plus_s" else frame + s                       # scene_kernels.cuh:152, :157
    bn = blue_noise(table, x, y, index, mis)
    lens = bool(cam["lens_radius"] > 0)                                             # camera.cuh:157 `lens_radius <= 0`
    acc, draws, dec = np.zeros((n, 2)), np.zeros(n, np.int64), bn["decided"].copy()
    if lens:                                                                        # camera.cuh:23-30
        pending, step = np.ones(n, bool), (1 if mis == "lens_one_draw" else 2)
        while pending.any():
            rows = np.flatnonzero(pending)
            assert (draws[rows] + 2 <= uniforms.shape[1]).all(), "more rejection turns than uniforms were provided for"
            ab = np.stack([uniforms[rows, draws[rows]], uniforms[rows, draws[rows] + 1]], axis=1)
            pp = ((2.0 * ab - 1.0) ** 2).sum(axis=1)
            dec[rows] &= np.abs(pp - 1.0) > M_DISK
            ok = ~(pp >= 1.0)
            acc[rows[ok]] = ab[ok]
            draws[rows] += step
            pending[rows[ok]] = False
    X = {k: np.repeat(np.asarray(cam[k], np.float64).reshape(1, 3), n, axis=0) for k in CAMERA_VECTORS if k != "w"}
    X.update(lens_radius=np.full(n, float(cam["lens_radius"])), val=bn["val"], acc=acc)
    held = dict(x=x, y=y, W=W, H=H, taa=taa_jitter(index, mis), shift=bn["shift"], wrap=bn["wrap"], lens=lens, mis=mis)
    out = _ray_fn(X, held)
    out.update(draws=draws, decided=dec, ray_decided=dec.copy(), X=X, held=held)
    return out


def primary_ray(cam, x, y, W, H, frame, s, uniforms, table, mis=None):
    """-> (origin (n, 3), direction (n, 3), uniforms drawn (n,))"""
    r = primary_ray_detail(cam, x, y, W, H, frame, s, uniforms, table, mis)
    return r["origin"], r["direction"], r["draws"]


# ------------------------------------------------------------------------------------------------------------ rows
def band_rows(y0, rows):
    """global row of every local row of a band context: rows [y0, y0 + rows) (include/ptrt.h, ptrt_create)"""
    return y0 + np.arange(rows)


def strip_rows(H, phase, period):
    """the same for an interleaved context: every period-th 8-row strip from strip `phase` (strip t = rows 8t .. 8t+7), one
    after the other (include/ptrt.h, ptrt_create_interleaved)"""
    strips = range(phase, (H + 7) // 8, period)
    return np.concatenate([np.arange(8 * t, min(8 * t + 8, H)) for t in strips])


# ------------------------------------------------------------------------------------------------------------ the world
class World:
    """What a frame of the lab reads beside the camera: geometry for the brute force, each wall's emission, the sky, the
    blue-noise table; and `O` for xorwow_draw."""

    def __init__(self, P, O, scene):
        self.desc = scene.flatten()
        d = self.desc.contents
        self.geom = bf.Geometry.from_desc(self.desc)
        m = d.materials
        self.emission = np.ctypeslib.as_array(C.cast(m.emission, C.POINTER(C.c_float)), (int(m.count) * 3,)).astype(np.float64).reshape(-1, 3)
        assert d.light_count == 0 and not d.env_rgba
        self.sky = Sky(d.use_sky, (d.sky_top.x, d.sky_top.y, d.sky_top.z), (d.sky_bottom.x, d.sky_bottom.y, d.sky_bottom.z))
        self.table = _v(P.blue_noise_table())
        self.O = O


def uniforms(O, states, count):
    out = np.zeros((len(states), count))
    for i, s in enumerate(states):
        out[i] = O.xorwow_draw(s, count, uniform=True)[0]
    return out


def states_after(O, states, draws):
    out = np.zeros_like(states)
    for i, (s, k) in enumerate(zip(states, draws)):
        out[i] = O.xorwow_draw(s, int(k))[1]
    return out


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def frame(world, cam, W, H, rows, frame, spp, states, mis=None, units=True, uni=None):
    """path_trace_kernel with max_depth 1 over the pixels of the global rows `rows` (scene_kernels.cuh:130-193), `states`
    (len(rows) * W, 6) the generator states before the frame.  -> dict: normal, depth, object_id, hit (sample 0's, or the last
    sample's under that misreading), radiance (n, spp, 3), accum, draws, decided, samples (per sample: the ray's detail with
    `first` = the brute force's answer, `start` = uniforms drawn before it, and with `units` the unit of every quantity),
    unit_depth / unit_normal / unit_accum."""
    rows = np.asarray(rows, np.int64)
    n = len(rows) * W
    x, y = np.tile(np.arange(W), len(rows)), np.repeat(rows, W)
    per = 2 * TURNS + SCATTER_DRAWS
    if uni is None:
        uni = uniforms(world.O, states, spp * per)
    cursor, decided = np.zeros(n, np.int64), np.ones(n, bool)
    samples, radiance = [], np.zeros((n, spp, 3))
    for s in range(spp):
        u = uni[np.arange(n)[:, None], cursor[:, None] + np.arange(2 * TURNS)[None, :]]
        r = primary_ray_detail(cam, x, y, W, H, frame, s, u, world.table, mis)
        o, d = _f32(r["origin"]), _f32(r["direction"])                              # a Ray holds floats
        a = bf.closest(world.geom, o, d)
        hit = a["hit"]
        mesh, face = np.where(hit, a["mesh"], 0), np.where(hit, a["face"], 0)
        tri = np.zeros((n, 3, 3))
        for mi in np.unique(mesh[hit]):
            k = np.flatnonzero(hit & (mesh == mi))
            tri[k] = world.geom.meshes[mi].world_triangles()[face[k]]
        r["X"]["tri"] = tri.reshape(n, 9)
        r["held"].update(hit=hit, emission=world.emission[mesh], sky=world.sky)
        r["decided"] = r["decided"] & a["decided"] & ~a["quirk"] & (a["front_face"] | ~hit)
        r["first"], r["start"] = a, cursor.copy()
        if units:
            cond, q0 = condition(lambda Y: _ray_fn(Y, r["held"]), r["X"], RAY_QUANTITIES + ("depth", "normal", "radiance"))
            r["unit"] = {q: EPS32 * c for q, c in cond.items()}
            if NAMED_TERMS:
                r["unit"]["u"] += q0["term_u"]
                r["unit"]["v"] += q0["term_v"]
                r["unit"]["direction"] += q0["term_direction"]
                r["unit"]["depth"] += q0["term_depth"]
        else:
            q0 = _ray_fn(r["X"], r["held"])
        for q in ("depth", "normal", "radiance"):
            r[q] = q0[q]
        # the plane of the triangle the brute force names is where the brute force puts the hit
        front = hit & a["front_face"]
        assert np.allclose(r["depth"][front], a["t"][front], rtol=1e-5, atol=0) and (_dot(r["normal"][front], a["normal"][front]) > 0.999999).all()
        radiance[:, s] = r["radiance"]
        cursor = cursor + r["draws"] + SCATTER_DRAWS * hit                           # path_logic.cuh:810-815, :864
        decided &= r["decided"]
        samples.append(r)
    g = samples[-1] if mis == "gbuffer_last_sample" else samples[0]                 # scene_kernels.cuh:181-185
    total = radiance.sum(axis=1)
    out = dict(normal=g["normal"], depth=g["depth"], object_id=np.where(g["first"]["hit"], g["first"]["mesh"], -1), hit=g["first"]["hit"],
               radiance=radiance, accum=total if mis == "sum_not_mean" else total / float(spp), draws=cursor, decided=decided,
               samples=samples, x=x, y=y)
    if units:
        out["unit_depth"], out["unit_normal"] = g["unit"]["depth"], g["unit"]["normal"]
        out["unit_accum"] = sum(r["unit"]["radiance"] for r in samples) / spp + (spp + 1) * EPS32 * _mag(out["accum"])
    return out


def moved_depth(fr, what, amount):
    """|change of sample 0's predicted depth| in units when the jitter moves by `amount` pixels (what = 'jitter_x',
    'jitter_y') or the lens sample by `amount` x lens_radius ('lens_u', 'lens_v'), branches held; on the hit pixels."""
    r = fr["samples"][0]
    key, vec = {"jitter_x": ("nudge_jitter", (amount, 0.0)), "jitter_y": ("nudge_jitter", (0.0, amount)),
                "lens_u": ("nudge_lens", (amount, 0.0)), "lens_v": ("nudge_lens", (0.0, amount))}[what]
    moved = _ray_fn(r["X"], dict(r["held"], **{key: vec}))
    hit = fr["hit"]
    return (np.abs(moved["depth"] - r["depth"]) / r["unit"]["depth"])[hit & fr["decided"]]


# ------------------------------------------------------------------------------------------------------------ judging
def in_units(got, want, unit):
    """|got - want| / unit per row; 0 where both vanish"""
    dev = _mag(np.asarray(got, np.float64) - want)
    with np.errstate(all="ignore"):
        return np.where(dev == 0.0, 0.0, dev / unit)


def judge_rays(r, got, decided=None):
    """One sample's rays under test (`got`: jitter, uv, origin, direction, any subset) against the statement's: units per
    quantity on the decided pixels, 0 elsewhere."""
    dec = r["decided"] if decided is None else decided
    out = {}
    for q in RAY_QUANTITIES:
        g = got["uv"][:, "uv".index(q)] if q in ("u", "v") and "uv" in got else got.get(q)
        if g is not None:
            out[q] = np.where(dec, in_units(g, r[q], r["unit"][q]), 0.0)
    return out


def judge_frame(fr, got, states=None, states_got=None, O=None):
    """A frame's buffers under test (accum, normal, depth, object_id) against `frame`'s: units per quantity and the exact
    ones (`bad`: object_id, the miss values, and with the states before and after the states) on decided pixels."""
    dec, hit = fr["decided"], fr["hit"]
    units = dict(depth=np.where(dec & hit, in_units(got["depth"], fr["depth"], fr["unit_depth"]), 0.0),
                 normal=np.where(dec & hit, in_units(got["normal"], fr["normal"], fr["unit_normal"]), 0.0),
                 accum=np.where(dec, in_units(got["accum"], fr["accum"], fr["unit_accum"]), 0.0))
    miss = dec & ~hit
    bad = dict(object_id=dec & (np.asarray(got["object_id"]) != fr["object_id"]),
               miss_depth=miss & (np.asarray(got["depth"]) != np.float32(1e30)),
               miss_normal=miss & (np.asarray(got["normal"]) != 0.0).any(axis=1))
    if states_got is not None:
        if "states_after" not in fr:
            fr["states_after"] = states_after(O, states, fr["draws"])
        bad["states"] = dec & (states_got != fr["states_after"]).any(axis=1)
    return dict(units=units, bad=bad)


# ------------------------------------------------------------------------------------------------------------ the lab
ROOM_HALF = np.array([3.0, 2.0, 4.0])
ROOM_TURN = (0.35, 0.55, 0.25)                          # radians about x, then y, then z
APEX = 0.4
WALLS = ("-x", "+x", "-y", "+y", "-z", "+z")
OPEN_SIDE = "+x"
SKY_TOP, SKY_BOTTOM = (0.2, 0.4, 0.9), (1.0, 0.9, 0.8)


def _turn():
    a, b, c = ROOM_TURN
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


def lab_walls(open_side=False):
    """[(name, (4, 3, 3) float32 triangles wound to face the room's centre, emission)]"""
    R = _turn()
    out = []
    for i, name in enumerate(WALLS):
        if open_side and name == OPEN_SIDE:
            continue
        axis, sign = i // 2, (-1.0 if i % 2 == 0 else 1.0)
        a1, a2 = [k for k in range(3) if k != axis]
        corners = []
        for s1, s2 in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            p = np.zeros(3)
            p[axis], p[a1], p[a2] = sign * ROOM_HALF[axis], s1 * ROOM_HALF[a1], s2 * ROOM_HALF[a2]
            corners.append(p)
        apex = np.zeros(3)
        apex[axis] = sign * (ROOM_HALF[axis] + APEX)
        tris = []
        for k in range(4):
            t = np.array([corners[k], corners[(k + 1) % 4], apex])
            if np.dot(np.cross(t[1] - t[0], t[2] - t[0]), -t[0]) < 0.0:               # the centre must see the front
                t = t[[0, 2, 1]]
            tris.append(t @ R.T)
        emission = (0.25 + 0.25 * i, 1.5 - 0.2 * i, 0.5 + 0.1 * (i % 3))
        out.append((name, np.asarray(tris, np.float32), emission))
    return out


def build_lab(P, scene, open_side=True):
    """The lab into a Scene; -> {wall: mesh index}."""
    ids = {}
    for name, tris, emission in lab_walls(open_side):
        ids[name] = scene.addTriangles(tris, P.Material((0.7, 0.7, 0.7), 0.8, 0.0, emission=emission))
    if open_side:
        scene.setSkyGradient(SKY_TOP, SKY_BOTTOM)
    else:
        scene.disableSky()
    return ids


# the cameras of the frame cases: (lookfrom, lookat, vup, vfov, aperture, focus_dist)
# (poses found by a random search over the room for the sensitivity condition of the docstring: a narrow view along a wall, rolled)
CAMERAS = dict(pinhole=((0.04, -0.08, 1.17), (0.33, 3.03, -1.34), (0.51, 1.0, -0.14), 35.0, 0.0, 1.0),
               lens=((-1.21, 0.33, 1.04), (1.12, 3.11, -0.65), (0.66, 1.0, 0.28), 35.0, 0.6, 7.5),
               # the all-miss views: outside the room, 1,000 units out, looking away from it
               far_pinhole=((600.0, 640.0, -480.0), (900.0, 1100.0, -700.0), (0.1, 1.0, -0.05), 62.0, 0.0, 1.0),
               far_lens=((600.0, 640.0, -480.0), (900.0, 1100.0, -700.0), (0.1, 1.0, -0.05), 55.0, 0.6, 7.5))
SIZES = ((96, 48), (70, 33))
CONTEXTS = dict(whole=None, band=(16, 24), strips=(1, 3))                           # band: (y0, rows); strips: (phase, period)
FRAMES = ((0, 1), (15, 1), (14, 3), (1000003, 2))                                  # (frame index, samples)


def context_rows(H, ctx):
    if ctx == "whole":
        return np.arange(H)
    return band_rows(*CONTEXTS[ctx]) if ctx == "band" else strip_rows(H, *CONTEXTS[ctx])


def cases(far=False):
    """(camera, W, H, context, frame, spp) of every case: both sizes whole, 96 x 48 as a band and as strips too, every
    (frame, spp), both cameras; `far`: the two all-miss views on 70 x 33 instead."""
    if far:
        return [(c, 70, 33, "whole", f, spp) for c in ("far_pinhole", "far_lens") for f, spp in ((14, 3), (1000003, 2))]
    shapes = [(96, 48, "whole"), (70, 33, "whole"), (96, 48, "band"), (96, 48, "strips")]
    return [(c, W, H, ctx, f, spp) for c in ("pinhole", "lens") for W, H, ctx in shapes for f, spp in FRAMES]


def case_name(key):
    c, W, H, ctx, f, spp = key
    return f"{c}-{W}x{H}-{ctx}-f{f}-s{spp}"


def aspect_of(W, H):
    return float(np.float32(W) / np.float32(H))                                     # `static_cast<float>(width) / height`


def case_camera(key, mis=None):
    """the statement's own camera of a case, as a Camera stores it"""
    c, W, H = key[0], key[1], key[2]
    lookfrom, lookat, vup, vfov, aperture, focus = CAMERAS[c]
    return stored(camera(_v(lookfrom), _v(lookat), _v(vup), F(vfov), aspect_of(W, H), F(aperture), F(focus), mis=mis))


def case_states(O, key):
    n = len(context_rows(key[2], key[3])) * key[1]
    return O.xorwow_init(SEED, 0, n)


class Lab:
    """The open lab as a host-only scene, its world, and the statement of every case asked for (kept)."""

    def __init__(self, P, O, open_side=True):
        self.P, self.O = P, O
        self.scene = P.Scene(64, 64, device=P.HOST_ONLY)
        self.ids = build_lab(P, self.scene, open_side)
        self.world = World(P, O, self.scene)
        self._frames, self._uni = {}, {}

    def uniforms(self, key):
        k = (key[1], key[2], key[3], key[5])
        if k not in self._uni:
            self._uni[k] = uniforms(self.O, case_states(self.O, key), key[5] * (2 * TURNS + SCATTER_DRAWS))
        return self._uni[k]

    def frame(self, key, mis=None, units=True):
        if (key, mis, units) not in self._frames:
            c, W, H, ctx, f, spp = key
            self._frames[(key, mis, units)] = frame(self.world, case_camera(key, mis), W, H, context_rows(H, ctx), f, spp,
                                                    case_states(self.O, key), mis=mis, units=units, uni=self.uniforms(key))
        return self._frames[(key, mis, units)]

    def close(self):
        self.scene.close()


# ------------------------------------------------------------------------------------------------------------ the oracle's side
def set_camera(scene, name):
    lookfrom, lookat, vup, vfov, aperture, focus = CAMERAS[name]
    scene.setCamera(lookfrom, lookat, vup, vfov, aperture, focus)


def oracle_case(P, O, lab, key):
    """The oracle on a case: a host-only scene of the case's size with the lab and the mirror's camera; -> dict of
    oracle.render's buffers, `rng` (the states after) and `rays` (per sample oracle.primary_rays from the states the
    statement says that sample starts from)."""
    c, W, H, ctx, f, spp = key
    s = P.Scene(W, H, device=P.HOST_ONLY)
    build_lab(P, s, True)
    set_camera(s, c)
    desc = s.flatten()
    rows = context_rows(H, ctx)
    states = case_states(O, key)
    fr = lab.frame(key)
    out = dict(accum=np.zeros((len(rows) * W, 3), np.float32), normal=np.zeros((len(rows) * W, 3), np.float32),
               depth=np.zeros(len(rows) * W, np.float32), object_id=np.zeros(len(rows) * W, np.int32),
               rng=np.zeros((len(rows) * W, 6), np.uint32), rays=[{} for _ in range(spp)])
    # a context's rows, run by run of consecutive global rows (a band is one run, strips are several)
    cuts = np.flatnonzero(np.diff(rows) != 1) + 1
    for run in np.split(np.arange(len(rows)), cuts):
        sl = slice(run[0] * W, (run[-1] + 1) * W)
        rng = states[sl].copy()
        part = O.render(desc, W, H, spp, 1, f, lab.world.table.astype(np.float32), rng, tile_y0=int(rows[run[0]]), tile_rows=len(run))
        for k in ("accum", "normal", "depth", "object_id"):
            out[k][sl] = part[k]
        out["rng"][sl] = rng
        for i, r in enumerate(fr["samples"]):
            head = states_after(O, states[sl], r["start"][sl])
            got = O.primary_rays(desc, W, H, f + i, lab.world.table.astype(np.float32), head, tile_y0=int(rows[run[0]]), tile_rows=len(run))
            for k, v in got.items():
                out["rays"][i].setdefault(k, np.zeros((len(rows) * W,) + v.shape[1:], np.float32))[sl] = v
    s.close()
    return out


def measure_case(P, O, lab, key, mis=None, got=None):
    """{quantity: largest deviation of the oracle in units over the case's decided pixels}, and the exact ones' counts"""
    fr = lab.frame(key, mis)
    got = oracle_case(P, O, lab, key) if got is None else got
    row = {q: 0.0 for q in RAY_QUANTITIES}
    # a sample's rays are judged where the statement knows the state it starts from: every earlier sample decided
    before = np.ones(len(fr["decided"]), bool)
    for r, g, plain in zip(fr["samples"], got["rays"], lab.frame(key)["samples"]):
        # (the oracle's rays were made from the states the UNCHANGED statement gives the sample; a misreading that moves them
        # is judged by the frame alone)
        same = before & (r["start"] == plain["start"])
        for q, u in judge_rays(r, g, r["decided"] & same).items():
            row[q] = max(row[q], float(u.max()))
        before &= r["decided"]
    j = judge_frame(fr, got, case_states(O, key), got["rng"], O)
    for q, u in j["units"].items():
        row[q] = float(u.max())
    return row, {q: int(b.sum()) for q, b in j["bad"].items()}


# ------------------------------------------------------------------------------------------------------------ the host camera
# (name, W, H, [calls]): calls are ("set", lookfrom, lookat, vup, vfov, aperture, focus), ("simple",), ("move", pos), ("look", at)
_GEN = ((-0.9, 0.35, -1.3), (2.2, -0.6, 1.9), (0.1, 1.0, -0.05))
HOST_CAMERAS = [
    ("vfov20-aspect2", 96, 48, [("set",) + _GEN + (20.0, 0.0, 1.0)]),
    ("vfov90-aspect70/33", 70, 33, [("set",) + _GEN + (90.0, 0.0, 1.0)]),
    ("vfov140-lens-focus7.5", 96, 48, [("set",) + _GEN + (140.0, 0.6, 7.5)]),
    ("vup-oblique", 70, 33, [("set", (1.0, 2.0, 3.0), (-2.0, 0.5, -1.0), (0.6, 0.7, -0.4), 47.0, 0.6, 7.5)]),
    ("far-1000", 96, 48, [("set", (600.0, 640.0, -480.0), (601.5, 639.0, -482.0), (0.0, 1.0, 0.0), 40.0, 0.0, 1.0)]),
    ("simple", 70, 33, [("simple",)]),
    ("move-look-move", 96, 48, [("set",) + _GEN + (62.0, 0.6, 7.5), ("move", (1.5, 1.0, -2.0)), ("look", (-1.0, 0.2, 2.5)),
                                ("move", (0.4, -1.1, -3.0))]),
    ("simple-move-look", 70, 33, [("simple",), ("move", (2.0, 1.0, 3.0)), ("look", (0.5, -0.5, -4.0))]),
    ("far-move-look-move", 96, 48, [("set", (600.0, 640.0, -480.0), (601.5, 639.0, -482.0), (0.0, 1.0, 0.0), 40.0, 0.0, 3.0),
                                    ("move", (598.0, 641.0, -478.5)), ("look", (603.0, 640.0, -481.0)), ("move", (599.0, 642.0, -477.0))]),
]


def host_camera_inputs(W, H, calls):
    """The float32 arguments of the calls as one row each, keyed by call."""
    X = {"aspect": np.array([aspect_of(W, H)])}
    for i, c in enumerate(calls):
        if c[0] == "set":
            X.update({f"{i}from": _v(c[1])[None], f"{i}at": _v(c[2])[None], f"{i}up": _v(c[3])[None],
                      f"{i}s": _v([c[4], c[5], c[6]])[None]})
        elif c[0] in ("move", "look"):
            X[f"{i}p"] = _v(c[1])[None]
    return X


def host_camera_fn(calls, mis=None):
    def fn(X):
        cam = None
        for i, c in enumerate(calls):
            if c[0] == "set":
                s = X[f"{i}s"]
                cam = camera(X[f"{i}from"], X[f"{i}at"], X[f"{i}up"], s[:, 0], X["aspect"], s[:, 1], s[:, 2], mis=mis)
            elif c[0] == "simple":
                cam = camera_simple(X["aspect"])
            elif c[0] == "move":
                cam = set_position(cam, X[f"{i}p"])
            else:
                cam = look_at(cam, X[f"{i}p"])
        out = {k: cam[k] for k in CAMERA_VECTORS}
        out["lens_radius"] = np.asarray(cam["lens_radius"], np.float64).reshape(-1)
        out["view_proj"] = view_proj(cam)
        return out
    return fn


def host_camera(P, W, H, calls):
    """The mirror's camera after the calls: (camera dict, view_proj (16,))"""
    s = P.Scene(W, H, device=P.HOST_ONLY)
    build_lab(P, s)                                                                 # an empty scene flattens to nothing
    for c in calls:
        if c[0] == "set":
            s.setCamera(*c[1:])
        elif c[0] == "move":
            s.moveCamera(c[1])
        elif c[0] == "look":
            s.lookCameraAt(c[1])
        # ("simple",): a fresh Scene holds Camera(aspect, 2, 1), what setCameraSimple() sets (host/ptrt/scene.hpp)
    cam, vp = camera_of_desc(s.flatten()), s.view_proj(current=True).astype(np.float64)
    s.close()
    return cam, vp


def judge_host_camera(P, name, W, H, calls, mis=None):
    """-> (camera: the largest deviation of the seven vectors and the lens radius in units, view_proj: of the 16 entries)"""
    outputs = CAMERA_VECTORS + ("lens_radius", "view_proj")
    cond, q0 = condition(host_camera_fn(calls, mis), host_camera_inputs(W, H, calls), outputs, entrywise=("view_proj",))
    cam, vp = host_camera(P, W, H, calls)
    worst = 0.0
    for k in CAMERA_VECTORS + ("lens_radius",):
        got = np.asarray(cam[k], np.float64).reshape(1, -1) if k != "lens_radius" else np.array([cam[k]])
        worst = max(worst, float(in_units(got, q0[k], EPS32 * cond[k]).max()))
    dev = np.abs(vp - q0["view_proj"][0])
    with np.errstate(all="ignore"):
        entries = np.where(dev == 0.0, 0.0, dev / (EPS32 * cond["view_proj"][0]))
    return worst, float(entries.max())


def measure(P, O, verbose=False, which=None):
    """-> {quantity: (case, largest deviation in units)} over HOST_CAMERAS and every case (or those named)"""
    worst = {}

    def note(name, row):
        for q, v in row.items():
            if v > worst.get(q, ("", -1.0))[1]:
                worst[q] = (name, v)
        if verbose:
            print(f"{name:34s} " + " ".join(f"{q} {v:.3g}" for q, v in row.items()), flush=True)
    for name, W, H, calls in HOST_CAMERAS:
        if which is None or name in which:
            c, vp = judge_host_camera(P, name, W, H, calls)
            note(name, dict(camera=c, view_proj=vp))
    lab = Lab(P, O)
    for key in cases() + cases(far=True):
        if which is None or case_name(key) in which:
            row, bad = measure_case(P, O, lab, key)
            note(case_name(key), row)
            if verbose and any(bad.values()):
                print("    exact quantities differ:", bad)
    lab.close()
    return worst


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "ptrt-game-engine_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests", "golden")]
    import oracle
    import ptrt_amd
    w = measure(ptrt_amd, oracle, verbose=True)
    for q, (name, v) in w.items():
        print(f"    {q}=({name!r}, {v:.4g}),")
