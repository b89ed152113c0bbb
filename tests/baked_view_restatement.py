"""The baked-light view (ptrt_render_baked, include/ptrt.h; baked_view_kernel, csrc/pt_baked.hip.h) restated in numpy float32:
steps 3 to 6 of the definition -- the miss, the choice of the irradiance's source, the shading, the outputs -- over rows the
existing entry points return for the frame's primary rays:

    o, d    = Scene.camera_rays(frame)                       step 1
    closest = Scene.query_closest(o, d)                      step 2, (n, 16) int32
    lm      = Scene.query_lightmap(o, d, ...)                (n, 8) int32, or None without a lightmap
    pl      = Scene.query_probe_light(o, d, ...)             (n, 8) int32, or None without a volume

Every operation is one float32 operation, in the written order.  The kernel samples the volume only where the lightmap left a
pixel empty; query_probe_light's rows hold the sample for every ray, and the selection below takes the same ones.
"""
import ctypes as C

import numpy as np

import wireframe_restatement as W

F = np.float32
PI_F = F(3.14159265)
SKY, LIGHTMAP, PROBES, UNLIT = range(4)  # what lights a pixel
SOURCES = ("sky", "lightmap", "probes", "unlit")


def _words(rows, cols):
    r = np.asarray(rows.cpu().numpy() if hasattr(rows, "cpu") else rows)
    assert r.ndim == 2 and r.shape[1] == cols and r.dtype == np.int32, (r.shape, r.dtype)
    return np.ascontiguousarray(r)


def materials(P, scene):
    """(albedo, emission), (M, 3) float32 each: the flattened scene's materials, the words ptrt_upload_materials is handed"""
    m = C.cast(scene.flatten(), C.POINTER(P.SceneDesc)).contents.materials

    def rows(p):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (m.count * 3,)).reshape(m.count, 3).astype(F)
    return rows(m.albedo), rows(m.emission)


def sky(P, O, scene, directions):
    """step 3 for every ray: use_sky ? sampleSky(d) : 0, (n, 3) float32 (wireframe_restatement.sky)"""
    desc = C.cast(scene.flatten(), C.POINTER(P.SceneDesc)).contents
    d = np.asarray(directions.cpu().numpy() if hasattr(directions, "cpu") else directions, F)
    return W.sky(desc, d, O).astype(F)


def source(closest, lm=None, pl=None):
    """(n,) int: SKY on a miss; on a hit LIGHTMAP where the lightmap's sample has weight > 0, else PROBES where the volume's has,
    else UNLIT.  A NaN weight is not > 0."""
    h = _words(closest, 16)
    hit = h[:, 0] != 0
    src = np.where(hit, UNLIT, SKY)
    with np.errstate(invalid="ignore"):
        by_probe = hit & (_words(pl, 8)[:, 3].view(F) > 0) if pl is not None else np.zeros(len(h), bool)
        by_map = hit & (_words(lm, 8)[:, 3].view(F) > 0) if lm is not None else np.zeros(len(h), bool)
    src[by_probe] = PROBES
    src[by_map] = LIGHTMAP   # the lightmap goes first: set last
    return src


def shade(closest, sky_rgb, albedo, emission, lm=None, pl=None):
    """steps 3 to 6 without the tonemap: dict(hdr (n, 3) float32, normal (n, 3) float32, depth (n,) float32, object_id (n,) int32,
    source (n,) int).  sky_rgb: `sky`'s rows; albedo, emission: `materials`'."""
    h = _words(closest, 16)
    n = len(h)
    src = source(h, lm, pl)
    E = np.zeros((n, 3), F)                                   # +0 where nothing lights the hit
    if lm is not None:
        E[src == LIGHTMAP] = _words(lm, 8)[src == LIGHTMAP, 0:3].view(F)
    if pl is not None:
        E[src == PROBES] = _words(pl, 8)[src == PROBES, 0:3].view(F)
    mesh = h[:, 8]
    hit = h[:, 0] != 0
    m = np.where(hit, mesh, 0)
    a, e = np.asarray(albedo, F), np.asarray(emission, F)
    assert not hit.any() or (mesh[hit].min() >= 0 and mesh[hit].max() < len(a)), "a hit on a mesh without a material"
    with np.errstate(all="ignore"):
        lit = ((a[m] * E).astype(F) / PI_F).astype(F) + e[m]  # the product, the quotient, the sum
    hdr = np.where(hit[:, None], lit, np.asarray(sky_rgb, F)).astype(F)
    return dict(hdr=np.ascontiguousarray(hdr), normal=np.ascontiguousarray(h[:, 5:8].view(F)), depth=np.ascontiguousarray(h[:, 1].view(F)),
                object_id=np.ascontiguousarray(mesh), source=src)


def rgb8(O, hdr, width, rows):
    """step 6's RGB8: the path frame's tonemap of the HDR image, (rows, width, 3) uint8, bottom-up as render_to_host has it"""
    return O.tonemap(np.asarray(hdr, F).reshape(rows * width, 3), width, rows)
