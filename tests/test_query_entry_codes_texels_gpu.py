"""test_query_entry_codes_gpu.py continued, in its style, for the entry points of csrc/ptrt_query.hip.h that came after it:
ptrt_irradiance_rays, ptrt_query_irradiance, ptrt_direct_rays, ptrt_query_direct, ptrt_bounce_terms, ptrt_query_bounce,
ptrt_atlas_texels, ptrt_atlas_dilate, ptrt_atlas_filter, ptrt_atlas_sample, ptrt_query_lightmap, ptrt_probe_sample and
ptrt_query_probe_light -- return code AND ptrt_last_error text of every call they refuse, and, where two reasons apply at once,
which one wins.  The table was written from the source of the commit before their host side was folded (the order of the
checks in each function) and confirmed against a build of it.  Sizes: a 16x16 context of two meshes of two faces and two
lights, 8 texels or rays, 3 directions, 2 shadow samples, a 4x4 atlas, a 2x2x2 probe volume.  Nothing here reaches a kernel
with a bad argument: every refused call returns before it enqueues anything (the huge counts of the overflow rows included:
they are refused before any pointer is looked at).  One return is out of reach: ptrt_atlas_texels' `slots <= 0`, since
ptrt_upload_geometry refuses a mesh without faces."""
import ctypes as C

import numpy as np
import pytest

from test_query_entry_codes_gpu import INT_MAX, INVALID, NOT_READY, OK, VP, desc, ptr  # noqa: F401  (desc: a fixture)

pytestmark = pytest.mark.gpu

N, DIRS, SHADOW, LIGHTS, AW, AH, W, H = 8, 3, 2, 2, 4, 4, 16, 16
RAYS, TERMS = N * DIRS, LIGHTS * SHADOW
VOLUME_ROWS = 8
MAX_ITEMS = INT_MAX * 256  # one thread per item in blocks of 256


@pytest.fixture(scope="module")
def mem(P):
    """name -> pointer: the good device arrays of every entry point, one pageable and one pinned host block, the probe
    volumes (host structs)"""
    import torch
    dev = torch.device("cuda", 0)

    def f32(*shape):
        return torch.zeros(shape, dtype=torch.float32, device=dev)

    def i32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev)

    nrm = f32(N, 3)
    nrm[:, 2] = 1.0
    d = f32(N, 3)
    d[:, 2] = -1.0
    keep = {
        "pos": f32(N, 3), "nrm": nrm, "s2": f32(DIRS, 2) + 0.5, "sh2": f32(SHADOW, 2) + 0.5, "ph": f32(N),
        "st": i32(RAYS, 6) + 1, "o": f32(N, 3), "d": d, "hits": i32(RAYS, 16), "rdirs": f32(RAYS, 3),
        "ro": f32(RAYS, 3), "rd": f32(RAYS, 3),                                    # irradiance_rays' outputs
        "qo": f32(N * TERMS, 3), "qd": f32(N * TERMS, 3), "qt": f32(N * TERMS), "qw": f32(N * TERMS, 3),  # direct_rays'
        "bo": f32(RAYS * TERMS, 3), "bl": f32(RAYS * TERMS, 3), "bt": f32(RAYS * TERMS), "bv": f32(RAYS * TERMS, 3),  # bounce_terms'
        "out": f32(N, 8), "uv": f32(2, 6), "texels": i32(AW * AH, 8) - 1, "a": f32(AH, AW, 4), "b": f32(AH, AW, 4),
        "charts": f32(2, 6), "cf": i32(2), "image": f32(AH, AW, 4), "hits8": i32(N, 16), "probes": f32(VOLUME_ROWS, 32),
        "big": f32(1024), "pinned": torch.zeros(16384, dtype=torch.uint8).pin_memory(),
    }
    pageable = np.zeros(16384, np.uint8)
    m = {k: VP(t.data_ptr()) for k, t in keep.items()}
    m["pageable"] = VP(pageable.ctypes.data)
    vols = {"vol": ((0, 0, 0), (1, 1, 1), (2, 2, 2)), "vol_count0": ((0, 0, 0), (1, 1, 1), (2, 0, 2)),
            "vol_spacing": ((0, 0, 0), (0, 1, 1), (2, 2, 2)), "vol_origin": ((0, 0, float("nan")), (1, 1, 1), (2, 2, 2)),
            "vol_big": ((0, 0, 0), (1, 1, 1), (4097, 4096, 0)), "vol_inf": ((0, 0, 0), (1, float("inf"), 1), (2, 2, 2))}
    for k, (origin, spacing, counts) in vols.items():
        keep[k] = P.ProbeVolumeDesc((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*counts))
        m[k] = VP(C.addressof(keep[k]))
    m["_tensors"] = keep
    torch.cuda.synchronize()
    yield m
    torch.cuda.synchronize()
    del keep, pageable


@pytest.fixture(scope="module")
def ctxs(P, desc):
    """state -> context.  null: no context; empty: created, two lights, nothing else; geom: and the geometry; few: and one
    material for the two meshes; full: the scene and the two lights; dark: the scene without a light"""
    lib = P.lib
    _, d = desc
    lights = (P.Light * LIGHTS)()
    for i, l in enumerate(lights):
        l.type, l.position, l.color, l.intensity, l.range = 0, P.Vec3(0.5 * i, 0.0, -1.0), P.Vec3(1.0, 1.0, 1.0), 1.0, 100.0

    def create():
        ctx = VP()
        assert lib.ptrt_create(W, H, 0, 0, 0, C.byref(ctx)) == OK
        return ctx

    c = {"null": None, "empty": create(), "geom": create(), "few": create(), "full": create(), "dark": create()}
    for k in ("geom", "few"):
        assert lib.ptrt_upload_geometry(c[k], d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices,
                                        d.tlas_index_count) == OK
    one = P.Materials()
    C.memmove(C.byref(one), C.byref(d.materials), C.sizeof(P.Materials))
    one.count = 1
    assert lib.ptrt_upload_materials(c["few"], C.byref(one)) == OK
    for k in ("full", "dark"):
        assert lib.ptrt_upload_scene(c[k], C.byref(d)) == OK
    for k in ("empty", "geom", "few", "full"):
        assert lib.ptrt_upload_lights(c[k], lights, LIGHTS) == OK
    yield c
    for k in c:
        if c[k] is not None:
            assert lib.ptrt_sync(c[k]) == OK
            lib.ptrt_destroy(c[k])


# ---- the entry points: default (good) arguments by name, in the order of the C signature behind the context ------------
def good_args(m):
    texel = dict(pos=m["pos"], nrm=m["nrm"], n=N, s2=m["s2"])
    lm = dict(n=N, charts=m["charts"], ncf=2, cf=m["cf"], image=m["image"], aw=AW, ah=AH, mode=1, out=m["out"])
    pv = dict(n=N, vol=m["vol"], probes=m["probes"], mode=1, bias=0.0, out=m["out"])
    return {
        "irr_rays": dict(texel, k=DIRS, ph=m["ph"], offset=1e-4, o=m["ro"], d=m["rd"]),
        "irradiance": dict(texel, k=DIRS, ph=m["ph"], offset=1e-4, st=m["st"], samples=1, max_depth=2, max_distance=5.0, out=m["out"]),
        "dir_rays": dict(texel, k=SHADOW, ph=m["ph"], offset=1e-4, lf=0, lc=LIGHTS, o=m["qo"], d=m["qd"], t=m["qt"], w=m["qw"]),
        "direct": dict(texel, k=SHADOW, ph=m["ph"], offset=1e-4, lf=0, lc=LIGHTS, out=m["out"]),
        "terms": dict(hits=m["hits"], dirs=m["rdirs"], n=N, k=DIRS, sh2=m["sh2"], m=SHADOW, ph=m["ph"], lf=0, lc=LIGHTS, o=m["bo"],
                      l=m["bl"], t=m["bt"], v=m["bv"]),
        "bounce": dict(texel, k=DIRS, ph=m["ph"], offset=1e-4, sh2=m["sh2"], m=SHADOW, lf=0, lc=LIGHTS, out=m["out"]),
        "texels": dict(mesh=0, uv=m["uv"], aw=AW, ah=AH, clear=1, texels=m["texels"]),
        "dilate": dict(a=m["a"], b=m["b"], aw=AW, ah=AH, passes=1),
        "filter": dict(texels=m["texels"], a=m["a"], b=m["b"], aw=AW, ah=AH, passes=2, sd=1.0, sp=0.5, power=2),
        "sample": dict(dict(hits=m["hits8"]), **lm),
        "lightmap": dict(dict(o=m["o"], d=m["d"]), **lm),
        "psample": dict(dict(pos=m["pos"], nrm=m["nrm"]), **pv),
        "plight": dict(dict(o=m["o"], d=m["d"]), **pv),
    }


FN = {"irr_rays": "ptrt_irradiance_rays", "irradiance": "ptrt_query_irradiance", "dir_rays": "ptrt_direct_rays",
      "direct": "ptrt_query_direct", "terms": "ptrt_bounce_terms", "bounce": "ptrt_query_bounce", "texels": "ptrt_atlas_texels",
      "dilate": "ptrt_atlas_dilate", "filter": "ptrt_atlas_filter", "sample": "ptrt_atlas_sample", "lightmap": "ptrt_query_lightmap",
      "psample": "ptrt_probe_sample", "plight": "ptrt_query_probe_light"}


def call(lib, entry, ctx, a):
    return getattr(lib, FN[entry])(ctx, *a.values())


# the pointer arguments that must be device memory, in the order they are checked: (argument, its name in the message, bytes)
TEXEL_SPANS = [("pos", "positions", N * 12), ("nrm", "normals", N * 12)]
LM_SPANS = [("charts", "charts", 48), ("cf", "chart_first", 8), ("image", "image", AW * AH * 16), ("out", "out", N * 32)]
PV_SPANS = [("probes", "probes", VOLUME_ROWS * 128), ("out", "out", N * 32)]
SPANS = {
    "irr_rays": TEXEL_SPANS + [("s2", "samples2", DIRS * 8), ("ph", "phases", N * 4), ("o", "origins", RAYS * 12), ("d", "directions", RAYS * 12)],
    "irradiance": TEXEL_SPANS + [("s2", "samples2", DIRS * 8), ("ph", "phases", N * 4), ("st", "rng_states", RAYS * 24), ("out", "out", N * 32)],
    "dir_rays": TEXEL_SPANS + [("s2", "samples2", SHADOW * 8), ("ph", "phases", N * 4), ("o", "origins", N * TERMS * 12),
                               ("d", "directions", N * TERMS * 12), ("t", "tmax", N * TERMS * 4), ("w", "weights", N * TERMS * 12)],
    "direct": TEXEL_SPANS + [("s2", "samples2", SHADOW * 8), ("ph", "phases", N * 4), ("out", "out", N * 32)],
    "terms": [("hits", "hits", RAYS * 64), ("dirs", "directions", RAYS * 12), ("sh2", "shadow2", SHADOW * 8), ("ph", "phases", N * 4),
              ("o", "origins", RAYS * TERMS * 12), ("l", "L", RAYS * TERMS * 12), ("t", "tmax", RAYS * TERMS * 4),
              ("v", "values", RAYS * TERMS * 12)],
    "bounce": TEXEL_SPANS + [("s2", "samples2", DIRS * 8), ("ph", "phases", N * 4), ("sh2", "shadow2", SHADOW * 8), ("out", "out", N * 32)],
    "texels": [("uv", "uv", 48), ("texels", "texels", AW * AH * 32)],
    "dilate": [("a", "a", AW * AH * 16), ("b", "b", AW * AH * 16)],
    "filter": [("texels", "texels", AW * AH * 32), ("a", "a", AW * AH * 16), ("b", "b", AW * AH * 16)],
    "sample": [("hits", "hits", N * 64)] + LM_SPANS,
    "lightmap": [("o", "origins", N * 12), ("d", "directions", N * 12)] + LM_SPANS,
    "psample": [("pos", "positions", N * 12), ("nrm", "normals", N * 12)] + PV_SPANS,
    "plight": [("o", "origins", N * 12), ("d", "directions", N * 12)] + PV_SPANS,
}
# what each entry point says of a NULL pointer or a bad count; {..} are the call's own arguments as printf prints them
BAD = {
    "irr_rays": "ptrt_irradiance_rays: bad argument (n_texels {n}, n_dirs {k}, positions {pos}, normals {nrm}, samples2 {s2}, origins {o}, directions {d})",
    "irradiance": "ptrt_query_irradiance: bad argument (n_texels {n}, n_dirs {k}, positions {pos}, normals {nrm}, samples2 {s2}, rng_states {st}, out {out})",
    "dir_rays": "ptrt_direct_rays: bad argument (origins {o}, directions {d}, tmax {t}, weights {w})",
    "direct": "ptrt_query_direct: bad argument (out {out})",
    "terms": "ptrt_bounce_terms: bad argument (hits {hits}, directions {dirs}, origins {o}, L {l}, tmax {t}, values {v})",
    "bounce": "ptrt_query_bounce: bad argument (positions {pos}, normals {nrm}, samples2 {s2}, out {out})",
    "texels": "ptrt_atlas_texels: bad argument (uv {uv}, texels {texels}, atlas {aw} x {ah}: 1 x 1 .. 2^28 texels)",
    "dilate": "ptrt_atlas_dilate: bad argument (a {a}, b {b}, atlas {aw} x {ah}: 1 x 1 .. 2^28 texels, passes {passes}: 1 .. 64)",
    "filter": "ptrt_atlas_filter: bad argument (texels {texels}, a {a}, b {b}, atlas {aw} x {ah}: 1 x 1 .. 2^28 texels, passes {passes}: 1 .. 8, "
              "normal_power {power}: 0 .. 7)",
}
BAD_DIRECT = "{fn}: bad argument (n_texels {n}, n_shadow {k}, positions {pos}, normals {nrm}, samples2 {s2})"      # check_direct
BAD_BOUNCE = "{fn}: bad argument (n_texels {n}, n_dirs {k}, n_shadow {m}, shadow2 {sh2})"                           # check_bounce
BAD_LM = ("{fn}: bad argument (n {n}, charts {charts}, n_chart_faces {ncf}: >= 1, chart_first {cf}, image {image}, atlas {aw} x {ah}: "
          "1 x 1 .. 2^28 texels, mode {mode}: 0 or 1, out {out})")                                                 # check_lightmap
BAD_PV = "{fn}: bad argument (n {n}, volume {vol}, probes {probes}, mode {mode}: 0 or 1, normal_bias {bias:g}: >= 0 and finite, out {out})"
LIGHTS_TEXT = "{fn}: lights {lf} .. {lf} + {lc} of {have} uploaded"
NO_GEOMETRY, NO_MATERIALS, FEW = "{fn}: geometry not uploaded", "{fn}: materials not uploaded", "{fn}: 1 materials for 2 meshes"
SAMPLES, DISTANCE = "{fn}: samples={samples} max_depth={max_depth} (1..32767)", "{fn}: max_distance={max_distance:g} (positive and finite)"
IN_ALIGN = "{fn}: {name} {p} must not be NULL and must be {align}-byte aligned"
LM_ALIGN = "{fn}: image {image} and out {out} must be 16-byte aligned, charts {charts} and chart_first {cf} 4-byte"
PV_ALIGN = "{fn}: probes {probes} and out {out} must be 16-byte aligned"
OVERLAPS = "{fn}: out {out} ({nout} bytes) overlaps {name} {p} ({bytes} bytes)"
SIGMAS = ("ptrt_atlas_filter: sigma_distance {sd:g}, sigma_plane {sp:g}: positive and finite, with finite non-zero squares in fp32 at every "
          "step of {passes} passes")
FILTER_ALIGN = "ptrt_atlas_filter: texels {texels}, a {a} and b {b} must be 16-byte aligned"
FILTER_OVERLAP = "ptrt_atlas_filter: a {a} and b {b} (256 bytes each) and texels {texels} (512 bytes) must not overlap"
DILATE_APART = "ptrt_atlas_dilate: a {a} and b {b} must be 16-byte aligned and 256 bytes apart"
TEXELS_ALIGN = "ptrt_atlas_texels: texels {texels} must be 16-byte aligned, uv {uv} 4-byte"
INF, NAN, HOST = float("inf"), float("nan"), "pageable"

# (entry point, context state, arguments that differ from the good ones, return code, message, what the message names beyond
# the call's arguments).  A string is a block of `mem`, (block, bytes) a pointer into it.
TABLE = [
    # ---- ptrt_irradiance_rays: needs no scene
    ("irr_rays", "empty", {"n": -1, "offset": INF}, INVALID, BAD["irr_rays"], {}),
    ("irr_rays", "empty", {"k": 0, "offset": NAN}, INVALID, BAD["irr_rays"], {}),
    ("irr_rays", "empty", {"offset": INF}, INVALID, "ptrt_irradiance_rays: offset=inf (finite)", {}),
    ("irr_rays", "empty", {"offset": NAN, "n": 0}, INVALID, "ptrt_irradiance_rays: offset=nan (finite)", {}),   # before n == 0
    ("irr_rays", "empty", {"n": 0, "pos": HOST, "nrm": HOST, "s2": HOST, "ph": HOST, "o": HOST, "d": HOST}, OK, None, {}),
    ("irr_rays", "empty", {"n": INT_MAX, "k": INT_MAX, "pos": HOST}, INVALID,
     "ptrt_irradiance_rays: 2147483647 texels x 2147483647 directions: the rays' byte count overflows", {}),
    ("irr_rays", "empty", {"n": INT_MAX, "k": 257, "pos": HOST}, INVALID,
     f"ptrt_irradiance_rays: 2147483647 texels x 257 directions: more than {MAX_ITEMS} rays in one call", {}),
    ("irr_rays", "empty", {}, OK, None, {}),
    ("irr_rays", "empty", {"ph": None}, OK, None, {}),
    # ---- ptrt_query_irradiance
    ("irradiance", "empty", {"n": -1, "offset": INF, "samples": 0}, INVALID, BAD["irradiance"], {}),
    ("irradiance", "full", {"k": 0}, INVALID, BAD["irradiance"], {}),
    ("irradiance", "empty", {"offset": -INF, "samples": 0}, INVALID, "ptrt_query_irradiance: offset=-inf (finite)", {}),
    ("irradiance", "empty", {"samples": 0, "max_distance": 0.0}, INVALID, SAMPLES, {}),
    ("irradiance", "full", {"max_depth": 32768}, INVALID, SAMPLES, {}),
    ("irradiance", "empty", {"max_distance": 0.0}, INVALID, DISTANCE, {}),                                        # before the scene
    ("irradiance", "full", {"max_distance": INF, "n": 0}, INVALID, DISTANCE, {}),
    ("irradiance", "empty", {}, NOT_READY, NO_GEOMETRY, {}),
    ("irradiance", "geom", {"n": 0}, NOT_READY, NO_MATERIALS, {}),                                                # n == 0 is OK only of a scene
    ("irradiance", "few", {}, NOT_READY, FEW, {}),
    ("irradiance", "full", {"n": 0, "pos": HOST, "nrm": HOST, "s2": HOST, "ph": HOST, "st": HOST, "out": HOST}, OK, None, {}),
    ("irradiance", "full", {"n": INT_MAX, "k": INT_MAX, "pos": HOST}, INVALID,
     "ptrt_query_irradiance: 2147483647 texels x 2147483647 directions: the states' byte count overflows", {}),
    ("irradiance", "full", {}, OK, None, {}),
    ("irradiance", "full", {"ph": None}, OK, None, {}),
    # ---- ptrt_direct_rays: its own pointers, then check_direct; needs no scene, only the lights
    ("dir_rays", "empty", {"o": None, "n": -1}, INVALID, BAD["dir_rays"], {}),
    ("dir_rays", "empty", {"n": -1, "lf": -1, "offset": INF}, INVALID, BAD_DIRECT, {}),
    ("dir_rays", "empty", {"k": 0}, INVALID, BAD_DIRECT, {}),
    ("dir_rays", "empty", {"s2": None, "lc": 3}, INVALID, BAD_DIRECT, {}),
    ("dir_rays", "empty", {"lf": -1, "offset": INF}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("dir_rays", "empty", {"lc": -1}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("dir_rays", "empty", {"lf": 1, "lc": 2}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("dir_rays", "empty", {"lf": INT_MAX, "lc": INT_MAX}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("dir_rays", "dark", {"lc": 1}, INVALID, LIGHTS_TEXT, {"have": 0}),
    ("dir_rays", "empty", {"offset": INF, "k": INT_MAX}, INVALID, "ptrt_direct_rays: offset=inf (finite)", {}),
    ("dir_rays", "empty", {"k": INT_MAX, "n": 0}, INVALID,
     "ptrt_direct_rays: 2 lights x 2147483647 shadow samples: more than 2147483647 terms per texel", {}),
    ("dir_rays", "empty", {"lc": 1, "k": INT_MAX, "n": INT_MAX, "pos": HOST}, INVALID,
     "ptrt_direct_rays: 2147483647 texels x 2147483647 terms: the rays' byte count overflows", {}),
    ("dir_rays", "empty", {"lc": 1, "k": 257, "n": INT_MAX, "pos": HOST}, INVALID,
     f"ptrt_direct_rays: 2147483647 texels x 257 terms: more than {MAX_ITEMS} rays in one call", {}),
    ("dir_rays", "empty", {"n": 0, "pos": HOST, "o": HOST}, OK, None, {}),
    ("dir_rays", "empty", {"lc": 0, "pos": HOST, "o": HOST}, OK, None, {}),                                       # no lights: no rays
    ("dir_rays", "dark", {"lc": 0, "lf": 0, "pos": HOST}, OK, None, {}),
    ("dir_rays", "empty", {}, OK, None, {}),
    ("dir_rays", "empty", {"ph": None, "lf": 1, "lc": 1}, OK, None, {}),
    # ---- ptrt_query_direct
    ("direct", "empty", {"out": None, "n": -1}, INVALID, BAD["direct"], {}),
    ("direct", "empty", {"n": -1, "lc": 3}, INVALID, BAD_DIRECT, {}),
    ("direct", "empty", {"pos": None}, INVALID, BAD_DIRECT, {}),
    ("direct", "empty", {"lc": 3, "offset": NAN}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("direct", "empty", {"offset": NAN}, INVALID, "ptrt_query_direct: offset=nan (finite)", {}),                  # before the scene
    ("direct", "empty", {"k": INT_MAX}, INVALID, "ptrt_query_direct: 2 lights x 2147483647 shadow samples: more than 2147483647 terms per texel", {}),
    ("direct", "empty", {"lc": 1, "k": INT_MAX, "n": INT_MAX}, INVALID,
     "ptrt_query_direct: 2147483647 texels x 2147483647 terms: the rays' byte count overflows", {}),
    ("direct", "empty", {}, NOT_READY, NO_GEOMETRY, {}),
    ("direct", "empty", {"n": 0}, NOT_READY, NO_GEOMETRY, {}),
    ("direct", "geom", {"n": 0, "pos": HOST, "nrm": HOST, "s2": HOST, "ph": HOST, "out": HOST}, OK, None, {}),  # (needs no materials)
    ("direct", "geom", {"lc": 0, "out": HOST}, INVALID, "ptrt_query_direct: out is not 256 bytes of device memory on device 0", {}),
    ("direct", "geom", {}, OK, None, {}),
    ("direct", "full", {"ph": None}, OK, None, {}),
    # ---- ptrt_bounce_terms: its own pointers, then check_bounce; needs the materials, no geometry
    ("terms", "full", {"hits": None, "n": -1}, INVALID, BAD["terms"], {}),
    ("terms", "full", {"n": -1, "lc": 3}, INVALID, BAD_BOUNCE, {}),
    ("terms", "full", {"k": 0}, INVALID, BAD_BOUNCE, {}),
    ("terms", "full", {"m": 0}, INVALID, BAD_BOUNCE, {}),
    ("terms", "empty", {"sh2": None}, INVALID, BAD_BOUNCE, {}),
    ("terms", "empty", {"lc": 3}, INVALID, LIGHTS_TEXT, {"have": 2}),                                             # before the materials
    ("terms", "full", {"lf": -1}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("terms", "full", {"m": INT_MAX}, INVALID,
     "ptrt_bounce_terms: 3 directions x 2 lights x 2147483647 shadow samples: more than 2147483647 terms per texel", {}),
    ("terms", "full", {"k": INT_MAX, "n": INT_MAX, "lc": 1}, INVALID,
     "ptrt_bounce_terms: 2147483647 directions x 1 lights x 2 shadow samples: more than 2147483647 terms per texel", {}),
    ("terms", "full", {"k": INT_MAX, "n": INT_MAX, "lc": 0, "hits": HOST}, INVALID,
     "ptrt_bounce_terms: 2147483647 texels x 2147483647 directions x 0 terms: a byte count overflows", {}),
    ("terms", "full", {"k": 32768, "n": INT_MAX, "lc": 1, "m": 32768, "hits": HOST}, INVALID,
     "ptrt_bounce_terms: 2147483647 texels x 32768 directions x 32768 terms: a byte count overflows", {}),
    ("terms", "empty", {"k": 1, "n": INT_MAX, "lc": 1, "m": 257, "hits": HOST}, INVALID,                          # before the materials
     f"ptrt_bounce_terms: 2147483647 rays x 257 terms: more than {MAX_ITEMS} rows in one call", {}),
    ("terms", "empty", {"n": 0}, NOT_READY, NO_MATERIALS, {}),
    ("terms", "geom", {}, NOT_READY, NO_MATERIALS, {}),
    ("terms", "full", {"n": 0, "hits": HOST, "o": HOST}, OK, None, {}),
    ("terms", "full", {"lc": 0, "hits": HOST, "o": HOST}, OK, None, {}),                                          # no lights: no rows
    ("terms", "few", {}, OK, None, {}),                                                                            # (any materials will do)
    ("terms", "full", {"ph": None}, OK, None, {}),
    # ---- ptrt_query_bounce
    ("bounce", "empty", {"pos": None, "n": -1}, INVALID, BAD["bounce"], {}),
    ("bounce", "empty", {"n": -1, "lc": 3}, INVALID, BAD_BOUNCE, {}),
    ("bounce", "empty", {"sh2": None, "offset": INF}, INVALID, BAD_BOUNCE, {}),
    ("bounce", "empty", {"lc": 3, "offset": INF}, INVALID, LIGHTS_TEXT, {"have": 2}),
    ("bounce", "empty", {"offset": INF, "m": INT_MAX}, INVALID, "ptrt_query_bounce: offset=inf (finite)", {}),
    ("bounce", "empty", {"m": INT_MAX}, INVALID,
     "ptrt_query_bounce: 3 directions x 2 lights x 2147483647 shadow samples: more than 2147483647 terms per texel", {}),
    ("bounce", "empty", {"k": INT_MAX, "n": INT_MAX, "lc": 0}, INVALID,
     "ptrt_query_bounce: 2147483647 texels x 2147483647 directions x 0 terms: a byte count overflows", {}),
    ("bounce", "empty", {}, NOT_READY, NO_GEOMETRY, {}),
    ("bounce", "geom", {"n": 0}, NOT_READY, NO_MATERIALS, {}),
    ("bounce", "few", {"n": 0}, NOT_READY, FEW, {}),
    ("bounce", "full", {"n": 0, "pos": HOST, "nrm": HOST, "s2": HOST, "ph": HOST, "sh2": HOST, "out": HOST}, OK, None, {}),
    ("bounce", "full", {"lc": 0, "out": HOST}, INVALID, "ptrt_query_bounce: out is not 256 bytes of device memory on device 0", {}),
    ("bounce", "full", {}, OK, None, {}),
    ("bounce", "full", {"ph": None}, OK, None, {}),
    # ---- ptrt_atlas_texels
    ("texels", "empty", {"uv": None}, INVALID, BAD["texels"], {}),
    ("texels", "empty", {"texels": None, "mesh": -1}, INVALID, BAD["texels"], {}),
    ("texels", "full", {"aw": 0}, INVALID, BAD["texels"], {}),
    ("texels", "full", {"ah": -1, "texels": ("texels", 4)}, INVALID, BAD["texels"], {}),
    ("texels", "full", {"aw": 2 ** 14 + 1, "ah": 2 ** 14}, INVALID, BAD["texels"], {}),
    ("texels", "empty", {"texels": ("texels", 8)}, INVALID, TEXELS_ALIGN, {}),                                    # before the scene
    ("texels", "full", {"uv": ("uv", 2)}, INVALID, TEXELS_ALIGN, {}),
    ("texels", "empty", {"mesh": -1}, NOT_READY, NO_GEOMETRY, {}),
    ("texels", "geom", {"mesh": -1, "uv": HOST}, INVALID, "ptrt_atlas_texels: mesh -1 of 2 uploaded", {}),
    ("texels", "geom", {"mesh": 2}, INVALID, "ptrt_atlas_texels: mesh 2 of 2 uploaded", {}),
    ("texels", "geom", {"mesh": 1, "clear": 0}, OK, None, {}),
    ("texels", "geom", {}, OK, None, {}),
    # ---- ptrt_atlas_dilate: needs no scene
    ("dilate", "empty", {"a": None}, INVALID, BAD["dilate"], {}),
    ("dilate", "empty", {"b": None, "passes": 0}, INVALID, BAD["dilate"], {}),
    ("dilate", "empty", {"aw": 0, "a": ("a", 4)}, INVALID, BAD["dilate"], {}),
    ("dilate", "empty", {"passes": 0}, INVALID, BAD["dilate"], {}),
    ("dilate", "empty", {"passes": 65, "b": "a"}, INVALID, BAD["dilate"], {}),
    ("dilate", "empty", {"a": ("a", 4)}, INVALID, DILATE_APART, {}),
    ("dilate", "empty", {"b": ("b", 8), "a": HOST}, INVALID, DILATE_APART, {}),
    ("dilate", "empty", {"b": "a"}, INVALID, DILATE_APART, {}),
    ("dilate", "empty", {"a": "big", "b": ("big", 240)}, INVALID, DILATE_APART, {}),
    ("dilate", "empty", {"a": ("big", 240), "b": "big"}, INVALID, DILATE_APART, {}),
    ("dilate", "empty", {"a": HOST, "b": (HOST, 16)}, INVALID, DILATE_APART, {}),                                 # before the spans
    ("dilate", "empty", {"a": "big", "b": ("big", 256)}, OK, None, {}),
    ("dilate", "empty", {"passes": 64}, OK, None, {}),
    # ---- ptrt_atlas_filter: needs no scene
    ("filter", "empty", {"texels": None, "sd": 0.0}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"a": None}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"b": None}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"ah": 0}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"passes": 0}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"passes": 9, "sp": 0.0}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"power": -1, "a": ("a", 4)}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"power": 8}, INVALID, BAD["filter"], {}),
    ("filter", "empty", {"sd": 0.0, "a": ("a", 4)}, INVALID, SIGMAS, {}),
    ("filter", "empty", {"sd": -1.0}, INVALID, SIGMAS, {}),
    ("filter", "empty", {"sd": INF}, INVALID, SIGMAS, {}),
    ("filter", "empty", {"sp": NAN}, INVALID, SIGMAS, {}),
    ("filter", "empty", {"sp": 0.0, "b": "a"}, INVALID, SIGMAS, {}),
    ("filter", "empty", {"sp": 2.0 ** -80}, INVALID, SIGMAS, {}),                                                 # its square is 0 in fp32
    ("filter", "empty", {"sd": 2.0 ** 60, "passes": 5}, INVALID, SIGMAS, {}),                                     # (2^64)^2 at step 16
    ("filter", "empty", {"sd": 2.0 ** 60, "passes": 4}, OK, None, {}),
    ("filter", "empty", {"a": ("a", 4), "b": "a"}, INVALID, FILTER_ALIGN, {}),
    ("filter", "empty", {"b": ("b", 8)}, INVALID, FILTER_ALIGN, {}),
    ("filter", "empty", {"texels": ("texels", 4), "a": HOST}, INVALID, FILTER_ALIGN, {}),
    ("filter", "empty", {"b": "a"}, INVALID, FILTER_OVERLAP, {}),
    ("filter", "empty", {"a": "texels"}, INVALID, FILTER_OVERLAP, {}),
    ("filter", "empty", {"b": ("texels", 496)}, INVALID, FILTER_OVERLAP, {}),
    ("filter", "empty", {"texels": ("big", 240), "b": "big"}, INVALID, FILTER_OVERLAP, {}),
    ("filter", "empty", {"a": HOST, "b": (HOST, 16), "texels": (HOST, 32)}, INVALID, FILTER_OVERLAP, {}),      # before the spans
    ("filter", "empty", {"texels": ("big", 512), "a": "big", "b": ("big", 256)}, OK, None, {}),
    ("filter", "empty", {"passes": 8, "power": 7}, OK, None, {}),
    ("filter", "empty", {"passes": 1, "power": 0}, OK, None, {}),
]


def lm_rows(e, ins, align):
    """check_lightmap's refusals for entry point `e` whose own inputs are `ins`, aligned to `align` bytes"""
    first = ins[0]
    rows = [
        (e, "empty", {"n": -1, first: None}, INVALID, BAD_LM, {}),
        (e, "empty", {"ncf": 0}, INVALID, BAD_LM, {}),
        (e, "empty", {"charts": None}, INVALID, BAD_LM, {}),
        (e, "empty", {"cf": None}, INVALID, BAD_LM, {}),
        (e, "empty", {"image": None}, INVALID, BAD_LM, {}),
        (e, "empty", {"out": None}, INVALID, BAD_LM, {}),
        (e, "empty", {"aw": 0, "image": ("image", 4)}, INVALID, BAD_LM, {}),
        (e, "empty", {"aw": 2 ** 14, "ah": 2 ** 14 + 1}, INVALID, BAD_LM, {}),
        (e, "empty", {"mode": 2}, INVALID, BAD_LM, {}),
        (e, "empty", {"mode": -1, "n": 0}, INVALID, BAD_LM, {}),
        (e, "empty", {"image": ("image", 4), "charts": ("charts", 2)}, INVALID, LM_ALIGN, {}),                   # before the scene
        (e, "full", {"out": ("out", 8)}, INVALID, LM_ALIGN, {}),
        (e, "full", {"charts": ("charts", 2)}, INVALID, LM_ALIGN, {}),
        (e, "full", {"cf": ("cf", 1), "n": 0}, INVALID, LM_ALIGN, {}),
        (e, "empty", {}, NOT_READY, NO_GEOMETRY, {}),
        (e, "empty", {"n": 0}, NOT_READY, NO_GEOMETRY, {}),                                                        # n == 0 is OK only of a scene
        (e, "geom", dict({"n": 0, "charts": HOST, "cf": HOST, "image": HOST, "out": HOST}, **{k: HOST for k in ins}), OK, None, {}),
        (e, "geom", {"n": 0, "out": "image"}, OK, None, {}),                                                       # (nothing to overlap)
        # out against the lightmap's three arrays in their order, then the caller's own; before the spans
        (e, "geom", {"out": "charts", "image": HOST}, INVALID, OVERLAPS, {"nout": 256, "name": "charts", "p": "charts", "bytes": 48}),
        (e, "geom", {"out": "cf"}, INVALID, OVERLAPS, {"nout": 256, "name": "chart_first", "p": "cf", "bytes": 8}),
        (e, "geom", {"out": "image"}, INVALID, OVERLAPS, {"nout": 256, "name": "image", "p": "image", "bytes": 256}),
        (e, "geom", {"out": "big", "image": ("big", 240)}, INVALID, OVERLAPS, {"nout": 256, "name": "image", "p": "image", "bytes": 256}),
        (e, "geom", {"out": ("big", 240), "image": "big", "charts": ("big", 480)}, INVALID, OVERLAPS,
         {"nout": 256, "name": "charts", "p": "charts", "bytes": 48}),                                            # charts before image
        (e, "geom", {"out": ("big", 48), "charts": "big", "n": 1}, OK, None, {}),                                  # (they touch)
        (e, "geom", {"out": "big", "image": ("big", 256)}, OK, None, {}),
        (e, "geom", {}, OK, None, {}),                                                                             # (needs no materials)
        (e, "full", {"mode": 0}, OK, None, {}),
    ]
    for k in ins:
        name = [nm for a, nm, _ in SPANS[e] if a == k][0]
        nbytes = [b for a, _, b in SPANS[e] if a == k][0]
        block = "hits8" if k == "hits" else k   # (its block of `mem`)
        rows += [
            (e, "empty", {k: None, "image": ("image", 4)}, INVALID, IN_ALIGN, {"name": name, "p": k, "align": align}),
            (e, "empty", {k: (block, align // 2), "n": 0}, INVALID, IN_ALIGN, {"name": name, "p": k, "align": align}),
            (e, "geom", {"out": block}, INVALID, OVERLAPS, {"nout": 256, "name": name, "p": k, "bytes": nbytes}),
        ]
    return rows


def pv_rows(e, ins, need_geometry):
    """check_probe_volume's refusals for entry point `e` whose own inputs are `ins`"""
    first = ins[0]
    axis = "{fn}: volume axis {a}: count {count} (>= 1), spacing {spacing:g} (positive and finite), origin {origin:g} (finite)"
    rows = [
        (e, "empty", {"n": -1, first: None}, INVALID, BAD_PV, {}),
        (e, "empty", {"vol": None}, INVALID, BAD_PV, {}),
        (e, "empty", {"probes": None, "vol": "vol_count0"}, INVALID, BAD_PV, {}),
        (e, "empty", {"out": None}, INVALID, BAD_PV, {}),
        (e, "empty", {"mode": 2}, INVALID, BAD_PV, {}),
        (e, "empty", {"mode": -1, "n": 0}, INVALID, BAD_PV, {}),
        (e, "empty", {"bias": -1.0}, INVALID, BAD_PV, {}),
        (e, "empty", {"bias": INF}, INVALID, BAD_PV, {}),
        (e, "empty", {"bias": NAN, first: None}, INVALID, BAD_PV, {}),
        (e, "empty", {"vol": "vol_count0", first: None}, INVALID, axis, dict(a=1, count=0, spacing=1.0, origin=0.0)),
        (e, "empty", {"vol": "vol_spacing"}, INVALID, axis, dict(a=0, count=2, spacing=0.0, origin=0.0)),
        (e, "empty", {"vol": "vol_inf"}, INVALID, axis, dict(a=1, count=2, spacing=INF, origin=0.0)),
        (e, "empty", {"vol": "vol_origin", "n": 0}, INVALID, axis, dict(a=2, count=2, spacing=1.0, origin=NAN)),
        (e, "empty", {"vol": "vol_big"}, INVALID, "{fn}: a volume of 4097 x 4096 x 0 probes (at most 2^24)", {}),   # before axis 2
        (e, "empty", {"probes": ("probes", 4), "out": ("out", 8)}, INVALID, PV_ALIGN, {}),
        (e, "empty", {"out": ("out", 8), "n": 0}, INVALID, PV_ALIGN, {}),
        (e, "full", {"n": 0, "probes": HOST, "out": HOST, **{k: HOST for k in ins}}, OK, None, {}),
        (e, "full", {"out": "probes", first: HOST}, INVALID, OVERLAPS, {"nout": 256, "name": "probes", "p": "probes", "bytes": 1024}),
        (e, "full", {"out": ("probes", 1008)}, INVALID, OVERLAPS, {"nout": 256, "name": "probes", "p": "probes", "bytes": 1024}),
        (e, "full", {"out": "big", "probes": ("big", 240)}, INVALID, OVERLAPS, {"nout": 256, "name": "probes", "p": "probes", "bytes": 1024}),
        (e, "full", {"out": "big", "probes": ("big", 256)}, OK, None, {}),
        (e, "full", {"mode": 0, "bias": 0.25}, OK, None, {}),
    ]
    if need_geometry:
        rows += [(e, "empty", {}, NOT_READY, NO_GEOMETRY, {}), (e, "empty", {"n": 0}, NOT_READY, NO_GEOMETRY, {}),
                 (e, "empty", {"out": ("out", 8)}, INVALID, PV_ALIGN, {}), (e, "geom", {}, OK, None, {})]
    else:
        rows += [(e, "empty", {}, OK, None, {}), (e, "empty", {"n": 0, "probes": HOST}, OK, None, {})]
    for k in ins:
        name = [nm for a, nm, _ in SPANS[e] if a == k][0]
        rows += [
            (e, "empty", {k: None, "probes": ("probes", 4)}, INVALID, IN_ALIGN, {"name": name, "p": k, "align": 4}),
            (e, "empty", {k: (k, 2), "n": 0}, INVALID, IN_ALIGN, {"name": name, "p": k, "align": 4}),
            (e, "full", {"out": k}, INVALID, OVERLAPS, {"nout": 256, "name": name, "p": k, "bytes": N * 12}),
        ]
    return rows


TABLE += lm_rows("sample", ["hits"], 16) + lm_rows("lightmap", ["o", "d"], 4)
TABLE += pv_rows("psample", ["pos", "nrm"], False) + pv_rows("plight", ["o", "d"], True)


def resolve(m, v):
    if isinstance(v, tuple):
        return VP(m[v[0]].value + v[1])
    return m[v] if isinstance(v, str) else v


def shown(v):
    return ptr(v) if v is None or isinstance(v, VP) else v


def check(lib, ctxs, mem, entry, state, over, rc, text, extra=None):
    a = dict(good_args(mem)[entry])
    assert set(over) <= set(a), (entry, over)
    a.update({k: resolve(mem, v) for k, v in over.items()})
    got = call(lib, entry, ctxs[state], a)
    said = lib.ptrt_last_error(ctxs[state]).decode()
    print(f"{FN[entry]} [{state}] {over}: {got} {said if got else ''}")
    assert got == rc, (entry, state, over, said)
    if text is not None:
        f = {k: shown(v) for k, v in a.items()}
        f.update({k: (shown(a[v]) if k == "p" else v) for k, v in (extra or {}).items()})
        assert said == text.format(fn=FN[entry], **f), (entry, state, over)


def test_no_context(P, ctxs, mem):
    """NULL: PTRT_E_INVALID whatever else is wrong"""
    for entry in FN:
        check(P.lib, ctxs, mem, entry, "null", {}, INVALID, "{fn}: bad context")
        first = [k for k, v in good_args(mem)[entry].items() if isinstance(v, VP)][0]
        check(P.lib, ctxs, mem, entry, "null", {first: None}, INVALID, "{fn}: bad context")


def test_table(P, ctxs, mem):
    for entry, state, over, rc, text, extra in TABLE:
        check(P.lib, ctxs, mem, entry, state, over, rc, text, extra)


NULL_TEXT = dict(BAD, sample=BAD_LM, lightmap=BAD_LM, psample=BAD_PV, plight=BAD_PV)
SHARED_NULL = {"dir_rays": (("pos", "nrm", "s2"), BAD_DIRECT), "direct": (("pos", "nrm", "s2"), BAD_DIRECT),
               "terms": (("sh2",), BAD_BOUNCE), "bounce": (("sh2",), BAD_BOUNCE)}
OWN_NULL = {"sample": ("hits",), "lightmap": ("o", "d"), "psample": ("pos", "nrm"), "plight": ("o", "d")}   # (IN_ALIGN: the table)


def test_each_pointer_null(P, ctxs, mem):
    """a NULL pointer is PTRT_E_INVALID before the scene is looked at, and with n == 0 as well; phases alone may be NULL"""
    args = good_args(mem)
    for entry in FN:
        names = [k for k, v in args[entry].items() if isinstance(v, VP)]
        assert len(names) == dict(irr_rays=6, irradiance=6, dir_rays=8, direct=5, terms=8, bounce=6, texels=2, dilate=2, filter=3,
                                  sample=5, lightmap=6, psample=5, plight=5)[entry]
        for k in names:
            if k == "ph" or k in OWN_NULL.get(entry, ()):
                continue
            shared, text = SHARED_NULL.get(entry, ((), None))
            for state in ("empty", "full"):
                for over in ({k: None}, {k: None, "n": 0}) if "n" in args[entry] else ({k: None},):
                    check(P.lib, ctxs, mem, entry, state, over, INVALID, text if k in shared else NULL_TEXT[entry])


def test_each_pointer_in_host_memory(P, ctxs, mem):
    """pageable and pinned host memory where device memory is needed: PTRT_E_INVALID, the argument's name and ITS byte count;
    of several, the first in the order of the checks; behind every other refusal.  The optional phases: named when present
    and bad, skipped when absent"""
    lib = P.lib
    for entry, spans in SPANS.items():
        for host in ("pageable", "pinned"):
            for k, name, nbytes in spans:
                check(lib, ctxs, mem, entry, "full", {k: host}, INVALID, f"{FN[entry]}: {name} is not {nbytes} bytes of device memory on device 0")
            for first in range(len(spans)):
                _, name, nbytes = spans[first]
                # (2 KB apart: ptrt_atlas_dilate's and _filter's distance and the overlap checks come before the spans)
                over = {k: (host, 2048 * i) for i, (k, _, _) in enumerate(spans[first:])}
                check(lib, ctxs, mem, entry, "full", over, INVALID, f"{FN[entry]}: {name} is not {nbytes} bytes of device memory on device 0")
            if any(k == "ph" for k, _, _ in spans):
                after = spans[[k for k, _, _ in spans].index("ph") + 1]
                check(lib, ctxs, mem, entry, "full", {"ph": None, after[0]: host}, INVALID,
                      f"{FN[entry]}: {after[1]} is not {after[2]} bytes of device memory on device 0")
    # the byte counts follow the counts of the call
    check(lib, ctxs, mem, "irr_rays", "full", {"n": 3, "k": 2, "d": HOST}, INVALID, "ptrt_irradiance_rays: directions is not 72 bytes of device memory on device 0")
    check(lib, ctxs, mem, "irradiance", "full", {"n": 3, "k": 2, "st": HOST}, INVALID, "ptrt_query_irradiance: rng_states is not 144 bytes of device memory on device 0")
    check(lib, ctxs, mem, "dir_rays", "full", {"n": 3, "lc": 1, "t": HOST}, INVALID, "ptrt_direct_rays: tmax is not 24 bytes of device memory on device 0")
    check(lib, ctxs, mem, "terms", "full", {"n": 2, "k": 2, "lc": 1, "m": 1, "v": HOST}, INVALID, "ptrt_bounce_terms: values is not 48 bytes of device memory on device 0")
    check(lib, ctxs, mem, "texels", "full", {"aw": 2, "ah": 3, "texels": HOST}, INVALID, "ptrt_atlas_texels: texels is not 192 bytes of device memory on device 0")
    check(lib, ctxs, mem, "sample", "full", {"n": 3, "ncf": 1, "charts": HOST}, INVALID, "ptrt_atlas_sample: charts is not 24 bytes of device memory on device 0")
    check(lib, ctxs, mem, "psample", "full", {"n": 3, "out": HOST}, INVALID, "ptrt_probe_sample: out is not 96 bytes of device memory on device 0")
    # every other refusal comes first
    check(lib, ctxs, mem, "irradiance", "few", {"pos": HOST}, NOT_READY, FEW)
    check(lib, ctxs, mem, "direct", "empty", {"pos": HOST}, NOT_READY, NO_GEOMETRY)
    check(lib, ctxs, mem, "terms", "geom", {"hits": HOST}, NOT_READY, NO_MATERIALS)
    check(lib, ctxs, mem, "bounce", "few", {"pos": HOST}, NOT_READY, FEW)
    check(lib, ctxs, mem, "texels", "full", {"uv": HOST, "mesh": 2}, INVALID, "ptrt_atlas_texels: mesh 2 of 2 uploaded")
    check(lib, ctxs, mem, "lightmap", "empty", {"o": HOST}, NOT_READY, NO_GEOMETRY)
    check(lib, ctxs, mem, "plight", "empty", {"o": HOST}, NOT_READY, NO_GEOMETRY)


def test_no_lights_asked_for_gives_zeroed_rows(P, ctxs, mem):
    """light_count == 0: ptrt_query_direct and ptrt_query_bounce write rows of zero bytes in stream order, on a scene with
    lights and on one without"""
    import torch
    out = mem["_tensors"]["out"]
    for entry in ("direct", "bounce"):
        for state, over in (("full", {"lc": 0}), ("full", {"lc": 0, "lf": 2}), ("dark", {"lc": 0})):
            out.fill_(1.0)
            torch.cuda.synchronize()
            check(P.lib, ctxs, mem, entry, state, over, OK, None)
            assert P.lib.ptrt_sync(ctxs[state]) == OK
            assert not out.any(), (entry, state)
        out.fill_(1.0)
        torch.cuda.synchronize()
        check(P.lib, ctxs, mem, entry, "full", {"lc": 0, "n": 3}, OK, None)   # 3 rows of the 8
        assert P.lib.ptrt_sync(ctxs["full"]) == OK
        assert not out[:3].any() and bool((out[3:] == 1.0).all()), entry


def test_the_good_calls_still_answer(P, ctxs, mem):
    """after all the refusals the contexts are in order: the good arguments of every entry point are accepted, and the atlas
    of mesh 0 under its zero charts stays uncovered"""
    import torch
    for entry in FN:
        check(P.lib, ctxs, mem, entry, "full", {}, OK, None)
    assert P.lib.ptrt_sync(ctxs["full"]) == OK
    torch.cuda.synchronize()
    assert bool((mem["_tensors"]["texels"][:, 7] == -1).all())
