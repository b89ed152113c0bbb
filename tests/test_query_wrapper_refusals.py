"""What Scene's device queries (ptrt_amd/__init__.py) refuse before they need a device, word for word, on a HOST_ONLY scene:
an argument that is no tensor, a tensor on the wrong device, a bad `mode`, `volume`, `normal_bias` or `lights`, what the ray
queries and the atlas image checks say ahead of their device check, and the PtrtError of a scene without a back end.  The
wrapper checks the device before the shapes, so the rest needs device tensors: test_query_wrapper_refusals_gpu.py.  Written
from the source of the commit before the wrapper's argument handling was folded, in the order of its checks.

And the nine `*_fields` functions: key set, shapes, dtypes, and that every value is a view of the input."""
import re
import types

import numpy as np
import pytest
import torch

F, I = np.float32, np.int32
HOST = "no device (host-only)"
NO_BACK_END = "host-only Scene (device < 0) has no GPU back end"


def refused(text, fn, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        fn(*args, **kw)


@pytest.fixture(scope="module")
def s(P):
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    mat = P.Material((0.7, 0.7, 0.7), 0.5)
    for z in (-3.0, -4.0):
        a, b, c, d = (-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)
        s.addTriangles([a + b + c, a + c + d], mat)
    for x in (0.0, 0.5):
        s.addPointLight((x, 0.0, -1.0), (1.0, 1.0, 1.0))
    assert s.lightCount() == 2
    yield s
    s.close()


def good(P):
    """method -> (positional arguments on the CPU, the name of the first tensor argument)"""
    f3, f2 = torch.zeros(8, 3), torch.zeros(3, 2)
    st, hits = torch.zeros((24, 6), dtype=torch.int32), torch.zeros((24, 16), dtype=torch.int32)
    vol = P.probes.ProbeVolume((0, 0, 0), (1, 1, 1), (2, 2, 2))
    lm = (torch.zeros(2, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 4, 4))
    return {
        "query_radiance": ((f3, f3, st[:8]), "origins"), "query_probes": ((f3, f3[:3], st), "positions"),
        "query_irradiance": ((f3, f3, f2, st), "positions"), "irradiance_rays": ((f3, f3, f2), "positions"),
        "query_direct": ((f3, f3, f2), "positions"), "direct_rays": ((f3, f3, f2), "positions"),
        "query_bounce": ((f3, f3, f2, f2), "positions"), "bounce_terms": ((hits, torch.zeros(24, 3), 3, f2), "hits"),
        "atlas_texels": ((0, torch.zeros(2, 6), 4, 4), "uv"),
        "atlas_sample": ((hits[:8],) + lm, "hits"), "query_lightmap": ((f3, f3) + lm, "origins"),
        "probe_sample": ((f3, f3, vol, torch.zeros(8, 32)), "positions"), "query_probe_light": ((f3, f3, vol, torch.zeros(8, 32)), "origins"),
    }


def test_first_tensor_argument(P, s):
    """no tensor, then a tensor that is not on the scene's device: the first tensor argument of every method"""
    for name, (args, first) in good(P).items():
        at = [i for i, a in enumerate(args) if torch.is_tensor(a)][0]
        bad = args[:at] + (np.zeros(tuple(args[at].shape), F),) + args[at + 1:]
        refused(f"{name}: {first}: needs a torch tensor on the scene's device, got ndarray", getattr(s, name), *bad)
        bad = args[:at] + ([[0.0] * 3],) + args[at + 1:]
        refused(f"{name}: {first}: needs a torch tensor on the scene's device, got list", getattr(s, name), *bad)
        refused(f"{name}: {first}: tensor on cpu, this scene renders on {HOST}", getattr(s, name), *args)
        # the device before the shape
        bad = args[:at] + (torch.zeros(5, 7, 2, dtype=torch.float64),) + args[at + 1:]
        refused(f"{name}: {first}: tensor on cpu, this scene renders on {HOST}", getattr(s, name), *bad)


def test_ray_queries(P, s):
    """query_closest / query_occluded check shapes and types before the device, on arrays and tensors alike"""
    o, d, t = np.zeros((8, 3), F), np.zeros((8, 3), F), np.ones(8, F)
    to, tt = torch.zeros(8, 3), torch.ones(8)
    refused("query_occluded needs tmax", s.query_occluded, o, d, None)
    refused("ray query: pass all torch tensors or all numpy arrays", s.query_closest, to, d)
    refused("ray query: pass all torch tensors or all numpy arrays", s.query_occluded, o, d, tt)
    refused("ray query: pass all torch tensors or all numpy arrays", s.query_closest, to, [[0.0] * 3] * 8)
    refused("ray query: expected a numpy array or a torch tensor, got list", s.query_closest, [[0.0] * 3] * 8, d)
    refused("ray query: expected a numpy array or a torch tensor, got list", s.query_occluded, o, d, [1.0] * 8)
    refused("ray query: shape (8, 2), expected (n, 3)", s.query_closest, o[:, :2], d)
    refused("ray query: shape (8, 2), expected (n, 3)", s.query_closest, to, to[:, :2])
    refused("ray query: shape (24,), expected (n, 3)", s.query_closest, o.reshape(-1), d)
    refused("ray query: shape (2, 4, 3), expected (n, 3)", s.query_closest, o.reshape(2, 4, 3), d)
    refused("ray query: tmax shape (8, 1), expected (n,)", s.query_occluded, o, d, t[:, None])
    refused("ray query: tmax shape (8, 1), expected (n,)", s.query_occluded, to, to, tt[:, None])
    refused("ray query: 8 origins but 7 rows in another input", s.query_closest, o, d[:7])
    refused("ray query: 8 origins but 7 rows in another input", s.query_occluded, to, to, tt[:7])
    refused("ray query: dtype float64, expected float32", s.query_closest, o.astype(np.float64), d)
    refused("ray query: dtype torch.float64, expected float32", s.query_closest, to, to.double())
    refused("ray query: dtype int32, expected float32", s.query_occluded, o, d, t.astype(I))
    # the first argument at fault, and of one argument shape, then rows, then dtype
    refused("ray query: shape (8, 2), expected (n, 3)", s.query_closest, o[:, :2].astype(np.float64), d[:7])
    refused("ray query: 8 origins but 7 rows in another input", s.query_closest, o, d[:7].astype(np.float64))
    refused("ray query: dtype float64, expected float32", s.query_occluded, o.astype(np.float64), d, t[:, None])
    # tensors: the device, then contiguity, both behind the shapes
    refused(f"ray query: tensor on cpu, this scene renders on {HOST}", s.query_closest, to, to)
    refused(f"ray query: tensor on cpu, this scene renders on {HOST}", s.query_occluded, to, torch.zeros(16, 3)[::2], tt)
    refused("ray query: shape (8, 2), expected (n, 3)", s.query_closest, torch.zeros(8, 4)[:, :2], to)
    # arrays: nothing left to refuse but the scene itself
    for call in (lambda: s.query_closest(o, d), lambda: s.query_occluded(o, d, t), lambda: s.query_closest(o[:0], d[:0]),
                 lambda: s.camera_rays(0), lambda: s.init_rng_states(1, 0, 4), lambda: s.init_rng_states(1, 0, 0)):
        with pytest.raises(P.PtrtError, match="^" + re.escape(NO_BACK_END) + "$"):
            call()


def test_modes_volumes_and_lights(P, s):
    """what is checked before the first tensor"""
    g = good(P)
    for name in ("atlas_sample", "query_lightmap"):
        args = g[name][0]
        refused(f"{name}: mode 'cubic' ('nearest' or 'bilinear')", getattr(s, name), *args, mode="cubic")
        refused(f"{name}: mode 1 ('nearest' or 'bilinear')", getattr(s, name), None, *args[1:], mode=1)     # before the tensors
    try:
        None.origin
    except AttributeError as e:
        no_origin = str(e)
    try:
        float("x")
    except ValueError as e:
        no_float = str(e)
    ns = types.SimpleNamespace
    for name in ("probe_sample", "query_probe_light"):
        a, b, vol, probes = g[name][0]
        fn = getattr(s, name)
        refused(f"{name}: mode 'nearest' ('trilinear' or 'visibility')", fn, a, b, vol, probes, mode="nearest")
        refused(f"{name}: mode None ('trilinear' or 'visibility')", fn, a, b, None, probes, mode=None, normal_bias=-1.0)
        refused(f"{name}: volume: needs a probes.ProbeVolume (origin, spacing, counts): {no_origin}", fn, a, b, None, probes, normal_bias=-1.0)
        refused(f"{name}: volume: needs a probes.ProbeVolume (origin, spacing, counts): {no_float}", fn, a, b,
                ns(origin=("x", 0, 0), spacing=(1, 1, 1), counts=(2, 2, 2)), probes)
        for counts in ((2, 0, 2), (-1, 2, 2), (4097, 4096, 1)):
            refused(f"{name}: volume: counts {list(counts)} (each >= 1, at most 2^24 probes)", fn, a, b,
                    ns(origin=(0, 0, 0), spacing=(0, 1, 1), counts=counts), probes)                        # the counts before the spacing
        refused(f"{name}: volume: spacing [0.0, 1.0, 1.0] (positive and finite), origin [0.0, 0.0, 0.0] (finite)", fn, a, b,
                ns(origin=(0, 0, 0), spacing=(0, 1, 1), counts=(2, 2, 2)), probes, normal_bias=-1.0)
        refused(f"{name}: volume: spacing [1.0, inf, 1.0] (positive and finite), origin [0.0, 0.0, 0.0] (finite)", fn, a, b,
                ns(origin=(0, 0, 0), spacing=(1, float("inf"), 1), counts=(2, 2, 2)), probes)
        refused(f"{name}: volume: spacing [1.0, 1.0, 1.0] (positive and finite), origin [0.0, nan, 0.0] (finite)", fn, a, b,
                ns(origin=(0, float("nan"), 0), spacing=(1, 1, 1), counts=(2, 2, 2)), probes)
        for bias in (-1.0, float("inf"), float("nan")):
            refused(f"{name}: normal_bias {bias} (>= 0 and finite)", fn, None, b, vol, probes, normal_bias=bias)  # before the tensors
    for name in ("query_direct", "direct_rays", "query_bounce", "bounce_terms"):
        args = g[name][0]
        fn = getattr(s, name)
        for bad in (3, (0,), 2.5):
            refused(f"{name}: lights={bad!r}, expected None or (first, count)", fn, *args, lights=bad)
        for bad in ((-1, 1), (0, 3), (1, 2), (0, -1), (3, 0)):
            refused(f"{name}: lights ({bad[0]}, {bad[1]}) of the scene's 2", fn, *args, lights=bad)
        refused(f"{name}: lights (0, 3) of the scene's 2", fn, None, *args[1:], lights=(0, 3))                 # before the tensors
        refused(f"{name}: {g[name][1]}: tensor on cpu, this scene renders on {HOST}", fn, *args, lights=(1, 1))


def test_atlas_images(P, s):
    """atlas_dilate and atlas_filter look at the image's shape, size and layout before its device, and atlas_filter at its
    numbers in between"""
    img, tex = torch.zeros(4, 4, 4), torch.zeros((16, 8), dtype=torch.int32)
    cases = {"atlas_dilate": lambda im, **kw: s.atlas_dilate(im, **kw),
             "atlas_filter": lambda im, **kw: s.atlas_filter(tex, im, **dict(dict(passes=2, sigma_distance=1.0, sigma_plane=0.5), **kw))}
    for name, fn in cases.items():
        for bad in (np.zeros((4, 4, 4), F), torch.zeros(16, 4), torch.zeros(1, 4, 4, 4), None):
            refused(f"{name}: image: needs a torch tensor of shape (H, W, 4) on the scene's device", fn, bad)
        refused(f"{name}: a 4 x 0 atlas (1 x 1 .. 2^28 texels)", fn, torch.zeros(0, 4, 4))
        refused(f"{name}: a 0 x 4 atlas (1 x 1 .. 2^28 texels)", fn, torch.zeros(4, 0, 4))
        refused(f"{name}: a 16385 x 16384 atlas (1 x 1 .. 2^28 texels)", fn, torch.zeros(1, 1, 1).expand(16384, 16385, 4))
        refused(f"{name}: image: tensors must be contiguous", fn, torch.zeros(4, 4, 8)[:, :, ::2])
        refused(f"{name}: image: tensors must be contiguous", fn, torch.zeros(4, 4, 8)[:, :, ::2], passes=0)
        refused(f"{name}: image: tensor on cpu, this scene renders on {HOST}", fn, img)
        refused(f"{name}: image: tensor on cpu, this scene renders on {HOST}", fn, torch.zeros(4, 4, 3, dtype=torch.float64))
    # atlas_dilate: the image's device before the passes; atlas_filter: its numbers before the image's device
    refused(f"atlas_dilate: image: tensor on cpu, this scene renders on {HOST}", s.atlas_dilate, img, 0)
    fn = cases["atlas_filter"]
    refused("atlas_filter: 0 passes (1 .. 8)", fn, img, passes=0, normal_power=9)
    refused("atlas_filter: 9 passes (1 .. 8)", fn, img, passes=9)
    refused("atlas_filter: normal_power -1 (0 .. 7)", fn, img, normal_power=-1, sigma_distance=0.0)
    refused("atlas_filter: normal_power 8 (0 .. 7)", fn, img, normal_power=8)
    refused("atlas_filter: sigma_distance 0.0 (positive and finite)", fn, img, sigma_distance=0, sigma_plane=0)
    refused("atlas_filter: sigma_distance inf (positive and finite)", fn, img, sigma_distance=float("inf"))
    refused("atlas_filter: sigma_plane -1.0 (positive and finite)", fn, img, sigma_plane=-1)
    refused("atlas_filter: sigma_plane nan (positive and finite)", fn, img, sigma_plane=float("nan"))
    refused(f"atlas_filter: image: tensor on cpu, this scene renders on {HOST}", s.atlas_filter, None, img, 2, 1.0, 0.5)  # before texels


# ---- the *_fields functions ---------------------------------------------------------------------------------------------
# (function, its table, the rows' dtype, the columns reinterpreted as the other 4-byte type, the kinds of input it takes)
def fields_table(P):
    both = ("tensor", "numpy")
    return [
        (P.hit_fields, P.HIT_COLUMNS, "int32", {"t", "point", "normal", "u", "v", "local_point"}, ("tensor",)),
        (P.radiance_fields, P.RADIANCE_COLUMNS, "float32", {"object_id"}, ("tensor",)),
        (P.probe_fields, P.PROBE_COLUMNS, "float32", set(), both),
        (P.irradiance_fields, P.IRRADIANCE_COLUMNS, "float32", set(), both),
        (P.direct_fields, P.DIRECT_COLUMNS, "float32", set(), both),
        (P.bounce_fields, P.BOUNCE_COLUMNS, "float32", set(), both),
        (P.atlas_fields, P.ATLAS_COLUMNS, "int32", {"position", "normal"}, both),
        (P.lightmap_sample_fields, P.LIGHTMAP_SAMPLE_COLUMNS, "int32", {"rgb", "weight", "x", "y"}, both),
        (P.probes.probe_light_fields, P.probes.PROBE_LIGHT_COLUMNS, "int32", {"irradiance", "weight"}, both),
    ]


def test_fields_are_named_views(P):
    n = 5
    other = {"int32": "float32", "float32": "int32"}
    for fn, columns, base, swapped, kinds in fields_table(P):
        width = max(c[1] for c in columns.values())
        assert sorted(c[:2] for c in columns.values())[0][0] == 0 and sum(c[1] - c[0] for c in columns.values()) == width
        assert swapped <= set(columns)
        for kind in kinds:
            rec = np.arange(n * width).astype(base).reshape(n, width)
            before = rec.copy()
            if kind == "tensor":
                rec = torch.from_numpy(rec)
            out = fn(rec)
            assert list(out) == list(columns), fn.__name__
            for i, (name, (a, b, *_)) in enumerate(columns.items()):
                v = out[name]
                want = other[base] if name in swapped else base
                shape = (n, 9, 3) if (fn is P.probe_fields and name == "sh") else (n,) if b - a == 1 else (n, b - a)
                assert tuple(v.shape) == shape, (fn.__name__, kind, name)
                assert str(v.dtype).replace("torch.", "") == want, (fn.__name__, kind, name)
                assert isinstance(v, np.ndarray) == (kind == "numpy")
                # the values are the input's own bits ...
                bits = np.asarray(v).view(base).reshape(n, b - a)
                assert (bits == before[:, a:b]).all(), (fn.__name__, kind, name)
                # ... and a view of it: writing through changes the input, in these columns and no others
                v[...] = 100 + i
                now = np.asarray(rec)
                assert (now[:, a:b].view(want) == 100 + i).all(), (fn.__name__, kind, name)
                mask = np.ones(width, bool)
                mask[a:b] = False
                assert (now[:, mask] == before[:, mask]).all(), (fn.__name__, kind, name)
                before = now.copy()
