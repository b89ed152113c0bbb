"""Every ValueError of Scene's device queries (ptrt_amd/__init__.py), word for word, and which of two faults wins: query_closest,
query_occluded, query_radiance, query_probes, query_irradiance, irradiance_rays, query_direct, direct_rays, query_bounce,
bounce_terms, atlas_texels, atlas_dilate, atlas_filter, atlas_sample, query_lightmap, probe_sample, query_probe_light.  The
wrapper checks a tensor's device before its shape, so these cases need tensors on the device; what needs none is in
test_query_wrapper_refusals.py.  Written from the source of the commit before the wrapper's argument handling was folded, in
the order of its checks, and confirmed against it.  Sizes: 8 texels or rays, 3 directions, 2 shadow samples, 2 lights, a 4x4
atlas, a 2x2x2 volume.  Every refusal comes before the wrapper calls the library; four counts (2^31 rays, terms per texel) are
out of reach of a test's memory."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K, M = 8, 3, 2
ON = "this scene renders on cuda:0"


def refused(text, fn, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        fn(*args, **kw)


@pytest.fixture(scope="module")
def s(P):
    s = P.Scene(16, 16, device=0)
    mat = P.Material((0.7, 0.7, 0.7), 0.5)
    for z in (-3.0, -4.0):
        a, b, c, d = (-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)
        s.addTriangles([a + b + c, a + c + d], mat)
    for x in (0.0, 0.5):
        s.addPointLight((x, 0.0, -1.0), (1.0, 1.0, 1.0))
    s.setCamera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0)
    s.uploadToGPU()
    yield s
    s.close()


@pytest.fixture(scope="module")
def g(P):
    """method -> its good keyword arguments, tensors on the device"""
    import torch
    dev = torch.device("cuda", 0)

    def f(*shape):
        return torch.zeros(shape, dtype=torch.float32, device=dev)

    def i(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev)

    nrm = f(N, 3)
    nrm[:, 2] = 1.0
    d = f(N, 3)
    d[:, 2] = -1.0
    texel = dict(positions=f(N, 3), normals=nrm, samples2=f(K, 2) + 0.5)
    lm = dict(charts=f(2, 6), chart_first=i(2), image=f(4, 4, 4))
    vol = dict(volume=P.probes.ProbeVolume((0, 0, 0), (1, 1, 1), (2, 2, 2)), probes=f(8, 32))
    return {
        "query_radiance": dict(origins=f(N, 3), directions=d, rng_states=i(N, 6) + 1),
        "query_probes": dict(positions=f(N, 3), directions=d[:K].clone(), rng_states=i(N * K, 6) + 1),
        "query_irradiance": dict(texel, rng_states=i(N * K, 6) + 1, phases=f(N)),
        "irradiance_rays": dict(texel, phases=f(N)),
        "query_direct": dict(texel, phases=f(N)), "direct_rays": dict(texel, phases=f(N)),
        "query_bounce": dict(texel, shadow2=f(M, 2) + 0.5, phases=f(N)),
        "bounce_terms": dict(hits=i(N * K, 16), directions=f(N * K, 3), n_dirs=K, shadow2=f(M, 2) + 0.5, phases=f(N)),
        "atlas_texels": dict(mesh=0, uv=f(2, 6), width=4, height=4),
        "atlas_dilate": dict(image=f(4, 4, 4)),
        "atlas_filter": dict(texels=i(16, 8) - 1, image=f(4, 4, 4), passes=2, sigma_distance=1.0, sigma_plane=0.5),
        "atlas_sample": dict(dict(hits=i(N, 16)), **lm),
        "query_lightmap": dict(dict(origins=f(N, 3), directions=d), **lm),
        "probe_sample": dict(dict(positions=f(N, 3), normals=nrm), **vol),
        "query_probe_light": dict(dict(origins=f(N, 3), directions=d), **vol),
    }


# the (n, cols) tensor arguments of each method in the order they are checked: (argument, columns, the dtypes as the message has them)
F32, I32, STATE = "torch.float32", "torch.int32", "torch.int32|torch.uint32"
TEXEL = [("positions", 3, F32), ("normals", 3, F32), ("samples2", 2, F32)]
TENSORS = {
    "query_radiance": [("origins", 3, F32), ("directions", 3, F32), ("rng_states", 6, STATE), ("out", 8, F32)],
    "query_probes": [("positions", 3, F32), ("directions", 3, F32), ("rng_states", 6, STATE), ("out", 32, F32)],
    "query_irradiance": TEXEL + [("rng_states", 6, STATE), ("out", 8, F32)],
    "irradiance_rays": TEXEL,
    "query_direct": TEXEL + [("out", 8, F32)], "direct_rays": TEXEL,
    "query_bounce": TEXEL + [("shadow2", 2, F32), ("out", 8, F32)],
    "bounce_terms": [("hits", 16, I32), ("directions", 3, F32), ("shadow2", 2, F32)],
    "atlas_texels": [("uv", 6, F32), ("out", 8, I32)],
    "atlas_filter": [("texels", 8, I32)],
    "atlas_sample": [("hits", 16, I32), ("charts", 6, F32), ("out", 8, I32)],
    "query_lightmap": [("origins", 3, F32), ("directions", 3, F32), ("charts", 6, F32), ("out", 8, I32)],
    "probe_sample": [("positions", 3, F32), ("normals", 3, F32), ("probes", 32, F32), ("out", 8, I32)],
    "query_probe_light": [("origins", 3, F32), ("directions", 3, F32), ("probes", 32, F32), ("out", 8, I32)],
}
OUT_ROWS = {"atlas_texels": 16}


def test_each_tensor_argument(P, s, g):
    """no tensor; not on the device; shape or dtype; layout -- in that order, for every (n, cols) argument in turn"""
    import torch
    for name, tensors in TENSORS.items():
        fn = getattr(s, name)
        for at, (arg, cols, dtypes) in enumerate(tensors):
            dt = getattr(torch, dtypes.split("|")[0].split(".")[1])
            good = g[name][arg] if arg != "out" else torch.zeros((OUT_ROWS.get(name, N), cols), dtype=dt, device="cuda:0")
            n = good.shape[0]
            what = f"{name}: {arg}"
            expected = f"expected (n, {cols}) of {dtypes}"
            other = torch.float64 if dt == torch.float32 else torch.int64

            def bad(v, **more):
                return dict(dict(g[name], **{arg: v}), **more)

            refused(f"{what}: needs a torch tensor on the scene's device, got ndarray", fn, **bad(good.cpu().numpy()))
            refused(f"{what}: tensor on cpu, {ON}", fn, **bad(good.cpu()))
            refused(f"{what}: tensor on cpu, {ON}", fn, **bad(good.cpu()[:, :-1].to(other)))
            refused(f"{what}: shape ({n}, {cols - 1}) of {dt}, {expected}", fn, **bad(good[:, :-1]))
            refused(f"{what}: shape ({n}, {cols}, 1) of {dt}, {expected}", fn, **bad(good[:, :, None]))
            refused(f"{what}: shape ({n * cols},) of {dt}, {expected}", fn, **bad(good.reshape(-1)))
            refused(f"{what}: shape ({n}, {cols}) of {other}, {expected}", fn, **bad(good.to(other)))
            refused(f"{what}: shape ({n}, {cols}) of {other}, {expected}", fn, **bad(good.to(other).repeat(2, 1)[::2]))
            refused(f"{what}: tensors must be contiguous", fn, **bad(good.repeat(2, 1)[::2]))
            # of two arguments at fault the earlier one is named
            if at + 1 < len(tensors):
                later = tensors[at + 1][0]
                refused(f"{what}: tensors must be contiguous", fn, **bad(good.repeat(2, 1)[::2], **{later: None}))


def test_ray_queries(P, s, g):
    """query_closest / query_occluded: what is left behind the shape checks of test_query_wrapper_refusals.py"""
    import torch
    o, d = g["query_radiance"]["origins"], g["query_radiance"]["directions"]
    t = torch.ones(N, device="cuda:0")
    refused(f"ray query: tensor on cpu, {ON}", s.query_closest, o.cpu(), d.cpu())
    refused(f"ray query: tensor on cpu, {ON}", s.query_closest, o, d.cpu())
    refused(f"ray query: tensor on cpu, {ON}", s.query_occluded, o.cpu().repeat(2, 1)[::2], d, t)            # of one argument, the device first
    refused("ray query: tensors must be contiguous", s.query_occluded, o, d.repeat(2, 1)[::2], t.cpu())       # in the order of the arguments
    refused("ray query: tensors must be contiguous", s.query_closest, o.repeat(2, 1)[::2], d.cpu())
    refused("ray query: tensors must be contiguous", s.query_closest, o, d.repeat(2, 1)[::2])
    refused("ray query: tensors must be contiguous", s.query_occluded, o, d, t.repeat(2)[::2])
    refused("ray query: shape (8, 2), expected (n, 3)", s.query_closest, o[:, :2], d.cpu())               # the shapes first
    refused("query_occluded needs tmax", s.query_occluded, o, d, None)
    assert tuple(s.query_closest(o[:0], d[:0]).shape) == (0, 16) and tuple(s.query_occluded(o[:0], d[:0], t[:0]).shape) == (0,)
    hits = P.hit_fields(s.query_closest(o, d))
    assert tuple(s.query_occluded(o, d, t * 10).shape) == (N,)
    torch.cuda.synchronize()
    assert bool((hits["hit"] == 1).all()) and bool((hits["t"] == 3.0).all())


def test_counts(P, s, g):
    """rows that do not go together, and the `out` that does not fit them"""
    import torch
    a = g["query_radiance"]
    refused("query_radiance: 8 origins, 7 directions, 8 states", s.query_radiance, **dict(a, directions=a["directions"][:7]))
    refused("query_radiance: 8 origins, 8 directions, 5 states", s.query_radiance, **dict(a, rng_states=a["rng_states"][:5]))
    refused("query_radiance: 8 origins, 7 directions, 8 states", s.query_radiance, **dict(a, directions=a["directions"][:7], out=7))
    refused("query_radiance: out has 7 rows for 8 rays", s.query_radiance, **dict(a, out=torch.zeros((7, 8), device="cuda:0")))
    a = g["query_probes"]
    refused("query_probes: no directions", s.query_probes, **dict(a, directions=a["directions"][:0], rng_states=a["rng_states"][:0]))
    refused("query_probes: 8 probes x 3 directions need 24 states, got 23", s.query_probes, **dict(a, rng_states=a["rng_states"][:23]))
    refused("query_probes: 8 probes x 2 directions need 16 states, got 24", s.query_probes, **dict(a, directions=a["directions"][:2]))
    refused("query_probes: out has 9 rows for 8 probes", s.query_probes, **dict(a, out=torch.zeros((9, 32), device="cuda:0")))
    for name in ("query_irradiance", "irradiance_rays", "query_direct", "direct_rays", "query_bounce"):
        a, fn = g[name], getattr(s, name)
        refused(f"{name}: 8 positions, 7 normals", fn, **dict(a, normals=a["normals"][:7], samples2=a["samples2"][:0]))
        refused(f"{name}: no directions", fn, **dict(a, samples2=a["samples2"][:0], phases=a["phases"][:7]))
        refused(f"{name}: 8 positions, 7 phases", fn, **dict(a, phases=a["phases"][:7]))
        refused(f"{name}: 8 positions, 9 phases", fn, **dict(a, phases=torch.zeros(9, device="cuda:0")))
    a = g["query_irradiance"]
    refused("query_irradiance: 8 texels x 3 directions need 24 states, got 8", s.query_irradiance, **dict(a, rng_states=a["rng_states"][:8]))
    refused("query_irradiance: 8 texels x 3 directions need 24 states, got 8", s.query_irradiance,
            **dict(a, rng_states=a["rng_states"][:8], out=torch.zeros((7, 8), device="cuda:0")))
    for name in ("query_irradiance", "query_direct", "query_bounce"):
        refused(f"{name}: out has 7 rows for 8 texels", getattr(s, name), **dict(g[name], out=torch.zeros((7, 8), device="cuda:0")))
    for name in ("query_bounce", "bounce_terms"):
        a = g[name]
        refused(f"{name}: no shadow samples", getattr(s, name), **dict(a, shadow2=a["shadow2"][:0]))
    refused("query_bounce: 8 positions, 7 phases", s.query_bounce, **dict(g["query_bounce"], phases=g["query_bounce"]["phases"][:7],
                                                                          shadow2=g["query_bounce"]["shadow2"][:0]))
    a = g["bounce_terms"]
    refused("bounce_terms: 24 hits, 23 directions", s.bounce_terms, **dict(a, directions=a["directions"][:23], n_dirs=5))
    refused("bounce_terms: 24 hits are not a multiple of n_dirs = 5", s.bounce_terms, **dict(a, n_dirs=5))
    refused("bounce_terms: 24 hits are not a multiple of n_dirs = 0", s.bounce_terms, **dict(a, n_dirs=0))
    refused("bounce_terms: 24 hits are not a multiple of n_dirs = -3", s.bounce_terms, **dict(a, n_dirs=-3, phases=a["phases"][:7]))
    refused("bounce_terms: 8 texels, 7 phases", s.bounce_terms, **dict(a, phases=a["phases"][:7], shadow2=a["shadow2"][:0]))
    refused("bounce_terms: 12 texels, 8 phases", s.bounce_terms, **dict(a, n_dirs=2))
    a = g["atlas_texels"]
    for w, h in ((0, 4), (4, -1), (2 ** 14 + 1, 2 ** 14)):
        refused(f"atlas_texels: a {w} x {h} atlas (1 x 1 .. 2^28 texels)", s.atlas_texels, **dict(a, width=w, height=h, uv=a["uv"][:1]))
    refused("atlas_texels: uv has 1 rows, mesh 0 has 2 faces", s.atlas_texels, **dict(a, uv=a["uv"][:1], clear=False))
    refused("atlas_texels: clear=False needs the atlas of an earlier call as `out`", s.atlas_texels, **dict(a, clear=False))
    refused("atlas_texels: out has 15 rows for 4 x 4 texels", s.atlas_texels, **dict(a, out=torch.zeros((15, 8), dtype=torch.int32, device="cuda:0")))
    refused("atlas_texels: out has 16 rows for 3 x 5 texels", s.atlas_texels,
            **dict(a, width=3, height=5, out=torch.zeros((16, 8), dtype=torch.int32, device="cuda:0")))
    a = g["atlas_filter"]
    refused("atlas_filter: texels has 15 rows for 4 x 4 texels", s.atlas_filter, **dict(a, texels=a["texels"][:15]))
    for name in ("atlas_sample", "query_lightmap"):
        a, fn = g[name], getattr(s, name)
        refused(f"{name}: charts has no rows", fn, **dict(a, charts=a["charts"][:0], chart_first=None))
        refused(f"{name}: out has 7 rows for 8", fn, **dict(a, out=torch.zeros((7, 8), dtype=torch.int32, device="cuda:0")))
    a = g["query_lightmap"]
    refused("query_lightmap: 8 origins, 7 directions", s.query_lightmap, **dict(a, directions=a["directions"][:7], charts=None))
    for name, rows in (("probe_sample", "8 positions, 7 normals"), ("query_probe_light", "8 origins, 7 directions")):
        a, fn = g[name], getattr(s, name)
        second = "normals" if name == "probe_sample" else "directions"
        refused(f"{name}: {rows}", fn, **dict(a, **{second: a[second][:7], "probes": None}))
        refused(f"{name}: probes has 7 rows for a volume of 8 probes", fn, **dict(a, probes=a["probes"][:7], out=7))
        refused(f"{name}: probes has 8 rows for a volume of 4 probes", fn, **dict(a, volume=P.probes.ProbeVolume((0, 0, 0), (1, 1, 1), (2, 2, 1))))
        refused(f"{name}: out has 9 rows for 8", fn, **dict(a, out=torch.zeros((9, 8), dtype=torch.int32, device="cuda:0")))


def test_phases_chart_first_and_images(P, s, g):
    """the arguments that are not (n, cols): phases (n,), chart_first (M,), image (H, W, 4)"""
    import torch
    for name in ("query_irradiance", "irradiance_rays", "query_direct", "direct_rays", "query_bounce", "bounce_terms"):
        a, fn = g[name], getattr(s, name)
        ph, what = a["phases"], f"{name}: phases"
        for bad in (np.zeros(N, np.float32), ph[:, None], [0.0] * N):
            refused(f"{what}: needs a torch tensor of shape (n,) on the scene's device", fn, **dict(a, phases=bad))
        refused(f"{what}: tensor on cpu, {ON}", fn, **dict(a, phases=ph.cpu()[:7].double()))
        refused(f"{what}: shape (8, 1) of torch.float64, expected (n, 1) of torch.float32", fn, **dict(a, phases=ph.double()))
        refused(f"{what}: shape (7, 1) of torch.float64, expected (n, 1) of torch.float32", fn, **dict(a, phases=ph.double()[:7]))
        refused(f"{what}: tensors must be contiguous", fn, **dict(a, phases=ph.repeat(2)[::2]))
        refused(f"{what}: tensors must be contiguous", fn, **dict(a, phases=ph.repeat(2)[:14:2]))
        assert fn(**dict(a, phases=None)) is not None
    for name in ("atlas_sample", "query_lightmap"):
        a, fn = g[name], getattr(s, name)
        cf, what = a["chart_first"], f"{name}: chart_first"
        for bad in (np.zeros(2, np.int32), cf[:, None], [0, 0]):
            refused(f"{what}: needs an (M,) int32 tensor on the scene's device, one entry per uploaded mesh", fn, **dict(a, chart_first=bad, image=None))
        refused(f"{what}: tensor on cpu, {ON}", fn, **dict(a, chart_first=cf.cpu().long()))
        refused(f"{what}: shape (2, 1) of torch.int64, expected (n, 1) of torch.int32", fn, **dict(a, chart_first=cf.long(), image=None))
        refused(f"{what}: shape (2, 1) of torch.int64, expected (n, 1) of torch.int32", fn, **dict(a, chart_first=cf.long().repeat(2)[::2]))
        refused(f"{what}: tensors must be contiguous", fn, **dict(a, chart_first=cf.repeat(2)[::2], image=None))
    for name in ("atlas_dilate", "atlas_filter", "atlas_sample", "query_lightmap"):
        a, fn = g[name], getattr(s, name)
        img, what = a["image"], f"{name}: image"
        for bad in (img.cpu().numpy(), img.view(16, 4), img[None], None):
            refused(f"{what}: needs a torch tensor of shape (H, W, 4) on the scene's device", fn, **dict(a, image=bad))
        refused(f"{name}: a 4 x 0 atlas (1 x 1 .. 2^28 texels)", fn, **dict(a, image=img[:0]))
        refused(f"{name}: a 0 x 4 atlas (1 x 1 .. 2^28 texels)", fn, **dict(a, image=img[:, :0].cpu()))
        refused(f"{name}: a 16384 x 16385 atlas (1 x 1 .. 2^28 texels)", fn, **dict(a, image=img[:1, :1, :1].expand(16385, 16384, 4)))
        refused(f"{what}: tensors must be contiguous", fn, **dict(a, image=img.repeat(1, 1, 2)[:, :, ::2]))
        refused(f"{what}: tensors must be contiguous", fn, **dict(a, image=torch.zeros(4, 4, 8)[:, :, ::2]))   # before the device
        refused(f"{what}: tensor on cpu, {ON}", fn, **dict(a, image=torch.zeros(4, 4, 3)))
        refused(f"{what}: shape (16, 3) of torch.float32, expected (n, 4) of torch.float32", fn, **dict(a, image=img[:, :, :3].contiguous()))
        refused(f"{what}: shape (16, 4) of torch.float64, expected (n, 4) of torch.float32", fn, **dict(a, image=img.double()))
    # behind the image: the passes of atlas_dilate, the texels of atlas_filter, the row count and `out` of the two samplers
    a = g["atlas_dilate"]
    for passes in (0, 65, -1):
        refused(f"atlas_dilate: {passes} passes (1 .. 64)", s.atlas_dilate, a["image"], passes)
    refused(f"atlas_dilate: image: tensor on cpu, {ON}", s.atlas_dilate, a["image"].cpu(), 0)
    a = g["atlas_filter"]
    refused("atlas_filter: 0 passes (1 .. 8)", s.atlas_filter, **dict(a, passes=0, normal_power=8, image=a["image"].cpu()))   # before the device
    refused("atlas_filter: 9 passes (1 .. 8)", s.atlas_filter, **dict(a, passes=9))
    refused("atlas_filter: normal_power 8 (0 .. 7)", s.atlas_filter, **dict(a, normal_power=8, sigma_distance=0.0))
    refused("atlas_filter: normal_power -1 (0 .. 7)", s.atlas_filter, **dict(a, normal_power=-1))
    refused("atlas_filter: sigma_distance 0.0 (positive and finite)", s.atlas_filter, **dict(a, sigma_distance=0.0, sigma_plane=0.0))
    refused("atlas_filter: sigma_plane nan (positive and finite)", s.atlas_filter, **dict(a, sigma_plane=float("nan"), image=a["image"].cpu()))
    refused("atlas_filter: sigma_plane inf (positive and finite)", s.atlas_filter, **dict(a, sigma_plane=float("inf"), texels=None))
    refused(f"atlas_filter: image: tensor on cpu, {ON}", s.atlas_filter, **dict(a, image=a["image"].cpu(), texels=None))          # before texels
    for name in ("atlas_sample", "query_lightmap"):
        a, fn = g[name], getattr(s, name)
        refused(f"{name}: image: shape (16, 3) of torch.float32, expected (n, 4) of torch.float32", fn,
                **dict(a, image=a["image"][:, :, :3].contiguous(), out=7))
        refused(f"{name}: mode 'linear' ('nearest' or 'bilinear')", fn, **dict(a, mode="linear", charts=None))                 # before any tensor


def test_no_rows_and_the_good_calls(P, s, g):
    """n == 0 answers with an empty tensor (the caller's `out` when given); the good arguments of every method are accepted"""
    import torch
    z3 = torch.zeros((0, 3), device="cuda:0")
    out = torch.zeros((0, 8), device="cuda:0")
    assert s.query_radiance(z3, z3, torch.zeros((0, 6), dtype=torch.int32, device="cuda:0"), out=out) is out
    a = g["query_probes"]
    assert tuple(s.query_probes(z3, a["directions"], a["rng_states"][:0]).shape) == (0, 32)
    a = g["query_irradiance"]
    assert s.query_irradiance(z3, z3, a["samples2"], a["rng_states"][:0], out=out) is out
    assert [tuple(t.shape) for t in s.irradiance_rays(z3, z3, a["samples2"])] == [(0, 3), (0, 3)]
    assert s.query_direct(z3, z3, a["samples2"], out=out) is out
    assert [tuple(t.shape) for t in s.direct_rays(z3, z3, a["samples2"])] == [(0, 3), (0, 3), (0,), (0, 3)]
    assert [tuple(t.shape) for t in s.direct_rays(a["positions"], a["normals"], a["samples2"], lights=(1, 0))] == [(0, 3), (0, 3), (0,), (0, 3)]
    assert s.query_bounce(z3, z3, a["samples2"], out=out) is out
    b = g["bounce_terms"]
    assert [tuple(t.shape) for t in s.bounce_terms(b["hits"][:0], z3, K)] == [(0, 3), (0, 3), (0,), (0, 3)]
    assert [tuple(t.shape) for t in s.bounce_terms(b["hits"], b["directions"], K, lights=(0, 0))] == [(0, 3), (0, 3), (0,), (0, 3)]
    iout = torch.zeros((0, 8), dtype=torch.int32, device="cuda:0")
    a = g["atlas_sample"]
    assert s.atlas_sample(a["hits"][:0], a["charts"], a["chart_first"], a["image"], out=iout) is iout
    assert tuple(s.query_lightmap(z3, z3, a["charts"], a["chart_first"], a["image"]).shape) == (0, 8)
    a = g["probe_sample"]
    assert s.probe_sample(z3, z3, a["volume"], a["probes"], out=iout) is iout
    assert tuple(s.query_probe_light(z3, z3, a["volume"], a["probes"]).shape) == (0, 8)
    shapes = {"query_radiance": (N, 8), "query_probes": (N, 32), "query_irradiance": (N, 8), "irradiance_rays": [(N * K, 3)] * 2,
              "query_direct": (N, 8), "direct_rays": [(N * 2 * K, 3), (N * 2 * K, 3), (N * 2 * K,), (N * 2 * K, 3)], "query_bounce": (N, 8),
              "bounce_terms": [(N * K * 2 * M, 3), (N * K * 2 * M, 3), (N * K * 2 * M,), (N * K * 2 * M, 3)], "atlas_texels": (16, 8),
              "atlas_dilate": (4, 4, 4), "atlas_filter": (4, 4, 4), "atlas_sample": (N, 8), "query_lightmap": (N, 8),
              "probe_sample": (N, 8), "query_probe_light": (N, 8)}
    for name, a in g.items():
        got = getattr(s, name)(**a)
        assert ([tuple(t.shape) for t in got] if isinstance(got, tuple) else tuple(got.shape)) == shapes[name], name
    torch.cuda.synchronize()
