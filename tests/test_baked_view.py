"""The baked-light view without a device (ptrt_render_baked; Scene.render_baked; tests/baked_view_restatement.py): the symbol is
declared and exported, the record's layout is the header's, the restatement takes every branch of the source rule on synthetic
rows -- a NaN weight and a zero weight among them --, and the wrapper names a wrong shape or dtype on a scene without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import baked_view_restatement as R

F = np.float32
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported(P):
    header = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    assert re.search(r"int ptrt_render_baked\(ptrt_ctx \*ctx, int frame_index, const ptrt_baked_view \*view, void \*out_rgb8, "
                     r"int out_is_device\);", header)
    assert "typedef struct ptrt_baked_view {" in header and "} ptrt_baked_view;" in header
    assert hasattr(P.lib, "ptrt_render_baked") and hasattr(P.lib, "hs_render_baked")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    assert hasattr(P.Scene, "render_baked") and hasattr(P.baked, "baked_view")
    V = P.baked.BakedView
    # the header's layout on a 64-bit target: pointers on 8, the 36-byte volume behind three ints
    assert C.sizeof(V) == 128
    assert [getattr(V, n).offset for n in ("d_charts", "n_chart_faces", "d_chart_first", "d_image", "atlas_w", "atlas_h", "lightmap_mode",
                                           "volume", "d_probes", "probe_mode", "normal_bias", "d_hdr", "d_normal", "d_depth",
                                           "d_object_id")] == [0, 8, 16, 24, 32, 36, 40, 44, 80, 88, 92, 96, 104, 112, 120]


def test_refusals_that_need_no_device(P):
    view = P.baked.BakedView()
    out = np.full(64, 7, np.uint8)
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_render_baked(ctx, 0, C.byref(view), out.ctypes.data_as(C.c_void_p), 0) == -1
        assert b"ptrt_render_baked" in P.lib.ptrt_last_error(stale)
    assert (out == 7).all()


def closest_rows(mesh, t=2.0):
    """query_closest's (n, 16) int32 rows for hits on `mesh` (negative: a miss, the defaults)"""
    mesh = np.asarray(mesh, np.int32)
    h = np.zeros((len(mesh), 16), np.int32)
    hit = mesh >= 0
    h[:, 0] = hit
    h[:, 1] = np.where(hit, F(t), F(1e30)).astype(F).view(np.int32)
    h[hit, 5:8] = F([0.0, 0.6, 0.8]).view(np.int32)
    h[:, 8] = np.where(hit, mesh, -1)
    h[:, 9] = 1
    h[:, 12] = np.where(hit, 3, -1)
    return h


def light_rows(rgb, weight):
    """(n, 8) int32 rows of either sampler: the colour (0:3) and the weight (3) are all the view reads"""
    r = np.zeros((len(weight), 8), np.int32)
    r[:, 0:3] = np.asarray(rgb, F).view(np.int32)
    r[:, 3] = np.asarray(weight, F).view(np.int32)
    return r


def test_the_restatement_takes_every_branch():
    albedo = F([[0.5, 0.25, 1.0], [0.8, 0.8, 0.8]])
    emission = F([[0.0, 0.0, 0.0], [2.0, 0.5, 0.25]])
    #            miss  map   map   probe  probe  probe  unlit  unlit  unlit  map(emissive)
    mesh = [-1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    lm_w = [0.0, 1.0, 0.3, 0.0, NAN, -1.0, 0.0, NAN, 0.0, 2.5]
    pl_w = [0.0, 1.0, 0.0, 0.7, 2.0, 1.0, 0.0, NAN, -0.0, 1.0]
    n = len(mesh)
    lm_rgb = np.tile(F([[1.0, 2.0, 3.0]]), (n, 1))
    pl_rgb = np.tile(F([[10.0, 20.0, 30.0]]), (n, 1))
    lm_rgb[[3, 4, 6, 7]] = NAN   # what an unused sample holds reaches nothing
    pl_rgb[[6, 7, 8]] = INF
    h = closest_rows(mesh)
    sky = np.tile(F([[0.1, 0.2, 0.3]]), (n, 1))
    lm, pl = light_rows(lm_rgb, lm_w), light_rows(pl_rgb, pl_w)
    out = R.shade(h, sky, albedo, emission, lm, pl)
    S = R
    assert out["source"].tolist() == [S.SKY, S.LIGHTMAP, S.LIGHTMAP, S.PROBES, S.PROBES, S.PROBES, S.UNLIT, S.UNLIT, S.UNLIT, S.LIGHTMAP]
    pi = F(3.14159265)
    by_map = (albedo[0] * F([1.0, 2.0, 3.0])) / pi
    by_probe = (albedo[0] * F([10.0, 20.0, 30.0])) / pi
    want = np.stack([sky[0], by_map, by_map, by_probe, by_probe, by_probe, F([0, 0, 0]), F([0, 0, 0]), F([0, 0, 0]),
                     (albedo[1] * F([1.0, 2.0, 3.0])) / pi + emission[1]]).astype(F)
    assert np.array_equal(out["hdr"].view(np.int32), want.view(np.int32))
    assert np.isfinite(out["hdr"]).all(), "a NaN of an unused sample came through"
    assert not np.signbit(out["hdr"][6:9]).any(), "an unlit hit is +0"
    # one half absent, and both
    assert R.source(h, lm, None).tolist() == [S.SKY, S.LIGHTMAP, S.LIGHTMAP, S.UNLIT, S.UNLIT, S.UNLIT, S.UNLIT, S.UNLIT, S.UNLIT, S.LIGHTMAP]
    assert R.source(h, None, pl).tolist() == [S.SKY, S.PROBES, S.UNLIT, S.PROBES, S.PROBES, S.PROBES, S.UNLIT, S.UNLIT, S.UNLIT, S.PROBES]
    bare = R.shade(h, sky, albedo, emission)
    assert bare["source"].tolist() == [S.SKY] + [S.UNLIT] * 9
    assert np.array_equal(bare["hdr"][1:9], np.zeros((8, 3), F)) and np.array_equal(bare["hdr"][9], emission[1])
    # what a frame keeps of a first hit
    assert out["object_id"].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert out["depth"][0] == F(1e30) and (out["depth"][1:] == F(2.0)).all()
    assert not out["normal"][0].any() and np.array_equal(out["normal"][1], F([0.0, 0.6, 0.8]))


def test_the_restatement_uses_float32_pi():
    import math
    assert R.PI_F == F(math.pi), "lightmap.shade_samples divides by float32(pi): the same number"


def test_the_wrapper_names_what_is_wrong(P):
    import torch
    s = P.Scene(16, 8, device=P.HOST_ONLY)
    n = 16 * 8
    vol = P.probes.ProbeVolume((0, 0, 0), (1, 1, 1), (2, 1, 1))
    lightmap = dict(charts=torch.zeros((4, 6)), chart_first=torch.zeros(3, dtype=torch.int32), image=torch.zeros((5, 7, 4)))
    probes = dict(volume=vol, probes=torch.zeros((2, 32)))
    good = dict(lightmap, **probes)
    cases = [
        (dict(charts=torch.zeros((4, 5))), "charts: shape"), (dict(charts=torch.zeros((4, 6), dtype=torch.float64)), "charts: dtype"),
        (dict(charts=np.zeros((4, 6), F)), "charts: needs a torch tensor"), (dict(charts=torch.zeros((0, 6))), "charts has no rows"),
        (dict(charts=torch.zeros((4, 12))[:, ::2]), "charts: tensors must be contiguous"),
        (dict(chart_first=torch.zeros((3, 1), dtype=torch.int32)), "chart_first: shape"),
        (dict(chart_first=torch.zeros(3, dtype=torch.int64)), "chart_first: dtype"),
        (dict(image=torch.zeros((5, 7, 3))), "image: shape"), (dict(image=torch.zeros((35, 4))), "image: shape"),
        (dict(image=torch.zeros((5, 7, 4), dtype=torch.float16)), "image: dtype"), (dict(image=torch.zeros((0, 7, 4))), "atlas"),
        (dict(charts=None), "together"), (dict(image=None), "together"), (dict(volume=None), "together"), (dict(probes=None), "together"),
        (dict(lightmap_mode="cubic"), "lightmap_mode"), (dict(lightmap_mode=1), "lightmap_mode"), (dict(probe_mode="nearest"), "probe_mode"),
        (dict(probes=torch.zeros((3, 32))), "probes: shape"), (dict(probes=torch.zeros((2, 31))), "probes: shape"),
        (dict(probes=torch.zeros((2, 32), dtype=torch.int32)), "probes: dtype"), (dict(volume=(0, 0, 0)), "volume"),
        (dict(normal_bias=-0.1), "normal_bias"), (dict(normal_bias=NAN), "normal_bias"), (dict(normal_bias=INF), "normal_bias"),
        (dict(hdr=torch.zeros((n, 4))), "hdr: shape"), (dict(hdr=torch.zeros((n + 1, 3))), "hdr: shape"),
        (dict(hdr=torch.zeros((n, 3), dtype=torch.float64)), "hdr: dtype"),
        (dict(gbuffers=(torch.zeros((n, 3)), torch.zeros((n, 1)), torch.zeros(n, dtype=torch.int32))), "depth: shape"),
        (dict(gbuffers=(torch.zeros((n, 3)), torch.zeros(n), torch.zeros(n))), "object_id: dtype"),
        (dict(gbuffers=(torch.zeros((n, 2)), torch.zeros(n), torch.zeros(n, dtype=torch.int32))), "normal: shape"),
        (dict(gbuffers=(torch.zeros((n, 3)),)), "gbuffers"), (dict(gbuffers=3), "gbuffers"),
        (dict(target=torch.zeros((8, 16, 3))), "target: dtype"), (dict(target=torch.zeros((8, 16), dtype=torch.uint8)), "target"),
        (dict(target=np.zeros((8, 16, 3), np.uint8)), "target"), (dict(target=False), "no target at all"),
        (dict(frame=-1), "frame"), (dict(frame=1.5), "frame"),
        (dict(), "device"),   # what is left: tensors that are not on a device
        (dict(hdr=True), "device"),
    ]
    for change, word in cases:
        with pytest.raises(ValueError, match=word):
            s.render_baked(**dict(good, **change))
    for half in (lightmap, probes):
        with pytest.raises(ValueError, match="device"):
            s.render_baked(**half)
    s.close()


def test_the_lab_view_has_all_four_sources(P, O):
    """The camera, atlas and volume of tests/test_baked_view_gpu.py's lab frame, judged here with the oracle's hits for the
    unjittered pixel centres of the 67 x 37 frame and the two samplers' restatements: sky 2137, lightmap 128, probes 102, unlit
    112.  The jitter moves a ray by less than a pixel; 32 of each is what the GPU test asks of the frame itself."""
    import lightmap_sample_restatement as LR
    import probe_sample_restatement as PR
    import wireframe_restatement as WR
    import test_baked_view_gpu as G
    W, H = G.SIZES[-1]
    s = G.build_lab(G._Sized(P, W, H), device=P.HOST_ONLY)
    s.setCamera(*G.LAB_CAMERA)
    desc = C.cast(s.flatten(), C.POINTER(P.SceneDesc)).contents
    o, d = WR.primary_rays(desc.camera, W, H, 0, H, O)
    h = np.frombuffer(O.trace_rays(s.flatten(), o, d).tobytes(), np.int32).reshape(-1, 16)
    G.dev = lambda a: a   # the inputs as arrays: no device here
    try:
        lm, pv = G.lab_inputs(P)
    finally:
        from test_irradiance_gpu import dev
        G.dev = dev
    lm_rows = LR.sample(h, lm["charts"], lm["chart_first"], lm["image"], lm["lightmap_mode"])
    pl_rows = PR.sample_hits(h, pv["volume"], pv["probes"], pv["probe_mode"], pv["normal_bias"])
    n = np.bincount(R.source(h, lm_rows, pl_rows), minlength=4).tolist()
    assert n == [2137, 128, 102, 112], dict(zip(R.SOURCES, n))
    assert np.bincount(R.source(h, lm_rows, None), minlength=4).tolist() == [2137, 128, 0, 214]
    s.close()
