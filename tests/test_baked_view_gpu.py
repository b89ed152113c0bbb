"""The baked-light view on the GPU (Scene.render_baked -> ptrt_render_baked -> baked_view_kernel<GEOM, PMODE>).  Every comparison
is words, tolerance 0: the HDR image and the G-buffers equal tests/baked_view_restatement.py over the rows camera_rays,
query_closest, query_lightmap and query_probe_light return for the same frame, and RGB8 equals the oracle's tonemap of that HDR
image -- under every traversal the queries have, at frames of one pixel, one tile and partial tiles on both edges, with more
tiles than workgroups, for either half alone, both and neither, at two frame indices, under the three skies, in band contexts
and assembled from them.  What must be refused is refused with every output untouched; path frames around a baked frame do
not notice it; a whole bake, viewed through it, equals lightmap.shade_samples."""
import ctypes as C

import numpy as np
import pytest

import baked_view_restatement as R
from test_irradiance_gpu import PATTERN, dev
from test_lightmap_sample_gpu import BALL, CUBE, SPHERE, TRI, XCUBE, build_lab, face_counts, random_image, table_for
from test_probe_sample_gpu import probe_records, volume
from test_ray_query_gpu import VARIANTS

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (8, 8), (67, 37)]
# the lab's view, its atlas and its volume: chosen on the CPU with the oracle's hits (test_the_lab_frame_is_not_vacuous)
LAB_CAMERA = ((-2.0, 0.5, 4.0), (-2.0, 0.5, -4.0), (0.0, 1.0, 0.0), 30.0)
LAB_SKY = ((0.2, 0.4, 1.5), (3.0, 0.5, 0.1))
LAB_ATLAS = (20, 14)
IMAGE_SEED, PROBE_SEED = 7, 3

_scenes = {}


class _Sized:
    """the package with Scene(w, h, ..) answering at another size: build_lab makes its scene 64 x 64"""

    def __init__(self, P, W, H):
        self._P, self._size = P, (W, H)

    def __getattr__(self, name):
        return getattr(self._P, name)

    def Scene(self, w, h, **kw):
        return self._P.Scene(*self._size, **kw)


def make(P, name, W, H, **kw):
    if name == "lab":
        s = build_lab(_Sized(P, W, H), **kw)
        s.setCamera(*LAB_CAMERA)
        s.setSkyGradient(*LAB_SKY)
    else:
        s = P.Scene(W, H, **kw)
        P.scenes.cornell(s)
    s.uploadToGPU()
    return s


def scene(P, name, W, H):
    key = (name, W, H)
    if key not in _scenes:
        _scenes[key] = make(P, name, W, H)
    return _scenes[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _scenes.values():
        s.close()
    _scenes.clear()


def lab_inputs(P):
    """(lightmap, volume) as render_baked's keywords.  Chart tables for two of the five meshes -- the cube moved by its vertices
    and the small sphere, whose charts lie mostly outside the 20 x 14 atlas --, an image with a fifth of its texels invalid, read
    'nearest' so that an invalid texel is a pixel the lightmap leaves empty; a 5 x 3 x 2 VISIBILITY volume of synthetic records
    round the lab whose rows from x index 3 on are NaN: what stands right of x = -0.5 and has no lightmap is unlit."""
    L = P.lightmap
    entries = [None] * 5
    entries[CUBE] = L.triangle_charts(12, 6)[0]
    entries[SPHERE] = L.triangle_charts(128, 4)[0]
    charts, first = L.chart_table(entries)
    w, h = LAB_ATLAS
    vol = P.probes.ProbeVolume.from_corners((-6.5, -4.0, -6.5), (1.5, 4.0, -2.0), (5, 3, 2))
    rec = probe_records(vol, "visibility", PROBE_SEED)
    rec[np.arange(vol.rows) % vol.counts[0] >= 3] = np.nan
    return (dict(charts=dev(charts), chart_first=dev(first), image=dev(random_image(w, h, IMAGE_SEED)), lightmap_mode="nearest"),
            dict(volume=vol, probes=dev(rec), probe_mode="visibility", normal_bias=0.05))


def cornell_inputs(P, s):
    """test_lightmap_sample_gpu's table for the box (a mesh without a lightmap, authored corners outside the atlas, a table that
    ends inside a mesh) over a 33 x 40 image, bilinear; test_probe_sample_gpu's 2 x 2 x 2 volume over the box"""
    w, h = 33, 40
    charts, first = table_for(P, face_counts(s), w, h)
    vol = volume(P, "cell")
    return (dict(charts=dev(charts), chart_first=dev(first), image=dev(random_image(w, h)), lightmap_mode="bilinear"),
            dict(volume=vol, probes=dev(probe_records(vol, "visibility")), probe_mode="visibility", normal_bias=0.05))


def inputs(P, name, s):
    return lab_inputs(P) if name == "lab" else cornell_inputs(P, s)


def chain(P, O, s, frame, lm=None, pv=None):
    """the restatement over the existing entry points' rows for frame `frame` of the scene's rows"""
    o, d = s.camera_rays(frame)
    assert o.shape == (s.tile_rows * s.width, 3)
    closest = s.query_closest(o, d)
    lm_rows = s.query_lightmap(o, d, lm["charts"], lm["chart_first"], lm["image"], lm["lightmap_mode"]) if lm else None
    pl_rows = s.query_probe_light(o, d, pv["volume"], pv["probes"], pv["probe_mode"], pv["normal_bias"]) if pv else None
    albedo, emission = R.materials(P, s)
    want = R.shade(closest, R.sky(P, O, s, d), albedo, emission, lm_rows, pl_rows)
    want["rgb8"] = R.rgb8(O, want["hdr"], s.width, s.tile_rows)
    return want


def assert_same(got, want, what):
    for key, words in (("hdr", np.int32), ("normal", np.int32), ("depth", np.int32), ("object_id", np.int32), ("rgb8", np.uint8)):
        g = got[key]
        g = np.ascontiguousarray(g.cpu().numpy() if hasattr(g, "cpu") else g).view(words)
        x = np.ascontiguousarray(want[key]).view(words)
        assert g.shape == x.shape, (what, key, g.shape, x.shape)
        bad = np.argwhere(g != x)
        assert bad.size == 0, (f"{what}: {key}: {len(bad)} of {g.size} words differ, first {bad[:4].tolist()}: "
                               f"{g[tuple(bad[0])]:#x} vs {x[tuple(bad[0])]:#x}")


def check(P, O, s, frame, lm, pv, what):
    """one baked frame with every output against the chain; returns (got, want)"""
    want = chain(P, O, s, frame, lm, pv)
    got = s.render_baked(frame=frame, hdr=True, gbuffers=True, **(lm or {}), **(pv or {}))
    assert set(got) == {"rgb8", "hdr", "normal", "depth", "object_id"}
    assert_same(got, want, what)
    return got, want


# ---- 1. equality under every traversal ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
@pytest.mark.parametrize("name", ["lab", "cornell"])
def test_the_view_equals_the_chain(P, O, name, fg, pt):
    for W, H in SIZES:
        s = scene(P, name, W, H)
        lm, pv = inputs(P, name, s)
        s.set_option("force_geom", fg)
        s.set_option("pair_trace", pt)
        try:
            check(P, O, s, 0, lm, pv, f"{name} {W} x {H}")
            pm = s.get_option("query_pmode")
            if pt == 0:
                assert pm == 0
            elif name == "cornell":
                assert pm == {-1: 1, 1: 2, 2: 3}[fg]
            elif fg == 2:
                assert pm == 3
            if (W, H) == SIZES[-1]:   # either half alone, and neither: emission and sky
                check(P, O, s, 0, lm, None, f"{name} {W} x {H}, no volume")
                check(P, O, s, 0, None, pv, f"{name} {W} x {H}, no lightmap")
                check(P, O, s, 0, None, None, f"{name} {W} x {H}, neither")
        finally:
            s.set_option("force_geom", -1)
            s.set_option("pair_trace", 1)


def test_the_lab_frame_is_not_vacuous(P, O):
    """In the 67 x 37 lab frame each source owns at least 32 pixels.  With the oracle's hits for the unjittered pixel centres
    the CPU counts were: sky 2137, lightmap 128, probes 102, unlit 112 of 2479; without the volume sky 2137, lightmap 128,
    unlit 214 -- 14 of the cube's 142 pixels fall on invalid texels and go to the volume, the sphere's 17 lie outside the atlas
    (tests/test_baked_view.py holds these figures).  The jittered frame 0 on an MI355X: sky 2117, lightmap 142, probes 107,
    unlit 113."""
    W, H = SIZES[-1]
    s = scene(P, "lab", W, H)
    lm, pv = lab_inputs(P)
    _, want = check(P, O, s, 0, lm, pv, "the lab")
    n = np.bincount(want["source"], minlength=4)
    print("the lab's sources:", dict(zip(R.SOURCES, n.tolist())))
    assert (n >= 32).all(), dict(zip(R.SOURCES, n.tolist()))
    hit_mesh = want["object_id"]
    assert (want["source"][hit_mesh == TRI] == R.PROBES).all(), "a moving object without a chart is lit by the volume"
    assert (want["source"][hit_mesh == XCUBE] != R.LIGHTMAP).all() and (want["source"][hit_mesh == BALL] != R.LIGHTMAP).all()
    assert (want["source"][hit_mesh == CUBE] == R.LIGHTMAP).sum() >= 32 and (want["source"][hit_mesh == CUBE] == R.PROBES).sum() >= 4
    assert np.isfinite(want["hdr"]).all(), "a NaN of an invalid texel or probe came through"
    _, bare = check(P, O, s, 0, lm, None, "the lab without the volume")
    m = np.bincount(bare["source"], minlength=4)
    assert m[R.PROBES] == 0 and m[R.LIGHTMAP] == n[R.LIGHTMAP] and m[R.UNLIT] == n[R.UNLIT] + n[R.PROBES] and m[R.UNLIT] >= 32
    lit = want["source"] == R.PROBES
    assert not np.array_equal(want["hdr"][lit], bare["hdr"][lit]), "the volume lights nothing"


def test_more_tiles_than_workgroups(P, O):
    """200 x 136 is 25 x 17 = 425 tiles; with option persist = 1 the grid is one workgroup per CU and strides"""
    s = make(P, "cornell", 200, 136)
    try:
        lm, pv = cornell_inputs(P, s)
        s.set_option("persist", 1)
        assert s.get_option("persist") == 1
        got, _ = check(P, O, s, 0, lm, pv, "persist 1")
        s.set_option("persist", 0)
        again, _ = check(P, O, s, 0, lm, pv, "persist 0")
        assert np.array_equal(got["rgb8"], again["rgb8"])
    finally:
        s.close()


# ---- 2. the frame index, the sky ----------------------------------------------------------------------------------------------
def test_frame_indices(P, O):
    W, H = SIZES[-1]
    s = scene(P, "cornell", W, H)
    lm, pv = cornell_inputs(P, s)
    a, _ = check(P, O, s, 0, lm, pv, "frame 0")
    b, _ = check(P, O, s, 5, lm, pv, "frame 5")
    assert not np.array_equal(a["hdr"].cpu().numpy(), b["hdr"].cpu().numpy()), "the jitter of frame 5 is frame 0's"
    # frame=None: the index render_to_device would use next, which is not advanced
    s.setFrameCount(5)
    c = s.render_baked(hdr=True, **lm, **pv)
    assert s.getFrameCount() == 5 and np.array_equal(c["hdr"].cpu().numpy().view(np.int32), b["hdr"].cpu().numpy().view(np.int32))
    s.setFrameCount(0)


@pytest.mark.parametrize("sky", ["gradient", "off", "envmap"])
def test_sky_modes(P, O, sky):
    s = P.Scene(96, 64)
    P.scenes.cornell(s)
    s.setCamera((0, 0, 12), (0, 0, -5), (0, 1, 0), 70.0)  # the box in the middle, sky around it
    if sky != "off":
        s.setSkyGradient((0.2, 0.4, 1.5), (3.0, 0.5, 0.1))
    if sky == "envmap":
        env = np.random.RandomState(7).uniform(0.0, 4.0, (32, 64, 4)).astype(F)
        env[..., 3] = 1.0
        s.setEnvironmentMap(env)
    s.uploadToGPU()
    try:
        lm, pv = cornell_inputs(P, s)
        got, want = check(P, O, s, 3, lm, pv, sky)
        miss = want["source"] == R.SKY
        assert miss.sum() >= 500 and (~miss).sum() >= 500
        assert want["hdr"][miss].any() == (sky != "off")
    finally:
        s.close()


# ---- 3. bands ------------------------------------------------------------------------------------------------------------------
def test_band_contexts(P, O):
    import torch
    W, H = 200, 136
    full = make(P, "cornell", W, H)
    lm, pv = cornell_inputs(P, full)
    ref, _ = check(P, O, full, 2, lm, pv, "full")   # (rgb8 bottom-up: row r of the frame is ref[H - 1 - r])
    ref_hdr = ref["hdr"].cpu().numpy().view(np.int32)
    frame = torch.full((H, W, 3), 9, dtype=torch.uint8, device="cuda")
    bands = []
    for y0, rows in ((0, 64), (64, 72)):
        b = make(P, "cornell", W, H, tile_y0=y0, tile_rows=rows)
        got, _ = check(P, O, b, 2, lm, pv, f"band {y0}")
        assert np.array_equal(got["rgb8"], ref["rgb8"][H - y0 - rows:H - y0])
        assert np.array_equal(got["hdr"].cpu().numpy().view(np.int32), ref_hdr[y0 * W:(y0 + rows) * W])
        own = torch.zeros((rows, W, 3), dtype=torch.uint8, device="cuda")
        out = b.render_baked(own, frame=2, **lm, **pv)
        assert out["rgb8"] is own and np.array_equal(own.cpu().numpy(), got["rgb8"])
        bands.append(b)
    for b in bands:   # PTRT_OUT_DEVICE_FRAME: each band writes its rows where they belong in the whole frame
        b.render_baked(frame, frame=2, **lm, **pv)
    for b in bands:
        b.sync()
    assert np.array_equal(frame.cpu().numpy(), ref["rgb8"])
    for b in bands:
        b.close()
    full.close()


def test_interleaved_and_thin_lens_are_refused(P):
    import torch
    s = P.Scene(64, 64, interleave=(0, 2))
    P.scenes.cornell(s)
    hdr = torch.full((s.tile_rows * 64, 3), 7.0, device="cuda")
    with pytest.raises(P.PtrtError, match="interleaved"):
        s.render_baked(hdr=hdr)
    s.close()
    s = P.Scene(64, 64)
    P.scenes.cornell(s)
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0, aperture=0.6, focus_dist=8.0)
    hdr = torch.full((64 * 64, 3), 7.0, device="cuda")
    with pytest.raises(P.PtrtError, match="thin lens"):
        s.render_baked(hdr=hdr)
    torch.cuda.synchronize()
    assert bool((hdr == 7.0).all())
    s.close()


# ---- 4. neighbours -----------------------------------------------------------------------------------------------------------
def _path_state(P, s, rgb, post):
    st = dict(rgb=rgb, frame=s.getFrameCount(), stats=s.stats())
    for k in (P.BUF_ACCUM, P.BUF_NORMAL, P.BUF_DEPTH, P.BUF_OBJECT_ID, P.BUF_RGB8, P.BUF_RNG) + \
             ((P.BUF_DENOISED, P.BUF_MOTION, P.BUF_RENDER_ACCUM) if post else ()):
        st[k] = s.read(k)
    return st


@pytest.mark.parametrize("preset", [None, "balanced"])
def test_a_baked_frame_between_path_frames_changes_nothing(P, O, blue_noise, preset):
    W, H = 160, 128

    def run(baked):
        s = P.Scene(W, H)
        P.scenes.cornell(s)
        if preset:
            s.setPerformancePreset(preset)
        else:
            s.setPerfSamplesPerPixel(2)
            s.setMaxBounceDepth(3)
            s.setDenoiserEnabled(False)
            s.setBloomEnabled(False)
        s.initBlueNoise()
        s.uploadToGPU()
        s.set_option("count_rays", 1)
        lm, pv = cornell_inputs(P, s)
        out = []
        for k in range(3):
            rgb = s.render_to_host()
            out.append(_path_state(P, s, rgb, preset is not None))
            if baked and k == 1:
                hist = s.kernel_ms_history().copy()
                launches = [np.asarray(a).copy() for a in s.launch_ms_history()]
                got = s.render_baked(hdr=True, gbuffers=True, **lm, **pv)   # frame=None: frame 2's jitter
                assert got["hdr"].cpu().numpy().any()
                assert s.getFrameCount() == 2
                assert np.array_equal(s.kernel_ms_history(), hist)
                assert all(np.array_equal(a, b) for a, b in zip(launches, s.launch_ms_history()))
        s.close()
        return out

    a, b = run(False), run(True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["frame"] == y["frame"] and x["stats"] == y["stats"], k
        assert np.array_equal(x["rgb"], y["rgb"]), k
        for key in x:
            if key not in ("frame", "stats", "rgb"):
                assert np.array_equal(np.asarray(x[key]).view(np.uint8), np.asarray(y[key]).view(np.uint8)), (k, key)


# ---- 5. the loop closes ---------------------------------------------------------------------------------------------------------
def test_a_bake_viewed_through_the_baked_view(P, O):
    """test_lightmap_sample_gpu's bake of the Cornell box -- atlas_texels for every mesh into one atlas, query_direct +
    query_irradiance at 16 directions, scatter, atlas_filter, atlas_dilate -- and then render_baked at 64 x 64: its HDR image
    is lightmap.shade_samples over query_lightmap's rows with the scene's own albedo and emission, bit for bit."""
    import torch
    L = P.lightmap
    s = scene(P, "cornell", 64, 64)
    faces = face_counts(s)
    uv, w, h = L.triangle_charts(sum(faces), 12, gutter=2)
    starts = np.concatenate([[0], np.cumsum(faces)])
    per_mesh = [uv[starts[m]:starts[m + 1]] for m in range(len(faces))]
    rec = None
    for m, c in enumerate(per_mesh):
        rec = s.atlas_texels(m, dev(c), w, h, out=rec, clear=rec is None)
    idx = L.covered(rec)
    pos, nrm = L.atlas_inputs(rec)
    n, k = len(idx), 16
    direct = s.query_direct(pos, nrm, dev(L.hammersley2(4)))
    gather = s.query_irradiance(pos, nrm, dev(L.hammersley2(k)), s.init_rng_states(7, 0, n * k), samples=1, max_depth=3)
    img = L.scatter(dev(L.total_irradiance(direct, gather)), idx, w, h).reshape(h, w, 4)
    sd, sp = L.filter_sigmas(L.texel_pitch(rec, w, h))
    baked = s.atlas_dilate(s.atlas_filter(rec, img, 2, sd, sp), 2)
    charts, first = L.chart_table([dev(c) for c in per_mesh])
    got = s.render_baked(frame=0, charts=charts, chart_first=first, image=baked, hdr=True)
    o, d = s.camera_rays(0)
    rows = s.query_lightmap(o, d, charts, first, baked)
    albedo, emission = R.materials(P, s)
    want = L.shade_samples(rows, torch.as_tensor(albedo, device="cuda"), torch.as_tensor(emission, device="cuda"))
    hdr = got["hdr"]
    assert hdr.shape == (64 * 64, 3) and torch.equal(hdr.view(torch.int32), want.view(torch.int32)), "the view is not shade_samples"
    assert bool(torch.isfinite(hdr).all()) and float(hdr.mean()) > 1e-3, "the view is black"
    assert np.array_equal(got["rgb8"], R.rgb8(O, hdr.cpu().numpy(), 64, 64)) and got["rgb8"].any()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    lib, vp = P.lib, C.c_void_p
    OK, INVALID, NOT_READY = P.PTRT_OK, -1, -4
    W, H = 24, 16
    n = W * H
    s = make(P, "cornell", W, H)
    c = s.ctx
    lm, pv = cornell_inputs(P, s)
    want = s.render_baked(frame=0, hdr=True, **lm, **pv)   # (through the mirror, which hands the context its camera; the rest is the C ABI's)
    hdr = torch.full((n, 3), 7.0, device="cuda")
    nrm = torch.full((n, 3), 7.0, device="cuda")
    dep = torch.full((n,), 7.0, device="cuda")
    oid = torch.full((n,), PATTERN, dtype=torch.int32, device="cuda")
    rgb = torch.full((H, W, 3), 9, dtype=torch.uint8, device="cuda")
    big = torch.full((1 << 16,), PATTERN, dtype=torch.int32, device="cuda")  # something every span fits into, to overlap with
    host = np.zeros(1 << 16, np.uint8)
    hp = vp(host.ctypes.data)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return block.value + size - nbytes

    def untouched():
        torch.cuda.synchronize()
        return (bool((hdr == 7.0).all()) and bool((nrm == 7.0).all()) and bool((dep == 7.0).all()) and bool((oid == PATTERN).all())
                and bool((rgb == 9).all()) and bool((big == PATTERN).all()) and not host.any())

    def view(**change):
        v, keep = P.baked.baked_view(s, hdr=hdr, normal=nrm, depth=dep, object_id=oid, **lm, **pv)
        for k, x in change.items():
            if k == "counts":
                v.volume.counts[:] = x
            elif k in ("spacing", "origin"):
                getattr(v.volume, k)[:] = x
            else:
                setattr(v, k, x)
        return v, keep

    def call(ctx=c, frame=0, out=rgb.data_ptr(), mode=1, **change):
        v, keep = view(**change)
        rc = lib.ptrt_render_baked(ctx, frame, C.byref(v), vp(out) if out else None, mode)
        del keep
        return rc

    p = {k: t.data_ptr() for k, t in dict(lm, probes=pv["probes"]).items() if hasattr(t, "data_ptr")}
    n_faces, rows = int(lm["charts"].shape[0]), pv["volume"].rows
    aw, ah = int(lm["image"].shape[1]), int(lm["image"].shape[0])
    cases = [
        dict(frame=-1), dict(frame=-2 ** 31), dict(mode=3), dict(mode=-1), dict(out=None, d_hdr=None), dict(out=None, mode=0, d_hdr=None),
        # the lightmap half: what ptrt_query_lightmap refuses
        dict(n_chart_faces=0), dict(n_chart_faces=-5), dict(d_charts=None), dict(d_chart_first=None), dict(atlas_w=0), dict(atlas_h=-3),
        dict(atlas_w=1 << 14, atlas_h=(1 << 14) + 1), dict(lightmap_mode=2), dict(lightmap_mode=-1),
        dict(d_image=p["image"] + 4), dict(d_image=p["image"] + 8), dict(d_charts=p["charts"] + 2), dict(d_chart_first=p["chart_first"] + 1),
        dict(d_charts=hp.value), dict(d_chart_first=hp.value), dict(d_image=hp.value),
        dict(d_charts=tail(n_faces * 24 - 4)), dict(d_chart_first=tail(len(face_counts(s)) * 4 - 4)), dict(d_image=tail(aw * ah * 16 - 16)),
        dict(n_chart_faces=(size // 24) + 1, d_charts=block.value),
        # the probe half: what ptrt_query_probe_light refuses
        dict(probe_mode=2), dict(probe_mode=-1), dict(normal_bias=-0.1), dict(normal_bias=float("nan")), dict(normal_bias=float("inf")),
        dict(counts=(0, 2, 2)), dict(counts=(2, -1, 2)), dict(counts=(4096, 4096, 2)), dict(spacing=(1.0, 0.0, 1.0)),
        dict(spacing=(1.0, float("inf"), 1.0)), dict(spacing=(float("nan"), 1.0, 1.0)), dict(origin=(0.0, float("nan"), 0.0)),
        dict(d_probes=p["probes"] + 8), dict(d_probes=hp.value), dict(d_probes=tail(rows * 128 - 128)),
        # the outputs: the context's device memory, large enough, aligned, apart from every input and from each other
        dict(d_hdr=hp.value), dict(d_normal=hp.value), dict(d_depth=hp.value), dict(d_object_id=hp.value), dict(out=hp.value),
        dict(d_hdr=tail(n * 12 - 4)), dict(d_normal=tail(n * 12 - 4)), dict(d_depth=tail(n * 4 - 4)), dict(d_object_id=tail(n * 4 - 4)),
        dict(out=tail(n * 3 - 1)), dict(out=tail(n * 3 - 1), mode=2),
        dict(d_hdr=hdr.data_ptr() + 2), dict(d_depth=dep.data_ptr() + 1),
        dict(d_hdr=p["image"]), dict(d_hdr=p["charts"]), dict(d_normal=p["probes"]), dict(d_depth=p["chart_first"]), dict(out=p["image"]),
        dict(d_object_id=p["probes"] + 128 * rows - 4),
        dict(d_normal=hdr.data_ptr()), dict(d_depth=hdr.data_ptr() + 12 * n - 4), dict(d_object_id=dep.data_ptr()), dict(out=hdr.data_ptr()),
        dict(d_hdr=big.data_ptr(), d_charts=big.data_ptr() + n * 12 - 4), dict(d_hdr=big.data_ptr() + 16, d_probes=big.data_ptr()),
        dict(ctx=None),
    ]
    for change in cases:
        assert call(**change) == INVALID, change
        if "ctx" not in change:
            assert b"ptrt_render_baked" in lib.ptrt_last_error(c), change
    assert lib.ptrt_render_baked(c, 0, None, vp(rgb.data_ptr()), 1) == INVALID and b"view is NULL" in lib.ptrt_last_error(c)
    assert untouched()
    hip.hipFree(block)
    # contexts that are not ready, an interleaved one, a thin lens: each with good arguments
    d = C.cast(s.flatten(), C.POINTER(P.SceneDesc)).contents

    def create(interleaved=False):
        ctx = vp()
        if interleaved:
            assert lib.ptrt_create_interleaved(W, H, 0, 2, 0, C.byref(ctx)) == OK
        else:
            assert lib.ptrt_create(W, H, 0, 0, 0, C.byref(ctx)) == OK
        return ctx

    def geometry(ctx):
        assert lib.ptrt_upload_geometry(ctx, d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == OK

    empty, geom, few, lens, strips = create(), create(), create(), create(), create(True)
    geometry(geom)
    geometry(few)
    one = P.Materials()
    C.memmove(C.byref(one), C.byref(d.materials), C.sizeof(P.Materials))
    one.count = 1
    assert lib.ptrt_upload_materials(few, C.byref(one)) == OK
    for ctx in (lens, strips):
        assert lib.ptrt_upload_scene(ctx, C.byref(d)) == OK
    cam = P.Camera()
    C.memmove(C.byref(cam), C.byref(d.camera), C.sizeof(P.Camera))
    cam.lens_radius = 0.25
    assert lib.ptrt_set_camera(lens, C.byref(cam)) == OK
    for ctx, code, word in ((empty, NOT_READY, b"geometry not uploaded"), (geom, NOT_READY, b"materials not uploaded"),
                            (few, NOT_READY, b"materials for"), (lens, INVALID, b"thin lens"), (strips, INVALID, b"interleaved")):
        assert call(ctx=ctx) == code and word in lib.ptrt_last_error(ctx), word
        assert call(ctx=ctx, lightmap_mode=7) == INVALID   # a bad argument is named before the scene is looked at
    assert untouched()
    for ctx in (empty, geom, few, lens, strips):
        assert lib.ptrt_sync(ctx) == OK
        lib.ptrt_destroy(ctx)
    assert call(ctx=empty) == INVALID and untouched()   # a destroyed context
    # the call that is in order writes its pixels and no others
    G = 5
    guarded = torch.full((n + 2 * G, 3), 7.0, device="cuda")
    assert call(d_hdr=guarded.data_ptr() + 12 * G) == OK
    s.sync()
    assert bool((guarded[:G] == 7.0).all()) and bool((guarded[G + n:] == 7.0).all()), "a write outside the rows"
    assert bool((hdr == 7.0).all()) and not bool((nrm == 7.0).all()) and not bool((rgb == 9).all())
    assert torch.equal(guarded[G:G + n].view(torch.int32), want["hdr"].view(torch.int32)) and np.array_equal(rgb.cpu().numpy(), want["rgb8"])
    s.close()
