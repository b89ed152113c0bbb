"""The wireframe view on the GPU (Scene::render_to_device_wireframe -> ptrt_render_wireframe -> wireframe_kernel<GEOM>):
every image equals the CPU restatement (tests/wireframe_restatement.py) at tolerance 0, under every traversal variant
that applies; band contexts write their rows, interleaved contexts are refused; a wireframe between two path frames
changes nothing of them; it is ordered behind a pipelined path frame into the same target."""
import ctypes as C

import numpy as np
import pytest

import wireframe_restatement as R

pytestmark = pytest.mark.gpu

THICK = (0.0, 0.02, 0.05, 0.34)


def _check(P, O, s, th, what=""):
    got = s.render_wireframe_to_host(th)
    want = R.render(P, O, s, th)
    assert got.shape == want.shape == (s.tile_rows, s.width, 3)
    bad = np.flatnonzero((got != want).any(axis=2))
    assert bad.size == 0, f"{what} thickness {th}: {bad.size} pixels differ, first {bad[:6]}: " \
        f"gpu {got.reshape(-1, 3)[bad[:3]].tolist()} cpu {want.reshape(-1, 3)[bad[:3]].tolist()}"
    return got


def _all_geoms(P, O, s, th, what=""):
    """The scene's own variant, then force_geom raised to each more general one (a lower value changes nothing)."""
    imgs = []
    for g in (-1, 1, 2):
        s.set_option("force_geom", g)
        imgs.append(_check(P, O, s, th, f"{what} force_geom {g}"))
    s.set_option("force_geom", -1)
    return imgs


def _cornell(P, W=256, H=256, **kw):
    s = P.Scene(W, H, **kw)
    P.scenes.cornell(s)
    return s


def test_cornell_thicknesses(P, O):
    s = _cornell(P)
    for th in THICK:
        imgs = _all_geoms(P, O, s, th, "cornell")
        if th == 0.0:    # nothing is an edge: the sky, which is off -- black
            assert not imgs[0].any()
        elif th == 0.34:  # every hit is an edge (min(u, v, 1 - u - v) <= 1/3): the frame is lit where the box is
            assert (imgs[0] > 0).any(axis=2).mean() > 0.95
        else:
            lit = (imgs[0] > 0).any(axis=2).mean()
            assert 0.02 < lit < 0.9, lit
    s.close()


@pytest.mark.parametrize("sky", ["gradient", "off", "envmap"])
def test_sky_modes(P, O, sky):
    s = _cornell(P, 192, 128)
    s.setCamera((0, 0, 12), (0, 0, -5), (0, 1, 0), 70.0)  # the box in the middle, sky around it
    if sky == "gradient":
        s.setSkyGradient((0.2, 0.4, 1.5), (3.0, 0.5, 0.1))
    elif sky == "envmap":
        rs = np.random.RandomState(7)
        env = rs.uniform(0.0, 4.0, (32, 64, 4)).astype(np.float32)
        env[..., 3] = 1.0
        s.setSkyGradient((0.2, 0.4, 1.5), (3.0, 0.5, 0.1))
        s.setEnvironmentMap(env)
    for th in (0.0, 0.05):
        img = _all_geoms(P, O, s, th, sky)[0]
        corner = img[:8, :8]
        assert (corner.any() if sky != "off" else not corner.any()), sky
    s.close()


def test_emission_x_zero_edges_are_white(P, O):
    s = _cornell(P, 128, 128)
    green_glow = s.addCube(P.Material((0.1, 0.1, 0.1), 0.5, emission=(0.0, 5.0, 0.0)))
    s.scale(green_glow, (1.0, 1.0, 1.0))
    s.moveTo(green_glow, (0.0, 0.0, -2.0))
    img = _all_geoms(P, O, s, 0.34, "emission .x == 0")[0]
    c = img[64, 64]  # the cube's centre, an edge at this thickness: white (186 each), not green
    assert c.tolist() == [186, 186, 186], c
    s.close()


def test_thin_lens_camera(P, O):
    s = _cornell(P, 160, 120)
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0, aperture=0.6, focus_dist=8.0)
    desc = C.cast(s.flatten(), C.POINTER(P.SceneDesc)).contents
    assert desc.camera.lens_radius > 0
    for th in (0.02, 0.05):
        _all_geoms(P, O, s, th, "thin lens")
    s.close()


@pytest.mark.parametrize("leaf", [8, 2])
def test_coincident_geometry(P, O, leaf):
    s = P.Scene(160, 120)
    P.scenes.coincident(s, leaf=leaf)
    for th in (0.02, 0.34):
        _all_geoms(P, O, s, th, f"coincident leaf {leaf}")
    s.close()


def test_many_meshes_and_moved_instances(P, O):
    s = P.Scene(192, 144)
    P.scenes.many(s)
    for th in (0.02, 0.1):
        _all_geoms(P, O, s, th, "many")
    cube = s.addCube(P.Material((0.2, 0.3, 0.9), 0.4, emission=(3.0, 0.5, 0.2)))
    s.setPosition(cube, (1.0, -1.0, -5.0))
    s.setRotation(cube, (0.3, 0.5, 0.1))
    s.setInstanceScale(cube, (1.2, 0.7, 1.0))
    _check(P, O, s, 0.05, "many + instance")
    for f in range(1, 3):  # transform-only changes: ptrt_update_instances, not a new upload
        s.setPosition(cube, (1.0 - 0.8 * f, -1.0 + 0.3 * f, -5.0 + 0.5 * f))
        s.setRotation(cube, (0.3 + 0.4 * f, 0.5, 0.1 * f))
        s.commitObjectChanges()
        _all_geoms(P, O, s, 0.05, f"many, instance moved {f}")
    s.close()


def test_fluid_after_gpu_refit(P, O):
    """The refit is enqueued on the context's stream and the wireframe behind it, with no read-back in between."""
    s = P.Scene(160, 96)
    w, ship = P.scenes.fluid(s, cells=24, t=0.0, ship_segments=10)
    before = _check(P, O, s, 0.05, "fluid t=0")
    s.setVertices(w, P.scenes.water_vertices(24, 1.1))
    s.refitObjectChanges()
    after = _check(P, O, s, 0.05, "fluid after refit")
    assert not np.array_equal(before, after)  # the water did move
    _all_geoms(P, O, s, 0.05, "fluid after refit")
    s.close()


def test_showcase_1080p(P, O):
    s = P.Scene(1920, 1080)
    P.scenes.showcase(s)
    _check(P, O, s, 0.02, "showcase 1080p")
    s.close()


def test_band_contexts(P, O):
    import torch
    W, H, th = 200, 136, 0.05
    full = _cornell(P, W, H)
    ref = _check(P, O, full, th, "full")  # (bottom-up: row r of the frame is ref[H - 1 - r])
    frame = torch.full((H, W, 3), 9, dtype=torch.uint8, device="cuda")
    bands = []
    for y0, rows in ((0, 64), (64, 72)):
        b = _cornell(P, W, H, tile_y0=y0, tile_rows=rows)
        host = _check(P, O, b, th, f"band {y0}")
        assert np.array_equal(host, ref[H - y0 - rows:H - y0])
        dev = torch.zeros((rows, W, 3), dtype=torch.uint8, device="cuda")
        b.render_to_device_wireframe(dev.data_ptr(), th)
        assert np.array_equal(dev.cpu().numpy(), host)
        bands.append(b)
    for b in bands:  # PTRT_OUT_DEVICE_FRAME: each band writes its rows where they belong in the whole frame
        assert P.lib.ptrt_render_wireframe(b.ctx, th, C.c_void_p(frame.data_ptr()), 2) == 0
    for b in bands:
        b.sync()
    assert np.array_equal(frame.cpu().numpy(), ref)
    for b in bands:
        b.close()
    full.close()


def test_refusals(P):
    s = P.Scene(64, 64, interleave=(0, 2))
    P.scenes.cornell(s)
    with pytest.raises(P.PtrtError, match="interleaved"):
        s.render_wireframe_to_host(0.05)
    s.close()
    ctx = C.c_void_p()
    assert P.lib.ptrt_create(64, 64, 0, 0, 0, C.byref(ctx)) == 0
    out = np.full((64, 64, 3), 7, dtype=np.uint8)
    assert P.lib.ptrt_render_wireframe(ctx, 0.05, out.ctypes.data_as(C.c_void_p), 0) == -4  # PTRT_E_NOT_READY
    assert b"geometry not uploaded" in P.lib.ptrt_last_error(ctx)
    assert P.lib.ptrt_render_wireframe(ctx, 0.05, None, 0) == -1  # no target
    assert (out == 7).all()
    P.lib.ptrt_destroy(ctx)
    s = P.Scene(64, 64)  # no meshes: the reference's message, nothing rendered
    out = s.render_wireframe_to_host(0.05)
    s.close()


def _path_state(P, s, rgb, post):
    st = dict(rgb=rgb, frame=s.getFrameCount(), stats=s.stats())
    for k in (P.BUF_ACCUM, P.BUF_NORMAL, P.BUF_DEPTH, P.BUF_OBJECT_ID, P.BUF_RGB8, P.BUF_RNG) + \
             ((P.BUF_DENOISED, P.BUF_MOTION, P.BUF_RENDER_ACCUM) if post else ()):
        st[k] = s.read(k)
    return st


@pytest.mark.parametrize("preset", [None, "balanced"])
def test_wireframe_between_path_frames_changes_nothing(P, O, blue_noise, preset):
    W, H = 160, 128

    def run(wire):
        s = _cornell(P, W, H)
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
        out = []
        for k in range(3):
            rgb = s.render_to_host()
            out.append(_path_state(P, s, rgb, preset is not None))
            if wire and k == 1:
                hist = s.kernel_ms_history().copy()
                _check(P, O, s, 0.05, "between path frames")
                assert s.getFrameCount() == 2
                assert np.array_equal(s.kernel_ms_history(), hist)
        s.close()
        return out

    a, b = run(False), run(True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["frame"] == y["frame"] and x["stats"] == y["stats"], k
        assert np.array_equal(x["rgb"], y["rgb"]), k
        for key in x:
            if key not in ("frame", "stats", "rgb"):
                assert np.array_equal(np.asarray(x[key]).view(np.uint8), np.asarray(y[key]).view(np.uint8)), (k, key)


def test_resolution_scale_leaves_the_wireframe_full_size(P, O):
    s = _cornell(P, 160, 128)
    ref = _check(P, O, s, 0.05, "scale 1")
    s.setResolutionScale(0.5)
    assert s.renderSize() == (80, 64)
    s.render_to_host()  # a path frame at the reduced size, then the wireframe: still 160 x 128 and the same image
    assert np.array_equal(_check(P, O, s, 0.05, "scale 0.5"), ref)
    s.close()


def test_wireframe_follows_a_pipelined_path_frame(P, O):
    import torch
    W, H = 640, 360
    s = _cornell(P, W, H)
    s.setPerfSamplesPerPixel(4)
    s.setMaxBounceDepth(4)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.set_option("merged", 0)
    s.set_option("pipeline", 1)
    want = R.render(P, O, s, 0.05)
    tgt = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    for f in range(4):
        s.render_to_device(tgt[f & 1].data_ptr())
    assert s.get_option("pipelined") == 1  # the last path frame did overlap its predecessor
    s.render_to_device_wireframe(tgt[1].data_ptr(), 0.05)  # same target as that frame: the wireframe must land last
    assert np.array_equal(tgt[1].cpu().numpy(), want)
    # and the next path frame waits for the wireframe (the entry point touched the context)
    s.render_to_device(tgt[0].data_ptr())
    assert s.get_option("pipelined") == 0
    s.sync()
    s.close()
