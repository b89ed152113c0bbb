"""The post chain's kernels (csrc/pt_denoise.hip.h, pt_post.hip.h) on the synthetic items of tests/post_truth.py, driven through
the C ABI on a full-frame context: ptrt_set_camera, ptrt_denoiser_enable (through Scene.setDenoiserSettings), ptrt_set_bloom,
ptrt_set_prev_view_proj, ptrt_post_frame over device arrays, ptrt_read_buffer.  Scene.post_frame is not used: the mirror hands the
context its own previous view-projection.  Every item, frame and settings variant is held to the oracle's bits; option atrous_exp = 1
is judged by the float64 statement at the table's tolerances on decided pixels."""
import ctypes as C

import numpy as np
import pytest

import post_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def items():
    return T.ITEMS()


def _set_camera(P, s, cam):
    c = P.Camera()
    for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        setattr(c, k, P.Vec3(*cam[k]))
    c.lens_radius = cam["lens_radius"]
    s._cchk(P.lib.ptrt_set_camera(s.ctx, C.byref(c)))


def _post(P, s, torch, fr):
    """One ptrt_post_frame over the frame's arrays in device memory -> RGB8 (bottom-up, as the buffer is)."""
    dev = [torch.from_numpy(a).cuda() for a in T.frame_arrays(fr)]
    H, W = fr["depth"].shape
    rgb = np.empty((H, W, 3), np.uint8)
    s._cchk(P.lib.ptrt_post_frame(s.ctx, *(t.data_ptr() for t in dev), rgb.ctypes.data_as(C.c_void_p), 0))   # (synchronous)
    return rgb


def _bits_equal(got, want, W, what):
    """Bit equality of two images given as (pixels, channels) or (H, W, channels); the message names the first differing pixel."""
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want, g.dtype).reshape(g.shape)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    g, w = g.reshape(-1, g.shape[-1]), w.reshape(-1, g.shape[-1])
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} px differ, first (x, y) = ({bad[0] % W}, {bad[0] // W}): {got.reshape(g.shape)[bad[0]]} " \
                          f"against {np.asarray(want).reshape(g.shape)[bad[0]]}"


def _run(P, O, torch, s, item, k, name, bloom=False, exp=0):
    """The item's frames through the context with atrous_iterations = k, beside an oracle.Denoiser.  Every frame: motion vectors,
    denoised (bloomed) image and RGB8 equal to the oracle's bits (exp = 0); yields (f, device image, oracle image)."""
    W, H, S = item["W"], item["H"], dict(item["settings"], atrous_iterations=k)
    s.setDenoiserSettings(P.DenoiserSettings(**S))
    s.set_option("atrous_exp", exp)
    s._cchk(P.lib.ptrt_set_bloom(s.ctx, 1 if bloom else 0))
    dn = O.Denoiser(W, H, O.DenoiserSettings(**S))
    out = []
    for f, fr in enumerate(item["frames"]):
        what = f"{name}, atrous_iterations {k}, frame {f}"
        _set_camera(P, s, fr["cam"])
        s.set_option("motion_vectors", 0 if fr["pvp"] is None else 1)
        color, normal, depth, obj = T.frame_arrays(fr)
        if fr["pvp"] is None:                                           # vectors off: the zeros the context starts with
            mv = np.zeros((W * H, 2), np.float32)
        else:
            pvp = np.ascontiguousarray(fr["pvp"], np.float32)
            s._cchk(P.lib.ptrt_set_prev_view_proj(s.ctx, pvp.ctypes.data_as(C.POINTER(C.c_float))))
            mv = O.motion_vectors(depth, W, H, T.CameraView(fr["cam"]), pvp)
        rgb = _post(P, s, torch, fr)
        _bits_equal(s.read(P.BUF_MOTION), mv, W, what + ", motion vectors")
        den = dn.denoise(color, normal, depth, mv, obj)
        want = O.bloom(den, W, H) if bloom else den
        got = s.read(P.BUF_DENOISED)
        if exp == 0:
            _bits_equal(got, want, W, what + (", bloomed image" if bloom else ", denoised image"))
            _bits_equal(rgb[::-1], O.tonemap(want, W, H)[::-1], W, what + ", RGB8")
            _bits_equal(s.read(P.BUF_RGB8), rgb, W, what + ", RGB8 buffer")
        out.append((f, got, want))
    return out


def _scene(P, W, H):
    return P.Scene(W, H)


def test_every_item_has_the_oracles_bits(P, O, torch_, items):
    """Each item at its own settings and at 0 and 2 passes (another kernel writes the image: c4_to_output_kernel, and pass 2 as
    LAST), the threshold items included."""
    for name, item in items.items():
        s = _scene(P, item["W"], item["H"])
        for k in sorted({item["settings"]["atrous_iterations"], 0, 2}):
            _run(P, O, torch_, s, item, k, name)
        s.close()


def test_plain_sequence_at_every_iteration_count_has_the_oracles_bits(P, O, torch_, items):
    for name in ("plain/131x77", "plain/65x17", "plain_moved/131x77"):
        item = items[name]
        s = _scene(P, item["W"], item["H"])
        for k in T.ATROUS_VARIANTS:
            _run(P, O, torch_, s, item, k, name)
        s.close()


def test_static_frames_with_the_vectors_on_have_the_oracles_bits(P, O, torch_, items):
    """The items' static frames run with the motion vectors off (post_truth.py says why); here the same frames with the vectors
    computed for an unmoved camera, rounding noise and all, and the issue's (+2.25, -1.5) px shift, which puts `nearest` on a row
    border: oracle bits only."""
    for name in ("plain/96x64", "checker1/65x17", "sky/65x17"):
        item = dict(items[name])
        W, H = item["W"], item["H"]
        item["frames"] = [dict(fr, pvp=T.view_proj(W, H) if fr["pvp"] is None else T.view_proj(W, H, (2.25, -1.5)))
                          for fr in item["frames"]]
        s = _scene(P, W, H)
        for k in (5, 1):
            _run(P, O, torch_, s, item, k, name + " (vectors on)")
        s.close()


def test_bloom_has_the_oracles_bits_and_fits_the_statement(P, O, torch_, items):
    """The pass scheduler of run_bloom over the sizes of post_truth.BLOOM_SIZES, denoiser off: the bloomed image and RGB8 equal the
    oracle's bits, the image fits the statement, RGB8 equals the statement's on decided bytes.  Two sizes behind the denoiser."""
    worst = 0.0
    for (W, H) in T.BLOOM_SIZES:
        s = _scene(P, W, H)
        s.set_option("denoiser_active", 0)
        s._cchk(P.lib.ptrt_set_bloom(s.ctx, 1))
        for kind, img in T.bloom_images(W, H).items():
            fr = dict(color=img.reshape(H, W, 3), normal=np.zeros((H, W, 3), np.float32), depth=np.ones((H, W), np.float32),
                      obj=np.zeros((H, W), np.int32))
            rgb = _post(P, s, torch_, fr)
            got, want = s.read(P.BUF_ACCUM), O.bloom(img, W, H)
            _bits_equal(got, want, W, f"bloom {kind} {W}x{H}")
            _bits_equal(rgb[::-1], O.tonemap(want, W, H)[::-1], W, f"bloom {kind} {W}x{H}, RGB8")
            truth = T.bloom(img, W, H)
            units = T.deviation(got, truth)[0]
            worst = max(worst, units)
            assert units <= T.TOL["bloom"], f"bloom {kind} {W}x{H}: {units:.3f} units"
            _, byte, dec = T.tonemap(got)
            assert np.array_equal(rgb[::-1].reshape(-1, 3).astype(np.int64)[dec], byte[dec]), f"bloom {kind} {W}x{H}: decided RGB8 bytes"
        s.close()
    print(f"bloom: largest deviation of the device from the statement {worst:.3f} units (table {T.MEASURED['bloom'][1]})")
    for (W, H) in T.BLOOM_BEHIND_DENOISER:
        item = T.plain(W, H)
        s = _scene(P, W, H)
        _run(P, O, torch_, s, item, 5, f"plain/{W}x{H} + bloom", bloom=True)
        s.close()


def test_hardware_exponential_fits_the_statement(P, O, torch_, items):
    """Option atrous_exp = 1 (v_exp_f32 in the luminance weight, what the reference's __expf is) on the plain and checkerboard
    sequences: the image after k = 1..5 passes within the table's tolerance of the statement on decided pixels; the motion vectors
    and the temporal history (the image after 0 passes) keep the oracle's bits."""
    worst = {}
    for name in ("plain/131x77", "plain_moved/65x17", "checker1/65x17", "checker2/64x4"):
        item = items[name]
        W, H = item["W"], item["H"]
        records = list(T.oracle_frames(O, item))                        # the statement, stage by stage on the oracle's history
        s = _scene(P, W, H)
        for f, got, want in _run(P, O, torch_, s, item, 0, name, exp=1):
            _bits_equal(got, want, W, f"{name}, frame {f}: temporal history with atrous_exp = 1")
        for k in range(1, 6):
            differs = False
            for f, got, want in _run(P, O, torch_, s, item, k, name, exp=1):
                r = records[f]["T"]
                units = T.deviation(got.reshape(H, W, 3), r["out"][k], r["decided"][k])[0]
                if units > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (units, f"{name} f{f}")
                assert units <= T.TOL[f"out{k}"], f"{name}, frame {f}, {k} passes: {units:.3f} units, tolerance {T.TOL[f'out{k}']:.3f}"
                differs = differs or not np.array_equal(got.view(np.uint32), want.view(np.uint32))
            assert differs or name.startswith("checker"), (name, k)     # (the mode really takes the other exponential)
        s.close()
    for k, (units, where) in sorted(worst.items()):
        print(f"atrous_exp = 1, {k} passes: largest deviation {units:.3f} units on {where} (table {T.MEASURED[f'out{k}'][1]}, "
              f"tolerance {T.TOL[f'out{k}']:.3f})")


def test_upscale_at_a_ratio_that_is_not_two(P, O):
    """131x99 at resolution scale 0.75: the path tracer, the denoiser (default settings, set through setDenoiserSettings) and the
    tonemap's input run at 98x74 and upscale_bilinear_kernel fills the frame."""
    W, H = 131, 99
    s = P.Scene(W, H)
    P.scenes.cornell(s)
    s.setPerfSamplesPerPixel(1)
    s.setMaxBounceDepth(4)
    s.setDenoiserEnabled(True)
    s.setBloomEnabled(False)
    s.setResolutionScale(0.75)
    rw, rh = s.renderSize()
    assert (rw, rh) == (98, 74)
    s.initBlueNoise()
    s.uploadToGPU()
    s.setDenoiserSettings(P.DenoiserSettings())
    for f in range(2):
        rgb = s.render_to_host()
        den = s.read(P.BUF_DENOISED)
        assert den.shape == (rw * rh, 3) and den.any()
        want = O.upscale(den, W, H, rw, rh)
        got = s.read(P.BUF_ACCUM)
        _bits_equal(got, want, W, f"up-scale 98x74 -> 131x99, frame {f}")
        units = T.deviation(got, T.upscale(den, W, H, rw, rh))[0]
        print(f"up-scale 98x74 -> 131x99, frame {f}: {units:.3f} units from the statement (table {T.MEASURED['upscale'][1]})")
        assert units <= T.TOL["upscale"]
        _bits_equal(rgb[::-1], O.tonemap(want, W, H)[::-1], W, f"RGB8, frame {f}")
        _, byte, dec = T.tonemap(got)
        g8 = rgb[::-1].reshape(-1, 3).astype(np.int64)
        assert np.array_equal(g8[dec], byte[dec]) and np.abs(g8 - byte).max() <= 1
    s.close()
