"""The device's primary rays (Scene.camera_rays) and frames on the lab of tests/frame_truth.py, held to the float64 statement of
the camera ray and of what a frame keeps of a sample within the table tests/test_frame_truth.py measures on the CPU (DESIGN.md
5.5): both sizes, a band and an interleaved context, the four (frame, samples) pairs, a pinhole and a lens, under every loop shape
that carries its own copy or variant of phase [A] -- each test asserting through the read-only options that the shape it names
ran -- and the all-miss views' generator states.  Nothing of the oracle but oracle.xorwow_draw is used."""
import numpy as np
import pytest

import frame_truth as FT

pytestmark = pytest.mark.gpu

SHAPES = [(96, 48, "whole"), (70, 33, "whole"), (96, 48, "band"), (96, 48, "strips")]

# loop shape -> (options, the facts the read-only options must report afterwards)
MEGA = dict(render_mode=0)
LOOPS = {
    "pm1-stage7-sync0": (dict(stage=7, sample_sync=0), dict(MEGA, pmode=1, sample_sync_eff=0, refilled=0)),
    "pm1-stage7-sync1": (dict(stage=7, sample_sync=1), dict(MEGA, pmode=1, sample_sync_eff=1, refilled=0)),
    "pm1-stage0-sync0": (dict(stage=0, sample_sync=0), dict(MEGA, pmode=1, sample_sync_eff=0, refilled=0)),
    "pm1-stage0-sync1": (dict(stage=0, sample_sync=1), dict(MEGA, pmode=1, sample_sync_eff=1, refilled=0)),
    # refill 1 refills only where it was measured to pay (spp x depth >= 16, two tiles per resident wave, a pipelined frame):
    # never at these sizes, so its decision is taken and the kernel without refill runs; refill 2 always refills
    "pm1-refill1": (dict(refill=1), dict(MEGA, pmode=1, refilled=0)),
    "pm1-refill2": (dict(refill=2), dict(MEGA, pmode=1, refilled=1)),
    "pm2-force_geom1": (dict(force_geom=1, merged=0), dict(MEGA, pmode=2)),
    "pm3-force_geom2": (dict(force_geom=2), dict(MEGA, pmode=3)),
    "pm4-merged": (dict(force_geom=1, merged=1), dict(MEGA, pmode=4)),
    "pm0-lockstep": (dict(pair_trace=0), dict(MEGA, pmode=0)),
    "wavefront": (dict(wavefront=1), dict(render_mode=1)),
    "async_lanes": (dict(async_lanes=1), dict(render_mode=2)),
}
DEFAULTS = dict(stage=7, sample_sync=-1, refill=1, force_geom=-1, merged=-1, pair_trace=1, wavefront=0, async_lanes=0, split=2)


class GpuLab:
    def __init__(self, P, O):
        self.P, self.O = P, O
        self.lab = FT.Lab(P, O)                       # the statement's side: a host-only scene and its world
        self.scenes = {}
        self.defaults = None

    def scene(self, W, H, ctx):
        if (W, H, ctx) not in self.scenes:
            P = self.P
            if ctx == "whole":
                s = P.Scene(W, H)
            elif ctx == "band":
                s = P.Scene(W, H, tile_y0=FT.CONTEXTS[ctx][0], tile_rows=FT.CONTEXTS[ctx][1])
            else:
                s = P.Scene(W, H, interleave=FT.CONTEXTS[ctx])
            FT.build_lab(P, s)
            s.setMaxBounceDepth(1)
            s.setDenoiserEnabled(False)
            s.setBloomEnabled(False)
            s.initBlueNoise()
            s.uploadToGPU()
            assert s.tile_rows == len(FT.context_rows(H, ctx))
            if self.defaults is None:
                self.defaults = {k: s.get_option(k) for k in DEFAULTS}
            self.scenes[(W, H, ctx)] = s
        return self.scenes[(W, H, ctx)]

    def render(self, key, options=None, states=None):
        """the case's frame under `options`; -> (buffers, facts)"""
        P = self.P
        c, W, H, ctx, f, spp = key
        s = self.scene(W, H, ctx)
        FT.set_camera(s, c)
        s.setPerfSamplesPerPixel(spp)
        for k, v in (options or {}).items():
            s.set_option(k, v)
        try:
            s.write_rng(FT.case_states(self.O, key) if states is None else states)
            s.setFrameCount(f)
            s.render_to_host()
            facts = {k: s.get_option(k) for k in ("render_mode", "pmode", "sample_sync_eff", "refilled", "split_eff")}
            got = dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                       object_id=s.read(P.BUF_OBJECT_ID), rng=s.read(P.BUF_RNG))
        finally:
            for k in (options or {}):
                s.set_option(k, self.defaults[k])
        return got, facts

    def close(self):
        for s in self.scenes.values():
            s.close()
        self.lab.close()


@pytest.fixture(scope="module")
def gpu(P, O):
    g = GpuLab(P, O)
    yield g
    g.close()


def judge(gpu, key, got, what, fr=None, states=None):
    fr = gpu.lab.frame(key) if fr is None else fr
    states = FT.case_states(gpu.O, key) if states is None else states
    j = FT.judge_frame(fr, got, states, got["rng"], gpu.O)
    worst = {q: float(u.max()) for q, u in j["units"].items()}
    print(f"{what} {FT.case_name(key)}: " + " ".join(f"{q} {v:.3g}" for q, v in worst.items()) + f" decided {fr['decided'].mean():.4f}")
    for q, b in j["bad"].items():
        assert not b.any(), f"{what}, {FT.case_name(key)}: {q} differs at decided pixels {np.flatnonzero(b)[:8]}"
    for q, v in worst.items():
        assert v <= FT.TOL[q], f"{what}, {FT.case_name(key)}: {q} is {v:.3g} units off (allowed {FT.TOL[q]})"
    assert fr["decided"].mean() >= 1.0 - FT.MAX_UNDECIDED


# ---------------------------------------------------------------------------------------------------- ptrt_camera_rays
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}-{c}" for w, h, c in SHAPES])
def test_camera_rays_are_the_statements(gpu, shape):
    """Every pixel's primary ray of samples 0 and 1 at the four frame indices, straight from ptrt_camera_rays."""
    W, H, ctx = shape
    s = gpu.scene(W, H, ctx)
    FT.set_camera(s, "pinhole")
    for f, _ in FT.FRAMES:
        fr = gpu.lab.frame(("pinhole", W, H, ctx, f, 2))
        for sample in (0, 1):
            o, d = s.camera_rays(f, sample)
            s.sync()
            r = fr["samples"][sample]
            j = FT.judge_rays(r, dict(origin=o.cpu().numpy(), direction=d.cpu().numpy()), r["ray_decided"])
            print(f"{W}x{H}-{ctx} frame {f} sample {sample}: origin {j['origin'].max():.3g} direction {j['direction'].max():.3g} units")
            assert j["origin"].max() <= FT.TOL["origin"] and j["direction"].max() <= FT.TOL["direction"], (f, sample)
            assert r["ray_decided"].mean() > 0.999


def test_camera_rays_refuse_a_lens(gpu, P):
    """include/ptrt.h: a thin lens's sample belongs to the pixel's generator stream, not to the camera."""
    s = gpu.scene(70, 33, "whole")
    FT.set_camera(s, "lens")
    with pytest.raises(P.PtrtError):
        s.camera_rays(0, 0)
    FT.set_camera(s, "pinhole")


# ---------------------------------------------------------------------------------------------------- the frame kernels
@pytest.mark.parametrize("camera", ["pinhole", "lens"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}-{c}" for w, h, c in SHAPES])
@pytest.mark.parametrize("loop", list(LOOPS))
def test_frames_are_the_statements(gpu, loop, shape, camera):
    options, facts = LOOPS[loop]
    W, H, ctx = shape
    for f, spp in FT.FRAMES:
        key = (camera, W, H, ctx, f, spp)
        got, seen = gpu.render(key, options)
        for k, v in facts.items():
            assert seen[k] == v, f"{loop}, {FT.case_name(key)}: {k} is {seen[k]}, the shape named reports {v} ({seen})"
        judge(gpu, key, got, loop)


@pytest.mark.parametrize("camera", ["pinhole", "lens"])
@pytest.mark.parametrize("size", FT.SIZES, ids=[f"{w}x{h}" for w, h in FT.SIZES])
def test_split_launches_are_the_statements(gpu, P, O, size, camera):
    """A frame dealt to two concurrent launches: only a frame that follows another into a different device target is
    (csrc/ptrt_render.hip.h), so frame 14 renders first and frame 15 is the one judged, from the states frame 14 leaves."""
    import torch
    W, H = size
    key = (camera, W, H, "whole", 14, 3)
    s = gpu.scene(W, H, "whole")
    FT.set_camera(s, camera)
    s.setPerfSamplesPerPixel(3)
    s.set_option("split", 2)
    tgt = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    states = FT.case_states(O, key)
    s.write_rng(states)
    s.setFrameCount(14)
    s.render_to_device(tgt[0].data_ptr())
    s.render_to_device(tgt[1].data_ptr())
    seen = {k: s.get_option(k) for k in ("render_mode", "pmode", "split_eff")}
    s.sync()
    s.set_option("split", gpu.defaults["split"])
    got = dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH), object_id=s.read(P.BUF_OBJECT_ID),
               rng=s.read(P.BUF_RNG))
    assert seen == dict(render_mode=0, pmode=1, split_eff=2), seen
    first = gpu.lab.frame(key)
    between = FT.states_after(O, states, first["draws"])
    fr = FT.frame(gpu.lab.world, FT.case_camera(key), W, H, np.arange(H), 15, 3, between)
    fr["decided"] = fr["decided"] & first["decided"]           # where frame 14 is undecided the states between are unknown
    judge(gpu, (camera, W, H, "whole", 15, 3), got, "split=2", fr=fr, states=between)


@pytest.mark.parametrize("loop", ["pm1-stage7-sync1", "pm1-refill2", "pm0-lockstep", "wavefront", "async_lanes"])
@pytest.mark.parametrize("key", FT.cases(far=True), ids=[FT.case_name(k) for k in FT.cases(far=True)])
def test_an_all_miss_view_leaves_the_states_the_statement_says(gpu, O, key, loop):
    options, facts = LOOPS[loop]
    got, seen = gpu.render(key, options)
    fr = gpu.lab.frame(key)
    for k, v in facts.items():
        assert seen[k] == v, (loop, k, seen)
    states, dec = FT.case_states(O, key), fr["decided"]
    assert (got["object_id"] == -1).all() and (got["depth"] == np.float32(1e30)).all() and not got["normal"].any()
    if key[0] == "far_pinhole":
        assert dec.all() and np.array_equal(got["rng"], states), "a pinhole draws nothing"
    else:
        assert dec.mean() > 0.99 and np.array_equal(got["rng"][dec], FT.states_after(O, states, fr["draws"])[dec])
    judge(gpu, key, got, loop)
