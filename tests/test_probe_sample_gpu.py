"""Probe volumes read at surface points on the device (ptrt_probe_sample, ptrt_query_probe_light; Scene.probe_sample /
query_probe_light).  Every comparison with the numpy restatement (tests/probe_sample_restatement.py) is words, tolerance 0:
query_probe_light equals probe_sample over the point and normal columns of query_closest's records and both equal the
restatement, under every traversal the queries have, at the batch sizes round a wave, in both modes, with and without a
normal bias, over volumes of one probe, of one cell, with an axis of one probe, and one that covers the middle third of the box
so that every hit is clamped onto it; the probe records are synthetic, some all NaN, some without variance.  Independently of
that statement, a constant field comes back as pi L and a linear one as the linear function at the point.  Caller points that
are no hits -- a non-finite one among them --, refusals with every byte untouched, frames that do not notice a call, and a
volume baked by query_probes and viewed through the camera.

(The one exception to "words": IEEE 754 leaves a NaN's payload and sign open, and TRILINEAR has no test that keeps a NaN probe
out, so where the restatement's irradiance is a NaN the device's has to be one -- any one.  The NaN rows are placed so that
this arises only where a test says so.)"""
import ctypes as C
import math

import numpy as np
import pytest

import probe_sample_restatement as R
from test_irradiance_gpu import PATTERN, buffers, dev
from test_probe_sample import (CONSTANT_L, check_constant, check_linear, constant_case, linear_case)
from test_ray_query_gpu import VARIANTS, ray_set

pytestmark = pytest.mark.gpu

F = np.float32
NS = (1, 63, 64, 65, 4097)
MODES = ("trilinear", "visibility")
BIASES = (0.0, 0.05)
# the Cornell scene's box (the root of its top-level tree: the walls are slabs 0.1 thick, so their inner faces lie inside it)
BOX_LO, BOX_HI = (-5.05, -5.05, -10.05), (5.05, 5.05, 0.0)
VOLUMES = ("one", "cell", "flat", "middle")
RAY_SEED, PROBE_SEED = 11, 3  # chosen on the CPU, with the oracle's hits: test_the_volumes_are_not_vacuous holds for them

_scene = {}


def scene(P):
    if "cornell" not in _scene:
        s = P.Scene(64, 64)
        P.scenes.cornell(s)
        s.uploadToGPU()
        _scene["cornell"] = s
    return _scene["cornell"]


@pytest.fixture(scope="module", autouse=True)
def _close_scene():
    yield
    for s in _scene.values():
        s.close()
    _scene.clear()


def volume(P, name):
    """'one' probe, one 'cell' of 2 x 2 x 2, a 'flat' 3 x 2 x 1 -- all over the box --, and 4 x 4 x 4 over its 'middle' third"""
    V = P.probes.ProbeVolume.from_corners
    lo, hi = np.float64(BOX_LO), np.float64(BOX_HI)
    if name == "middle":
        third = (hi - lo) / 3.0
        return V(lo + third, hi - third, (4, 4, 4))
    return V(lo, hi, dict(one=(1, 1, 1), cell=(2, 2, 2), flat=(3, 2, 1))[name])


def probe_records(vol, mode, seed=PROBE_SEED):
    """(rows, 32) float32, synthetic: sh in [-1, 2], mean_distance 0.2 .. 2 spacings, mean_distance_sq = mean^2 + |noise|; one
    boundary row in eight (at least one where there are eight rows) without variance; every interior row -- no footprint of a
    clamped point reaches one with a positive weight -- all NaN, and for VISIBILITY, whose selection keeps a NaN out, one
    boundary row in sixteen as well"""
    rng = np.random.default_rng(seed * 100 + vol.rows)
    rec = np.zeros((vol.rows, 32), F)
    rec[:, :27] = rng.uniform(-1.0, 2.0, (vol.rows, 27))
    sp = float(np.mean(vol.spacing))
    rec[:, 27] = rng.uniform(0.2, 2.0, vol.rows) * sp
    rec[:, 28] = rec[:, 27] * rec[:, 27] + np.abs(rng.normal(size=vol.rows)).astype(F) * F(0.1 * sp * sp)
    rec[:, 29] = 1.0
    nx, ny, nz = vol.counts
    i, j, k = np.arange(vol.rows) % nx, np.arange(vol.rows) // nx % ny, np.arange(vol.rows) // (nx * ny)
    interior = (i > 0) & (i < nx - 1) & (j > 0) & (j < ny - 1) & (k > 0) & (k < nz - 1)
    edge = np.flatnonzero(~interior)
    pick = rng.permutation(edge)
    flat = pick[:len(edge) // 8 if len(edge) >= 16 else (1 if len(edge) >= 8 else 0)]
    rec[flat, 28] = rec[flat, 27] * rec[flat, 27]
    rec[interior] = np.nan
    if R.MODES[mode] == R.VISIBILITY:
        rec[pick[len(pick) - len(edge) // 16:] if len(edge) >= 16 else []] = np.nan
    return rec


def assert_rows_equal(got, want, what):
    g, x = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, np.int32), np.asarray(want, np.int32)
    assert g.shape == x.shape, what
    both_nan = np.zeros(g.shape, bool)
    both_nan[:, 0:3] = np.isnan(g[:, 0:3].view(F)) & np.isnan(x[:, 0:3].view(F))
    bad = np.argwhere((g != x) & ~both_nan)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} words differ, first (row, word) {bad[:6].tolist()}: "
                           f"{R.fields(g[bad[0][0]:bad[0][0] + 1])} vs {R.fields(x[bad[0][0]:bad[0][0] + 1])}")


def columns(hits):
    """the point and normal columns of query_closest's (n, 16) int32 rows, as contiguous float32 tensors"""
    import torch
    f = hits.view(torch.float32)
    return f[:, 2:5].contiguous(), f[:, 5:8].contiguous()


def check_all(P, s, o, d, names, what):
    """both entry points against the restatement over the device's own hit records, for the volumes `names`, both modes and both
    biases; returns (hit records, {(volume, mode, bias): rows})"""
    do, dd = dev(o), dev(d)
    hits = s.query_closest(do, dd)
    pos, nrm = columns(hits)
    h = hits.cpu().numpy()
    hit = h[:, 0] != 0
    rows = {}
    for name in names:
        vol = volume(P, name)
        for mode in MODES:
            rec = probe_records(vol, mode)
            dp = dev(rec)
            for bias in BIASES:
                want = R.sample_hits(h, vol, rec, mode, bias)
                key = f"{what}, {name}, {mode}, bias {bias}"
                assert_rows_equal(s.query_probe_light(do, dd, vol, dp, mode, bias), want, key + ": query_probe_light")
                # probe_sample knows no hits: its rows for the hits' points, with face and mesh -1
                loose = want.copy()
                loose[:, 6:8] = -1
                got = s.probe_sample(pos, nrm, vol, dp, mode, bias).cpu().numpy()
                assert_rows_equal(got[hit], loose[hit], key + ": probe_sample")
                rows[(name, mode, bias)] = want
    return h, rows


# ---- 1. bytes against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
def test_both_entry_points_equal_the_restatement(P, fg, pt):
    s = scene(P)
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    try:
        for n in NS:
            o, d = ray_set("cornell", n, RAY_SEED + n if n != 4097 else RAY_SEED)
            check_all(P, s, o, d, VOLUMES, f"n {n}")
            # every traversal runs: the per-lane walk without pairs, PMODE 1, 2 and 3 by force_geom
            assert s.get_option("query_pmode") == (0 if pt == 0 else {-1: 1, 1: 2, 2: 3}[fg])
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)


# ---- 2. the byte test is not vacuous ---------------------------------------------------------------------------------------------
def vacuity(h, rows, vol_of, rec_of):
    """the conditions of test_the_volumes_are_not_vacuous over hit records h (n, 16) int32 and the restatement's rows; a function
    of its own so that the seeds can be chosen from the oracle's hits without a device"""
    hit = h[:, 0] != 0
    assert (~hit).sum() >= 20
    pts = h[:, 2:5].view(F)
    out = {}
    for (name, mode, bias), r in rows.items():
        f = R.fields(r)
        lit = f["weight"] > 0
        assert (r[~hit] == R.MISS).all(), "a miss without the miss record"
        assert lit[hit].mean() >= 0.5, f"{name}, {mode}: {lit[hit].mean():.2f} of the hits have a weight"
        assert np.isfinite(f["irradiance"][lit]).all() and np.isfinite(f["weight"]).all(), f"{name}, {mode}: a NaN row came through"
        assert np.isnan(rec_of(name, mode)).any() == (name == "middle"), "NaN rows where the volume has room for them"
        out[(name, mode, bias)] = dict(lit=float(lit[hit].mean()), all8=int((f["used"] == 255).sum()))
    for mode in MODES:
        for bias in BIASES:
            assert out[("cell", mode, bias)]["all8"] >= 20, f"{mode}: no footprint with all eight corners used"
    vol = vol_of("middle")
    lo, hi = vol.corners()
    outside = hit & ((pts < lo) | (pts > hi)).any(axis=1)
    assert outside.sum() >= 20
    for bias in BIASES:
        e = R.evaluate(pts[hit], h[hit, 5:8].view(F), vol, rec_of("middle", "visibility"), "visibility", bias)
        rejected = ((e["wt"] > 0) & ~e["sel"][:, :, 1] & np.isfinite(e["mean"])).any(axis=1)
        skipped_nan = ((e["wt"] > 0) & np.isnan(e["mean"])).any(axis=1)
        assert rejected.sum() >= 20, "the visibility branch (r > mean) never ran"
        assert skipped_nan.sum() >= 20, "no NaN row was skipped by visibility's selection"
        out[("middle", "rejected", bias)] = int(rejected.sum())
    return out


def test_the_volumes_are_not_vacuous(P):
    """over the 4097 rays the restatement itself lights, rejects by visibility, uses all eight corners, clamps and misses"""
    s = scene(P)
    o, d = ray_set("cornell", 4097, RAY_SEED)
    h, rows = check_all(P, s, o, d, VOLUMES, "the 4097 rays")
    print(vacuity(h, rows, lambda name: volume(P, name), lambda name, mode: probe_records(volume(P, name), mode)))


# ---- 3. the analytic checks, on the device's output ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_constant_field_is_pi_L(P, mode):
    s = scene(P)
    vol, pts, nrm, rec = constant_case(P)
    rows = s.probe_sample(dev(pts), dev(nrm), vol, dev(rec), mode, 0.05).cpu().numpy()
    lit = check_constant(rows, vol, pts, nrm, rec, mode, 0.05)
    assert lit == len(pts) if mode == "trilinear" else lit > len(pts) // 2
    assert CONSTANT_L.min() > 0


def test_a_linear_field_is_the_linear_function(P):
    s = scene(P)
    vol, pts, nrm, rec = linear_case(P)
    check_linear(s.probe_sample(dev(pts), dev(nrm), vol, dev(rec), "trilinear", 0.0).cpu().numpy(), vol, pts, nrm, rec)


# ---- 4. caller points that are no hits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_probe_sample_on_caller_points(P, n):
    """points in and far round the middle volume, a non-finite one in every seventh row: face and mesh are -1, a non-finite P gives
    the no-cell record.  Nothing is read out of range: probe_light returns on a non-finite P before an index exists, and every
    index it forms afterwards is a conversion of g, which is clamped into [0, count - 1] first (and is never a NaN: P and the
    origin are finite, the spacing positive and finite, so the quotient is a number or an infinity the clamp takes)."""
    s = scene(P)
    vol = volume(P, "middle")
    rng = np.random.default_rng(40 + n)
    lo, hi = vol.corners()
    pts = (lo + (rng.random((n, 3)) * 3 - 1) * (hi - lo)).astype(F)
    pts[3::7] *= F(1e30)
    bad = np.arange(n) % 7 == 6
    pts[bad, rng.integers(0, 3, bad.sum())] = rng.choice(F([np.nan, np.inf, -np.inf]), bad.sum())
    nrm = rng.normal(size=(n, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    for mode in MODES:
        rec = probe_records(vol, mode)
        got = s.probe_sample(dev(pts), dev(nrm), vol, dev(rec), mode, 0.05)
        assert_rows_equal(got, R.sample(pts, nrm, -1, -1, 1, vol, rec, mode, 0.05), f"n {n}, {mode}")
        g = got.cpu().numpy()
        assert (g[:, 6:8] == -1).all() and (g[bad] == np.int32([0, 0, 0, 0, -1, 0, -1, -1])).all() and (g[~bad, 4] >= 0).all()
        assert (g[~bad, 4] < vol.rows).all()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    smp, qry = P.lib.ptrt_probe_sample, P.lib.ptrt_query_probe_light
    vp = C.c_void_p
    OK, INVALID, NOT_READY = P.PTRT_OK, -1, -4
    s = scene(P)
    c = s.ctx
    n = 70
    o, d = ray_set("cornell", n, RAY_SEED)
    vol = volume(P, "middle")
    rec = probe_records(vol, "visibility")
    do, dd, dp = dev(o), dev(d), dev(rec)
    hits = s.query_closest(do, dd)
    pos, nrm = columns(hits)
    out = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    big = torch.full((4096, 8), PATTERN, dtype=torch.int32, device="cuda")  # something every input fits into, to overlap with
    host = np.zeros((4096, 8), np.float32)
    hp = vp(host.ctypes.data)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    def p(t, off=0):
        return vp(t.data_ptr() + off)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == PATTERN).all()) and bool((big == PATTERN).all()) and not host.any()

    def desc(origin=None, spacing=None, counts=None):
        return P.ProbeVolumeDesc((C.c_float * 3)(*(vol.origin if origin is None else origin)),
                                 (C.c_float * 3)(*(vol.spacing if spacing is None else spacing)),
                                 (C.c_int32 * 3)(*(vol.counts if counts is None else counts)))

    keep = []  # the descriptors stay alive while the calls read them

    def vol_p(**kw):
        keep.append(desc(**kw))
        return C.cast(C.pointer(keep[-1]), vp)

    inf, nan = float("inf"), float("nan")
    common = dict(c=c, n=n, vol=vol_p(), probes=p(dp), mode=1, bias=C.c_float(0.05), out=p(out))
    S = dict(common, a=p(pos), b=p(nrm))
    Q = dict(common, a=p(do), b=p(dd))
    order = ("c", "a", "b", "n", "vol", "probes", "mode", "bias", "out")
    cases = [dict(n=-1), dict(vol=None), dict(probes=None), dict(out=None), dict(a=None), dict(b=None),
             dict(vol=vol_p(counts=(0, 4, 4))), dict(vol=vol_p(counts=(4, -1, 4))), dict(vol=vol_p(counts=(4, 4, 0))),
             dict(vol=vol_p(counts=(4096, 4096, 2))), dict(vol=vol_p(counts=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))),
             dict(vol=vol_p(counts=(1 << 16, 1 << 16, 1 << 16))),
             dict(vol=vol_p(spacing=(0.0, 1.0, 1.0))), dict(vol=vol_p(spacing=(1.0, -1.0, 1.0))), dict(vol=vol_p(spacing=(1.0, 1.0, inf))),
             dict(vol=vol_p(spacing=(nan, 1.0, 1.0))), dict(vol=vol_p(origin=(nan, 0.0, 0.0))), dict(vol=vol_p(origin=(0.0, inf, 0.0))),
             dict(vol=vol_p(origin=(0.0, 0.0, -inf))),
             dict(bias=C.c_float(-1e-3)), dict(bias=C.c_float(nan)), dict(bias=C.c_float(inf)), dict(mode=2), dict(mode=-1),
             dict(probes=p(dp, 4)), dict(probes=p(dp, 8)), dict(out=p(out, 4)), dict(out=p(big, 8)), dict(a=p(do, 2)), dict(b=p(dd, 1)),
             dict(probes=hp), dict(out=hp), dict(a=hp), dict(b=hp),
             dict(probes=tail(64 * 128 - 128)), dict(out=tail(n * 32 - 32)), dict(a=tail(n * 12 - 4)), dict(b=tail(n * 12 - 4)),
             dict(vol=vol_p(counts=(128, 128, 2)), probes=block),  # a volume of more rows than the probes' allocation holds
             dict(out=p(dp)), dict(out=p(dp, 128 * 63 + 96)), dict(out=p(big), probes=p(big, n * 32 - 16)),
             dict(out=p(big), a=p(big, n * 32 - 4)), dict(out=p(big, 16), b=p(big)), dict(c=None)]
    for fn, name, D in ((smp, b"ptrt_probe_sample", S), (qry, b"ptrt_query_probe_light", Q)):
        for change in cases:
            args = dict(D, **change)
            assert fn(*[args[x] for x in order]) == INVALID, (name, change)
            if "c" not in change:
                assert name in P.lib.ptrt_last_error(c), (name, change)
        assert untouched(), name
        args = dict(D, n=0)
        assert fn(*[args[x] for x in order]) == OK and untouched(), "n == 0 is accepted and does nothing"
        assert fn(*[D[x] for x in order]) == OK
        s.sync()
        want = R.sample_hits(hits.cpu().numpy(), vol, rec, "visibility", 0.05)
        hit = want[:, 7] >= 0
        if fn is smp:
            want[:, 6:8] = -1
        assert_rows_equal(out[torch.from_numpy(hit).cuda()], want[hit], f"{name}: the call that is in order")
        out.fill_(PATTERN)
    hip.hipFree(block)
    # the calls that are in order write their rows and no others
    G = 3
    for fn, D in ((smp, S), (qry, Q)):
        guarded = torch.full((n + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
        args = dict(D, out=p(guarded, 32 * G), mode=0)
        assert fn(*[args[x] for x in order]) == OK
        s.sync()
        assert (guarded[:G] == PATTERN).all() and (guarded[G + n:] == PATTERN).all(), "a write outside the rows"
    # before geometry is uploaded: the fused query needs it, the sampler does not; a destroyed context
    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    args = dict(Q, c=ctx)
    assert qry(*[args[x] for x in order]) == NOT_READY and b"ptrt_query_probe_light" in P.lib.ptrt_last_error(ctx)
    assert untouched()
    args = dict(S, c=ctx)
    assert smp(*[args[x] for x in order]) == OK
    torch.cuda.synchronize()
    want = R.sample_hits(hits.cpu().numpy(), vol, rec, "visibility", 0.05)
    hit = torch.from_numpy(want[:, 7] >= 0).cuda()
    want[:, 6:8] = -1
    assert_rows_equal(out[hit], want[hit.cpu().numpy()], "probe_sample on a context without geometry")
    out.fill_(PATTERN)
    for fn, D in ((smp, S), (qry, Q)):
        args = dict(D, c=ctx, mode=7)
        assert fn(*[args[x] for x in order]) == INVALID
    P.lib.ptrt_destroy(ctx)
    for fn, D in ((smp, S), (qry, Q)):
        args = dict(D, c=ctx)
        assert fn(*[args[x] for x in order]) == INVALID
    assert untouched()
    # the binding
    good = dict(volume=vol, probes=dp)
    for change in (dict(mode="nearest"), dict(probes=dp[:, :31]), dict(probes=dp.cpu()), dict(probes=dp[:63]), dict(probes=dp.to(torch.float64)),
                   dict(volume=None), dict(normal_bias=-1.0), dict(normal_bias=float("nan")),
                   dict(out=torch.zeros((n + 1, 8), dtype=torch.int32, device="cuda")),
                   dict(out=torch.zeros((n, 8), dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            s.probe_sample(pos, nrm, **dict(good, **change))
        with pytest.raises(ValueError):
            s.query_probe_light(do, dd, **dict(good, **change))
    with pytest.raises(ValueError):
        s.probe_sample(pos, nrm[:-1], **good)
    with pytest.raises(ValueError):
        s.query_probe_light(do, dd[:, :2], **good)
    mine = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    assert s.query_probe_light(do, dd, out=mine, **good) is mine and s.probe_sample(pos[:0], nrm[:0], **good).shape == (0, 8)


# ---- 6. neighbours ---------------------------------------------------------------------------------------------------------------
def test_a_call_between_frames_changes_nothing(P, O, blue_noise):
    import torch
    from common import render_both
    runs = []
    for with_call in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        rng = s.read(P.BUF_RNG)
        stats = s.stats()
        if with_call:
            vol = volume(P, "cell")
            rec = dev(probe_records(vol, "visibility"))
            o, d = ray_set("cornell", 4097, RAY_SEED)
            rows = s.query_probe_light(dev(o), dev(d), vol, rec, "visibility", 0.05)
            pos, nrm = columns(s.query_closest(dev(o), dev(d)))
            again = s.probe_sample(pos, nrm, vol, rec, "visibility", 0.05)
            torch.cuda.synchronize()
            hit = rows[:, 7] >= 0
            assert torch.equal(rows[hit][:, :6], again[hit][:, :6]) and bool((rows[:, 3] != 0).any())
            assert s.kernel_ms_history().tobytes() == hist
            assert np.array_equal(s.read(P.BUF_RNG), rng) and s.stats() == stats
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), hist=s.kernel_ms_history()))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and len(a["hist"]) == len(b["hist"])


# ---- 7. the loop closes ----------------------------------------------------------------------------------------------------------
BAKE_INSET = 0.5  # the baked grid stands this far inside the box: checked on the CPU, from the oracle's probe records (below)


def bake_volume(P):
    lo, hi = np.float64(BOX_LO) + BAKE_INSET, np.float64(BOX_HI) - BAKE_INSET
    return P.probes.ProbeVolume.from_corners(lo, hi, (4, 4, 4))


def test_a_baked_volume_viewed_through_the_camera(P):
    """a 4 x 4 x 4 ProbeVolume baked by query_probes (64 Fibonacci directions, 1 sample), then camera_rays at 64 x 64,
    query_probe_light in 'visibility' mode and shade_probe_light.  No brightness is asserted -- no tolerance for "looks right"
    can be derived --; the mean irradiance is printed beside query_irradiance's at the same points, for the record."""
    import torch
    L = P.probes
    s = scene(P)
    vol = bake_volume(P)
    dirs = L.fibonacci_sphere(64)
    baked = s.query_probes(dev(vol.positions()), dev(dirs), s.init_rng_states(7, 0, vol.rows * 64), samples=1, max_depth=4, max_distance=30.0)
    assert baked.shape == (64, 32) and bool(torch.isfinite(baked).all())
    o, d = s.camera_rays(0)
    assert o.shape == (64 * 64, 3)
    bias = 0.05
    rows = s.query_probe_light(o, d, vol, baked, "visibility", bias)
    hits = s.query_closest(o, d)
    pos, nrm = columns(hits)
    loose = s.probe_sample(pos, nrm, vol, baked, "visibility", bias)
    torch.cuda.synchronize()
    f = L.probe_light_fields(rows)
    hit = f["mesh"] >= 0
    assert float(hit.float().mean()) > 0.5
    assert torch.equal(rows[hit][:, :6], loose[hit][:, :6]), "the fused bytes are not the unfused ones"
    assert torch.equal(f["mesh"], hits[:, 8]) and torch.equal(f["face"], hits[:, 12])
    assert bool((rows[~hit] == torch.tensor(R.MISS.tolist(), dtype=torch.int32, device="cuda")).all())
    assert_rows_equal(rows, R.sample_hits(hits.cpu().numpy(), vol, baked.cpu().numpy(), "visibility", bias), "the samples of the view")
    assert bool(torch.isfinite(f["irradiance"]).all()) and bool(torch.isfinite(f["weight"]).all())
    lit = float((f["weight"][hit] > 0).float().mean())
    assert lit >= 0.9, f"only {lit:.3f} of the camera's hits are lit by the volume"
    meshes = s.flatten().contents.mesh_count
    view = L.shade_probe_light(rows, torch.full((meshes, 3), 0.7, device="cuda"))
    assert view.shape == (64 * 64, 3) and bool(torch.isfinite(view).all()) and float(view[hit].min()) >= 0.0
    assert np.array_equal(L.shade_probe_light(rows.cpu().numpy(), np.full((meshes, 3), 0.7, F)).view(np.int32),
                          view.cpu().numpy().view(np.int32)), "arrays and tensors shade alike"
    n = int(hit.sum())
    k = 64
    gather = s.query_irradiance(pos[hit].contiguous(), nrm[hit].contiguous(), dev(P.lightmap.hammersley2(k)), s.init_rng_states(9, 0, n * k),
                                samples=1, max_depth=4)
    print(f"lit {lit:.3f}; mean irradiance from the probes {f['irradiance'][hit].mean(0).tolist()}, "
          f"from query_irradiance at the same points {(math.pi * gather[:, 0:3]).mean(0).tolist()}")
