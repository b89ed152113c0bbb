"""The lightmap filter on the device (ptrt_atlas_filter; Scene.atlas_filter).  Every comparison is bytes, tolerance 0, with the
numpy restatement (tests/atlas_filter_restatement.py): atlases on both sides of every tile and halo, pass counts up to 8, real
guides from Scene.atlas_texels with and without an instance transform, synthetic ones with holes that carry NaN and +-1e30,
zero normals and two meshes, images whose invalid texels carry NaN and infinity and whose `valid` is not always 1, every
normal_power and sigmas at which all, some and none of the off-centre taps survive -- under each `atlas_filter_tile`.  Guard
rows stay, the guides are only read, the other buffer holds the pass before; what must be refused is refused with every byte
untouched; frames around a call do not notice it; a bake with the filter between scatter and dilation holds together."""
import ctypes as C

import numpy as np
import pytest

import atlas_filter_restatement as R
from test_irradiance_gpu import PATTERN, buffers, dev

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (1, 7), (7, 1), (9, 7), (33, 17), (70, 5)]
PASSES = (1, 2, 3, 5, 8)
TILE_OPTIONS = (-1, 0, 1)
TILED_STEPS = 3  # the LDS tile fits steps 1, 2 and 4
SIGMAS = {"all": (100.0, 100.0), "some": (0.75, 0.125), "none": (0.01, 0.125)}  # for guides on a pitch of 0.25

_lab = {}


def lab(P):
    """the Cornell scene and a cube with an instance transform"""
    if "s" not in _lab:
        s = P.Scene(64, 64)
        P.scenes.cornell(s)
        c = s.addCube(P.Material((0.8, 0.8, 0.8), 0.5))
        s.setPosition(c, (0.0, 0.0, -3.0))
        s.setRotation(c, (0.3, 0.5, 0.1))
        s.setInstanceScale(c, (1.2, 1.2, 1.2))
        s.uploadToGPU()
        _lab["s"], _lab["cube"] = s, c
    return _lab["s"]


@pytest.fixture(scope="module", autouse=True)
def _close_lab():
    yield
    if "s" in _lab:
        _lab.pop("s").close()
        _lab.clear()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def synthetic(w, h, seed, pitch=0.25):
    """(records, image): a wavy sheet on a `pitch` grid in two meshes, unit normals, a few zero normals; holes (mesh -1) whose
    positions and normals are NaN, +-1e30 or infinite; valid colours in (-1, 3), `valid` 1.0, 2.5 or -1.0; invalid texels
    (valid 0.0 or -0.0) carrying NaN and infinities."""
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:h, 0:w]
    pos = (np.stack([ii * pitch, jj * pitch, np.zeros((h, w))], -1) + rng.normal(0, pitch * 0.1, (h, w, 3))).reshape(-1, 3)
    nrm = np.stack([rng.normal(0, 0.2, (h, w)), rng.normal(0, 0.2, (h, w)), np.ones((h, w))], -1).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    n = w * h
    nrm[rng.random(n) < 0.04] = 0.0
    mesh = rng.integers(0, 2, n) * 3
    hole = rng.random(n) < 0.15
    mesh[hole] = -1
    rec = R.records(pos, nrm, mesh, face=rng.integers(0, 50, n))
    poison = F([[np.nan, 1e30, -1e30], [1e30, 1e30, 1e30], [np.inf, -np.inf, np.nan], [0, 0, 0]]).view(np.int32)
    k = np.flatnonzero(hole)
    rec[k, 0:3] = poison[rng.integers(0, 4, len(k))]
    rec[k, 4:7] = poison[rng.integers(0, 4, len(k))]
    img = (rng.random((n, 4)) * 4 - 1).astype(F)
    img[:, 3] = rng.choice(F([1.0, 1.0, 1.0, 2.5, -1.0]), n)
    bad = np.flatnonzero(rng.random(n) < 0.15)
    img[bad, 0:3] = F([[np.nan, np.inf, -np.inf], [np.inf, 1.0, np.nan], [3.0, 4.0, 5.0]])[rng.integers(0, 3, len(bad))]
    img[bad, 3] = rng.choice(F([0.0, -0.0]), len(bad))
    if n > 1:  # the first texel live, whatever the draw
        rec[0] = R.records(pos[:1], [[0.0, 0.0, 1.0]], [0])[0]
        img[0] = [0.5, 1.5, 2.5, 1.0]
    return rec, img.reshape(h, w, 4)


def check(s, rec, img, passes, sd, sp, k, what, options=TILE_OPTIONS):
    """the device's bytes under every option against the restatement's; returns the restatement's result"""
    h, w, _ = img.shape
    want = R.filter(rec, img, passes, sd, sp, k)
    before = R.filter(rec, img, passes - 1, sd, sp, k)
    d_rec = dev(rec)
    try:
        for opt in options:
            s.set_option("atlas_filter_tile", opt)
            a = dev(img)
            out = s.atlas_filter(d_rec, a, passes, sd, sp, k)
            assert (out is a) == (passes % 2 == 0), "the result is in the second buffer for odd pass counts, in the image for even"
            eff = s.get_option("atlas_filter_tile_eff")
            assert eff in {0: (0,), 1: (min(passes, TILED_STEPS),), -1: range(0, min(passes, TILED_STEPS) + 1)}[opt], (opt, eff)
            got = out.cpu().numpy()
            bad = np.argwhere(bits(got) != bits(want))
            assert bad.size == 0, (f"{what}, {w} x {h}, {passes} passes, sigmas {sd} / {sp}, power {k}, atlas_filter_tile {opt}: "
                                   f"{len(bad)} words differ, first (j, i, word) {bad[:4].tolist()}: "
                                   f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")
            if passes % 2:  # the image is then the buffer that does not hold the result: the pass before
                assert np.array_equal(bits(a.cpu().numpy()), bits(before)), f"{what}: the other buffer, atlas_filter_tile {opt}"
        assert np.array_equal(d_rec.cpu().numpy(), rec), "the guides were written"
    finally:
        s.set_option("atlas_filter_tile", -1)
    return want


# ---- 1. bytes against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_guides_equal_the_restatement(P, w, h):
    s = lab(P)
    rec, img = synthetic(w, h, w * 100 + h)
    for passes in PASSES:
        want = check(s, rec, img, passes, *SIGMAS["some"], 2, "synthetic")
        live = (rec[:, 7].reshape(h, w) >= 0) & (img[:, :, 3] != 0)
        assert np.isfinite(want[live]).all() and np.array_equal(bits(want)[~live], bits(img)[~live])
        assert np.array_equal(bits(want[:, :, 3]), bits(img[:, :, 3])), "valid is copied through bit for bit"
    if w * h >= 63:
        assert not np.array_equal(bits(want)[live], bits(img)[live]), "nothing was filtered"


@pytest.mark.parametrize("normal_power", [0, 2, 7])
@pytest.mark.parametrize("sigmas", list(SIGMAS))
def test_parameters(P, sigmas, normal_power):
    s = lab(P)
    w, h = 33, 17
    rec, img = synthetic(w, h, 7)
    sd, sp = SIGMAS[sigmas]
    want = check(s, rec, img, 3, sd, sp, normal_power, sigmas)
    # what the names promise, on one pass of the restatement: the weight that reaches a live texel from the others
    one = R.filter(rec, img, 1, sd, sp, normal_power)
    live = (rec[:, 7].reshape(h, w) >= 0) & (img[:, :, 3] != 0) & (rec[:, 4:7].reshape(h, w, 3) != 0).any(-1)
    moved = (bits(one)[live] != bits(img)[live]).any(-1).mean()
    if sigmas == "none":
        assert np.abs(one[live, 0:3] - img[live, 0:3]).max() <= 2 ** -22 * 3.0, "only the centre tap: (w c) / w"
    else:
        assert moved > 0.9
    assert want.shape == img.shape


@pytest.mark.parametrize("mesh", ["box", "transformed cube"])
def test_real_guides_equal_the_restatement(P, mesh):
    L = P.lightmap
    s = lab(P)
    m = 6 if mesh == "box" else _lab["cube"]
    uv, w, h = L.triangle_charts(12, 8)
    d_rec = s.atlas_texels(m, dev(uv), w, h)
    rec = d_rec.cpu().numpy()
    assert (rec[:, 7] == m).sum() >= 120
    pitch = L.texel_pitch(d_rec, w, h)
    assert pitch > 0 and abs(pitch - L.texel_pitch(rec, w, h)) <= 1e-6 * pitch
    sd, sp = L.filter_sigmas(pitch)
    rng = np.random.default_rng(3)
    img = np.zeros((h * w, 4), F)
    idx = L.covered(rec)
    img[idx, 0:3] = rng.random((len(idx), 3)) + 1.0
    img[idx, 3] = 1.0
    img = img.reshape(h, w, 4)
    for passes in (1, 3):
        want = check(s, rec, img, passes, sd, sp, 2, mesh)
    cov = rec[:, 7].reshape(h, w) >= 0
    assert want[cov, 0:3].std() < img[cov, 0:3].std() * 0.8, "the noise did not go down"


# ---- 2. guard rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 2, 5])
def test_guard_rows(P, passes):
    import torch
    s = lab(P)
    vp = C.c_void_p
    w, h, G = 33, 17, 3
    rec, img = synthetic(w, h, 21)
    n = w * h
    want, before = R.filter(rec, img, passes, 0.75, 0.125, 2), R.filter(rec, img, passes - 1, 0.75, 0.125, 2)
    for opt in TILE_OPTIONS:
        s.set_option("atlas_filter_tile", opt)
        gt = torch.full((n + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
        ga, gb = (torch.full((n + 2 * G, 4), PATTERN, dtype=torch.int32, device="cuda") for _ in range(2))
        gt[G:G + n] = dev(rec)
        ga[G:G + n] = dev(img.reshape(n, 4)).view(torch.int32)
        assert P.lib.ptrt_atlas_filter(s.ctx, vp(gt[G:].data_ptr()), vp(ga[G:].data_ptr()), vp(gb[G:].data_ptr()), w, h, passes,
                                       0.75, 0.125, 2) == P.PTRT_OK
        s.sync()
        for t in (gt, ga, gb):
            assert (t[:G] == PATTERN).all() and (t[G + n:] == PATTERN).all(), "a write outside the atlas"
        assert np.array_equal(gt[G:G + n].cpu().numpy(), rec), "the guides were written"
        res, other = (gb, ga) if passes % 2 else (ga, gb)
        assert np.array_equal(res[G:G + n].cpu().numpy().view(np.uint32), bits(want).reshape(n, 4))
        assert np.array_equal(other[G:G + n].cpu().numpy().view(np.uint32), bits(before).reshape(n, 4)), "the pass before"
    s.set_option("atlas_filter_tile", -1)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    flt = P.lib.ptrt_atlas_filter
    vp = C.c_void_p
    INVALID = -1
    w, h = 9, 7
    n = w * h
    rec, img = synthetic(w, h, 2)
    s = lab(P)
    c = s.ctx
    gt = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    ia, ib = (torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda") for _ in range(2))
    pt, pa, pb = (vp(x.data_ptr()) for x in (gt, ia, ib))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((x == PATTERN).all()) for x in (gt, ia, ib))

    host = np.zeros((n, 8), np.float32)
    hp = vp(host.ctypes.data)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    D = dict(c=c, t=pt, a=pa, b=pb, w=w, h=h, passes=3, sd=0.75, sp=0.125, k=2)
    order = ("c", "t", "a", "b", "w", "h", "passes", "sd", "sp", "k")
    nan, inf = float("nan"), float("inf")
    bad = [dict(passes=0), dict(passes=9), dict(passes=-1), dict(k=-1), dict(k=8),
           dict(sd=nan), dict(sd=inf), dict(sd=-inf), dict(sd=0.0), dict(sd=-0.75), dict(sp=nan), dict(sp=inf), dict(sp=0.0), dict(sp=-0.125),
           dict(sd=2e19, passes=1),            # r * r overflows
           dict(sd=1e18, passes=8),            # ... at step 128 only
           dict(sd=1e-23, passes=1),           # r * r is 0 in fp32
           dict(sp=2e19), dict(sp=1e-23),      # and sigma_plane's square
           dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 14, h=(1 << 14) + 1), dict(w=2 ** 31 - 1, h=2 ** 31 - 1),
           dict(t=None), dict(a=None), dict(b=None),
           dict(t=vp(gt.data_ptr() + 4)), dict(a=vp(ia.data_ptr() + 4)), dict(b=vp(ib.data_ptr() + 8)),
           dict(b=pa), dict(b=vp(ia.data_ptr() + 16)), dict(a=pt), dict(b=pt), dict(b=vp(gt.data_ptr() + n * 16)),
           dict(a=vp(gt.data_ptr() + n * 32 - 16)), dict(t=vp(ia.data_ptr() + 16 * (n - 1))),
           dict(t=hp), dict(a=hp), dict(b=hp),
           dict(t=tail(n * 32 - 32)), dict(a=tail(n * 16 - 16)), dict(b=tail(n * 16 - 16)),
           dict(c=None)]
    for change in bad:
        args = dict(D, **change)
        assert flt(*[args[x] for x in order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_atlas_filter" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    assert flt(c, pt, pa, pb, w, h, 1, 1e18, 0.125, 2) == P.PTRT_OK   # (1e18 is fine while the step is 1)
    hip.hipFree(block)
    # a context with no scene uploaded filters; a destroyed one refuses
    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    d_rec, a, b = dev(rec), dev(img), torch.empty((h, w, 4), device="cuda")
    assert flt(ctx, vp(d_rec.data_ptr()), vp(a.data_ptr()), vp(b.data_ptr()), w, h, 3, 0.75, 0.125, 2) == P.PTRT_OK
    assert P.lib.ptrt_sync(ctx) == P.PTRT_OK
    assert np.array_equal(bits(b.cpu().numpy()), bits(R.filter(rec, img, 3, 0.75, 0.125, 2)))
    P.lib.ptrt_destroy(ctx)
    assert flt(ctx, vp(d_rec.data_ptr()), vp(a.data_ptr()), vp(b.data_ptr()), w, h, 3, 0.75, 0.125, 2) == INVALID
    # the binding
    for kw in (dict(passes=0), dict(passes=9), dict(normal_power=8), dict(sigma_distance=0.0), dict(sigma_plane=nan)):
        with pytest.raises(ValueError):
            s.atlas_filter(**dict(dict(texels=d_rec, image=a, passes=1, sigma_distance=0.75, sigma_plane=0.125), **kw))
    with pytest.raises(ValueError):
        s.atlas_filter(d_rec[:-1], a, 1, 0.75, 0.125)
    with pytest.raises(ValueError):
        s.atlas_filter(d_rec.cpu(), a, 1, 0.75, 0.125)
    with pytest.raises(P.PtrtError):
        s.atlas_filter(d_rec, a, 1, 2e19, 0.125)
    for v in (2, -7):
        s.set_option("atlas_filter_tile", v)
        assert s.get_option("atlas_filter_tile") == (1 if v > 0 else -1)
    s.set_option("atlas_filter_tile", -1)


# ---- 4. side effects and ordering ----------------------------------------------------------------------------------------------
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
            uv, w, h = P.lightmap.triangle_charts(12, 8)
            rec = s.atlas_texels(6, dev(uv), w, h)
            img = s.atlas_filter(rec, torch.rand((h, w, 4), device="cuda").round(), 3, 1.0, 0.2)
            torch.cuda.synchronize()
            assert img.shape == (h, w, 4)
            assert s.kernel_ms_history().tobytes() == hist
            assert np.array_equal(s.read(P.BUF_RNG), rng) and s.stats() == stats
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), n_hist=len(s.kernel_ms_history())))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["n_hist"] == b["n_hist"]


def test_a_call_queued_behind_texels_and_scatter_sees_them(P):
    import torch
    L = P.lightmap
    s = lab(P)
    uv, w, h = L.triangle_charts(12, 8)
    d_uv = dev(uv)
    first = s.atlas_texels(6, d_uv, w, h)
    idx = L.covered(first)                       # (synchronises: everything below is queued without one)
    want_rec = first.cpu().numpy()
    values = torch.rand((len(idx), 3), device="cuda") + 0.5
    rec = torch.full((w * h, 8), PATTERN, dtype=torch.int32, device="cuda")
    img = torch.zeros((h * w, 4), device="cuda")
    s.atlas_texels(6, d_uv, w, h, out=rec)       # on the context's stream
    img[idx, 0:3] = values                       # on torch's
    img[idx, 3] = 1.0
    src = img.clone()
    out = s.atlas_filter(rec, img.reshape(h, w, 4), 3, 1.0, 0.2)
    got, rec_h, src_h = out.cpu().numpy(), rec.cpu().numpy(), src.cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(rec_h, want_rec) and src_h[:, :, 3].sum() == len(idx)
    assert np.array_equal(bits(got), bits(R.filter(rec_h, src_h, 3, 1.0, 0.2, 2)))


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
def test_a_bake_with_the_filter_between_scatter_and_dilation(P):
    L = P.lightmap
    s = lab(P)
    c = _lab["cube"]
    uv, w, h = L.triangle_charts(12, 12, gutter=3)
    rec = s.atlas_texels(c, dev(uv), w, h)
    idx = L.covered(rec)
    pos, nrm = L.atlas_inputs(rec)
    n, k = len(idx), 16
    direct = s.query_direct(pos, nrm, dev(L.hammersley2(4)))
    gather = s.query_irradiance(pos, nrm, dev(L.hammersley2(k)), s.init_rng_states(7, 0, n * k), samples=1, max_depth=3)
    total = L.total_irradiance(direct, gather)
    img = L.scatter(dev(total), idx, w, h).reshape(h, w, 4)
    src = img.cpu().numpy()
    sd, sp = L.filter_sigmas(L.texel_pitch(rec, w, h))
    filtered = s.atlas_filter(rec, img, 3, sd, sp)
    f = filtered.cpu().numpy()
    rec_h = rec.cpu().numpy()
    assert np.array_equal(bits(f), bits(R.filter(rec_h, src, 3, sd, sp, 2))), "the restatement on the read-back inputs"
    cov = (rec_h[:, 7] >= 0).reshape(h, w)
    assert np.array_equal(bits(f)[~cov], bits(src)[~cov]), "an uncovered texel changed"
    assert not np.array_equal(bits(f)[cov], bits(src)[cov])
    out = s.atlas_dilate(filtered, 2).cpu().numpy()
    assert np.isfinite(out).all() and (out[cov, 3] != 0).all()
    assert np.array_equal(bits(out)[cov], bits(f)[cov]), "dilation leaves covered texels alone"
    assert (out[:, :, 3] != 0).sum() > cov.sum()
