"""Direct light at lightmap texels on the device (ptrt_query_direct, ptrt_direct_rays; Scene.query_direct).  Everything about
the sums and the visibility at tolerance 0, compared as bytes: a texel's row must be the numpy restatement
(tests/direct_restatement.py) of the weights direct_rays writes and of what query_occluded answers for direct_rays' rays --
under every traversal, for every segment width and group size at which padding, a partial last group, a group boundary and the
chunked path can go wrong, on a grid smaller than the batch; closed forms; the sample against a float64 statement of the
reference's light sampling; no trace left in the frames around a call; what must be refused is refused with everything
untouched."""
import ctypes as C

import numpy as np
import pytest

import direct_restatement as D
import irradiance_restatement as R
import path_truth as PT
from test_irradiance_gpu import PATTERN, assert_rows_equal, buffers, dev, texels
from test_ray_query_gpu import VARIANTS, build

pytestmark = pytest.mark.gpu

W = H = 64
F = np.float32

_cache = {}

# four lights beside Cornell's own hard point light: a sphere, a hard cone, a soft cone with a radius, the sun
LAB_LIGHTS = 5


def lab(P):
    s = P.Scene(W, H)
    P.scenes.cornell(s)
    s.addPointLight((2.0, 3.0, -4.0), (0.8, 0.8, 1.0), 5.0, 15.0, 0.3)
    s.addSpotLight((-3.0, 4.0, -6.0), (0.3, -1.0, 0.1), (1.0, 1.0, 1.0), 12.0, 0.3, 0.3, 30.0, 0.0)
    s.addSpotLight((1.0, 4.5, -7.0), (0.0, -1.0, 0.0), (1.0, 0.7, 0.4), 15.0, 0.2, 0.6, 25.0, 0.2)
    s.addDirectionalLight((-0.4, -1.0, -0.3), (1.0, 0.96, 0.9), 3.0)
    s.uploadToGPU()
    assert s.lightCount() == LAB_LIGHTS
    return s


def slabs(P):
    """Three texels on the plane y = 0, each under a light 4 above it and a slab half way: one that transmits 0.9, one that
    transmits 0.1, and an opaque one whose edge lies on the line from the third texel to its light, a sphere of radius 0.5."""
    s = P.Scene(W, H)
    for x, z, tr in ((-3.0, 0.0, 0.9), (3.0, 0.0, 0.1), (1.0, -6.0, 0.0)):
        m = s.addCube(P.Material((0.8, 0.8, 0.8), 0.5, 0.0, transmission=tr, ior=1.4))
        s.scale(m, (2.0, 0.1, 2.0))
        s.moveTo(m, (x, 2.0, z))
    s.addPointLight((-3.0, 4.0, 0.0), (1.0, 1.0, 1.0), 10.0, 20.0)
    s.addPointLight((3.0, 4.0, 0.0), (1.0, 1.0, 1.0), 10.0, 20.0)
    s.addPointLight((0.0, 4.0, -6.0), (1.0, 1.0, 1.0), 10.0, 20.0, 0.5)
    s.setCamera((0, 3, 12), (0, 1, -2), (0, 1, 0), 45.0)
    s.uploadToGPU()
    return s


def scene(P, name):
    if name not in _cache:
        _cache[name] = lab(P) if name == "lab" else slabs(P) if name == "slabs" else build(P, name, W, H)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cached():
    yield
    for s in _cache.values():
        s.close()
    _cache.clear()


def unfused(s, pos, nrm, s2, ph=None, lights=None, offset=1e-4):
    """the restatement of direct_rays' weights and of query_occluded on direct_rays' rays; a ray that is not walked is
    replaced by one of length 0, which nothing blocks"""
    import torch
    k = 1 if s2 is None else len(s2)
    count = s.lightCount() if lights is None else lights[1]
    o, d, t, w = s.direct_rays(dev(pos), dev(nrm), dev(s2), phases=dev(ph), offset=offset, lights=lights)
    assert o.shape == d.shape == w.shape == (len(pos) * count * k, 3) and t.shape == (len(pos) * count * k,)
    walked = (w > 0).any(dim=1)
    o = torch.where(walked[:, None], o, torch.zeros_like(o)).contiguous()
    d = torch.where(walked[:, None], d, torch.tensor([0.0, 1.0, 0.0], device="cuda").expand_as(d)).contiguous()
    t = torch.where(walked, t, torch.zeros_like(t)).contiguous()
    flags = s.query_occluded(o, d, t).cpu().numpy()
    assert not flags[~walked.cpu().numpy()].any()
    return D.restate(w.cpu().numpy(), flags, k, count)


def fused(s, pos, nrm, s2, ph=None, lights=None, offset=1e-4):
    return s.query_direct(dev(pos), dev(nrm), dev(s2), phases=dev(ph), offset=offset, lights=lights).cpu().numpy()


# ---- 1. the restatement, as bytes ---------------------------------------------------------------------------------------------
def check_restatement(P, s, name):
    n, k = 37, 4
    pos, nrm = texels(P, name, n)
    s2, ph = P.lightmap.hammersley2(k), P.lightmap.texel_phases(n, 3)
    want = unfused(s, pos, nrm, s2, ph)
    got = fused(s, pos, nrm, s2, ph)
    pm = s.get_option("query_pmode")
    assert_rows_equal(got, want, name)
    assert got[:, :3].any() and not got[:, 5:].any()
    f = P.direct_fields(got)
    assert (f["lit_fraction"] >= 0).all() and (f["lit_fraction"] + f["shadowed_fraction"] <= 1).all()
    assert (f["lit_fraction"] > 0).any()
    return pm, got


@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
def test_cornell_equals_the_restatement_under_every_variant(P, fg, pt):
    s = scene(P, "cornell")
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    try:
        pm, got = check_restatement(P, s, "cornell")
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)
    assert pm == (0 if pt == 0 else {-1: 1, 1: 2, 2: 3}[fg])
    assert (got[:, 4] > 0).any()  # the boxes do shadow some floor texels


@pytest.mark.parametrize("name", ["showcase", "many", "fluid"])
def test_scenes_equal_the_restatement(P, name):
    s = scene(P, name)
    pm, got = check_restatement(P, s, name)
    if name == "many":
        assert pm == 3
    if name == "showcase":
        assert s.lightCount() == 6  # Q = 24: w = 32, two texels per wave, eight dead lanes per segment


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------
SHAPES = {1: ((0, 1), 1), 2: ((0, 2), 1), 3: ((0, 3), 1), 4: ((1, 4), 1), 5: ((0, 5), 1), 8: ((1, 4), 2), 16: ((0, 4), 4),
          17: ((1, 1), 17), 32: ((0, 4), 8), 33: ((1, 3), 11), 63: ((0, 3), 21), 64: ((1, 4), 16), 65: ((0, 5), 13),
          130: ((0, 5), 26)}


@pytest.mark.parametrize("Q", sorted(SHAPES))
def test_shapes(P, Q):
    """Per term count, with g = 64 / w texels per wave (1 beyond 64 terms): 1, g - 1, g, g + 1 and 2 g + 1 texels -- segment
    padding, a partial last group, a full one, a group boundary, and more than two groups."""
    s = scene(P, "lab")
    lights, k = SHAPES[Q]
    assert lights[1] * k == Q
    g = 64 // R.width(Q) if Q <= 64 else 1
    s2 = P.lightmap.hammersley2(k)
    lit = False
    for n in sorted({1, g - 1, g, g + 1, 2 * g + 1} - {0}):
        pos, nrm = texels(P, "cornell", n)
        ph = P.lightmap.texel_phases(n, Q)
        want = unfused(s, pos, nrm, s2, ph, lights)
        got = fused(s, pos, nrm, s2, ph, lights)
        assert_rows_equal(got, want, f"{n} x {Q}")
        lit = lit or bool(got[:, :3].any())
    assert lit


def test_more_groups_than_workgroups(P):
    import torch
    s = scene(P, "lab")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lights, k = (0, 4), 4        # Q = 16: four texels per wave
    n = 4 * (cus + 3)            # n_cus + 3 groups: with persist 1 the grid is one wave per CU, three of them stride twice
    pos, nrm = texels(P, "cornell", n)
    rs = np.random.RandomState(5)
    pos = (pos + rs.uniform(-0.04, 0.04, pos.shape) * (1 - np.abs(nrm))).astype(np.float32)  # (moved within their planes)
    s2 = P.lightmap.hammersley2(k)
    want = unfused(s, pos, nrm, s2, None, lights)
    s.set_option("persist", 1)
    try:
        narrow = fused(s, pos, nrm, s2, None, lights)
    finally:
        s.set_option("persist", 0)
    wide = fused(s, pos, nrm, s2, None, lights)
    assert_rows_equal(narrow, want, "persist 1 vs the restatement")
    assert_rows_equal(wide, want, "the default grid vs the restatement")
    assert len(np.unique(wide[:, :3], axis=0)) > n // 2  # other places, other texels


# ---- 3. closed forms ----------------------------------------------------------------------------------------------------------
def test_cornell_closed_forms(P):
    s = scene(P, "cornell")
    up, down = [0, 1, 0], [0, -1, 0]
    # right under the light (0, 4.5, -5), clear of both boxes; under the tall box; the first texel again, facing away
    pos = np.float32([[0, -4.95, -5], [-1.5, -4.95, -6], [0, -4.95, -5]])
    nrm = np.float32([up, up, down])
    got = fused(s, pos, nrm, None)
    f = P.direct_fields(got)
    # toLight = (0, 4.5 - -4.95, 0): every float32 operation of the sample, in the header's order (the dot products' two
    # zero terms are exact, so the chain of fused multiply-adds rounds once, as the plain product does)
    y = F(4.5) - F(-4.95)
    dist = np.sqrt(y * y)
    Ly = y / dist
    att = F(20.0) / (F(20.0) + dist)
    att = att * att
    radiance = np.float32([1.0, 0.9, 0.8]) * F(3.0)
    want = ((radiance * att) * Ly) / F(1.0)
    assert want.dtype == np.float32 and Ly == 1
    assert np.array_equal(f["irradiance"][0].view(np.uint32), ((F(0.0) + want) / F(1.0)).view(np.uint32))
    assert f["lit_fraction"][0] == 1 and f["shadowed_fraction"][0] == 0
    assert not f["irradiance"][1].any() and f["lit_fraction"][1] == 0 and f["shadowed_fraction"][1] == 1
    assert not f["irradiance"][2].any() and f["lit_fraction"][2] == 0 and f["shadowed_fraction"][2] == 0
    assert not got[:, 5:].any()
    assert P.lightmap.penumbra_texels(got).tolist() == [False, False, False]
    # samples2=None is the one point of hammersley2(1); a hard light reads neither number
    assert_rows_equal(fused(s, pos, nrm, P.lightmap.hammersley2(1)), got, "samples2=None")
    assert_rows_equal(fused(s, pos, nrm, np.float32([[0.9, 0.1]]), ph=np.float32([0.5, 0.25, 0.75])), got, "a hard light's samples")
    # no lights asked for: rows of zero bytes
    import torch
    out = torch.full((3, 8), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    assert s.query_direct(dev(pos), dev(nrm), lights=(0, 0), out=out) is out
    assert not out.view(torch.int32).cpu().numpy().any()
    assert not s.query_direct(dev(pos), dev(nrm), lights=(1, 0)).view(torch.int32).cpu().numpy().any()
    o, d, t, w = s.direct_rays(dev(pos), dev(nrm), lights=(0, 0))
    assert o.shape == (0, 3) and t.shape == (0,)


def test_outside_a_spot_cone(P):
    s = scene(P, "lab")
    # light 2: a cone of 0.3 rad from (-3, 4, -6) about (0.3, -1, 0.1): the far corner of the floor is outside it, the floor
    # under it inside
    pos = np.float32([[4.0, -4.95, -1.0], [-0.4, -4.95, -5.2]])
    nrm = np.float32([[0, 1, 0], [0, 1, 0]])
    f = P.direct_fields(fused(s, pos, nrm, None, lights=(2, 1)))
    assert f["lit_fraction"][0] == 0 and f["shadowed_fraction"][0] == 0 and not f["irradiance"][0].any()
    assert f["lit_fraction"][1] + f["shadowed_fraction"][1] == 1


def test_transmission_and_penumbra(P):
    s = scene(P, "slabs")
    up = [0, 1, 0]
    pos, nrm = np.float32([[-3, 0, 0], [3, 0, 0], [0, 0, -6]]), np.float32([up, up, up])
    a = P.direct_fields(fused(s, pos[0:1], nrm[0:1], None, lights=(0, 1)))
    assert a["lit_fraction"][0] == 1 and a["shadowed_fraction"][0] == 0 and a["irradiance"][0].all()   # transmission 0.9: no shadow
    b = P.direct_fields(fused(s, pos[1:2], nrm[1:2], None, lights=(1, 1)))
    assert b["lit_fraction"][0] == 0 and b["shadowed_fraction"][0] == 1 and not b["irradiance"][0].any()  # 0.1: a shadow
    s2 = P.lightmap.hammersley2(16)
    rows = fused(s, pos[2:3], nrm[2:3], s2, lights=(2, 1))
    c = P.direct_fields(rows)
    print(f"half hidden sphere light: lit {c['lit_fraction'][0]}, shadowed {c['shadowed_fraction'][0]}")
    assert 0 < c["lit_fraction"][0] < 1 and c["lit_fraction"][0] + c["shadowed_fraction"][0] == 1
    assert P.lightmap.penumbra_texels(rows).tolist() == [True]
    assert_rows_equal(rows, unfused(s, pos[2:3], nrm[2:3], s2, lights=(2, 1)), "penumbra")
    # a light with a radius contributes radiance * solid angle: every unblocked sample the same density
    assert c["irradiance"][0].all()


def test_directional_light_has_no_end(P):
    s = scene(P, "fluid")
    pos, nrm = texels(P, "fluid", 12)
    o, d, t, w = s.direct_rays(dev(pos), dev(nrm), dev(P.lightmap.hammersley2(2)))
    assert (t.cpu().numpy() == F(1e30)).all() and t.shape == (24,)
    d = d.cpu().numpy()
    assert (d == d[0]).all() and abs(float(d[0].astype(np.float64) @ d[0]) - 1.0) < 1e-6 and d[0, 1] > 0


# ---- 4. the sample against float64 --------------------------------------------------------------------------------------------
def test_sample_against_the_float64_statement(P):
    """ptrt_direct_rays on a context that holds lights and nothing else: L, tmax and the weight within direct_restatement.
    margins of statement64 on the samples it decides; the origin exact."""
    import torch
    arr, pos, nrm, s2, ph = D.statement_inputs(P)
    nl, k, n = len(D.STATEMENT_LIGHTS), D.STATEMENT_SHADOW, D.STATEMENT_TEXELS
    rays = n * nl * k
    vp = C.c_void_p
    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    try:
        assert P.lib.ptrt_upload_lights(ctx, arr, nl) == P.PTRT_OK
        tp, tn, ts, tph = dev(pos), dev(nrm), dev(s2), dev(ph)
        o, d, w = (torch.zeros((rays, 3), device="cuda") for _ in range(3))
        t = torch.zeros(rays, device="cuda")
        off = F(1e-4)
        rc = P.lib.ptrt_direct_rays(ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                    C.c_float(off), 0, nl, vp(o.data_ptr()), vp(d.data_ptr()), vp(t.data_ptr()), vp(w.data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(ctx)
        assert P.lib.ptrt_sync(ctx) == P.PTRT_OK
        # a range of the lights: the same rays, light by light
        o2, d2, w2 = (torch.zeros((n * 3 * k, 3), device="cuda") for _ in range(3))
        t2 = torch.zeros(n * 3 * k, device="cuda")
        rc = P.lib.ptrt_direct_rays(ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                    C.c_float(off), 2, 3, vp(o2.data_ptr()), vp(d2.data_ptr()), vp(t2.data_ptr()), vp(w2.data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(ctx)
        assert P.lib.ptrt_sync(ctx) == P.PTRT_OK
    finally:
        P.lib.ptrt_destroy(ctx)
    o, d, t, w = o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(w2.cpu().numpy().reshape(n, 3, k, 3).view(np.uint32), w.reshape(n, nl, k, 3)[:, 2:5].view(np.uint32))
    assert np.array_equal(d2.cpu().numpy().reshape(n, 3, k, 3).view(np.uint32), d.reshape(n, nl, k, 3)[:, 2:5].view(np.uint32))
    # the origin: position + 1e-4f * normal, the product rounded and then the sum -- with a unit normal the path tracer's own
    # shadow origin (hit.point + hit.normal * 1e-4f), bit for bit
    want_o = (pos + off * nrm).astype(np.float32)
    assert (off * nrm).dtype == np.float32
    assert np.array_equal(o.view(np.uint32), np.repeat(want_o, nl * k, axis=0).view(np.uint32))
    assert np.array_equal(o.view(np.uint32), D.origins32(pos, nrm, off, nl * k).view(np.uint32))
    st, decided = D.statement64(pos, nrm, PT.lights64(arr, nl), 0, nl, s2, ph, k)
    share = 1.0 - decided.mean()
    print(f"direct_rays: {share:.4f} of {rays} samples undecided")
    assert share <= 0.02
    E_L, E_t, E_w = D.margins(st)
    light = np.tile(np.repeat(np.arange(nl), k), n)
    for name, got, want, E in (("L", d, st["L"], E_L[:, None]), ("tmax", t, st["tmax"], E_t), ("weight", w, st["weight"], E_w)):
        err = np.abs(got.astype(np.float64) - want)
        ok = decided if err.ndim == 1 else decided[:, None]
        ratio = np.where(ok, err / np.maximum(E, 1e-300), 0.0)
        ratio = np.where(ok & (err == 0), 0.0, ratio)
        worst = np.unravel_index(np.argmax(ratio), ratio.shape)[0]
        print(f"direct_rays: {name}: worst error / margin {ratio.max():.3f} (light {light[worst]}, error "
              f"{np.max(err[worst]):.3e}); largest error {np.where(ok, err, 0.0).max():.3e}; per light " +
              ", ".join(f"{ratio[light == j].max():.3f}" for j in range(nl)))
        assert ratio.max() <= 1.0, name
    # walked where the statement's weight is clear of zero, not walked where its cosine is clear below it
    yes, no = decided & (st["weight"].max(axis=1) > 1e-6), decided & (st["cos"] < -1e-6)
    assert yes.any() and no.any() and D.walked32(w)[yes].all() and not D.walked32(w)[no].any()
    assert not w[no].any()


# ---- 5. no trace --------------------------------------------------------------------------------------------------------------
def test_guard_rows(P):
    """`d_out` and the four ray targets between pattern rows, before and after: the rows stay."""
    import torch
    s = scene(P, "lab")
    vp = C.c_void_p
    for n, lights, k in ((5, (0, 3), 4), (3, (0, 5), 14)):  # segments of 16 with a partial group; the chunked path with a tail chunk
        Q = lights[1] * k
        pos, nrm = texels(P, "cornell", n)
        s2, ph = P.lightmap.hammersley2(k), P.lightmap.texel_phases(n, 2)
        batch = fused(s, pos, nrm, s2, ph, lights)
        G = 3
        out = torch.full((n + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
        ro, rd, rw = (torch.full((n * Q + 2 * G, 3), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3))
        rt = torch.full((n * Q + 2 * G,), PATTERN, dtype=torch.int32, device="cuda")
        tp, tn, ts, tph = dev(pos), dev(nrm), dev(s2), dev(ph)
        rc = P.lib.ptrt_query_direct(s.ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                     C.c_float(1e-4), lights[0], lights[1], vp(out[G:].data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        rc = P.lib.ptrt_direct_rays(s.ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                    C.c_float(1e-4), lights[0], lights[1], vp(ro[G:].data_ptr()), vp(rd[G:].data_ptr()),
                                    vp(rt[G:].data_ptr()), vp(rw[G:].data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        s.sync()
        for name, t, rows in (("out", out, n), ("origins", ro, n * Q), ("directions", rd, n * Q), ("tmax", rt, n * Q),
                              ("weights", rw, n * Q)):
            assert (t[:G] == PATTERN).all() and (t[G + rows:] == PATTERN).all(), f"{name}: a write outside the batch"
        assert_rows_equal(out[G:G + n].view(torch.float32).cpu().numpy(), batch, "raw call")
        o, d, t, w = s.direct_rays(tp, tn, ts, phases=tph, lights=lights)
        assert torch.equal(ro[G:G + n * Q], o.view(torch.int32)) and torch.equal(rd[G:G + n * Q], d.view(torch.int32))
        assert torch.equal(rt[G:G + n * Q], t.view(torch.int32)) and torch.equal(rw[G:G + n * Q], w.view(torch.int32))


def test_a_bake_between_frames_changes_nothing(P, O, blue_noise):
    import torch
    from common import render_both
    runs = []
    for with_bake in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        lhist = [x.tobytes() for x in s.launch_ms_history()]
        rng = s.read(P.BUF_RNG)
        stats = s.stats()
        if with_bake:
            pos, nrm = texels(P, "cornell", 70)
            rows = s.query_direct(dev(pos), dev(nrm), dev(P.lightmap.hammersley2(4)))
            o, d, t, w = s.direct_rays(dev(pos), dev(nrm), dev(P.lightmap.hammersley2(4)))
            torch.cuda.synchronize()
            assert rows.shape == (70, 8) and rows[:, :3].any() and o.shape == d.shape == w.shape == (70 * 4, 3)
            assert s.kernel_ms_history().tobytes() == hist
            assert [x.tobytes() for x in s.launch_ms_history()] == lhist
            assert np.array_equal(s.read(P.BUF_RNG), rng) and s.stats() == stats
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), n_hist=len(s.kernel_ms_history()),
                         n_lhist=len(s.launch_ms_history()[0])))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["n_hist"] == b["n_hist"] and a["n_lhist"] == b["n_lhist"]


def test_a_second_light_upload_is_seen(P):
    s = build(P, "cornell", 32, 32)
    pos, nrm = texels(P, "cornell", 9)
    first = fused(s, pos, nrm, None)
    s.moveLightTo(0, (2.0, 3.0, -3.0))          # uploaded by the next call's commit, no sync in between
    second = fused(s, pos, nrm, None)
    assert_rows_equal(second, unfused(s, pos, nrm, None), "behind ptrt_upload_lights")
    assert not np.array_equal(first[:, :3], second[:, :3])
    s.close()


def awning(x0):
    """two triangles at y = 3 over x0 .. x0 + 6, z -8 .. 4"""
    a, b, c, d = (x0, 3.0, -8.0), (x0 + 6.0, 3.0, -8.0), (x0 + 6.0, 3.0, 4.0), (x0, 3.0, 4.0)
    return np.float32([a + b + c, a + c + d])


def test_a_bake_sees_a_refit_without_a_sync(P):
    s = P.Scene(64, 48)
    w, ship = P.scenes.fluid(s, cells=24, t=0.0, ship_segments=10)
    roof = s.addTriangles(awning(-6.0), P.Material((0.5, 0.5, 0.5), 0.5))
    s.uploadToGPU()
    pos, nrm = P.lightmap.quad_texels((-6.0, -1.5, 2.0), (12.0, 0, 0), (0, 0, -8.0), 5, 5)  # under the ship and the water, looking up
    assert np.array_equal(nrm[0], np.float32([0, 1, 0]))
    before = fused(s, pos, nrm, None)
    s.setVertices(w, P.scenes.water_vertices(24, 0.9))
    s.setVertices(roof, awning(0.0).reshape(-1, 3))
    s.refitObjectChanges()
    unsynced = fused(s, pos, nrm, None)
    s.sync()
    synced = fused(s, pos, nrm, None)
    assert_rows_equal(unsynced, synced, "behind ptrt_refit")
    assert_rows_equal(synced, unfused(s, pos, nrm, None), "the refitted scene vs the restatement")
    assert synced[:, 3].any() and synced[:, 4].any()       # the water lets the sun through, the ship and the awning do not
    assert not np.array_equal(before[:, 3], synced[:, 3])  # the awning moved: another shadow
    s.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    q, rays = P.lib.ptrt_query_direct, P.lib.ptrt_direct_rays
    vp, cf = C.c_void_p, C.c_float
    INVALID, NOT_READY = -1, -4
    n, k = 3, 8
    pos = torch.tensor([[0.0, -4.95, -5.0], [0.3, -4.95, -2.0], [1.0, -4.95, -3.0]], device="cuda")  # on the Cornell floor
    nrm = torch.tensor([0.0, 1.0, 0.0], device="cuda").repeat(n, 1)
    s2 = dev(P.lightmap.hammersley2(k))
    ph = torch.zeros(n, device="cuda")
    out = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    ro, rd, rw = (torch.full((n * k, 3), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3))
    rt = torch.full((n * k,), PATTERN, dtype=torch.int32, device="cuda")
    pp, pn, ps2, pph, pout, pro, prd, prt, prw = (vp(x.data_ptr()) for x in (pos, nrm, s2, ph, out, ro, rd, rt, rw))
    off = cf(1e-4)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((x == PATTERN).all()) for x in (out, ro, rd, rt, rw))

    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    assert q(ctx, pp, pn, n, ps2, k, pph, off, 0, 0, pout) == NOT_READY      # no geometry
    assert b"ptrt_query_direct" in P.lib.ptrt_last_error(ctx)
    assert q(ctx, pp, pn, n, ps2, k, pph, off, 0, 1, pout) == INVALID        # (and no lights: the range is refused first)
    assert rays(ctx, pp, pn, n, ps2, k, pph, off, 0, 1, pro, prd, prt, prw) == INVALID
    assert rays(ctx, pp, pn, n, ps2, k, pph, off, 0, 0, pro, prd, prt, prw) == P.PTRT_OK   # no lights, no rays: nothing launched
    assert untouched()
    P.lib.ptrt_destroy(ctx)
    assert q(ctx, pp, pn, n, ps2, k, pph, off, 0, 0, pout) == INVALID        # a destroyed context
    assert rays(ctx, pp, pn, n, ps2, k, pph, off, 0, 0, pro, prd, prt, prw) == INVALID
    s = build(P, "cornell", 32, 32)
    c = s.ctx
    host = np.zeros((n * k, 8), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((n, 8), dtype=torch.int32).pin_memory()
    # device memory that ends before the call's last element: an allocation of the runtime's own ends where it ends
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    inf, nan = float("inf"), float("nan")
    big = 2 ** 31 - 1
    Qa = dict(c=c, pos=pp, nrm=pn, n=n, s2=ps2, k=k, ph=pph, off=off, first=0, count=1, out=pout)
    order = ("c", "pos", "nrm", "n", "s2", "k", "ph", "off", "first", "count", "out")
    bad_q = [dict(n=-1), dict(k=0), dict(k=-3), dict(first=-1), dict(count=-1), dict(count=2), dict(first=1), dict(first=big, count=big),
             dict(pos=None), dict(nrm=None), dict(s2=None), dict(out=None),                                          # NULL
             dict(pos=hp), dict(nrm=hp), dict(s2=hp), dict(ph=hp), dict(out=hp),                                     # host memory
             dict(out=vp(pinned.data_ptr())),                                                                        # pinned host memory
             dict(pos=tail(n * 12 - 12)), dict(nrm=tail(n * 12 - 12)), dict(s2=tail(k * 8 - 8)), dict(ph=tail(n * 4 - 4)),
             dict(out=tail(n * 32 - 4)),                                                                             # short buffers
             dict(off=cf(nan)), dict(off=cf(inf)), dict(off=cf(-inf)), dict(c=None)]
    for change in bad_q:
        args = dict(Qa, **change)
        assert q(*[args[a] for a in order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_query_direct" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    Rr = dict(c=c, pos=pp, nrm=pn, n=n, s2=ps2, k=k, ph=pph, off=off, first=0, count=1, o=pro, d=prd, t=prt, w=prw)
    r_order = ("c", "pos", "nrm", "n", "s2", "k", "ph", "off", "first", "count", "o", "d", "t", "w")
    bad_r = [dict(n=-1), dict(k=0), dict(first=-1), dict(count=-1), dict(count=2), dict(first=1),
             dict(pos=None), dict(nrm=None), dict(s2=None), dict(o=None), dict(d=None), dict(t=None), dict(w=None),
             dict(pos=hp), dict(nrm=hp), dict(s2=hp), dict(ph=hp), dict(o=hp), dict(d=hp), dict(t=hp), dict(w=hp),
             dict(pos=tail(n * 12 - 12)), dict(s2=tail(k * 8 - 8)), dict(ph=tail(n * 4 - 4)), dict(o=tail(n * k * 12 - 12)),
             dict(d=tail(n * k * 12 - 4)), dict(t=tail(n * k * 4 - 4)), dict(w=tail(n * k * 12 - 4)),
             dict(n=big, k=big), dict(n=big, k=257),                     # 2^62 rays; more rays than the grid holds
             dict(off=cf(nan)), dict(off=cf(-inf)), dict(c=None)]
    for change in bad_r:
        args = dict(Rr, **change)
        assert rays(*[args[a] for a in r_order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_direct_rays" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    hip.hipFree(block)
    assert q(c, pp, pn, 0, ps2, k, pph, off, 0, 1, pout) == P.PTRT_OK          # n_texels == 0: nothing launched
    assert rays(c, pp, pn, 0, ps2, k, pph, off, 0, 1, pro, prd, prt, prw) == P.PTRT_OK
    assert untouched()
    assert s.get_option("query_pmode") == -1                                    # (and no refusal set it)
    assert q(c, pp, pn, n, ps2, k, None, off, 0, 1, pout) == P.PTRT_OK         # and the calls that are in order run
    assert rays(c, pp, pn, n, ps2, k, None, off, 0, 1, pro, prd, prt, prw) == P.PTRT_OK
    s.sync()
    assert not bool((out == PATTERN).any()) and bool((out[:, 5:] == 0).all())
    assert not any(bool((x == PATTERN).any()) for x in (ro, rd, rt, rw))
    assert s.get_option("query_pmode") == 1

    # the binding
    with pytest.raises(ValueError):
        s.query_direct(pos.cpu(), nrm.cpu(), s2.cpu())
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm[:2], s2)
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm, s2[:0])
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm, s2, phases=ph[:2])
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm, s2, phases=ph.cpu())
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm, s2, out=torch.zeros((n + 1, 8), device="cuda"))
    with pytest.raises(ValueError):
        s.query_direct(torch.zeros((3, n), device="cuda").t(), nrm, s2)  # not contiguous
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm, s2, lights=(0, 2))
    with pytest.raises(ValueError):
        s.direct_rays(pos, nrm[:2], s2)
    with pytest.raises(P.PtrtError):
        s.query_direct(pos, nrm, s2, offset=nan)
    with pytest.raises(P.PtrtError):
        s.direct_rays(pos, nrm, s2, offset=inf)
    keep = torch.zeros((n, 8), device="cuda")
    assert s.query_direct(pos, nrm, s2, out=keep) is keep
    assert s.query_direct(pos[:0], nrm[:0], s2).shape == (0, 8)
    o, d, t, w = s.direct_rays(pos[:0], nrm[:0], s2)
    assert o.shape == d.shape == w.shape == (0, 3) and t.shape == (0,)
    s.close()
