"""Lightmap texels on the device (ptrt_query_irradiance, ptrt_irradiance_rays; Scene.query_irradiance).  Everything about the
sums at tolerance 0, compared as bytes: a texel's row must be the numpy restatement (tests/irradiance_restatement.py) of what
query_radiance returns for the texel's rays -- irradiance_rays writes them -- from equal generator states, and the states left
behind must be equal too: under every traversal and both material sets, for every segment width and group size at which
padding, a partial last group, a group boundary and the chunked path can go wrong, on a grid smaller than the batch, across
calls; closed forms where 16 equal terms make the sums exact; the rays against a float64 statement of the cosine map and the
basis; no trace left in the frames around a call; what must be refused is refused with everything untouched."""
import ctypes as C

import numpy as np
import pytest

import irradiance_restatement as R
from test_ray_query_gpu import VARIANTS, build

pytestmark = pytest.mark.gpu

W = H = 64
SEED, DEPTH = 12345, 4
PATTERN = 0x7badbeef
OFFSET = np.float32(1e-3)

_cache = {}


def scene(P, name):
    if name not in _cache:
        _cache[name] = build(P, name, W, H)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cached():
    yield
    for s in _cache.values():
        s.close()
    _cache.clear()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_states(states):
    """(n, 6) uint32 on the host -> a fresh (n, 6) int32 tensor on the device (the calls advance it in place)"""
    return dev(np.ascontiguousarray(states).view(np.int32).copy())


def host_states(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def fresh_states(s, n, first=0):
    return host_states(s.init_rng_states(SEED, first, n))


def texels(P, name, n):
    """n texels on two surfaces of the scene, alternating: (positions, normals).  Cornell (and `many`, which stands in it): the
    inner faces of the floor and the left wall (the slabs are 0.1 thick); showcase: its floor, and a wall-like quad facing the
    spheres; fluid: a quad above the water looking down, and one looking along +x."""
    L = P.lightmap
    if name in ("cornell", "many"):
        a = L.quad_texels((-4.95, -4.95, -9.95), (0, 0, 9.0), (9.9, 0, 0), 7, 5)      # floor, normal +y
        b = L.quad_texels((-4.95, -4.95, -9.95), (0, 9.9, 0), (0, 0, 9.0), 5, 7)      # left wall, normal +x
    elif name == "showcase":
        a = L.quad_texels((-9.0, -3.0, -14.0), (0, 0, 10.0), (18.0, 0, 0), 7, 5)     # floor, normal +y
        b = L.quad_texels((-9.0, -2.0, -3.0), (0, 6.0, 0), (18.0, 0, 0), 5, 7)        # in front of the spheres, normal -z: towards them
    else:
        a = L.quad_texels((-8.0, 3.0, -8.0), (16.0, 0, 0), (0, 0, 16.0), 7, 5)       # above the water, normal -y
        b = L.quad_texels((-9.0, 0.5, -8.0), (0, 5.0, 0), (0, 0, 16.0), 5, 7)         # beside the ship, normal +x
    assert abs(float(a[1][0] @ a[1][0]) - 1.0) < 1e-6 and abs(float(b[1][0] @ b[1][0]) - 1.0) < 1e-6
    pos = np.empty((70, 3), np.float32)
    nrm = np.empty((70, 3), np.float32)
    pos[0::2], pos[1::2], nrm[0::2], nrm[1::2] = a[0], b[0], a[1], b[1]
    reps = (n + 69) // 70
    return np.ascontiguousarray(np.tile(pos, (reps, 1))[:n]), np.ascontiguousarray(np.tile(nrm, (reps, 1))[:n])


def unfused(P, s, pos, nrm, s2, states, samples=1, maxd=1e30, phases=None):
    """(rows, states afterwards): the restatement of query_radiance on irradiance_rays' rays from a copy of `states`"""
    st = dev_states(states)
    o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET, phases=dev(phases))
    r = s.query_radiance(o, d, st, samples=samples, max_depth=DEPTH)
    r = np.ascontiguousarray(r.cpu().numpy()).view(P.RADIANCE_DTYPE).reshape(len(pos) * len(s2))
    return R.restate(r["radiance"], r["depth"], r["object_id"], len(s2), maxd), host_states(st)


def fused(s, pos, nrm, s2, states, samples=1, maxd=1e30, phases=None):
    """(rows, states afterwards): query_irradiance from a copy of `states`"""
    st = dev_states(states)
    rows = s.query_irradiance(dev(pos), dev(nrm), dev(s2), st, samples=samples, max_depth=DEPTH, max_distance=maxd, offset=OFFSET,
                              phases=dev(phases))
    return rows.cpu().numpy(), host_states(st)


def assert_rows_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, f"{what}: {got.shape} {got.dtype}"
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} words differ, first (texel, column) {bad[:6].tolist()}: "
                           f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


# ---- 1. the restatement, as bytes ---------------------------------------------------------------------------------------------
def check_restatement(P, s, name, maxd):
    n, k = 37, 24  # w = 32: two texels per wave, the last wave half empty, eight dead lanes per segment
    pos, nrm = texels(P, name, n)
    s2, ph = P.lightmap.hammersley2(k), P.lightmap.texel_phases(n, 3)
    st0 = fresh_states(s, n * k)
    want, want_st = unfused(P, s, pos, nrm, s2, st0, maxd=maxd, phases=ph)
    got, got_st = fused(s, pos, nrm, s2, st0, maxd=maxd, phases=ph)
    pm = s.get_option("query_pmode")
    assert_rows_equal(got, want, name)
    assert np.array_equal(got_st, want_st), f"{name}: states differ"
    assert not np.array_equal(got_st, st0) and got[:, :3].any() and not got[:, 6:].any()
    f = P.irradiance_fields(got)
    assert (f["hit_fraction"] > 0).any() and (f["mean_distance"] > 0).all() and (f["mean_distance"] <= np.float32(maxd)).all()
    return pm


@pytest.mark.parametrize("full", [0, 1], ids=["force_full=0", "force_full=1"])
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
def test_cornell_equals_the_restatement_under_every_variant(P, fg, pt, full):
    s = scene(P, "cornell")
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    s.set_option("force_full", full)
    try:
        pm = check_restatement(P, s, "cornell", 6.5)  # (the box is 10 across: some rays clamp)
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)
        s.set_option("force_full", 0)
    assert pm == (0 if pt == 0 else {-1: 1, 1: 2, 2: 3}[fg])


@pytest.mark.parametrize("name", ["showcase", "many", "fluid"])
def test_scenes_equal_the_restatement(P, name):
    pm = check_restatement(P, scene(P, name), name, 1e30)
    if name == "many":
        assert pm == 3


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dirs", [1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 63, 64, 65, 130])
def test_shapes(P, n_dirs):
    """Per direction count, with g = 64 / w texels per wave (1 beyond 64 directions): 1, g - 1, g, g + 1 and 2 g + 1 texels --
    segment padding, a partial last group, a full one, a group boundary, and two strides of a one-wave grid's worth."""
    s = scene(P, "cornell")
    g = 64 // R.width(n_dirs) if n_dirs <= 64 else 1
    s2 = P.lightmap.hammersley2(n_dirs)
    for n in sorted({1, g - 1, g, g + 1, 2 * g + 1} - {0}):
        pos, nrm = texels(P, "cornell", n)
        ph = P.lightmap.texel_phases(n, n_dirs)
        st0 = fresh_states(s, n * n_dirs, first=1000)
        want, want_st = unfused(P, s, pos, nrm, s2, st0, samples=2, maxd=20.0, phases=ph)
        got, got_st = fused(s, pos, nrm, s2, st0, samples=2, maxd=20.0, phases=ph)
        assert_rows_equal(got, want, f"{n} x {n_dirs}")
        assert np.array_equal(got_st, want_st), f"{n} x {n_dirs}: states"
        assert got[:, :3].any()


# ---- 3. the grid strides over groups ------------------------------------------------------------------------------------------
def test_more_groups_than_workgroups(P):
    import torch
    s = scene(P, "cornell")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = 16                       # four texels per wave
    n = 4 * (2 * cus + 3) + 1    # with persist 1 the grid is one wave per CU: every wave strides twice, four of them three times
    pos, nrm = texels(P, "cornell", n)
    rs = np.random.RandomState(5)
    pos = (pos + rs.uniform(-0.04, 0.04, pos.shape) * (1 - np.abs(nrm))).astype(np.float32)  # (moved within their planes)
    s2 = P.lightmap.hammersley2(k)
    st0 = fresh_states(s, n * k)
    want, want_st = unfused(P, s, pos, nrm, s2, st0)
    s.set_option("persist", 1)
    try:
        narrow, narrow_st = fused(s, pos, nrm, s2, st0)
    finally:
        s.set_option("persist", 0)
    wide, wide_st = fused(s, pos, nrm, s2, st0)
    assert_rows_equal(narrow, want, "persist 1 vs the restatement")
    assert np.array_equal(narrow_st, want_st)
    assert_rows_equal(wide, want, "the default grid vs the restatement")
    assert np.array_equal(wide_st, want_st)
    assert len(np.unique(wide[:, :3], axis=0)) > n // 2  # other places, other texels


# ---- 4. the rays --------------------------------------------------------------------------------------------------------------
def test_rays_against_the_float64_statement(P):
    s = scene(P, "cornell")
    rs = np.random.RandomState(9)
    n, k = 41, 24
    nrm = rs.normal(size=(n, 3))
    nrm[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]  # the walls' own, z = -1 (the basis' other sign) included
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    pos = rs.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    s2, ph = P.lightmap.hammersley2(k), P.lightmap.texel_phases(n, 1)
    # the two ends of the map: u1 the largest float32 below 1 -- cos(theta) = 2^-12, the ray that grazes the texel's plane, where
    # a direction below the horizon would show -- and u1 = 0, the normal itself
    s2[-2:] = [[np.nextafter(np.float32(1.0), np.float32(0.0)), 0.3], [0.0, 0.7]]
    ph[:3] = [0.0, 0.999999, 0.5]
    o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET, phases=dev(ph))
    o, d = o.cpu().numpy(), d.cpu().numpy()
    assert o.shape == d.shape == (n * k, 3) and o.dtype == d.dtype == np.float32
    assert np.array_equal(o.view(np.uint32), R.origins32(pos, nrm, OFFSET, k).view(np.uint32))  # p + offset * N, exactly
    margin = R.ray_margin()
    err = np.abs(d.astype(np.float64) - R.rays64(nrm, s2, ph))
    print(f"irradiance_rays: worst direction error {err.max():.3e}, margin {margin:.3e}")
    assert err.max() <= margin
    cosine = np.einsum("tkc,tc->tk", d.astype(np.float64).reshape(n, k, 3), nrm.astype(np.float64))
    print(f"irradiance_rays: smallest dot(d, N) {cosine.min():.3e}")
    assert cosine.min() >= -margin and cosine[:, -2].max() <= 2.0 ** -12 + 4.0 * margin
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 3.0 * margin
    # cosine-distributed: cos(theta) is sqrt(1 - u1) of the shared set, whatever the normal and the phase
    want_cos = np.sqrt(1.0 - s2[:, 0].astype(np.float64))
    assert np.abs(cosine - want_cos[None, :]).max() <= 4.0 * margin
    # no phases and zero phases: the same bits
    o0, d0 = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET)
    oz, dz = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET, phases=dev(np.zeros(n, np.float32)))
    assert np.array_equal(o0.cpu().numpy().view(np.uint32), oz.cpu().numpy().view(np.uint32))
    assert np.array_equal(d0.cpu().numpy().view(np.uint32), dz.cpu().numpy().view(np.uint32))
    assert not np.array_equal(d0.cpu().numpy(), d)
    st0 = fresh_states(s, n * k)
    a, a_st = fused(s, pos, nrm, s2, st0)
    b, b_st = fused(s, pos, nrm, s2, st0, phases=np.zeros(n, np.float32))
    assert_rows_equal(a, b, "phases=None vs zeros")
    assert np.array_equal(a_st, b_st)


def test_rays_about_a_degenerate_normal(P):
    """|N|^2 < 1e-20 takes createOrthoNormalBasis's fixed T = (1, 0, 0), B = (0, 1, 0): the direction is
    local.x * T + local.y * B + local.z * N with N as given, and the origin the position (offset * 0 is 0)."""
    s = scene(P, "cornell")
    k = 16
    nrm = np.float32([[0, 0, 0], [1e-11, -2e-11, 1e-11], [0, 0, 1]])  # zero; tiny; and a unit normal beside them
    pos = np.float32([[1, 2, -3], [0.5, -1, -2], [0, 0, -5]])
    s2, ph = P.lightmap.hammersley2(k), np.float32([0.25, 0.5, 0.75])
    o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET, phases=dev(ph))
    o, d = o.cpu().numpy(), d.cpu().numpy().reshape(3, k, 3)
    assert np.array_equal(o.view(np.uint32), R.origins32(pos, nrm, OFFSET, k).view(np.uint32))
    assert np.array_equal(o[:k], np.repeat(pos[:1], k, axis=0))
    want = R.rays64(nrm, s2, ph).reshape(3, k, 3)
    err = np.abs(d.astype(np.float64) - want)
    print(f"irradiance_rays, degenerate normals: worst direction error {err.max():.3e}")
    assert err.max() <= R.ray_margin()
    # the zero normal: (local.x, local.y, 0) -- a circle of radius sqrt(u1) in the xy plane -- and dot(d, N) = 0
    assert (d[0, :, 2] == 0).all()
    assert np.abs(np.hypot(d[0, :, 0].astype(np.float64), d[0, :, 1]) - np.sqrt(s2[:, 0].astype(np.float64))).max() <= 2 * R.ray_margin()
    assert np.abs(d[1, :, 2]).max() <= 1e-11 and d[:2, :, :2].any()


# ---- 5. guards ----------------------------------------------------------------------------------------------------------------
def test_guard_rows(P):
    """`d_out`, the states and the ray targets between pattern rows, before and after: the rows stay."""
    import torch
    s = scene(P, "cornell")
    vp = C.c_void_p
    for n, k in ((5, 12), (3, 70)):  # segments of 16 with a partial group; the chunked path with a tail chunk
        pos, nrm = texels(P, "cornell", n)
        s2, ph = P.lightmap.hammersley2(k), P.lightmap.texel_phases(n, 2)
        st0 = fresh_states(s, n * k)
        batch, batch_st = fused(s, pos, nrm, s2, st0, phases=ph)
        G = 3
        st = torch.full((n * k + 2 * G, 6), PATTERN, dtype=torch.int32, device="cuda")
        st[G:G + n * k] = dev_states(st0)
        out = torch.full((n + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
        ro = torch.full((n * k + 2 * G, 3), PATTERN, dtype=torch.int32, device="cuda")
        rd = torch.full((n * k + 2 * G, 3), PATTERN, dtype=torch.int32, device="cuda")
        tp, tn, ts, tph = dev(pos), dev(nrm), dev(s2), dev(ph)
        rc = P.lib.ptrt_query_irradiance(s.ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                         C.c_float(OFFSET), vp(st[G:].data_ptr()), 1, DEPTH, C.c_float(1e30), vp(out[G:].data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        rc = P.lib.ptrt_irradiance_rays(s.ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                        C.c_float(OFFSET), vp(ro[G:].data_ptr()), vp(rd[G:].data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        s.sync()
        for name, t, rows in (("out", out, n), ("states", st, n * k), ("origins", ro, n * k), ("directions", rd, n * k)):
            assert (t[:G] == PATTERN).all() and (t[G + rows:] == PATTERN).all(), f"{name}: a write outside the batch"
        assert_rows_equal(out[G:G + n].view(torch.float32).cpu().numpy(), batch, "raw call")
        assert np.array_equal(host_states(st[G:G + n * k]), batch_st)
        o, d = s.irradiance_rays(tp, tn, ts, offset=OFFSET, phases=tph)
        assert torch.equal(ro[G:G + n * k], o.view(torch.int32)) and torch.equal(rd[G:G + n * k], d.view(torch.int32))


# ---- 6. continuation ----------------------------------------------------------------------------------------------------------
def test_a_second_call_continues_the_streams(P):
    s = scene(P, "showcase")
    n, k = 9, 16
    pos, nrm = texels(P, "showcase", n)
    s2 = P.lightmap.hammersley2(k)
    st0 = fresh_states(s, n * k)
    st = dev_states(st0)
    tp, tn, ts = dev(pos), dev(nrm), dev(s2)
    first = s.query_irradiance(tp, tn, ts, st, max_depth=DEPTH, offset=OFFSET).cpu().numpy()
    second = s.query_irradiance(tp, tn, ts, st, max_depth=DEPTH, offset=OFFSET).cpu().numpy()
    ref = dev_states(st0)
    o, d = s.irradiance_rays(tp, tn, ts, offset=OFFSET)
    rows = []
    for _ in range(2):  # the second from the states the first call left
        r = np.ascontiguousarray(s.query_radiance(o, d, ref, max_depth=DEPTH).cpu().numpy()).view(P.RADIANCE_DTYPE).reshape(n * k)
        rows.append(R.restate(r["radiance"], r["depth"], r["object_id"], k, 1e30))
    assert_rows_equal(first, rows[0], "first call")
    assert_rows_equal(second, rows[1], "second call")
    assert np.array_equal(host_states(st), host_states(ref))
    assert not np.array_equal(first[:, :3], second[:, :3])
    assert np.array_equal(first[:, 3:], second[:, 3:])  # the same first hits


# ---- 7. closed forms ----------------------------------------------------------------------------------------------------------
def test_texels_under_a_uniform_sky(P):
    """16 equal terms fold and divide exactly."""
    s = scene(P, "many")
    sky = (0.5, 1.0, 2.0)
    s.setSkyGradient(sky, sky)
    try:
        n, k = 5, 16
        pos = np.float32([[x, 50.0, 0.0] for x in range(n)])
        nrm = np.tile(np.float32([0, 1, 0]), (n, 1))
        s2 = P.lightmap.hammersley2(k)
        st0 = fresh_states(s, n * k)
        maxd = np.float32(7.3)
        got, _ = fused(s, pos, nrm, s2, st0, maxd=maxd, phases=P.lightmap.texel_phases(n, 4))
        o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET)
        r = s.query_radiance(o, d, dev_states(st0), max_depth=DEPTH).cpu().numpy().view(P.RADIANCE_DTYPE).reshape(n * k)
    finally:
        s.disableSky()
    assert (r["object_id"] == -1).all() and (r["radiance"] == r["radiance"][0]).all() and r["radiance"][0].all()
    f = P.irradiance_fields(got)
    assert np.array_equal(f["radiance"], np.tile(r["radiance"][0], (n, 1)))
    assert np.array_equal(f["radiance"], np.tile(np.float32(sky), (n, 1)))  # the sky's colour itself: 16 equal terms fold and divide exactly
    assert (f["hit_fraction"] == 0).all() and (f["mean_distance"] == maxd).all() and (f["mean_distance_sq"] == maxd * maxd).all()
    assert (maxd * maxd).dtype == np.float32


def test_distances(P):
    s = scene(P, "cornell")
    k = 16
    # on the floor where the tall box stands on it (the box reaches from y = -5 to -2 around (-1.5, -6)): every ray ends on the
    # box's own faces, from inside -- the texel a baker marks invalid
    pos, nrm = np.float32([[-1.5, -4.95, -6.0]]), np.float32([[0, 1, 0]])
    s2 = P.lightmap.hammersley2(k)
    st0 = fresh_states(s, k)
    got, _ = fused(s, pos, nrm, s2, st0, maxd=100.0)
    want, _ = unfused(P, s, pos, nrm, s2, st0, maxd=100.0)
    f = P.irradiance_fields(got)
    assert f["hit_fraction"][0] == 1 and f["mean_distance"][0] == want[0, 3] and 0 < f["mean_distance"][0] < 4
    assert P.lightmap.invalid_texels(got, 4.0).tolist() == [True] and P.lightmap.invalid_texels(got, 0.1).tolist() == [False]
    assert f["mean_distance_sq"][0] == want[0, 4]
    # and what hits is what query_closest hits, no nearer than it says
    o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=OFFSET)
    hits = P.hit_fields(s.query_closest(o, d))
    t = hits["t"].cpu().numpy()
    assert (hits["hit"].cpu().numpy() != 0).all()
    maxd = np.float32(0.01)
    assert t.min() > maxd
    got, _ = fused(s, pos, nrm, s2, st0, maxd=maxd)
    f = P.irradiance_fields(got)
    assert f["mean_distance"][0] == maxd and f["mean_distance_sq"][0] == maxd * maxd and f["hit_fraction"][0] == 1


# ---- 8. neighbours ------------------------------------------------------------------------------------------------------------
def buffers(P, s):
    return dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                object_id=s.read(P.BUF_OBJECT_ID), rng=s.read(P.BUF_RNG))


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
        if with_bake:
            pos, nrm = texels(P, "cornell", 70)
            st = s.init_rng_states(4, 0, 70 * 16)
            rows = s.query_irradiance(dev(pos), dev(nrm), dev(P.lightmap.hammersley2(16)), st, samples=2)
            o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(P.lightmap.hammersley2(16)))
            torch.cuda.synchronize()
            assert rows.shape == (70, 8) and rows[:, :3].any() and o.shape == d.shape == (70 * 16, 3)
            assert s.kernel_ms_history().tobytes() == hist
            assert [x.tobytes() for x in s.launch_ms_history()] == lhist
            assert np.array_equal(s.read(P.BUF_RNG), rng)
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), n_hist=len(s.kernel_ms_history()),
                         n_lhist=len(s.launch_ms_history()[0])))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["n_hist"] == b["n_hist"] and a["n_lhist"] == b["n_lhist"]


def test_a_bake_sees_a_refit_without_a_sync(P):
    s = P.Scene(64, 48)
    w, ship = P.scenes.fluid(s, cells=24, t=0.0, ship_segments=10)
    s.uploadToGPU()
    pos, nrm = P.lightmap.quad_texels((-3.0, 3.0, -3.0), (6.0, 0, 0), (0, 0, 6.0), 3, 3)  # above the water, looking down
    s2 = P.lightmap.hammersley2(16)
    st0 = fresh_states(s, 9 * 16)
    before, _ = fused(s, pos, nrm, s2, st0)
    s.setVertices(w, P.scenes.water_vertices(24, 0.9))
    s.refitObjectChanges()
    unsynced, st_a = fused(s, pos, nrm, s2, st0)
    s.sync()
    synced, st_b = fused(s, pos, nrm, s2, st0)
    assert_rows_equal(unsynced, synced, "behind ptrt_refit")
    assert np.array_equal(st_a, st_b)
    assert synced[:, 5].any() and not np.array_equal(before[:, 3], synced[:, 3])  # the water moved: other distances
    s.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    q, rays = P.lib.ptrt_query_irradiance, P.lib.ptrt_irradiance_rays
    vp, cf = C.c_void_p, C.c_float
    INVALID, NOT_READY = -1, -4
    n, k = 3, 8
    pos = torch.tensor([[0.0, -4.95, -5.0], [0.3, -4.95, -2.0], [1.0, -4.95, -3.0]], device="cuda")  # on the Cornell floor
    nrm = torch.tensor([0.0, 1.0, 0.0], device="cuda").repeat(n, 1)
    s2 = dev(P.lightmap.hammersley2(k))
    ph = torch.zeros(n, device="cuda")
    st = torch.full((n * k, 6), 5, dtype=torch.int32, device="cuda")
    out = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    ro = torch.full((n * k, 3), PATTERN, dtype=torch.int32, device="cuda")
    rd = torch.full((n * k, 3), PATTERN, dtype=torch.int32, device="cuda")
    pp, pn, ps2, pph, ps, pout, pro, prd = (vp(x.data_ptr()) for x in (pos, nrm, s2, ph, st, out, ro, rd))
    off, ok = cf(1e-3), cf(10.0)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == PATTERN).all()) and bool((st == 5).all()) and bool((ro == PATTERN).all()) and bool((rd == PATTERN).all())

    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    assert q(ctx, pp, pn, n, ps2, k, pph, off, ps, 1, 4, ok, pout) == NOT_READY   # no geometry, no materials
    assert b"ptrt_query_irradiance" in P.lib.ptrt_last_error(ctx)
    assert untouched()
    P.lib.ptrt_destroy(ctx)
    assert q(ctx, pp, pn, n, ps2, k, pph, off, ps, 1, 4, ok, pout) == INVALID     # a destroyed context
    assert rays(ctx, pp, pn, n, ps2, k, pph, off, pro, prd) == INVALID
    s = build(P, "cornell", 32, 32)
    c = s.ctx
    host = np.zeros((n * k, 8), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((n, 8), dtype=torch.int32).pin_memory()
    # device memory that ends before the call's last element.  (torch hands tensors out of larger blocks, inside which a short
    # tensor is still device memory; an allocation of the runtime's own ends where it ends.)
    hip = C.CDLL("libamdhip64.so")      # the runtime libptrt_amd.so itself is linked against
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    inf, nan = float("inf"), float("nan")
    Q = dict(c=c, pos=pp, nrm=pn, n=n, s2=ps2, k=k, ph=pph, off=off, st=ps, samples=1, depth=4, maxd=ok, out=pout)
    order = ("c", "pos", "nrm", "n", "s2", "k", "ph", "off", "st", "samples", "depth", "maxd", "out")
    bad_q = [dict(n=-1), dict(k=0), dict(k=-3),
             dict(pos=None), dict(nrm=None), dict(s2=None), dict(st=None), dict(out=None),                       # NULL
             dict(pos=hp), dict(nrm=hp), dict(s2=hp), dict(ph=hp), dict(st=hp), dict(out=hp),                    # host memory
             dict(out=vp(pinned.data_ptr())),                                                                    # pinned host memory
             dict(pos=tail(n * 12 - 12)), dict(nrm=tail(n * 12 - 12)), dict(s2=tail(k * 8 - 8)), dict(ph=tail(n * 4 - 4)),
             dict(st=tail(n * k * 24 - 24)), dict(out=tail(n * 32 - 4)),                                        # short buffers
             dict(n=2 ** 31 - 1, k=2 ** 31 - 1),                                                                 # 2^62 rays
             dict(samples=0), dict(samples=-1), dict(samples=32768), dict(depth=0), dict(depth=32768),
             dict(maxd=cf(0.0)), dict(maxd=cf(-1.0)), dict(maxd=cf(inf)), dict(maxd=cf(nan)),
             dict(off=cf(nan)), dict(off=cf(inf)), dict(c=None)]
    for change in bad_q:
        args = dict(Q, **change)
        assert q(*[args[a] for a in order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_query_irradiance" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    Rr = dict(c=c, pos=pp, nrm=pn, n=n, s2=ps2, k=k, ph=pph, off=off, o=pro, d=prd)
    r_order = ("c", "pos", "nrm", "n", "s2", "k", "ph", "off", "o", "d")
    bad_r = [dict(n=-1), dict(k=0), dict(pos=None), dict(nrm=None), dict(s2=None), dict(o=None), dict(d=None),
             dict(pos=hp), dict(nrm=hp), dict(s2=hp), dict(ph=hp), dict(o=hp), dict(d=hp),
             dict(pos=tail(n * 12 - 12)), dict(s2=tail(k * 8 - 8)), dict(ph=tail(n * 4 - 4)), dict(o=tail(n * k * 12 - 12)),
             dict(d=tail(n * k * 12 - 4)), dict(n=2 ** 31 - 1, k=2 ** 31 - 1), dict(n=2 ** 31 - 1, k=257),                # 2^62 rays; more rays than the grid holds
             dict(off=cf(nan)), dict(off=cf(-inf)), dict(c=None)]
    for change in bad_r:
        args = dict(Rr, **change)
        assert rays(*[args[a] for a in r_order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_irradiance_rays" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    # (buffers that do reach: the distance is what is refused)
    assert q(c, tail(n * 12), tail(n * 12), n, tail(k * 8), k, None, off, ps, 1, 4, cf(-1.0), tail(n * 32)) == INVALID
    hip.hipFree(block)
    assert q(c, pp, pn, 0, ps2, k, pph, off, ps, 1, 4, ok, pout) == P.PTRT_OK      # n_texels == 0: nothing launched
    assert rays(c, pp, pn, 0, ps2, k, pph, off, pro, prd) == P.PTRT_OK
    assert untouched()
    assert s.get_option("query_pmode") == -1                                        # (and no refusal set it)
    assert q(c, pp, pn, n, ps2, k, None, off, ps, 1, 4, ok, pout) == P.PTRT_OK     # and the calls that are in order run
    assert rays(c, pp, pn, n, ps2, k, None, off, pro, prd) == P.PTRT_OK
    s.sync()
    assert not bool((out[:, :6] == PATTERN).any()) and bool((out[:, 6:] == 0).all()) and not bool((st == 5).all())
    assert not bool((ro == PATTERN).any()) and not bool((rd == PATTERN).any())
    assert s.get_option("query_pmode") == 1

    # the binding
    st2 = torch.full((n * k, 6), 5, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        s.query_irradiance(pos.cpu(), nrm.cpu(), s2.cpu(), st2.cpu())
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm, s2, st2[:4])
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm[:2], s2, st2)
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm, s2[:0], st2[:0])
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm, s2, st2, phases=ph[:2])
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm, s2, st2, phases=ph.cpu())
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm, s2, st2, out=torch.zeros((n + 1, 8), device="cuda"))
    with pytest.raises(ValueError):
        s.query_irradiance(torch.zeros((3, n), device="cuda").t(), nrm, s2, st2)  # not contiguous
    with pytest.raises(ValueError):
        s.irradiance_rays(pos, nrm[:2], s2)
    with pytest.raises(P.PtrtError):
        s.query_irradiance(pos, nrm, s2, st2, samples=0)
    with pytest.raises(P.PtrtError):
        s.query_irradiance(pos, nrm, s2, st2, max_distance=0.0)
    with pytest.raises(P.PtrtError):
        s.query_irradiance(pos, nrm, s2, st2, offset=nan)
    torch.cuda.synchronize()
    assert bool((st2 == 5).all())
    keep = torch.zeros((n, 8), device="cuda")
    assert s.query_irradiance(pos, nrm, s2, st2, out=keep) is keep
    assert s.query_irradiance(pos[:0], nrm[:0], s2, st2[:0]).shape == (0, 8)
    o, d = s.irradiance_rays(pos[:0], nrm[:0], s2)
    assert o.shape == d.shape == (0, 3)
    s.close()
