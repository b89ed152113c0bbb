"""Light probes on the device (ptrt_query_probes; Scene.query_probes).  Everything at tolerance 0, compared as bytes: a probe's
row must be the numpy restatement (tests/probe_restatement.py) of what query_radiance returns for the probe's rays from equal
generator states, and the states left behind must be equal too -- under every traversal and both material sets, for chunk
counts around the wave size, on a grid smaller than the batch, across calls; closed forms where 64 equal terms make the sums
exact; no trace left in the frames around a call; what must be refused is refused with `out` and the states untouched."""
import ctypes as C

import numpy as np
import pytest

import probe_restatement as R
from test_ray_query_gpu import VARIANTS, build

pytestmark = pytest.mark.gpu

W = H = 64
SEED, DEPTH = 12345, 4
PATTERN = 0x7badbeef
CAMERA = {"cornell": (0.0, 0.0, 5.0), "showcase": (0.0, 1.5, -2.0), "many": (0.0, 0.0, 5.0), "fluid": (0.0, 6.0, 18.0)}
AROUND = np.float32([[0, 0, 0], [0.4, 0.1, -1.5], [-0.7, 0.3, -3.0], [0.2, -0.6, -6.0], [0.0, 0.5, -9.0]])  # towards -z: into Cornell

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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_states(states):
    """(n, 6) uint32 on the host -> a fresh (n, 6) int32 tensor on the device (the calls advance it in place)"""
    return dev(np.ascontiguousarray(states).view(np.int32).copy())


def host_states(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def fresh_states(s, n, first=0):
    return host_states(s.init_rng_states(SEED, first, n))


def positions(name, n=5):
    """n probes at and around the scene's camera origin (for showcase, whose camera looks along +z, mirrored)"""
    off = AROUND[:n] * (np.float32([1, 1, -1]) if name == "showcase" else np.float32(1))
    return np.ascontiguousarray(np.float32(CAMERA[name])[None, :] + off)


def radiance_records(P, s, pos, dirs, st, samples=1):
    """query_radiance on the probes' rays, ray (p, k) in row p * k_dirs + k, advancing the device tensor `st`"""
    n, k = len(pos), len(dirs)
    o = dev(np.repeat(pos, k, axis=0))
    d = dev(np.tile(dirs, (n, 1)))
    r = s.query_radiance(o, d, st, samples=samples, max_depth=DEPTH)
    return np.ascontiguousarray(r.cpu().numpy()).view(P.RADIANCE_DTYPE).reshape(n * k)


def unfused(P, s, pos, dirs, states, samples=1, maxd=1e30):
    """(rows, states afterwards): the restatement of query_radiance from a copy of `states`"""
    st = dev_states(states)
    r = radiance_records(P, s, pos, dirs, st, samples)
    return R.restate(r["radiance"], r["depth"], r["object_id"], dirs, len(dirs), maxd), host_states(st)


def fused(s, pos, dirs, states, samples=1, maxd=1e30):
    """(rows, states afterwards): query_probes from a copy of `states`"""
    st = dev_states(states)
    rows = s.query_probes(dev(pos), dev(dirs), st, samples=samples, max_depth=DEPTH, max_distance=maxd)
    return rows.cpu().numpy(), host_states(st)


def assert_rows_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, f"{what}: {got.shape} {got.dtype}"
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} words differ, first (probe, column) {bad[:6].tolist()}: "
                           f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


# ---- 1. the restatement, as bytes ---------------------------------------------------------------------------------------------
def check_restatement(P, s, name, maxd):
    pos, dirs = positions(name), P.probes.fibonacci_sphere(130)
    st0 = fresh_states(s, 5 * 130)
    want, want_st = unfused(P, s, pos, dirs, st0, maxd=maxd)
    got, got_st = fused(s, pos, dirs, st0, maxd=maxd)
    pm = s.get_option("query_pmode")
    assert_rows_equal(got, want, name)
    assert np.array_equal(got_st, want_st), f"{name}: states differ"
    assert not np.array_equal(got_st, st0) and got[:, :27].any() and not got[:, 30:].any()
    f = P.probe_fields(got)
    assert (f["hit_fraction"] > 0).all() and (f["mean_distance"] > 0).all() and (f["mean_distance"] <= np.float32(maxd)).all()
    return pm


@pytest.mark.parametrize("full", [0, 1], ids=["force_full=0", "force_full=1"])
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
def test_cornell_equals_the_restatement_under_every_variant(P, fg, pt, full):
    s = scene(P, "cornell")
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    s.set_option("force_full", full)
    try:
        pm = check_restatement(P, s, "cornell", 6.5)  # (the box is 10 across and the first probe stands 5 in front of it: some rays clamp)
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
@pytest.mark.parametrize("n_probes", [1, 3])
@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 128, 130])
def test_shapes(P, n_dirs, n_probes):
    s = scene(P, "cornell")
    pos, dirs = positions("cornell", n_probes), P.probes.fibonacci_sphere(n_dirs)
    st0 = fresh_states(s, n_probes * n_dirs, first=1000)
    want, want_st = unfused(P, s, pos, dirs, st0, samples=3, maxd=20.0)
    got, got_st = fused(s, pos, dirs, st0, samples=3, maxd=20.0)
    assert_rows_equal(got, want, f"{n_probes} x {n_dirs}")
    assert np.array_equal(got_st, want_st)


# ---- 3. the grid strides over probes ------------------------------------------------------------------------------------------
def test_more_probes_than_workgroups(P):
    import torch
    s = scene(P, "cornell")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus + 7
    rs = np.random.RandomState(3)
    pos = (np.float32(CAMERA["cornell"]) + rs.uniform(-0.8, 0.8, (n, 3)) * np.float32([1, 1, 0]) - np.float32([0, 0, 1]) *
           rs.uniform(0.0, 9.0, (n, 1))).astype(np.float32)
    dirs = P.probes.fibonacci_sphere(65)
    st0 = fresh_states(s, n * 65)
    wide, wide_st = fused(s, pos, dirs, st0)
    s.set_option("persist", 1)
    try:
        narrow, narrow_st = fused(s, pos, dirs, st0)  # one workgroup per CU: seven of them take two probes
    finally:
        s.set_option("persist", 0)
    assert_rows_equal(narrow, wide, "persist 1 vs the default grid")
    assert np.array_equal(narrow_st, wide_st)
    assert len(np.unique(wide[:, :3], axis=0)) == n  # other places, other probes


# ---- 4. guards and order ------------------------------------------------------------------------------------------------------
def test_guard_rows_permutations_and_single_probes(P):
    import torch
    s = scene(P, "cornell")
    n, k = 5, 70
    pos, dirs = positions("cornell"), P.probes.fibonacci_sphere(k)
    st0 = fresh_states(s, n * k)
    batch, batch_st = fused(s, pos, dirs, st0)
    # guard rows behind `out` and behind the states
    st = torch.full((n * k + 4, 6), PATTERN, dtype=torch.int32, device="cuda")
    st[:n * k] = dev_states(st0)
    out = torch.full((n + 4, 32), PATTERN, dtype=torch.int32, device="cuda")
    tp, td = dev(pos), dev(dirs)
    rc = P.lib.ptrt_query_probes(s.ctx, C.c_void_p(tp.data_ptr()), n, C.c_void_p(td.data_ptr()), k, C.c_void_p(st.data_ptr()),
                                 1, DEPTH, C.c_float(1e30), C.c_void_p(out.data_ptr()))
    assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
    s.sync()
    assert (out[n:] == PATTERN).all() and (st[n * k:] == PATTERN).all(), "a write past the batch"
    assert_rows_equal(out[:n].view(torch.float32).cpu().numpy(), batch, "raw call")
    assert np.array_equal(host_states(st[:n * k]), batch_st)
    # permuted probes give permuted rows
    perm = np.array([3, 0, 4, 2, 1])
    st_blocks = st0.reshape(n, k, 6)
    got, got_st = fused(s, pos[perm], dirs, st_blocks[perm].reshape(n * k, 6))
    assert_rows_equal(got, batch[perm], "permuted")
    assert np.array_equal(got_st.reshape(n, k, 6), batch_st.reshape(n, k, 6)[perm])
    # one at a time
    for p in range(n):
        one, one_st = fused(s, pos[p:p + 1], dirs, st_blocks[p])
        assert_rows_equal(one, batch[p:p + 1], f"probe {p} alone")
        assert np.array_equal(one_st, batch_st.reshape(n, k, 6)[p])


# ---- 5. continuation ----------------------------------------------------------------------------------------------------------
def test_a_second_call_continues_the_streams(P):
    s = scene(P, "showcase")
    pos, dirs = positions("showcase", 3), P.probes.fibonacci_sphere(100)
    st0 = fresh_states(s, 300)
    st = dev_states(st0)
    first = s.query_probes(dev(pos), dev(dirs), st, max_depth=DEPTH).cpu().numpy()
    second = s.query_probes(dev(pos), dev(dirs), st, max_depth=DEPTH).cpu().numpy()
    ref = dev_states(st0)
    r1 = radiance_records(P, s, pos, dirs, ref)
    r2 = radiance_records(P, s, pos, dirs, ref)  # from the states the first call left
    assert_rows_equal(first, R.restate(r1["radiance"], r1["depth"], r1["object_id"], dirs, 100, 1e30), "first call")
    assert_rows_equal(second, R.restate(r2["radiance"], r2["depth"], r2["object_id"], dirs, 100, 1e30), "second call")
    assert np.array_equal(host_states(st), host_states(ref))
    assert not np.array_equal(first[:, :27], second[:, :27])
    assert np.array_equal(first[:, 27:], second[:, 27:])  # the same first hits


# ---- 6. closed forms: 64 equal terms sum and divide exactly -------------------------------------------------------------------
def upper_hemisphere(P):
    d = P.probes.fibonacci_sphere(128)[:64]
    assert (d[:, 2] > 0).all()
    return np.ascontiguousarray(d[:, [0, 2, 1]])  # the lattice's pole to +y: up


def test_a_probe_under_a_uniform_sky(P):
    s = scene(P, "many")
    sky = (0.5, 1.0, 2.0)
    s.setSkyGradient(sky, sky)
    try:
        pos, dirs = np.float32([[0.0, 50.0, 0.0]]), upper_hemisphere(P)
        st0 = fresh_states(s, 64)
        maxd = np.float32(7.3)
        got, _ = fused(s, pos, dirs, st0, maxd=maxd)
        r = radiance_records(P, s, pos, dirs, dev_states(st0))
    finally:
        s.disableSky()
    assert (r["object_id"] == -1).all() and (r["radiance"] == r["radiance"][0]).all() and r["radiance"][0].all()
    f = P.probe_fields(got)
    assert np.array_equal(f["sh"][0, 0], np.float32(0.282095) * r["radiance"][0])
    assert f["hit_fraction"][0] == 0 and f["mean_distance"][0] == maxd and f["mean_distance_sq"][0] == maxd * maxd
    assert (maxd * maxd).dtype == np.float32


def test_distances_and_hit_counts(P):
    s = scene(P, "cornell")
    dirs = P.probes.fibonacci_sphere(64)
    inside = np.float32([[0.5, -1.0, -4.0]])
    hits = P.hit_fields(s.query_closest(dev(np.repeat(inside, 64, axis=0)), dev(dirs)))
    t = hits["t"].cpu().numpy()[hits["hit"].cpu().numpy() != 0]
    maxd = np.float32(0.01)
    assert len(t) and t.min() > maxd
    got, _ = fused(s, inside, dirs, fresh_states(s, 64), maxd=maxd)
    f = P.probe_fields(got)
    assert f["mean_distance"][0] == maxd and f["mean_distance_sq"][0] == maxd * maxd
    # the hit fraction counts what query_closest hits: inside the box, and from outside its open front
    for name, pos in (("cornell", inside), ("many", np.float32([[0.0, 1.0, 9.0]]))):
        sc = scene(P, name)
        h = P.hit_fields(sc.query_closest(dev(np.repeat(pos, 64, axis=0)), dev(dirs)))["hit"].cpu().numpy()
        got, _ = fused(sc, pos, dirs, fresh_states(sc, 64))
        assert P.probe_fields(got)["hit_fraction"][0] * np.float32(64) == np.count_nonzero(h), name
        if name == "many":
            assert 0 < np.count_nonzero(h) < 64


# ---- 7. neighbours ------------------------------------------------------------------------------------------------------------
def buffers(P, s):
    return dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                object_id=s.read(P.BUF_OBJECT_ID), rng=s.read(P.BUF_RNG))


def test_probes_between_frames_change_nothing(P, O, blue_noise):
    import torch
    from common import render_both
    runs = []
    for with_probes in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        lhist = [x.tobytes() for x in s.launch_ms_history()]
        rng = s.read(P.BUF_RNG)
        if with_probes:
            st = s.init_rng_states(4, 0, 8 * 96)
            rows = s.query_probes(dev(P.probes.probe_grid((-0.8, -0.8, -7.0), (0.8, 0.8, -3.0), (2, 2, 2))),
                                  dev(P.probes.fibonacci_sphere(96)), st, samples=2)
            torch.cuda.synchronize()
            assert rows.shape == (8, 32) and rows[:, :27].any()
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


def test_probes_see_a_refit_and_a_tlas_refit_without_a_sync(P):
    dirs = P.probes.fibonacci_sphere(96)
    # a vertex refit on the stream (ptrt_refit), then the probes
    s = P.Scene(64, 48)
    w, ship = P.scenes.fluid(s, cells=24, t=0.0, ship_segments=10)
    s.uploadToGPU()
    pos = P.probes.probe_grid((-3.0, 2.0, -3.0), (3.0, 4.0, 3.0), (2, 1, 2))
    st0 = fresh_states(s, 4 * 96)
    before, _ = fused(s, pos, dirs, st0)
    s.setVertices(w, P.scenes.water_vertices(24, 0.9))
    s.refitObjectChanges()
    unsynced, st_a = fused(s, pos, dirs, st0)
    s.sync()
    synced, st_b = fused(s, pos, dirs, st0)
    again, st_c = fused(s, pos, dirs, st0)
    assert_rows_equal(unsynced, synced, "behind ptrt_refit")
    assert np.array_equal(st_a, st_b)
    assert_rows_equal(again, synced, "two runs from equal states")
    assert np.array_equal(st_c, st_b)
    assert not np.array_equal(before[:, 27], synced[:, 27])  # the water moved: other distances
    s.close()
    # moved instances behind the uploaded TLAS topology (ptrt_set_instance_transforms + ptrt_refit_tlas), then the probes
    s = P.Scene(64, 48)
    P.scenes.many(s, 40)
    s.uploadToGPU()
    pos = P.probes.probe_grid((-0.6, -0.5, -4.0), (0.6, 0.5, 1.0), (2, 1, 2))
    before, _ = fused(s, pos, dirs, st0)
    refits = s.get_option("tlas_refits")
    for m in (8, 11, 14):  # instances of scenes.many (every third mesh behind the Cornell box's eight)
        s.setPosition(m, (0.3 * (m - 11), 0.0, -1.0))
        s.setInstanceScale(m, (0.9, 0.9, 0.9))
    s.refitInstanceChanges()
    assert s.get_option("tlas_refits") == refits + 1
    unsynced, st_a = fused(s, pos, dirs, st0)
    s.sync()
    synced, st_b = fused(s, pos, dirs, st0)
    assert s.get_option("query_pmode") == 3
    assert_rows_equal(unsynced, synced, "behind ptrt_refit_tlas")
    assert np.array_equal(st_a, st_b)
    assert not np.array_equal(before[:, 27], synced[:, 27])
    s.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    q = P.lib.ptrt_query_probes
    vp, cf = C.c_void_p, C.c_float
    INVALID, NOT_READY = -1, -4
    n, k = 2, 8
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.3, 0.0, -2.0]], device="cuda")
    d = torch.tensor([0.0, 0.0, -1.0], device="cuda").repeat(k, 1)  # into the Cornell box: a hit, whose scatter draws
    st = torch.full((n * k, 6), 5, dtype=torch.int32, device="cuda")
    out = torch.full((n, 32), PATTERN, dtype=torch.int32, device="cuda")
    pp, pd, ps, pout = (vp(x.data_ptr()) for x in (pos, d, st, out))

    def untouched():
        torch.cuda.synchronize()
        return bool((out == PATTERN).all()) and bool((st == 5).all())

    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    assert q(ctx, pp, n, pd, k, ps, 1, 4, cf(10.0), pout) == NOT_READY   # no geometry, no materials
    assert untouched()
    P.lib.ptrt_destroy(ctx)
    assert q(ctx, pp, n, pd, k, ps, 1, 4, cf(10.0), pout) == INVALID     # a destroyed context
    s = build(P, "cornell", 32, 32)
    c = s.ctx
    host = np.zeros((n * k, 8), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((n, 32), dtype=torch.int32).pin_memory()
    ok = cf(10.0)
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

    for args in [(c, pp, -1, pd, k, ps, 1, 4, ok, pout),                                                       # n_probes < 0
                 (c, pp, n, pd, 0, ps, 1, 4, ok, pout), (c, pp, n, pd, -3, ps, 1, 4, ok, pout),                # n_dirs < 1
                 (c, None, n, pd, k, ps, 1, 4, ok, pout), (c, pp, n, None, k, ps, 1, 4, ok, pout),
                 (c, pp, n, pd, k, None, 1, 4, ok, pout), (c, pp, n, pd, k, ps, 1, 4, ok, None),               # NULL
                 (c, hp, n, pd, k, ps, 1, 4, ok, pout), (c, pp, n, hp, k, ps, 1, 4, ok, pout),
                 (c, pp, n, pd, k, hp, 1, 4, ok, pout), (c, pp, n, pd, k, ps, 1, 4, ok, hp),                   # host memory
                 (c, pp, n, pd, k, ps, 1, 4, ok, vp(pinned.data_ptr())),                                       # pinned host memory
                 (c, tail(n * 12 - 12), n, pd, k, ps, 1, 4, ok, pout), (c, pp, n, tail(k * 12 - 12), k, ps, 1, 4, ok, pout),
                 (c, pp, n, pd, k, tail(n * k * 24 - 24), 1, 4, ok, pout), (c, pp, n, pd, k, ps, 1, 4, ok, tail(n * 128 - 4)),  # short buffers
                 (c, pp, 2 ** 31 - 1, pd, 2 ** 31 - 1, ps, 1, 4, ok, pout),                                    # 2^62 rays
                 (c, pp, n, pd, k, ps, 0, 4, ok, pout), (c, pp, n, pd, k, ps, -1, 4, ok, pout), (c, pp, n, pd, k, ps, 32768, 4, ok, pout),
                 (c, pp, n, pd, k, ps, 1, 0, ok, pout), (c, pp, n, pd, k, ps, 1, 32768, ok, pout),             # samples / max_depth
                 (c, pp, n, pd, k, ps, 1, 4, cf(0.0), pout), (c, pp, n, pd, k, ps, 1, 4, cf(-1.0), pout),
                 (c, pp, n, pd, k, ps, 1, 4, cf(float("inf")), pout), (c, pp, n, pd, k, ps, 1, 4, cf(float("nan")), pout),  # max_distance
                 (None, pp, n, pd, k, ps, 1, 4, ok, pout)]:
        assert q(*args) == INVALID, args
    assert untouched() and not host.any()
    assert q(c, tail(n * 12), n, tail(k * 12), k, ps, 1, 4, cf(-1.0), tail(n * 128)) == INVALID  # (buffers that do reach: the distance)
    hip.hipFree(block)
    assert q(c, pp, 0, pd, k, ps, 1, 4, ok, pout) == P.PTRT_OK      # n_probes == 0: nothing launched
    assert untouched()
    assert s.get_option("query_pmode") == -1                          # (and no refusal set it)
    assert q(c, pp, n, pd, k, ps, 1, 4, ok, pout) == P.PTRT_OK      # and the call that is in order runs
    s.sync()
    assert not bool((out[:, :30] == PATTERN).any()) and not bool((st == 5).all())
    assert s.get_option("query_pmode") == 1

    # the binding
    st2 = torch.full((n * k, 6), 5, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        s.query_probes(pos.cpu(), d.cpu(), st2.cpu())
    with pytest.raises(ValueError):
        s.query_probes(pos, d, st2[:4])
    with pytest.raises(ValueError):
        s.query_probes(pos, d[:0], st2[:0])
    with pytest.raises(ValueError):
        s.query_probes(pos, d, st2, out=torch.zeros((n + 1, 32), device="cuda"))
    with pytest.raises(ValueError):
        s.query_probes(torch.zeros((3, n), device="cuda").t(), d, st2)  # not contiguous
    with pytest.raises(P.PtrtError):
        s.query_probes(pos, d, st2, samples=0)
    with pytest.raises(P.PtrtError):
        s.query_probes(pos, d, st2, max_distance=0.0)
    torch.cuda.synchronize()
    assert bool((st2 == 5).all())
    keep = torch.zeros((n, 32), device="cuda")
    assert s.query_probes(pos, d, st2, out=keep) is keep
    assert s.query_probes(pos[:0], d, st2[:0]).shape == (0, 32)
    s.close()
