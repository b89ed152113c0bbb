"""Batched ray queries on device memory (ptrt_query_rays; Scene.query_closest / query_occluded): CLOSEST against
oracle.trace_rays and ptrt_trace_rays, OCCLUDED against oracle.any_hit -- the whole 64-byte record and the flag, at tolerance 0 --
under every traversal the path tracer has (force_geom x pair_trace: the per-lane walk and PMODE 1, 2, 3), at the batch sizes that
exercise the tail wave and the grid-stride loop, at the edges of tmax, with glass that never occludes and with hostile rays;
after instance moves, GPU refits and rebuilds and behind pipelined frames without a sync; and without a trace left in the path
frames, generator states, stats or timing history."""
import ctypes as C

import numpy as np
import pytest

from common import render_both

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "showcase", "fluid", "many")
RADIUS = dict(cornell=5.0, showcase=10.0, fluid=20.0, many=8.0)
# (force_geom, pair_trace)
VARIANTS = [(-1, 1), (1, 1), (2, 1), (-1, 0), (1, 0), (2, 0)]


def build(P, name, w=64, h=64, **kw):
    s = P.Scene(w, h, **kw)
    if name == "cornell":
        P.scenes.cornell(s)
    elif name == "showcase":
        P.scenes.showcase(s)
    elif name == "fluid":
        P.scenes.fluid(s, cells=256, t=0.0)
    elif name == "many":
        P.scenes.many(s, 128, sphere_segments=32)
    s.uploadToGPU()
    return s


def hostile_rays():
    """zero and denormal directions, NaN origins, axis-parallel rays from a grid of points, rays from inside the boxes"""
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, -1, -1]], np.float32)
    axes /= np.linalg.norm(axes, axis=1, keepdims=True).astype(np.float32)
    o, d = [], []
    for x in (-3.0, 0.0, 1.0, 2.5):
        for y in (-4.0, 0.0, 3.0):
            for z in (-6.0, -5.0, 0.0, 4.0):
                for a in axes:
                    o.append((x, y, z))
                    d.append(a)
    o.append((0, 0, 0)); d.append((0, 0, 0))
    o.append((0, 0, -3)); d.append((0, 0, 0))
    o.append((np.nan, 0, 0)); d.append((0, 0, -1))
    o.append((0, np.nan, np.nan)); d.append((0, 1, 0))
    o.append((0, 0, 0)); d.append((1e-30, 0, -1e-39))
    return np.array(o, np.float32), np.array(d, np.float32)


def ray_set(name, n, seed=11):
    """n rays: half from random points in the scene's box in random directions, half from a camera-like point towards it,
    then the hostile rays (n counts them)"""
    R = RADIUS[name]
    rs = np.random.RandomState(seed)
    ho, hd = hostile_rays()
    m = max(n - len(ho), 0)
    o = rs.uniform(-R, R, (m, 3)).astype(np.float32)
    d = rs.normal(size=(m, 3)).astype(np.float32)
    k = m // 2
    o[:k] = np.array([0.0, 0.4 * R, 2.0 * R], np.float32)
    d[:k] = rs.uniform(-0.6 * R, 0.6 * R, (k, 3)).astype(np.float32) - o[:k]
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    o, d = np.concatenate([o, ho]), np.concatenate([d, hd])
    return np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])


def tmax_set(t):
    """per ray, from its closest-hit distance: exactly t, the float below t, t / 2, 0, -1, +inf, NaN, 1e30"""
    t = t.astype(np.float32)
    k = np.arange(len(t)) % 8
    out = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6],
                    [t, np.nextafter(t, np.float32(0)), t * np.float32(0.5), np.float32(0), np.float32(-1), np.float32(np.inf),
                     np.float32(np.nan)], np.float32(1e30))
    return out.astype(np.float32)


def assert_hits_equal(got, want, what=""):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), 64)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), 64)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} records differ, first {bad[:8]}: {got[bad[0]]} vs {want[bad[0]]}"


def as_hits(t):
    """query_closest's (n, 16) int32 rows as the HIT_DTYPE records they are"""
    import ptrt_amd
    return np.ascontiguousarray(t.cpu().numpy()).view(ptrt_amd.HIT_DTYPE).reshape(t.shape[0])


def to_dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def query_both(s, o, d, tmax):
    """CLOSEST and OCCLUDED through the torch path; (hits as HIT_DTYPE, flags) on the host"""
    to, td, tt = to_dev(o, d, tmax)
    h = s.query_closest(to, td)
    f = s.query_occluded(to, td, tt)
    return as_hits(h), f.cpu().numpy()


_cache = {}


def scene_and_truth(P, O, name, n=16384):
    if name not in _cache:
        s = build(P, name)
        o, d = ray_set(name, n)
        c = O.trace_rays(s.flatten(), o, d)
        tmax = tmax_set(c["t"])
        a = O.any_hit(s.flatten(), o, d, tmax)
        _cache[name] = (s, o, d, c, tmax, a)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cached():
    yield
    for v in _cache.values():
        v[0].close()
    _cache.clear()


@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
@pytest.mark.parametrize("name", SCENES)
def test_queries_equal_the_oracle(P, O, name, fg, pt):
    s, o, d, c, tmax, a = scene_and_truth(P, O, name)
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    try:
        h, f = query_both(s, o, d, tmax)
        pm = s.get_option("query_pmode")
        host = s.trace_rays(o, d)  # ptrt_trace_rays: the same traversal behind host staging
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)
    if pt == 0:
        assert pm == 0
    elif name == "cornell":
        assert pm == {-1: 1, 1: 2, 2: 3}[fg]
    elif fg == 2 or name == "many":
        assert pm == 3
    assert_hits_equal(h, c, f"{name} closest vs oracle")
    assert_hits_equal(host, c, f"{name} ptrt_trace_rays vs oracle")
    bad = np.flatnonzero(f != a)
    assert bad.size == 0, f"{name}: occlusion differs for {bad.size} rays, first {bad[:8]}, tmax {tmax[bad[:8]]}"
    assert c["hit"].mean() > 0.2 and 0 < a.mean() < 1


def test_transmissive_meshes_never_occlude(P, O):
    """A glass cube (transmission 1) in front of the wall: the closest hit is the glass, a ray that ends inside it is not
    occluded; a wax cube (transmission 0.2) in the same place occludes it."""
    for transmission, blocked in ((1.0, 0), (0.2, 1)):
        s = P.Scene(32, 32)
        P.scenes.cornell(s)
        m = s.addCube(P.Material((0.9, 0.9, 0.9), 0.1, transmission=transmission, ior=1.5))
        s.moveTo(m, (0.0, 0.0, -2.0))
        s.uploadToGPU()
        o = np.array([[0.0, 0.0, 4.0], [0.0, 0.0, 4.0]], np.float32)
        d = np.array([[0.0, 0.0, -1.0], [0.0, 0.01, -1.0]], np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
        c = O.trace_rays(s.flatten(), o, d)
        tm = (c["t"] + np.float32(0.3)).astype(np.float32)  # inside the cube: the cube is all that lies before tmax
        for pt in (1, 0):
            s.set_option("pair_trace", pt)
            h, f = query_both(s, o, d, tm)
            assert_hits_equal(h, c, "glass closest")
            assert (h["mesh_index"] == m).all()
            assert np.array_equal(f, O.any_hit(s.flatten(), o, d, tm))
            assert (f == blocked).all()
        s.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, (1 << 20) + 3])
@pytest.mark.parametrize("pt", [1, 0])
def test_batch_sizes(P, O, n, pt):
    """The tail wave (dead lanes in the wave collectives write nothing: the guard words behind the batch stay) and the
    grid-stride loop (2^20 + 3 rays: more chunks than the persistent grid has workgroups)."""
    import torch
    s, *_ = scene_and_truth(P, O, "cornell")
    o, d = ray_set("cornell", n, seed=n)
    c = O.trace_rays(s.flatten(), o, d)
    tmax = tmax_set(c["t"])
    a = O.any_hit(s.flatten(), o, d, tmax)
    s.set_option("pair_trace", pt)
    try:
        to, td, tt = to_dev(o, d, tmax)
        hits = torch.full((n + 4, 16), 0x7badbeef, dtype=torch.int32, device="cuda")
        flags = torch.full((n + 4,), 0x7badbeef, dtype=torch.int32, device="cuda")
        for kind, out, tm in ((P.QUERY_CLOSEST, hits, None), (P.QUERY_OCCLUDED, flags, tt)):
            rc = P.lib.ptrt_query_rays(s.ctx, kind, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()),
                                       C.c_void_p(tm.data_ptr()) if tm is not None else None, n, C.c_void_p(out.data_ptr()))
            assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        s.sync()
    finally:
        s.set_option("pair_trace", 1)
    assert (hits[n:] == 0x7badbeef).all() and (flags[n:] == 0x7badbeef).all(), "a dead lane wrote past the batch"
    assert_hits_equal(as_hits(hits[:n]), c, f"n={n}")
    assert np.array_equal(flags[:n].cpu().numpy(), a)


@pytest.mark.parametrize("fg", [-1, 2])
def test_queries_follow_instance_moves_refits_and_rebuilds(P, O, fg):
    """Each change is followed by a query with no sync in between; the answer is the new geometry's."""
    import torch
    s = P.Scene(64, 48)
    w, ship = P.scenes.fluid(s, cells=24, t=0.0, ship_segments=10)
    s.uploadToGPU()
    s.set_option("force_geom", fg)
    o, d = ray_set("fluid", 4096, seed=5)

    def check(what):
        to, td = to_dev(o, d)
        h = as_hits(s.query_closest(to, td))
        c = O.trace_rays(s.flatten(), o, d)
        assert_hits_equal(h, c, what)
        tm = tmax_set(c["t"])
        f = s.query_occluded(to, td, torch.from_numpy(tm).cuda()).cpu().numpy()
        assert np.array_equal(f, O.any_hit(s.flatten(), o, d, tm)), what
        return h

    h0 = check("initial")
    s.setPosition(ship, (1.5, 0.5, -2.0))     # an instance move: the query commits it (ptrt_update_instances)
    h1 = check("moved instance")
    assert not np.array_equal(h0["mesh_index"], h1["mesh_index"]) or not np.array_equal(h0["t"], h1["t"])
    s.setVertices(w, P.scenes.water_vertices(24, 0.9))
    s.refitObjectChanges()                     # GPU refit on the stream
    h2 = check("GPU refit")
    assert not np.array_equal(h1["t"], h2["t"])
    s.setVertices(w, P.scenes.water_vertices(24, 2.1))
    s.rebuildObjectChanges()                   # GPU rebuild on the stream
    h3 = check("GPU rebuild")
    assert not np.array_equal(h2["t"], h3["t"])
    s.close()


@pytest.mark.parametrize("split", [1, 2])
def test_query_behind_pipelined_and_split_frames(P, O, blue_noise, split):
    import torch
    s = P.Scene(256, 128)
    P.scenes.cornell(s)
    s.setPerfSamplesPerPixel(2)
    s.setMaxBounceDepth(4)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.uploadToGPU()
    s.set_option("pipeline", 1)
    s.set_option("split", split)
    bufs = [torch.empty(256 * 128 * 3, dtype=torch.uint8, device="cuda") for _ in range(2)]
    o, d = ray_set("cornell", 70000, seed=3)
    to, td = to_dev(o, d)
    for f in range(4):
        s.render_to_device(bufs[f & 1].data_ptr())
    if split > 1:
        assert s.get_option("pipelined") == 1
    h = as_hits(s.query_closest(to, td))
    assert_hits_equal(h, O.trace_rays(s.flatten(), o, d), "behind pipelined frames")
    s.close()


def test_query_between_frames_changes_nothing(P, O, blue_noise):
    """Two path frames with a query between them, and the same two frames without it: frames, generator states, stats
    identical; the timing history is the same bytes before and after the query."""
    import torch
    runs = []
    for with_query in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        gpu, cpu = render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        if with_query:
            o, d = ray_set("cornell", 5000)
            to, td = to_dev(o, d)
            tt = torch.full((5000,), 3.0, device="cuda")
            h = s.query_closest(to, td)
            f = s.query_occluded(to, td, tt)
            torch.cuda.synchronize()
            assert s.kernel_ms_history().tobytes() == hist
            assert h.shape == (5000, 16) and f.shape == (5000,)
        rgb = s.render_to_host()
        runs.append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                         object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats(),
                         n_hist=len(s.kernel_ms_history())))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["n_hist"] == b["n_hist"]


def test_torch_round_trip_on_a_side_stream(P, O):
    """Rays made by torch ops on a side stream, queried and consumed by torch ops with no synchronisation in between."""
    import torch
    s, o, d, c, tmax, a = scene_and_truth(P, O, "showcase")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.empty((len(o), 3), device="cuda")
        to = torch.from_numpy(o).to("cuda", non_blocking=False)
        td = torch.from_numpy(d).to("cuda", non_blocking=False)
        m = torch.rand((2048, 2048), device="cuda") / 2048
        for _ in range(20):             # keep the side stream busy: the query must wait for the copies that follow
            m = m @ m
        big.copy_(to)
        o2 = big.clone()                # the rays, produced on the side stream behind that work
        td2 = td.clone()
        h = s.query_closest(o2, td2)
        f = s.query_occluded(o2, td2, torch.from_numpy(tmax).cuda())
        h2 = h.clone()                 # consumed on the side stream
        f2 = f + 0
    side.synchronize()
    assert_hits_equal(as_hits(h2), c, "torch round trip")
    assert np.array_equal(f2.cpu().numpy(), a)
    fields = P.hit_fields(h2)
    assert np.array_equal(fields["t"].cpu().numpy().view(np.uint32), c["t"].view(np.uint32))
    assert np.array_equal(fields["mesh_index"].cpu().numpy(), c["mesh_index"])


def test_numpy_inputs_are_staged(P, O):
    s, o, d, c, tmax, a = scene_and_truth(P, O, "many")
    h = s.query_closest(o, d)
    assert h.dtype == P.HIT_DTYPE
    assert_hits_equal(h, c, "numpy")
    assert np.array_equal(s.query_occluded(o, d, tmax), a)


@pytest.mark.parametrize("kind", ["band", "interleaved"])
def test_band_and_interleaved_contexts_answer_for_the_whole_scene(P, O, kind):
    s = build(P, "showcase", 64, 64, **(dict(tile_y0=16, tile_rows=16) if kind == "band" else dict(interleave=(1, 2))))
    o, d = ray_set("showcase", 3000, seed=9)
    c = O.trace_rays(s.flatten(), o, d)
    tm = tmax_set(c["t"])
    h, f = query_both(s, o, d, tm)
    assert_hits_equal(h, c, kind)
    assert np.array_equal(f, O.any_hit(s.flatten(), o, d, tm))
    s.close()


def test_refusals(P):
    import torch
    q = P.lib.ptrt_query_rays
    vp = C.c_void_p
    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    o, d = torch.zeros((8, 3), device="cuda"), torch.ones((8, 3), device="cuda")
    t, out = torch.ones(8, device="cuda"), torch.zeros((8, 16), dtype=torch.int32, device="cuda")
    po, pd, pt_, pout = (vp(x.data_ptr()) for x in (o, d, t, out))
    assert q(ctx, 0, po, pd, None, 8, pout) == -4  # PTRT_E_NOT_READY: no geometry yet
    assert q(ctx, 1, po, pd, pt_, 8, pout) == -4
    P.lib.ptrt_destroy(ctx)
    s = build(P, "cornell", 32, 32)
    c = s.ctx
    assert q(c, 0, po, pd, None, 8, pout) == P.PTRT_OK
    assert q(c, 1, po, pd, pt_, 8, pout) == P.PTRT_OK
    assert q(c, 0, po, pd, None, 0, pout) == P.PTRT_OK  # n == 0
    host = np.zeros((8, 16), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((8, 16), dtype=torch.int32).pin_memory()
    for args in [(c, 2, po, pd, None, 8, pout), (c, -1, po, pd, None, 8, pout),      # bad kind
                 (c, 0, po, pd, None, -1, pout),                                      # n < 0
                 (c, 0, None, pd, None, 8, pout), (c, 0, po, None, None, 8, pout), (c, 0, po, pd, None, 8, None),
                 (c, 1, po, pd, None, 8, pout),                                        # OCCLUDED without tmax
                 (c, 0, po, pd, pt_, 8, pout),                                         # CLOSEST with tmax
                 (c, 0, hp, pd, None, 8, pout), (c, 0, po, hp, None, 8, pout), (c, 0, po, pd, None, 8, hp),
                 (c, 1, po, pd, hp, 8, pout),                                          # host memory
                 (c, 0, po, pd, None, 8, vp(pinned.data_ptr())),                       # pinned host memory
                 (None, 0, po, pd, None, 8, pout)]:
        assert q(*args) == -1, args  # PTRT_E_INVALID
    with pytest.raises(ValueError):
        s.query_closest(o.cpu(), d.cpu())
    with pytest.raises(ValueError):
        s.query_closest(o.double(), d.double())
    with pytest.raises(ValueError):
        s.query_occluded(o, d, t[:4])
    with pytest.raises(ValueError):
        s.query_closest(torch.zeros((3, 8), device="cuda").t(), d)  # not contiguous
    s.close()
