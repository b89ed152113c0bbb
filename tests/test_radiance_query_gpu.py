"""Path-traced radiance for caller-supplied rays on the device (ptrt_query_radiance; Scene.query_radiance, camera_rays,
init_rng_states).  Everything at tolerance 0, compared as bytes: a query fed a pinhole frame's own primary rays and the generator
states that frame started from must BE that frame -- ACCUM, DEPTH, NORMAL, OBJECT_ID and the states it leaves -- on the GPU and in
the oracle, under every traversal the geometric queries are tested under and with both material sets; samples continue across
calls and within one; order and batch size change nothing; rays that are no camera's agree with query_closest about what they
hit; the query leaves no trace in the frames around it and sees what was enqueued before it; what must be refused is refused
with `out` untouched."""
import ctypes as C

import numpy as np
import pytest

from test_ray_query_gpu import VARIANTS, build

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "showcase", "many", "fluid")
W = H = 64
SEED, FRAME, DEPTH = 12345, 3, 4
PATTERN = 0x7badbeef


def records(P, t):
    """query_radiance's (n, 8) float32 rows as the RADIANCE_DTYPE records they are"""
    return np.ascontiguousarray(t.cpu().numpy()).view(P.RADIANCE_DTYPE).reshape(t.shape[0])


def frame_records(P, b):
    """a frame's four buffers as the records a query of its rays must return"""
    r = np.zeros(len(b["depth"]), P.RADIANCE_DTYPE)
    r["radiance"], r["depth"], r["normal"], r["object_id"] = b["accum"], b["depth"], b["normal"], b["object_id"]
    return r


def assert_records_equal(got, want, what=""):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), 32)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), 32)
    assert g.shape == w.shape, f"{what}: {g.shape[0]} records for {w.shape[0]}"
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} records differ, first {bad[:8]}: {got[bad[0]]} vs {want[bad[0]]}"


def dev_states(states):
    """(n, 6) uint32 on the host -> a fresh (n, 6) int32 tensor on the device (the query advances it in place)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(states).view(np.int32).copy()).cuda()


def host_states(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def query(P, s, o, d, states, samples=1, depth=DEPTH):
    """one query from a copy of `states`; (records, states afterwards) on the host"""
    st = dev_states(states)
    r = s.query_radiance(o, d, st, samples=samples, max_depth=depth)
    return records(P, r), host_states(st)


def buffers(P, s):
    return dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                object_id=s.read(P.BUF_OBJECT_ID), rng=s.read(P.BUF_RNG))


def prepare(P, s, spp=1):
    s.setPerfSamplesPerPixel(spp)
    s.setMaxBounceDepth(DEPTH)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(SEED)


def render_frame(P, s, rng0, spp):
    """frame FRAME at `spp` samples from the states rng0; the buffers it leaves"""
    s.setPerfSamplesPerPixel(spp)
    s.write_rng(rng0)
    s.setFrameCount(FRAME)
    s.render_to_host()
    return buffers(P, s)


_cache = {}


def frame_case(P, O, blue_noise, name):
    """Per scene, once: the scene, the states before frame 3, the 1-spp frame on the GPU and in the oracle, its primary rays."""
    if name not in _cache:
        s = build(P, name, W, H)
        prepare(P, s)
        rng0 = s.read(P.BUF_RNG)
        assert np.array_equal(rng0, O.xorwow_init(SEED, 0, W * H))
        gpu = render_frame(P, s, rng0, 1)
        rng = rng0.copy()
        cpu = O.render(s.flatten(), W, H, 1, DEPTH, FRAME, blue_noise, rng, threads=8)
        cpu["rng"] = rng
        o, d = s.camera_rays(FRAME, 0)
        _cache[name] = dict(s=s, rng0=rng0, gpu=gpu, cpu=cpu, o=o, d=d)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cached():
    yield
    for v in _cache.values():
        v["s"].close()
    _cache.clear()


# ---- 1. a frame by query ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [0, 1], ids=["force_full=0", "force_full=1"])
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
@pytest.mark.parametrize("name", SCENES)
def test_a_frame_by_query(P, O, blue_noise, name, fg, pt, full):
    c = frame_case(P, O, blue_noise, name)
    s = c["s"]
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    s.set_option("force_full", full)
    try:
        got, after = query(P, s, c["o"], c["d"], c["rng0"])
        pm = s.get_option("query_pmode")
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)
        s.set_option("force_full", 0)
    if pt == 0:
        assert pm == 0
    elif name == "cornell":
        assert pm == {-1: 1, 1: 2, 2: 3}[fg]
    elif name == "showcase" and fg < 2:
        assert pm == 2
    elif fg == 2 or name == "many":
        assert pm == 3
    assert_records_equal(got, frame_records(P, c["gpu"]), f"{name} vs the GPU frame")
    assert np.array_equal(after, c["gpu"]["rng"]), f"{name}: states differ from the GPU frame's"
    assert_records_equal(got, frame_records(P, c["cpu"]), f"{name} vs the oracle")
    assert np.array_equal(after, c["cpu"]["rng"]), f"{name}: states differ from the oracle's"
    assert got["radiance"].any() and (got["object_id"] >= 0).any()


# ---- 2. two samples: the states continue across calls -----------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_two_samples_across_calls(P, O, blue_noise, name):
    c = frame_case(P, O, blue_noise, name)
    s = c["s"]
    frame = render_frame(P, s, c["rng0"], 2)
    st = dev_states(c["rng0"])
    r0 = records(P, s.query_radiance(c["o"], c["d"], st, samples=1, max_depth=DEPTH))
    o1, d1 = s.camera_rays(FRAME, 1)
    r1 = records(P, s.query_radiance(o1, d1, st, samples=1, max_depth=DEPTH))
    mean = (np.float32(0) + r0["radiance"] + r1["radiance"]) / np.float32(2)
    assert mean.dtype == np.float32
    assert np.array_equal(mean.view(np.uint32), frame["accum"].view(np.uint32)), "(0 + r0 + r1) / 2 is not the 2-spp ACCUM"
    want = frame_records(P, frame)
    want["radiance"] = r0["radiance"]
    assert_records_equal(r0, want, "first-hit fields of the first call vs the frame's G-buffers")
    assert np.array_equal(host_states(st), frame["rng"])
    assert not np.array_equal(o1.cpu().numpy(), c["o"].cpu().numpy()) or not np.array_equal(d1.cpu().numpy(), c["d"].cpu().numpy())


# ---- 3. samples > 1 on one ray set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_three_samples_in_one_call(P, O, blue_noise, name):
    c = frame_case(P, O, blue_noise, name)
    s = c["s"]
    one, after_one = query(P, s, c["o"], c["d"], c["rng0"], samples=3)
    st = dev_states(c["rng0"])
    parts = [records(P, s.query_radiance(c["o"], c["d"], st, samples=1, max_depth=DEPTH)) for _ in range(3)]
    want = parts[0].copy()
    want["radiance"] = (np.float32(0) + parts[0]["radiance"] + parts[1]["radiance"] + parts[2]["radiance"]) / np.float32(3)
    assert_records_equal(one, want, "samples=3 vs three chained calls")
    assert np.array_equal(after_one, host_states(st))
    assert not np.array_equal(parts[0]["radiance"], parts[1]["radiance"])


# ---- 4. order and batch size do not matter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "many"])
def test_permuted_rays_give_permuted_records(P, O, blue_noise, name):
    import torch
    c = frame_case(P, O, blue_noise, name)
    s = c["s"]
    want = frame_records(P, c["gpu"])
    n = W * H
    perm = np.random.RandomState(5).permutation(n)
    for p in (perm, np.arange(n)[::-1].copy()):
        tp = torch.from_numpy(p).cuda()
        got, after = query(P, s, c["o"][tp].contiguous(), c["d"][tp].contiguous(), c["rng0"][p])
        assert_records_equal(got, want[p], "permuted")
        assert np.array_equal(after, c["gpu"]["rng"][p])


@pytest.mark.parametrize("pt", [1, 0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 4096])
def test_prefixes(P, O, blue_noise, n, pt):
    """The tail chunk: dead lanes take part in the collectives and write nothing (the guard rows behind the batch stay)."""
    import torch
    c = frame_case(P, O, blue_noise, "cornell")
    s = c["s"]
    st = torch.full((n + 4, 6), PATTERN, dtype=torch.int32, device="cuda")
    st[:n] = dev_states(c["rng0"][:n])
    out = torch.full((n + 4, 8), PATTERN, dtype=torch.int32, device="cuda")
    s.set_option("pair_trace", pt)
    try:
        rc = P.lib.ptrt_query_radiance(s.ctx, C.c_void_p(c["o"].data_ptr()), C.c_void_p(c["d"].data_ptr()), C.c_void_p(st.data_ptr()),
                                       n, 1, DEPTH, C.c_void_p(out.data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        s.sync()
    finally:
        s.set_option("pair_trace", 1)
    assert (out[n:] == PATTERN).all() and (st[n:] == PATTERN).all(), "a dead lane wrote past the batch"
    assert_records_equal(records(P, out[:n].view(torch.float32)), frame_records(P, c["gpu"])[:n], f"prefix {n}")
    assert np.array_equal(host_states(st[:n]), c["gpu"]["rng"][:n])


@pytest.mark.parametrize("name", ["cornell", "showcase"])
def test_one_batch_of_nine_tiles_equals_nine_calls(P, O, blue_noise, name):
    """64 x 64 x 9 rays -- 576 chunks -- on a grid of one workgroup per CU (option persist): the grid-stride loop takes two or
    three chunks per workgroup.  Each copy of the ray set has fresh states of its own."""
    import torch
    c = frame_case(P, O, blue_noise, name)
    s = c["s"]
    n = W * H
    o, d = c["o"].repeat(9, 1), c["d"].repeat(9, 1)
    st = s.init_rng_states(777, 1000, 9 * n)
    st0 = st.clone()
    assert np.array_equal(host_states(st0), O.xorwow_init(777, 1000, 9 * n))
    s.set_option("persist", 1)
    try:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert cus < 576, f"{cus} CUs: one workgroup per CU would take a single chunk each"
        batch = records(P, s.query_radiance(o, d, st, samples=1, max_depth=DEPTH))
    finally:
        s.set_option("persist", 0)
    for k in range(9):
        part = st0[k * n:(k + 1) * n].clone()
        r = records(P, s.query_radiance(c["o"], c["d"], part, samples=1, max_depth=DEPTH))
        assert_records_equal(batch[k * n:(k + 1) * n], r, f"copy {k}")
        assert np.array_equal(host_states(st[k * n:(k + 1) * n]), host_states(part))
    assert not np.array_equal(batch["radiance"][:n], batch["radiance"][n:2 * n])  # other states, other samples
    assert np.array_equal(batch["depth"][:n], batch["depth"][n:2 * n])             # the same first hits


# ---- 5. rays that are no camera's -------------------------------------------------------------------------------------------
def env_map():
    rs = np.random.RandomState(2)
    rgba = rs.uniform(0.0, 2.0, (16, 32, 4)).astype(np.float32)
    rgba[:, :, 3] = 1.0
    return rgba


@pytest.mark.parametrize("sky", ["off", "gradient", "env"])
@pytest.mark.parametrize("name,origin", [("cornell", (0.5, -1.0, -4.0)), ("many", (0.0, 1.0, 9.0))], ids=["inside-cornell", "outside-many"])
def test_panorama_rays(P, O, blue_noise, name, origin, sky):
    c = frame_case(P, O, blue_noise, name)
    s = c["s"]
    o, d = P.cameras.equirect_rays(64, 32, origin, "cuda")
    n = 64 * 32
    if sky == "gradient":
        s.setSkyGradient((0.2, 0.4, 0.9), (1.0, 0.9, 0.8))
    elif sky == "env":
        s.setSkyGradient((0.2, 0.4, 0.9), (1.0, 0.9, 0.8))
        s.setEnvironmentMap(env_map())
    try:
        st0 = O.xorwow_init(99, 5, n)
        a, sa = query(P, s, o, d, st0, samples=2)
        b, sb = query(P, s, o, d, st0, samples=2)
        hits = s.query_closest(o, d)
        f = {k: v.cpu().numpy() for k, v in P.hit_fields(hits).items()}
    finally:
        if sky == "env":
            s.freeHDRI()
        s.disableSky()
    assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb), "two runs from equal states differ"
    assert not np.array_equal(sa, st0)
    for k in ("radiance", "depth", "normal"):
        assert np.isfinite(a[k]).all(), k
    miss = f["hit"] == 0
    if name == "many":
        assert miss.any() and (~miss).any()   # from outside: the open front of the box, and the sky around it
    else:
        assert (~miss).any()
    assert (a["depth"][miss] == np.float32(1e30)).all() and not a["normal"][miss].any() and (a["object_id"][miss] == -1).all()
    assert np.array_equal(a["depth"].view(np.uint32), f["t"].view(np.uint32))
    assert np.array_equal(a["normal"].view(np.uint32), f["normal"].view(np.uint32))
    assert np.array_equal(a["object_id"], f["mesh_index"])
    if miss.any():
        lit = a["radiance"][miss].any(axis=1)
        assert lit.all() if sky != "off" else not lit.any(), "a primary miss carries the sky's radiance, or none without a sky"


# ---- 6. init_rng_states -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,first,n", [(12345, 0, 4096), (7, 1000003, 65), (12345, 2 ** 33, 3)])
def test_init_rng_states_equals_the_oracle(P, O, blue_noise, seed, first, n):
    s = frame_case(P, O, blue_noise, "cornell")["s"]
    got = host_states(s.init_rng_states(seed, first, n))
    assert got.shape == (n, 6)
    assert np.array_equal(got, O.xorwow_init(seed, first, n))


# ---- 7. no trace left, and ordering -----------------------------------------------------------------------------------------
def test_query_between_frames_changes_nothing(P, O, blue_noise):
    """Two path frames with a query (and the two helper kernels) between them, and the same two frames without: frames,
    generator states, stats identical; the timing histories are the same bytes before and after the query."""
    import torch
    from common import render_both
    runs = []
    for with_query in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        lhist = [x.tobytes() for x in s.launch_ms_history()]
        rng = s.read(P.BUF_RNG)
        if with_query:
            o, d = s.camera_rays(1, 0)
            st = s.init_rng_states(4, 0, 96 * 64)
            r = s.query_radiance(o, d, st, samples=2)
            torch.cuda.synchronize()
            assert r.shape == (96 * 64, 8) and r[:, :3].any()
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


@pytest.mark.parametrize("split", [1, 2])
def test_query_behind_pipelined_and_split_frames(P, O, blue_noise, split):
    import torch
    s = P.Scene(256, 128)
    P.scenes.cornell(s)
    prepare(P, s, spp=2)
    s.set_option("pipeline", 1)
    s.set_option("split", split)
    bufs = [torch.empty(256 * 128 * 3, dtype=torch.uint8, device="cuda") for _ in range(2)]
    o, d = s.camera_rays(0, 0)
    st0 = O.xorwow_init(3, 0, 256 * 128)
    quiet, quiet_st = query(P, s, o, d, st0)  # nothing in flight
    s.sync()
    for f in range(4):
        s.render_to_device(bufs[f & 1].data_ptr())
    if split > 1:
        assert s.get_option("pipelined") == 1
    got, got_st = query(P, s, o, d, st0)      # behind the frames, no sync
    assert_records_equal(got, quiet, "behind pipelined frames")
    assert np.array_equal(got_st, quiet_st)
    s.close()


def test_query_sees_a_refit_and_a_tlas_refit_without_a_sync(P, O, blue_noise):
    # a vertex refit on the stream (ptrt_refit), then the query
    s = P.Scene(64, 48)
    w, ship = P.scenes.fluid(s, cells=24, t=0.0, ship_segments=10)
    prepare(P, s)
    o, d = s.camera_rays(0, 0)
    st0 = O.xorwow_init(8, 0, 64 * 48)
    before, _ = query(P, s, o, d, st0)
    s.setVertices(w, P.scenes.water_vertices(24, 0.9))
    s.refitObjectChanges()
    unsynced, st_a = query(P, s, o, d, st0)
    s.sync()
    synced, st_b = query(P, s, o, d, st0)
    assert_records_equal(unsynced, synced, "behind ptrt_refit")
    assert np.array_equal(st_a, st_b)
    assert not np.array_equal(before["depth"], synced["depth"])
    s.close()
    # moved instances behind the uploaded TLAS topology (ptrt_set_instance_transforms + ptrt_refit_tlas), then the query
    s = P.Scene(64, 48)
    P.scenes.many(s, 40)
    prepare(P, s)
    o, d = s.camera_rays(0, 0)
    before, _ = query(P, s, o, d, st0)
    refits = s.get_option("tlas_refits")
    for m in (8, 11, 14):  # instances of scenes.many (every third mesh behind the Cornell box's eight)
        s.setPosition(m, (0.3 * (m - 11), 0.0, -1.0))
        s.setInstanceScale(m, (0.9, 0.9, 0.9))
    s.refitInstanceChanges()
    assert s.get_option("tlas_refits") == refits + 1
    unsynced, st_a = query(P, s, o, d, st0)
    s.sync()
    synced, st_b = query(P, s, o, d, st0)
    assert s.get_option("query_pmode") == 3
    assert_records_equal(unsynced, synced, "behind ptrt_refit_tlas")
    assert np.array_equal(st_a, st_b)
    assert not np.array_equal(before["object_id"], synced["object_id"])
    s.close()


@pytest.mark.parametrize("kind", ["band", "interleaved"])
def test_band_and_interleaved_contexts_answer_for_the_whole_scene(P, O, blue_noise, kind):
    c = frame_case(P, O, blue_noise, "showcase")
    s = build(P, "showcase", W, H, **(dict(tile_y0=16, tile_rows=16) if kind == "band" else dict(interleave=(1, 2))))
    prepare(P, s)
    got, after = query(P, s, c["o"], c["d"], c["rng0"])
    assert_records_equal(got, frame_records(P, c["gpu"]), kind)
    assert np.array_equal(after, c["gpu"]["rng"])
    # and its own camera rays are its rows of the full frame's
    o, d = s.camera_rays(FRAME, 0)
    full_o, full_d = c["o"].cpu().numpy().reshape(H, W, 3), c["d"].cpu().numpy().reshape(H, W, 3)
    rows = np.arange(16, 32) if kind == "band" else np.array([r for r in range(H) if (r // 8) % 2 == 1])
    assert np.array_equal(o.cpu().numpy().reshape(-1, W, 3), full_o[rows])
    assert np.array_equal(d.cpu().numpy().reshape(-1, W, 3).view(np.uint32), full_d[rows].view(np.uint32))
    s.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(P, O, blue_noise):
    import torch
    q, cr, ir = P.lib.ptrt_query_radiance, P.lib.ptrt_camera_rays, P.lib.ptrt_init_rng_states
    vp = C.c_void_p
    INVALID, NOT_READY = -1, -4
    o = torch.zeros((8, 3), device="cuda")
    d = torch.tensor([0.0, 0.0, -1.0], device="cuda").repeat(8, 1)  # into the Cornell box: a hit, whose scatter draws
    st = torch.full((8, 6), 5, dtype=torch.int32, device="cuda")
    out = torch.full((8, 8), PATTERN, dtype=torch.int32, device="cuda")
    po, pd, ps, pout = (vp(x.data_ptr()) for x in (o, d, st, out))

    def untouched():
        torch.cuda.synchronize()
        return bool((out == PATTERN).all()) and bool((st == 5).all())

    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    assert q(ctx, po, pd, ps, 8, 1, 4, pout) == NOT_READY   # no geometry, no materials
    assert untouched()
    P.lib.ptrt_destroy(ctx)
    assert q(ctx, po, pd, ps, 8, 1, 4, pout) == INVALID     # a destroyed context
    s = build(P, "cornell", 32, 32)
    c = s.ctx
    host = np.zeros((8, 8), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((8, 8), dtype=torch.int32).pin_memory()
    for args in [(c, po, pd, ps, -1, 1, 4, pout),                                                  # n < 0
                 (c, None, pd, ps, 8, 1, 4, pout), (c, po, None, ps, 8, 1, 4, pout),
                 (c, po, pd, None, 8, 1, 4, pout), (c, po, pd, ps, 8, 1, 4, None),                 # NULL
                 (c, hp, pd, ps, 8, 1, 4, pout), (c, po, hp, ps, 8, 1, 4, pout),
                 (c, po, pd, hp, 8, 1, 4, pout), (c, po, pd, ps, 8, 1, 4, hp),                     # host memory
                 (c, po, pd, ps, 8, 1, 4, vp(pinned.data_ptr())),                                  # pinned host memory
                 (c, po, pd, ps, 8, 0, 4, pout), (c, po, pd, ps, 8, -1, 4, pout), (c, po, pd, ps, 8, 32768, 4, pout),
                 (c, po, pd, ps, 8, 1, 0, pout), (c, po, pd, ps, 8, 1, 32768, pout),               # samples / max_depth
                 (None, po, pd, ps, 8, 1, 4, pout)]:
        assert q(*args) == INVALID, args
    assert untouched() and not host.any()
    assert q(c, po, pd, ps, 0, 1, 4, pout) == P.PTRT_OK      # n == 0: nothing launched
    assert untouched()
    assert q(c, po, pd, ps, 8, 1, 4, pout) == P.PTRT_OK      # and the call that is in order runs
    torch.cuda.synchronize()
    s.sync()
    assert not bool((out == PATTERN).any()) and not bool((st == 5).all())

    # ptrt_camera_rays
    n = 32 * 32
    co = torch.full((n, 3), 7.0, device="cuda")
    cd = torch.full((n, 3), 7.0, device="cuda")
    pco, pcd = vp(co.data_ptr()), vp(cd.data_ptr())
    for args in [(c, -1, 0, pco, pcd), (c, 0, -1, pco, pcd), (c, 2 ** 31 - 1, 1, pco, pcd), (c, 0, 0, None, pcd), (c, 0, 0, pco, None),
                 (c, 0, 0, hp, pcd), (c, 0, 0, pco, hp), (None, 0, 0, pco, pcd)]:
        assert cr(*args) == INVALID, args
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0, 0.5, 5.0)  # a thin lens
    with pytest.raises(P.PtrtError, match="thin lens"):
        s.camera_rays(0)
    s.sync()
    assert bool((co == 7.0).all()) and bool((cd == 7.0).all())
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0)
    ro, rd = s.camera_rays(0)
    assert ro.shape == rd.shape == (n, 3) and torch.equal(ro, torch.tensor([0.0, 0.0, 5.0], device="cuda").expand(n, 3))

    # ptrt_init_rng_states
    buf = torch.full((8, 6), 5, dtype=torch.int32, device="cuda")
    pb = vp(buf.data_ptr())
    for args in [(c, 1, 0, -1, pb), (c, 1, 0, 8, None), (c, 1, 0, 8, hp),
                 (c, 1, 2 ** 40, 1, pb), (c, 1, 2 ** 40 - 4, 8, pb), (c, 1, 2 ** 64 - 4, 8, pb), (None, 1, 0, 8, pb)]:
        assert ir(*args) == INVALID, args
    assert ir(c, 1, 0, 0, pb) == P.PTRT_OK
    s.sync()
    assert bool((buf == 5).all())
    assert ir(c, 1, 2 ** 40 - 8, 8, pb) == P.PTRT_OK
    s.sync()
    assert np.array_equal(host_states(buf), O.xorwow_init(1, 2 ** 40 - 8, 8))

    # the binding
    with pytest.raises(ValueError):
        s.query_radiance(o.cpu(), d.cpu(), st.cpu())
    with pytest.raises(ValueError):
        s.query_radiance(o, d, st[:4])
    with pytest.raises(ValueError):
        s.query_radiance(o, d, st, out=torch.zeros((4, 8), device="cuda"))
    with pytest.raises(ValueError):
        s.query_radiance(torch.zeros((3, 8), device="cuda").t(), d, st)  # not contiguous
    with pytest.raises(P.PtrtError):
        s.query_radiance(o, d, st, samples=0)
    keep = torch.zeros((8, 8), device="cuda")
    assert s.query_radiance(o, d, st, out=keep) is keep
    assert s.query_radiance(o[:0], d[:0], st[:0]).shape == (0, 8)
    s.close()
