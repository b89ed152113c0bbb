"""TLAS refit on the device over the topology that was uploaded (ptrt_set_instance_transforms, ptrt_refit_tlas, ptrt_read_tlas;
Scene.refitInstanceChanges, the GpuRefitAll policy, the GPU refits / rebuilds behind a TLAS with inner nodes): frames against
the oracle over the host description, bit for bit; the geometry, without any tree, against the float64 brute force
(tests/brute_force.py); and that nothing waits for the stream.  No bound here is tuned against the GPU's output: the frames
are compared for equality, the queries with the constants tests/test_brute_force.py measured on the CPU."""
import ctypes as C

import numpy as np
import pytest

import brute_force as bf
from common import assert_frames_equal
from test_brute_force import COPLANAR, many_proper, plain_rays, ray_sets, truth
from test_brute_force_gpu import judge, judge_current, tall_water
from test_parity_gpu import _many_meshes
from test_ray_query_gpu import VARIANTS

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 88, 64, 2, 4
BASE = 8            # scenes.many / many_proper: the Cornell box's eight meshes come first


def prep(P, s, spp=SPP, depth=DEPTH):
    s.setPerfSamplesPerPixel(spp)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(P.DEFAULT_SEED)
    s.set_option("count_rays", 1)


def frame_both(P, O, s, blue_noise, rng, w=W, h=H, spp=SPP, depth=DEPTH):
    """one frame on the GPU and in the oracle over s.flatten(), from the same generator states (`rng` advances)"""
    fc = s.getFrameCount()
    rgb = s.render_to_host()
    g = dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
             object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats())
    c = O.render(s.flatten(), w, h, spp, depth, fc, blue_noise, rng, threads=8)
    c["rgb8"] = O.tonemap(c["accum"], w, h, threads=8)
    c["rng"] = rng.copy()
    return g, c


def upload_counts(P, s):
    out = (C.c_int * 2)()
    assert P.lib.ptrt_debug_upload_counts(s.ctx, out) == 0
    return out[0], out[1]


def host_tlas(s):
    d = s.flatten()
    n = d.contents.tlas_node_count
    a = np.ctypeslib.as_array(C.cast(d.contents.tlas_nodes, C.POINTER(C.c_int32)), (n, 10)).copy()
    return a[:, :6].copy().view(np.uint32), a[:, 6:]


def assert_device_tlas_is_the_hosts(P, s, topo0):
    box, topo = host_tlas(s)
    dev = s.read_tlas()
    dtopo = np.stack([dev["left"], dev["right"], dev["start"], dev["count"]], axis=1)
    assert np.array_equal(topo, topo0) and np.array_equal(dtopo, topo0), "the TLAS topology is not the upload's"
    dbox = np.concatenate([dev["bmin"], dev["bmax"]], axis=1).view(np.uint32)
    bad = np.flatnonzero((dbox != box).any(axis=1))
    assert bad.size == 0, f"TLAS nodes {bad[:8]} differ between device and host: {dbox[bad[0]].view(np.float32)} vs {box[bad[0]].view(np.float32)}"


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts,leaf", [(30, {}, None), (48, {}, None), (30, dict(pair_trace=0), None), (30, dict(pair_trace=1), None),
                                         (30, dict(force_geom=2), None), (30, dict(tlas_rounds=1), None), (30, {}, (2, 0))],
                         ids=["n30", "n48", "pair_trace0", "pair_trace1", "force_geom2", "tlas_rounds1", "leaf(2,0)"])
def test_frames_after_instance_refits_equal_the_oracle(P, O, blue_noise, n, opts, leaf):
    s = P.Scene(W, H)
    _many_meshes(P, s, n=n)
    if leaf:
        s.setBVHLeafTarget(*leaf)
    prep(P, s)
    for k, v in opts.items():
        s.set_option(k, v)
    cube, sphere, baked = BASE + 0, BASE + 3, BASE + 2      # an instanced cube, an instanced sphere, a cube with baked vertices
    d = s.flatten()
    assert d.contents.tlas_node_count > 1 and d.contents.meshes[baked].has_transform == 0
    assert d.contents.meshes[cube].has_transform == 1 and d.contents.meshes[sphere].has_transform == 1
    _, topo0 = host_tlas(s)
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, W * H)
    frames = []
    for f in range(4):
        if f == 1:
            s.setPosition(cube, (1.5, -1.0, -4.0))
            s.setRotation(cube, (0.4, -0.7, 0.2))
        elif f == 2:
            s.setPosition(sphere, (-2.5, 1.0, -3.0))
            s.setPosition(cube, (1.8, -0.6, -4.5))
            s.setRotation(cube, (0.9, -0.2, 0.5))
        elif f == 3:
            s.setPosition(baked, (0.4, 0.6, 0.9))               # has_transform 0 -> 1
            s.setPosition(sphere, (-3.0, 2.0, -2.5))
        if f:
            s.refitInstanceChanges()
            assert s.getFrameCount() == 0
        g, c = frame_both(P, O, s, blue_noise, rng)
        assert_frames_equal([g], [c])
        frames.append(g)
        assert upload_counts(P, s) == (1, 0)
        assert s.get_option("tlas_refits") == f and s.get_option("inst_pre_ok") == 1
        assert_device_tlas_is_the_hosts(P, s, topo0)
    assert s.flatten().contents.meshes[baked].has_transform == 1
    assert not np.array_equal(frames[0]["object_id"], frames[3]["object_id"]), "nothing moved in the image"
    s.close()


# ---- 2. geometry, no tree ------------------------------------------------------------------------------------------------
def many_proper_transforms(n=64):
    """the (position, rotation or None, scale) many_proper gives its instances, by replaying its draws"""
    rs = np.random.RandomState(3)
    out = {}
    for k in range(n):
        rs.uniform(0.2, 0.9, 3), rs.uniform(0.05, 0.8)
        pos = (float(rs.uniform(-4, 4)), float(rs.uniform(-4.5, 3.5)), float(rs.uniform(-9, -2)))
        rot, scl = tuple(rs.uniform(-1, 1, 3)), tuple(rs.uniform(0.2, 0.5, 3))
        if k % 6 == 0:
            out[BASE + k] = ((0.0, pos[1], pos[2]), rot, scl)
        elif k % 6 == 3:
            out[BASE + k] = (pos, None, scl)
    return out


def test_moved_instances_behind_the_kept_tlas_against_the_brute_force(P):
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    before = bf.Geometry.from_desc(s.flatten())
    assert len(before.meshes) > 17 and s.flatten().contents.tlas_node_count > 1
    box0, topo0 = host_tlas(s)
    moved = inst[:8]
    home = many_proper_transforms()
    for j, m in enumerate(moved):
        rotated = before.meshes[m].world[0, 1] != 0.0 or before.meshes[m].world[0, 2] != 0.0
        assert rotated == (home[m][1] is not None)
        # far outside the room and the old TLAS boxes; a rotated instance stays at x = 0 (the inverse stays a true inverse)
        s.setPosition(m, (0.0, 9.0 + 2.0 * j, 6.0 + j) if rotated else (11.0 + 2.0 * j, -3.0 + j, 5.0 - 2.0 * j))
        s.setInstanceScale(m, (1.5 + 0.25 * j, 1.0, 2.0))
    s.refitInstanceChanges()
    geom = bf.Geometry.from_desc(s.flatten())
    assert all(m.proper for m in geom.meshes) and geom.radius > before.radius + 5.0
    assert upload_counts(P, s) == (1, 0)
    assert_device_tlas_is_the_hosts(P, s, topo0)
    sets = []
    for kind, (o, d, mesh, face, small) in ray_sets(geom, "many", seed=7).items():
        c, tmax, a = truth(geom, o, d, mesh, face, small, ties=COPLANAR["many-proper"])
        sets.append((kind, o, d, c, tmax, a))
    kind, o, d, c, *_ = sets[1]
    assert np.isin(c["mesh"][c["decided"]], moved).sum() >= 8 * 12      # the moved instances are found where they are now
    for fg, pt in VARIANTS:
        s.set_option("force_geom", fg)
        s.set_option("pair_trace", pt)
        judge(s, geom, sets, f"instances refitted away force_geom={fg} pair_trace={pt}")
    # ... and back home: the boxes shrink to exactly the built ones
    for m in moved:
        pos, rot, scl = home[m]
        s.setPosition(m, pos)
        s.setInstanceScale(m, scl)
    s.refitInstanceChanges()
    back = bf.Geometry.from_desc(s.flatten())
    for m in moved:
        assert np.array_equal(back.meshes[m].world, before.meshes[m].world), f"mesh {m} is not where it was built"
    box1, _ = host_tlas(s)
    assert np.array_equal(box0, box1), "the refitted TLAS of the unmoved scene is not the built one"
    assert_device_tlas_is_the_hosts(P, s, topo0)
    assert upload_counts(P, s) == (1, 0) and s.get_option("tlas_refits") == 2
    sets = []
    for kind, (o, d, mesh, face, small) in ray_sets(back, "many", seed=7).items():
        c, tmax, a = truth(back, o, d, mesh, face, small, ties=COPLANAR["many-proper"])
        sets.append((kind, o, d, c, tmax, a))
    kind, o, d, c, *_ = sets[1]
    assert np.isin(c["mesh"][c["decided"]], moved).sum() >= 8 * 12
    for fg, pt in VARIANTS:
        s.set_option("force_geom", fg)
        s.set_option("pair_trace", pt)
        judge(s, back, sets, f"instances refitted home force_geom={fg} pair_trace={pt}")
    s.close()


# ---- 3. a deforming mesh behind a real TLAS --------------------------------------------------------------------------------
def fluid_among_cubes(P, s):
    """scenes.fluid (water grid + ship) and twenty small cubes high above the waves: 22 meshes, a TLAS with inner nodes"""
    w, ship = P.scenes.fluid(s, cells=40, t=0.0, ship_segments=24)
    rs = np.random.RandomState(17)
    for k in range(20):
        m = s.addCube(P.Material(tuple(rs.uniform(0.2, 0.9, 3)), 0.5))
        s.scale(m, tuple(rs.uniform(0.4, 0.9, 3)))
        s.moveTo(m, (-14.0 + 3.0 * (k % 10) + float(rs.uniform(-0.5, 0.5)), 10.0 + 2.0 * (k // 10), -6.0 + 5.0 * (k % 3)))
    return w, ship


def test_gpu_refits_and_rebuilds_behind_a_real_tlas_against_the_brute_force(P, O, blue_noise):
    import torch
    s = P.Scene(W, H)
    w, ship = fluid_among_cubes(P, s)
    prep(P, s)
    s.setDynamicGeometryPolicy("GpuRefitAll")       # (for the host description at the end; the calls below do not consult it)
    assert s.flatten().contents.mesh_count > 17 and s.flatten().contents.tlas_node_count > 1
    _, topo0 = host_tlas(s)
    judge_current(s, "real TLAS, built")

    v = tall_water(2.7, 5.0)
    dev = torch.from_numpy(v).cuda()
    s.refitFromDevice(w, dev.data_ptr())
    assert s.get_option("inst_pre_ok") == 1
    geom, _ = judge_current(s, "real TLAS, refitFromDevice", {w: v})
    assert np.abs(geom.meshes[w].verts[:, 1]).max() > 2.0

    v = tall_water(3.4, 9.0)
    buf = torch.from_numpy(v.copy())
    s.refitFromHost(w, buf.data_ptr())
    assert s.get_option("inst_pre_ok") == 1
    geom, _ = judge_current(s, "real TLAS, refitFromHost", {w: v})
    assert np.abs(geom.meshes[w].verts[:, 1]).max() > 4.0

    v = tall_water(2.2, 3.0)
    dev2 = torch.from_numpy(v).cuda()
    s.rebuildFromDevice(w, dev2.data_ptr())
    assert s.get_option("inst_pre_ok") == 1
    judge_current(s, "real TLAS, rebuildFromDevice", {w: v})

    s.setVertices(w, tall_water(0.8, 6.0))
    s.rebuildObjectChanges(False)
    assert s.get_option("inst_pre_ok") == 1
    judge_current(s, "real TLAS, rebuildObjectChanges(False)")
    assert upload_counts(P, s) == (1, 0)
    assert_device_tlas_is_the_hosts(P, s, topo0)

    # one full frame after refitFromDevice, against the oracle over the host description with those vertices: the host gets
    # them afterwards through the GpuRefitAll commit (same positions, so the device's boxes do not change), which keeps every
    # topology and lets flatten() follow the device
    v = tall_water(1.6, 4.0)
    dev3 = torch.from_numpy(v).cuda()
    s.refitFromDevice(w, dev3.data_ptr())
    s.reset_rng(P.DEFAULT_SEED)
    assert s.getFrameCount() == 0
    rgb = s.render_to_host()
    g = dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
             object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats())
    s.setVertices(w, v)
    s.commitObjectChanges()
    assert upload_counts(P, s) == (1, 0)
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, W * H)
    c = O.render(s.flatten(), W, H, SPP, DEPTH, 0, blue_noise, rng, threads=8)
    c["rgb8"] = O.tonemap(c["accum"], W, H, threads=8)
    c["rng"] = rng.copy()
    assert_frames_equal([g], [c])
    assert (g["object_id"] == w).sum() > 100
    assert_device_tlas_is_the_hosts(P, s, topo0)
    s.close()


# ---- 4. the GpuRefitAll policy ---------------------------------------------------------------------------------------------
def blob_scene(P, s):
    _many_meshes(P, s, n=24)
    return s.addSphere(16, P.Material((0.8, 0.4, 0.1), 0.3))


def blob_vertices(P, s, blob):
    md = s.flatten().contents.meshes[blob]
    return np.ctypeslib.as_array(C.cast(md.verts, C.POINTER(C.c_float)), (md.vert_count, 3)).copy()


def test_commit_under_gpu_refit_all_uploads_nothing_and_equals_the_oracle(P, O, blue_noise):
    """The caller's unchanged sequence -- setPosition, setVertices, commitObjectChanges() -- under GpuRefitAll: upload counts stay
    (1, 0) and every frame is the oracle's.  Under the default policy the same sequence re-uploads the geometry with every
    commit, as the parent commit does: the counts are (1 + k, 0) after k commits (a rewritten mesh makes the commit a geometry
    upload, which carries the instances along), and commits that only move an instance count (1, k)."""
    s = P.Scene(W, H)
    blob = blob_scene(P, s)
    prep(P, s)
    s.setDynamicGeometryPolicy("GpuRefitAll")
    base = blob_vertices(P, s, blob)
    cube = BASE + 0
    _, topo0 = host_tlas(s)
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, W * H)

    def step(sc, f):
        sc.setPosition(cube, (1.0 + 0.5 * f, -1.0 + 0.3 * f, -4.0))
        v = base * np.float32(1.0 + 0.4 * f) + np.array([0.6 * f, -0.3 * f, -4.0 - f], np.float32)
        sc.setVertices(blob, v.astype(np.float32))
        sc.commitObjectChanges()

    for f in range(4):
        if f:
            step(s, f)
        g, c = frame_both(P, O, s, blue_noise, rng)
        assert_frames_equal([g], [c])
        assert upload_counts(P, s) == (1, 0), f"frame {f}"
        assert_device_tlas_is_the_hosts(P, s, topo0)
    assert (g["object_id"] == blob).sum() > 20 and s.get_option("tlas_refits") == 3
    assert s.commitCounts() == (3, 1)
    s.close()

    r = P.Scene(W, H)
    blob_scene(P, r)
    prep(P, r)
    for f in range(1, 4):
        step(r, f)
        r.render_to_host()
        assert upload_counts(P, r) == (1 + f, 0)
    assert r.get_option("tlas_refits") == 0
    r.close()
    r = P.Scene(W, H)
    blob_scene(P, r)
    prep(P, r)
    for f in range(1, 4):
        r.setPosition(cube, (1.0 + 0.5 * f, -1.0 + 0.3 * f, -4.0))
        r.commitObjectChanges()
        r.render_to_host()
        assert upload_counts(P, r) == (1, f)
    r.close()


# ---- 5. the calls do not wait ----------------------------------------------------------------------------------------------
def test_instance_refit_returns_while_the_stream_is_busy(P):
    import torch
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    st = torch.cuda.Stream()
    s.set_stream(st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # calibrate the sleep on this device: no clock rate is assumed
    probe = 20_000_000
    with torch.cuda.stream(st):
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
    st.synchronize()
    probe_ms = e0.elapsed_time(e1)
    assert probe_ms > 0.0
    cycles = int(probe * 200.0 / probe_ms)               # aim at 200 ms
    home = many_proper_transforms()
    moved = [m for m in inst if home[m][1] is None][:3]   # unrotated instances: any translation keeps a true inverse
    s.setPosition(moved[0], (1.0, 1.0, -4.0))
    s.refitInstanceChanges()                              # the first call allocates the staging memory; the ones below must not
    for j, m in enumerate(moved):
        s.setPosition(m, (2.0 - 1.5 * j, 1.0 + 0.5 * j, -3.0 - j))
        s.setInstanceScale(m, (1.5, 1.2, 1.5))
    with torch.cuda.stream(st):
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
    s.refitInstanceChanges()                              # ptrt_set_instance_transforms per run + ptrt_refit_tlas
    assert P.lib.ptrt_refit_tlas(s.ctx) == 0
    busy = not st.query()
    st.synchronize()
    slept = e0.elapsed_time(e1)
    assert slept >= 100.0, f"the sleep took {slept:.1f} ms: the check proves nothing"
    assert busy, "ptrt_set_instance_transforms / ptrt_refit_tlas returned only after the stream had drained"
    assert s.get_option("tlas_refits") == 3
    geom = bf.Geometry.from_desc(s.flatten())
    assert all(m.proper for m in geom.meshes)
    o, d = plain_rays("many", 4096, 5)
    c, tmax, a = truth(geom, o, d)
    assert np.isin(c["mesh"][c["decided"]], moved).sum() > 0
    judge(s, geom, [("plain", o, d, c, tmax, a)], "after a refit behind a busy stream")
    s.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    s = P.Scene(32, 32)
    _many_meshes(P, s, n=20)
    xf = (P.InstanceXform * 4)()
    nodes = (P.BvhNode * 64)()
    assert P.lib.ptrt_set_instance_transforms(s.ctx, 0, 1, xf) == -4        # PTRT_E_NOT_READY
    assert P.lib.ptrt_refit_tlas(s.ctx) == -4
    assert P.lib.ptrt_read_tlas(s.ctx, nodes, 1) == -4
    s.uploadToGPU()
    n = s.flatten().contents.mesh_count
    for args in ((n - 1, 2, xf), (n, 1, xf), (-1, 1, xf), (0, -1, xf), (0, 1, None), (0, n + 1, xf)):
        assert P.lib.ptrt_set_instance_transforms(s.ctx, *args) == -1, args    # PTRT_E_INVALID
        assert b"ptrt_set_instance_transforms" in P.lib.ptrt_last_error(s.ctx)
    # nothing was enqueued or noted: the first-pass boxes are still the upload's, no refit was counted
    assert s.get_option("inst_pre_ok") == 1 and s.get_option("tlas_refits") == 0
    k = s.flatten().contents.tlas_node_count
    assert k > 1
    for bad in (k - 1, k + 1, 0, -3):
        assert P.lib.ptrt_read_tlas(s.ctx, nodes, bad) == -1
        assert b"ptrt_read_tlas" in P.lib.ptrt_last_error(s.ctx)
    assert P.lib.ptrt_read_tlas(s.ctx, None, k) == -1
    assert P.lib.ptrt_set_instance_transforms(s.ctx, 0, 0, xf) == 0           # an empty range is no error and no work
    assert s.get_option("inst_pre_ok") == 1
    assert P.lib.ptrt_refit_tlas(None) == -1
    # the TLAS read back right after the upload is the uploaded one
    box, topo = host_tlas(s)
    dev = s.read_tlas()
    assert np.array_equal(np.concatenate([dev["bmin"], dev["bmax"]], axis=1).view(np.uint32), box)
    assert P.lib.ptrt_refit_tlas(s.ctx) == 0                                   # ... and a refit of the unmoved scene leaves it so
    dev = s.read_tlas()
    assert np.array_equal(np.concatenate([dev["bmin"], dev["bmax"]], axis=1).view(np.uint32), box)
    assert np.array_equal(np.stack([dev["left"], dev["right"], dev["start"], dev["count"]], axis=1), topo)
    s.close()


# ---- 7. a single-leaf TLAS -------------------------------------------------------------------------------------------------
def test_single_leaf_scene_through_the_abi_equals_the_commit(P, O, blue_noise):
    """Cornell (8 meshes, one TLAS leaf): a box moved with commitObjectChanges() in one scene, and in a twin by handing the same
    matrices to ptrt_set_instance_transforms + ptrt_refit_tlas (the twin's host scene never hears of the move, so its renders
    commit nothing): the same frames, bit for bit."""
    a, b = P.Scene(W, H), P.Scene(W, H)
    for s in (a, b):
        P.scenes.cornell(s)
        prep(P, s)
    box = 6
    frames = {0: [], 1: []}
    for f in range(3):
        if f:
            a.setPosition(box, (0.8 * f, 0.5, -0.6 * f))
            a.setRotation(box, (0.0, 0.3 * f, 0.1))
            a.commitObjectChanges()
            md = a.flatten().contents.meshes[box]
            x = P.InstanceXform()
            C.memmove(x.world, md.world, 64)
            C.memmove(x.inverse, md.inverse, 64)
            C.memmove(x.normal, md.normal, 64)
            x.has_transform = md.has_transform
            assert x.has_transform == 1
            assert P.lib.ptrt_set_instance_transforms(b.ctx, box, 1, C.byref(x)) == 0
            assert b.get_option("inst_pre_ok") == 0
            assert P.lib.ptrt_refit_tlas(b.ctx) == 0
            b.setFrameCount(0)                              # (a's commit restarted its accumulation)
        for k, s in enumerate((a, b)):
            rgb = s.render_to_host()
            frames[k].append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                                  object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats()))
    assert_frames_equal(frames[1], frames[0])
    assert not np.array_equal(frames[0][0]["object_id"], frames[0][2]["object_id"])
    assert upload_counts(P, a) == (1, 2) and upload_counts(P, b) == (1, 0)
    ra, rb = a.read_tlas(), b.read_tlas()
    assert len(ra) == 1 and ra.tobytes() == rb.tobytes()
    a.close()
    b.close()
