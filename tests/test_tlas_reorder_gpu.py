"""Re-ordering the TLAS on the device (ptrt_reorder_tlas, ptrt_read_tlas_order; Scene.reorderTLAS / read_tlas_order): the order
the device holds against the numpy restatement (tests/tlas_reorder_restatement.py) and the host twin, exactly; the boxes
against the host refit, bit for bit; frames against the oracle over the host description, bit for bit; the geometry against the
float64 brute force; graph replay; more meshes than the one-workgroup sort takes; and that nothing waits for the stream.
Nothing here is tuned against the GPU's output."""
import ctypes as C

import numpy as np
import pytest

import brute_force as bf
import tlas_reorder_restatement as R
from common import assert_frames_equal
from test_brute_force import COPLANAR, many_proper, plain_rays, ray_sets, truth
from test_brute_force_gpu import judge
from test_parity_gpu import _many_meshes
from test_ray_query_gpu import VARIANTS
from test_tlas_refit_gpu import (BASE, H, W, assert_device_tlas_is_the_hosts, frame_both, host_tlas, many_proper_transforms, prep,
                                 upload_counts)

pytestmark = pytest.mark.gpu


def assert_order_everywhere(s, what=""):
    """device == numpy restatement == host twin; returns the order"""
    want, host = R.order_of(s)
    dev = s.read_tlas_order()
    assert np.array_equal(dev, want), f"{what}: device order {dev} is not the restatement's {want}"
    assert np.array_equal(dev, host), f"{what}: device order {dev} is not the host twin's {host}"
    return dev


def move_three(s, f):
    """the moves of test_tlas_refit_gpu.test_frames_after_instance_refits_equal_the_oracle before frame f"""
    cube, sphere, baked = BASE + 0, BASE + 3, BASE + 2
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


def four_frames(P, O, blue_noise, s, graphs=None):
    """four frames, reorderTLAS() before frames 1-3; every equality of case 1.  `graphs`: use_graphs per re-order."""
    _, topo0 = host_tlas(s)
    built = s.read_tlas_order()
    assert np.array_equal(built, R.order_of(s)[1])
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, W * H)
    frames, orders = [], [built]
    for f in range(4):
        move_three(s, f)
        if f:
            if graphs:
                s.set_option("use_graphs", graphs[f - 1])
            s.reorderTLAS()
            assert s.getFrameCount() == 0
            orders.append(assert_order_everywhere(s, f"frame {f}"))
        g, c = frame_both(P, O, s, blue_noise, rng)
        assert_frames_equal([g], [c])
        frames.append(g)
        assert upload_counts(P, s) == (1, 0)
        assert s.get_option("tlas_reorders") == f and s.get_option("tlas_refits") == 0 and s.get_option("inst_pre_ok") == 1
        assert_device_tlas_is_the_hosts(P, s, topo0)
    assert not np.array_equal(orders[1], built), "the built order already was the Morton order"
    assert not np.array_equal(frames[0]["object_id"], frames[3]["object_id"]), "nothing moved in the image"


# ---- 1. exact order and frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts,leaf", [(18, {}, None), (30, {}, None), (48, {}, None), (30, dict(pair_trace=0), None),
                                         (30, dict(pair_trace=1), None), (30, dict(force_geom=2), None), (30, dict(tlas_rounds=1), None),
                                         (30, {}, (2, 0))],
                         ids=["n18", "n30", "n48", "pair_trace0", "pair_trace1", "force_geom2", "tlas_rounds1", "leaf(2,0)"])
def test_order_boxes_and_frames_after_reorders(P, O, blue_noise, n, opts, leaf):
    s = P.Scene(W, H)
    _many_meshes(P, s, n=n)
    if leaf:
        s.setBVHLeafTarget(*leaf)
    prep(P, s)
    for k, v in opts.items():
        s.set_option(k, v)
    assert s.flatten().contents.tlas_node_count > 1
    four_frames(P, O, blue_noise, s)
    s.close()


# ---- 2. geometry, no tree ----------------------------------------------------------------------------------------------------
def judged_sets(geom):
    sets = []
    for kind, (o, d, mesh, face, small) in ray_sets(geom, "many", seed=7).items():
        c, tmax, a = truth(geom, o, d, mesh, face, small, ties=COPLANAR["many-proper"])
        sets.append((kind, o, d, c, tmax, a))
    return sets


def test_scrambled_instances_against_the_brute_force(P):
    s = P.Scene(64, 64)
    many_proper(P, s)
    s.uploadToGPU()
    built = bf.Geometry.from_desc(s.flatten())
    _, topo0 = host_tlas(s)
    home = many_proper_transforms()
    for back in (False, True):
        R.scramble(s, home, back=back)
        s.reorderTLAS()
        geom = bf.Geometry.from_desc(s.flatten())
        assert all(m.proper for m in geom.meshes)
        order = assert_order_everywhere(s, "home" if back else "scrambled")
        assert_device_tlas_is_the_hosts(P, s, topo0)
        assert upload_counts(P, s) == (1, 0)
        if back:                                              # the order of the BUILT scene's numpy restatement
            for m in home:
                assert np.array_equal(geom.meshes[m].world, built.meshes[m].world), f"mesh {m} is not where it was built"
            assert np.array_equal(order, R.tlas_morton_order(*R.desc_boxes_and_rows(s.flatten())))
        sets = judged_sets(geom)
        for fg, pt in VARIANTS:
            s.set_option("force_geom", fg)
            s.set_option("pair_trace", pt)
            judge(s, geom, sets, f"instances {'home' if back else 'scrambled'}, re-ordered, force_geom={fg} pair_trace={pt}")
    assert s.get_option("tlas_reorders") == 2
    s.close()


# ---- 3. graph replay ---------------------------------------------------------------------------------------------------------
def test_reorders_replayed_as_graphs(P, O, blue_noise):
    s = P.Scene(W, H)
    _many_meshes(P, s, n=30)
    prep(P, s)
    four_frames(P, O, blue_noise, s, graphs=(1, 1, 0))
    s.close()


# ---- 4. more meshes than the one-workgroup sort takes --------------------------------------------------------------------------
def test_wide_path(P):
    """4100 one-triangle meshes (the radix path starts above pt::TLAS_WIDE = 4096).  Building the scene through the mirror,
    flatten() and the host re-order take 0.1 s on the CPU here; the float64 brute force over 4100 meshes takes about 8 s."""
    n = 4100
    rs = np.random.RandomState(9)
    s = P.Scene(32, 32)
    mat = P.Material((0.6, 0.6, 0.6), 0.5)
    at = rs.uniform(-8, 8, (n, 1, 3)).astype(np.float32)
    tris = at + rs.uniform(-0.3, 0.3, (n, 3, 3)).astype(np.float32)
    for k in range(n):
        s.addTriangles(tris[k].reshape(1, 9), mat)
    s.setCamera((0, 0, 20), (0, 0, 0), (0, 1, 0), 40.0)
    s.uploadToGPU()
    _, topo0 = host_tlas(s)
    movers = list(range(0, n, 7))
    for m in movers:                                          # translations only: every inverse stays a true inverse
        s.setPosition(m, tuple(rs.uniform(-6, 6, 3)))
    s.reorderTLAS()
    order = assert_order_everywhere(s, "4100 meshes")
    assert sorted(order.tolist()) == list(range(n)) and not np.array_equal(order, np.arange(n))
    assert_device_tlas_is_the_hosts(P, s, topo0)
    assert upload_counts(P, s) == (1, 0) and s.get_option("tlas_reorders") == 1
    geom = bf.Geometry.from_desc(s.flatten())
    assert all(m.proper for m in geom.meshes)
    o = np.tile(np.array([0.0, 0.0, 30.0], np.float32), (4096, 1))
    to = rs.uniform(-8, 8, (4096, 3))
    d = (to - o).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    c, tmax, a = truth(geom, o, d)
    assert c["hit"].mean() > 0.2
    judge(s, geom, [("plain", o, d, c, tmax, a)], "4100 meshes re-ordered")
    s.close()


# ---- 5. the call does not wait -------------------------------------------------------------------------------------------------
def test_reorder_returns_while_the_stream_is_busy(P):
    import torch
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    st = torch.cuda.Stream()
    s.set_stream(st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 20_000_000                                     # calibrate the sleep on this device: no clock rate is assumed
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
    s.reorderTLAS()                                       # the first call allocates the staging memory; the ones below must not
    for j, m in enumerate(moved):
        s.setPosition(m, (2.0 - 1.5 * j, 1.0 + 0.5 * j, -3.0 - j))
        s.setInstanceScale(m, (1.5, 1.2, 1.5))
    with torch.cuda.stream(st):
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
    s.reorderTLAS()                                       # ptrt_set_instance_transforms per run + ptrt_reorder_tlas
    assert P.lib.ptrt_reorder_tlas(s.ctx) == 0
    busy = not st.query()
    st.synchronize()
    slept = e0.elapsed_time(e1)
    assert slept >= 100.0, f"the sleep took {slept:.1f} ms: the check proves nothing"
    assert busy, "ptrt_set_instance_transforms / ptrt_reorder_tlas returned only after the stream had drained"
    assert s.get_option("tlas_reorders") == 3
    assert_order_everywhere(s, "behind a busy stream")
    geom = bf.Geometry.from_desc(s.flatten())
    assert all(m.proper for m in geom.meshes)
    o, d = plain_rays("many", 4096, 5)
    c, tmax, a = truth(geom, o, d)
    assert np.isin(c["mesh"][c["decided"]], moved).sum() > 0
    judge(s, geom, [("plain", o, d, c, tmax, a)], "after a re-order behind a busy stream")
    s.close()


def test_device_transforms_return_while_the_stream_is_busy(P):
    """set_instance_transforms_device + ptrt_reorder_tlas behind a sleeping stream: both return while it sleeps"""
    import torch
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    st = torch.cuda.Stream()
    s.set_stream(st.cuda_stream)
    home = many_proper_transforms()
    moved = [m for m in inst if home[m][1] is None][:3]
    t = P.Scene(32, 32, device=P.HOST_ONLY)                 # a host twin computes the matrices
    many_proper(P, t)
    for j, m in enumerate(moved):
        t.setPosition(m, (2.0 - 1.5 * j, 1.0 + 0.5 * j, -3.0 - j))
        t.setInstanceScale(m, (1.5, 1.2, 1.5))
    recs = xform_records(P, t.flatten()).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 20_000_000                                     # calibrate the sleep on this device: no clock rate is assumed
    with torch.cuda.stream(st):
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
    st.synchronize()
    probe_ms = e0.elapsed_time(e1)
    assert probe_ms > 0.0
    cycles = int(probe * 200.0 / probe_ms)               # aim at 200 ms
    with torch.cuda.stream(st):
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        s.set_instance_transforms_device(0, recs)
    assert P.lib.ptrt_reorder_tlas(s.ctx) == 0
    busy = not st.query()
    st.synchronize()
    slept = e0.elapsed_time(e1)
    assert slept >= 100.0, f"the sleep took {slept:.1f} ms: the check proves nothing"
    assert busy, "ptrt_set_instance_transforms_device / ptrt_reorder_tlas returned only after the stream had drained"
    assert s.get_option("inst_pre_ok") == 1 and upload_counts(P, s) == (1, 0)
    assert np.array_equal(s.read_tlas_order(), R.tlas_morton_order(*R.desc_boxes_and_rows(t.flatten())))
    geom = bf.Geometry.from_desc(t.flatten())
    assert all(m.proper for m in geom.meshes)
    o, d = plain_rays("many", 4096, 5)
    c, tmax, a = truth(geom, o, d)
    assert np.isin(c["mesh"][c["decided"]], moved).sum() > 0
    judge(s, geom, [("plain", o, d, c, tmax, a)], "device transforms behind a busy stream")
    s.close()
    t.close()


# ---- 6. device-resident transforms ------------------------------------------------------------------------------------------------
def xform_records(P, d):
    """every mesh's ptrt_instance_xform record from a flattened scene: a (mesh_count, 49) int32 torch tensor on the host"""
    import torch
    n = d.contents.mesh_count
    xf = (P.InstanceXform * n)()
    for m in range(n):
        md = d.contents.meshes[m]
        C.memmove(xf[m].world, md.world, 64)
        C.memmove(xf[m].inverse, md.inverse, 64)
        C.memmove(xf[m].normal, md.normal, 64)
        xf[m].has_transform = md.has_transform
    assert C.sizeof(xf) == n * 196
    return torch.from_numpy(np.frombuffer(xf, dtype=np.int32).reshape(n, 49).copy())


def test_device_resident_transforms_equal_the_host_call(P, O, blue_noise):
    """Scene a moves its instances and calls reorderTLAS(); its twin b never hears of the moves on the host: it gets a's
    records as a device tensor (set_instance_transforms_device) and ptrt_reorder_tlas.  Same frames, same TLAS, bit for bit."""
    import torch
    a, b = P.Scene(W, H), P.Scene(W, H)
    for s in (a, b):
        _many_meshes(P, s, n=30)
        prep(P, s)
    frames = {0: [], 1: []}
    for f in range(4):
        move_three(a, f)
        if f:
            a.reorderTLAS()
            recs = xform_records(P, a.flatten()).cuda()
            if f == 2:                                         # a sub-range and another dtype: the moved cube alone
                b.set_instance_transforms_device(BASE + 0, recs[BASE + 0:BASE + 1].view(torch.uint8))
                b.set_instance_transforms_device(BASE + 1, recs[BASE + 1:])
            else:
                b.set_instance_transforms_device(0, recs)
            assert b.get_option("inst_pre_ok") == 0
            assert P.lib.ptrt_reorder_tlas(b.ctx) == 0
            b.setFrameCount(0)                                # (a's re-order restarted its accumulation)
        for k, s in enumerate((a, b)):
            rgb = s.render_to_host()
            frames[k].append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                                  object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats()))
        ra, rb = a.read_tlas(), b.read_tlas()
        assert ra.tobytes() == rb.tobytes(), f"frame {f}: the TLAS differs between the host call and the device call"
        assert np.array_equal(a.read_tlas_order(), b.read_tlas_order())
        assert upload_counts(P, b) == (1, 0) and b.get_option("tlas_reorders") == f and b.get_option("inst_pre_ok") == 1
    assert_frames_equal(frames[1], frames[0])
    assert not np.array_equal(frames[0][0]["object_id"], frames[0][3]["object_id"]), "nothing moved in the image"
    # a material upload rewrites the flag words from the host copy: it must fetch what only the device knew (the baked cube's
    # has_transform went 0 -> 1 on the device alone)
    for s in (a, b):                                          # (transmissive: the mesh's shadow-skip flag bit changes)
        s.setMeshMaterial(BASE + 5, P.Material((0.9, 0.1, 0.1), 0.4, transmission=1.0, ior=1.4))
    out = []
    for s in (a, b):
        s.reset_rng(P.DEFAULT_SEED)
        s.setFrameCount(0)
        rgb = s.render_to_host()
        out.append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                        object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats()))
    assert_frames_equal([out[1]], [out[0]])
    a.close()
    b.close()


def test_device_transform_tensors_are_checked(P):
    import torch
    s = P.Scene(32, 32)
    _many_meshes(P, s, n=20)
    s.uploadToGPU()
    good = xform_records(P, s.flatten())
    for bad in (good, good.cuda()[:, :48], good.cuda().t(), good.cuda().reshape(-1), good.cuda().to(torch.int64), np.zeros((2, 49), np.int32)):
        with pytest.raises(ValueError):
            s.set_instance_transforms_device(0, bad)
    s.set_instance_transforms_device(0, good.cuda().view(torch.float32))
    assert P.lib.ptrt_refit_tlas(s.ctx) == 0
    s.sync()
    s.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(P, O, blue_noise):
    s = P.Scene(W, H)
    _many_meshes(P, s, n=20)
    ids = (C.c_int32 * 64)()
    assert P.lib.ptrt_reorder_tlas(s.ctx) == -4                                # PTRT_E_NOT_READY
    assert P.lib.ptrt_read_tlas_order(s.ctx, ids, 1) == -4
    assert P.lib.ptrt_reorder_tlas(None) == -1
    assert P.lib.ptrt_set_instance_transforms_device(s.ctx, 0, 1, C.c_void_p(256)) == -4
    prep(P, s)
    d = s.flatten().contents
    n = d.tlas_index_count
    assert n == d.mesh_count == 28
    for bad in (n - 1, n + 1, 0, -3):
        assert P.lib.ptrt_read_tlas_order(s.ctx, ids, bad) == -1                # PTRT_E_INVALID
        assert b"ptrt_read_tlas_order" in P.lib.ptrt_last_error(s.ctx)
    assert P.lib.ptrt_read_tlas_order(s.ctx, None, n) == -1
    # device transforms with a bad range: refused before anything is read (the pointer is never followed)
    some = C.c_void_p(256)
    for args in ((n - 1, 2, some), (n, 1, some), (-1, 1, some), (0, -1, some), (0, 1, None), (0, n + 1, some)):
        assert P.lib.ptrt_set_instance_transforms_device(s.ctx, *args) == -1, args
        assert b"ptrt_set_instance_transforms_device" in P.lib.ptrt_last_error(s.ctx)
    assert P.lib.ptrt_set_instance_transforms_device(s.ctx, 0, 0, some) == 0        # an empty range is no error and no work
    assert s.get_option("inst_pre_ok") == 1
    built = s.read_tlas_order()
    assert np.array_equal(built, R.order_of(s)[1])
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, W * H)
    g0, c0 = frame_both(P, O, s, blue_noise, rng)
    assert_frames_equal([g0], [c0])
    # the same TLAS through the raw ABI with one mesh index repeated: valid to upload and to render, refused by the re-order
    twice = built.copy()
    twice[1] = twice[0]
    assert P.lib.ptrt_update_instances(s.ctx, d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count,
                                       twice.ctypes.data_as(C.POINTER(C.c_int32)), n) == 0
    s.reset_rng(P.DEFAULT_SEED)
    s.setFrameCount(0)
    before = s.render_to_host().copy()
    assert P.lib.ptrt_reorder_tlas(s.ctx) == -1
    assert b"ptrt_reorder_tlas" in P.lib.ptrt_last_error(s.ctx) and b"permutation" in P.lib.ptrt_last_error(s.ctx)
    assert s.get_option("tlas_reorders") == 0
    assert np.array_equal(s.read_tlas_order(), twice)
    s.reset_rng(P.DEFAULT_SEED)
    s.setFrameCount(0)
    assert np.array_equal(s.render_to_host(), before), "a refused re-order changed the frame"
    assert P.lib.ptrt_refit_tlas(s.ctx) == 0                                    # the refit takes any TLAS, as before
    s.close()


def test_single_leaf_tlas_keeps_its_order(P, O, blue_noise):
    """12 meshes, one TLAS leaf: the call succeeds, nothing is re-dealt, frames equal the oracle over the unchanged order."""
    s = P.Scene(W, H)
    _many_meshes(P, s, n=4)
    prep(P, s)
    d = s.flatten().contents
    assert d.mesh_count == 12 and d.tlas_node_count == 1
    order0 = s.read_tlas_order()
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, W * H)
    for f in range(2):
        if f:
            s.setPosition(BASE + 0, (1.5, -1.0, -4.0))
            s.reorderTLAS()
            assert s.get_option("tlas_reorders") == 1 and s.get_option("inst_pre_ok") == 1
            assert np.array_equal(s.read_tlas_order(), order0) and np.array_equal(R.order_of(s)[1], order0)
        g, c = frame_both(P, O, s, blue_noise, rng)
        assert_frames_equal([g], [c])
    assert upload_counts(P, s) == (1, 0)
    s.close()
