"""Instance poses on the device (ptrt_set_instance_poses_device, ptrt_read_instance_transforms; Scene.set_instance_poses_device /
read_instance_transforms): the matrices the device derives against the numpy restatement of the reference's arithmetic
(tests/pose_restatement.py), bit for bit; frames and TLAS against a twin that takes the same matrices through
ptrt_set_instance_transforms, byte for byte; the geometry, without any tree, against the float64 brute force; that nothing
waits for the stream or uploads; and the refusals.  Nothing here is tuned against the GPU's output."""
import ctypes as C

import numpy as np
import pytest

import brute_force as bf
import pose_restatement as R
import tlas_reorder_restatement as TR
from common import assert_frames_equal
from test_brute_force import COPLANAR, many_proper, ray_sets, truth
from test_brute_force_gpu import judge
from test_parity_gpu import _many_meshes
from test_ray_query_gpu import VARIANTS
from test_tlas_refit_gpu import BASE, H, W, many_proper_transforms, prep, upload_counts

pytestmark = pytest.mark.gpu

POSE_BYTES = 36


def pose_tensor(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, np.float32).reshape(-1, 9)).cuda()


def raw_records(P, s, first=0, count=None):
    """ptrt_read_instance_transforms as the C ABI returns it: an array of ptrt_instance_xform"""
    n = s.flatten().contents.mesh_count - first if count is None else count
    xf = (P.InstanceXform * n)()
    assert P.lib.ptrt_read_instance_transforms(s.ctx, first, n, C.cast(xf, C.c_void_p)) == 0, P.lib.ptrt_last_error(s.ctx)
    return xf


def same_bits(a, b):
    """equal in every bit, a NaN standing for any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- 1. matrices, bit for bit -------------------------------------------------------------------------------------------------
FAR_GLASS, FAR_OPAQUE = 8, 9          # rows of the table below


def pose_table():
    """(n, 9): the quirk cases of tests/test_pose_restatement.py, two poses far outside everything, random poses, angles beyond
    +-2 pi, and one pose with a NaN in scale.y"""
    rs = np.random.RandomState(21)
    unit = [0, 0, 0, 0, 0, 0, 1, 1, 1]

    def row(**kw):
        r = np.array(unit, np.float32)
        for k, v in kw.items():
            r[dict(pos=0, rot=3, scl=6)[k]:][:3] = v
        return r
    quirks = [row(scl=(1e-4, 1e-4, 1e-4)), row(pos=(0.0009, 0, 0)), row(pos=(0, 0.0011, 0)), row(rot=(0, 0.0009, 0)),
              row(rot=(0, 0, 0.0011)), row(scl=(1, 2, 1)), row(scl=(1.002, 1, 1)), row(),
              row(pos=(200, 0, 0)), row(pos=(-200, 0, 0))]
    n = 240
    rand = np.concatenate([rs.uniform(-10, 10, (n, 3)), rs.uniform(-np.pi, np.pi, (n, 3)), rs.uniform(0.2, 3.0, (n, 3))], axis=1)
    far = np.concatenate([rs.uniform(-10, 10, (16, 3)), rs.uniform(2 * np.pi, 8 * np.pi, (16, 3)) * rs.choice([-1.0, 1.0], (16, 3)),
                          rs.uniform(0.2, 3.0, (16, 3))], axis=1)
    nan = row(pos=(1, 2, 3), rot=(0.3, 0.2, 0.1), scl=(1.5, np.nan, 0.7))
    return np.concatenate([np.stack(quirks), rand, far, nan[None]]).astype(np.float32)


def test_matrices_equal_the_restatement_bit_for_bit(P, O):
    import torch
    s = P.Scene(32, 32)
    P.scenes.many(s, 300, True)
    s.uploadToGPU()
    d = s.flatten().contents
    n = d.mesh_count
    assert 256 < n <= 4096 and d.tlas_node_count > 1
    table = pose_table()
    T = len(table)
    want = R.compose(table[:, 0:3], table[:, 3:6], table[:, 6:9], R.detmath_sincos(O))
    assert np.isnan(table[T - 1]).sum() == 1 and np.isnan(want[0][T - 1]).any()
    glass, opaque = BASE + 3, BASE + 6          # scenes.many: mesh BASE + k, every k % 7 == 3 transmissive, every k % 3 == 0 an instance
    assert d.materials.transmission[glass] > 0.5 and not d.materials.transmission[opaque] > 0.5
    assert d.meshes[glass].has_transform == 1 and d.meshes[opaque].has_transform == 1
    ranges = [((7, 1), [0]), ((5, 64), 10 + np.arange(64)), ((3, 65), 100 + np.arange(65)), ((44, 256), (20 + np.arange(256)) % T),
              ((43, 257), (150 + np.arange(257)) % T), ((n - 1, 1), [T - 1]), ((0, n), np.arange(n) % T)]
    used = set()
    for (first, count), rows in ranges:
        rows = np.array(rows)
        if (first, count) == (5, 64):
            rows[glass - first], rows[opaque - first] = FAR_GLASS, FAR_OPAQUE
        used |= set(rows.tolist())
        before = s.read_instance_transforms()
        s.set_instance_poses_device(first, pose_tensor(table[rows]))
        assert s.get_option("inst_pre_ok") == 0
        got = s.read_instance_transforms()
        assert len(got) == n
        inside = np.zeros(n, bool)
        inside[first:first + count] = True
        for k, name in enumerate(("world", "inverse", "normal")):
            for j in range(count):
                assert same_bits(got[name][first + j], want[k][rows[j]]), \
                    f"range {(first, count)}: {name} of mesh {first + j} (pose {table[rows[j]]}):\n{got[name][first + j]}\nrestatement:\n{want[k][rows[j]]}"
            assert got[name][~inside].tobytes() == before[name][~inside].tobytes(), f"range {(first, count)}: {name} changed outside it"
        assert np.array_equal(got["has_transform"][inside], want[3][rows]), f"range {(first, count)}: has_transform"
        assert np.array_equal(got["has_transform"][~inside], before["has_transform"][~inside])
        if (first, count) == (5, 64):
            # the rewritten flags word kept the materials' bit: a shadow ray through the glass mesh alone is not occluded, one
            # through the opaque mesh is; the closest hits say that each ray does pass through its mesh
            assert P.lib.ptrt_refit_tlas(s.ctx) == 0
            o = torch.tensor([[200.0, 0.0, 50.0], [-200.0, 0.0, 50.0]], device="cuda")
            dd = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]], device="cuda")
            hit = P.hit_fields(s.query_closest(o, dd))
            assert hit["hit"].tolist() == [1, 1] and hit["mesh_index"].tolist() == [glass, opaque]
            assert s.query_occluded(o, dd, torch.full((2,), 100.0, device="cuda")).tolist() == [0, 1]
    assert used == set(range(T)), "a pose of the table was never handed to the device"
    assert set(want[3][:8].tolist()) == {0, 1} and np.array_equal(want[1][0], np.eye(4, dtype=np.float32)[:3])
    s.close()


# ---- 2. frames ---------------------------------------------------------------------------------------------------------------------
def frame(P, s):
    rgb = s.render_to_host()
    return dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH), object_id=s.read(P.BUF_OBJECT_ID),
                rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats())


def test_frames_equal_a_twin_moved_by_matrices(P):
    """Scene a moves three meshes by device poses; its twin b gets a's read-back records through ptrt_set_instance_transforms --
    the path tests/test_tlas_refit_gpu.py pins to the oracle.  Same TLAS, same frames, byte for byte."""
    a, b = P.Scene(W, H), P.Scene(W, H)
    for s in (a, b):
        _many_meshes(P, s, n=30)
        prep(P, s)
    cube, sphere, baked = BASE + 0, BASE + 3, BASE + 2      # an instanced cube, an instanced sphere, a cube with baked vertices
    home = TR.many_transforms(30)
    d = a.flatten().contents
    n = d.mesh_count
    assert d.tlas_node_count > 1 and d.meshes[baked].has_transform == 0 and d.meshes[cube].has_transform == 1
    steps = {1: [(cube, (1.5, -1.0, -4.0), (0.4, -0.7, 0.2), home[cube][2])],
             2: [(sphere, (-2.5, 1.0, -3.0), home[sphere][1], home[sphere][2]), (cube, (1.8, -0.6, -4.5), (0.9, -0.2, 0.5), home[cube][2])],
             3: [(baked, (0.4, 0.6, 0.9), (0, 0, 0), (1, 1, 1)), (sphere, (-3.0, 2.0, -2.5), home[sphere][1], home[sphere][2])],
             4: [(cube, (0.5, 0.5, -6.0), (0.1, 0.2, 0.3), home[cube][2]), (baked, (-0.8, 0.2, 0.5), (0, 0, 0), (1, 1, 1))]}
    frames = {0: [], 1: []}
    for f in range(5):
        if f:
            for mesh, pos, rot, scl in steps[f]:
                a.set_instance_poses_device(mesh, pose_tensor([*pos, *rot, *scl]))
            recs = raw_records(P, a)
            assert P.lib.ptrt_set_instance_transforms(b.ctx, 0, n, recs) == 0
            for s in (a, b):
                assert s.get_option("inst_pre_ok") == 0
                assert (P.lib.ptrt_reorder_tlas if f == 4 else P.lib.ptrt_refit_tlas)(s.ctx) == 0
                assert s.get_option("inst_pre_ok") == 1
                s.setFrameCount(0)
            assert recs[baked].has_transform == (1 if f >= 3 else 0)
        for k, s in enumerate((a, b)):
            frames[k].append(frame(P, s))
        assert a.read_tlas().tobytes() == b.read_tlas().tobytes(), f"step {f}: the TLAS differs between poses and matrices"
        assert np.array_equal(a.read_tlas_order(), b.read_tlas_order())
        assert a.read_instance_transforms().tobytes() == b.read_instance_transforms().tobytes()
        assert upload_counts(P, a) == (1, 0) and upload_counts(P, b) == (1, 0)
    assert_frames_equal(frames[0], frames[1])
    for f in range(1, 5):
        assert not np.array_equal(frames[0][f - 1]["object_id"], frames[0][f]["object_id"]), f"step {f}: nothing moved in the image"
    assert a.get_option("tlas_refits") == 3 and a.get_option("tlas_reorders") == 1
    a.close()
    b.close()


# ---- 3. geometry, no tree -----------------------------------------------------------------------------------------------------------
def test_posed_instances_against_the_brute_force(P):
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    desc = s.flatten()
    before = bf.Geometry.from_desc(desc)
    assert len(before.meshes) == 72 and desc.contents.tlas_node_count > 1
    moved = inst[:8]
    home = many_proper_transforms()
    for j, m in enumerate(moved):
        pos, rot, scl = home[m]
        # far outside the room and the old TLAS boxes; a rotated instance stays at x = 0 (the inverse stays a true inverse)
        at = (0.0, 9.0 + 2.0 * j, 6.0 + j) if rot is not None else (11.0 + 2.0 * j, -3.0 + j, 5.0 - 2.0 * j)
        s.set_instance_poses_device(m, pose_tensor([*at, *(rot if rot is not None else (0, 0, 0)), 1.5 + 0.25 * j, 1.0, 2.0]))
    assert P.lib.ptrt_reorder_tlas(s.ctx) == 0
    got = s.read_instance_transforms()
    meshes = list(before.meshes)
    row3 = np.array([[0, 0, 0, 1]], np.float32)
    for m in moved:
        old = before.meshes[m]
        assert got["has_transform"][m] == 1
        # (verts are float32 values held as float64: handed back as they are)
        meshes[m] = bf.Mesh(old.verts, old.faces, True, np.concatenate([got["world"][m], row3]), np.concatenate([got["inverse"][m], row3]),
                            old.transmission)
    geom = bf.Geometry(meshes)
    assert all(m.proper for m in geom.meshes) and geom.radius > before.radius + 5.0
    assert upload_counts(P, s) == (1, 0) and s.get_option("tlas_reorders") == 1
    sets = []
    for kind, (o, d, mesh, face, small) in ray_sets(geom, "many", seed=7).items():
        c, tmax, a = truth(geom, o, d, mesh, face, small, ties=COPLANAR["many-proper"])
        sets.append((kind, o, d, c, tmax, a))
    kind, o, d, c, *_ = sets[1]
    assert np.isin(c["mesh"][c["decided"]], moved).sum() >= 8 * 12      # the posed instances are found where they are now
    for fg, pt in VARIANTS:
        s.set_option("force_geom", fg)
        s.set_option("pair_trace", pt)
        judge(s, geom, sets, f"instances posed on the device force_geom={fg} pair_trace={pt}")
    s.close()


# ---- 4. no synchronisation, no upload ---------------------------------------------------------------------------------------------
def test_poses_return_while_the_stream_is_busy(P, O):
    import torch
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    st = torch.cuda.Stream()
    s.set_stream(st.cuda_stream)
    home = many_proper_transforms()
    moved = [m for m in inst if home[m][1] is None][:3]
    rows = np.array([[2.0 - 1.5 * j, 1.0 + 0.5 * j, -3.0 - j, 0, 0, 0, 1.5, 1.2, 1.5] for j in range(3)], np.float32)
    poses = [pose_tensor(r) for r in rows]
    counts, refits = upload_counts(P, s), s.get_option("tlas_refits")
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
        for m, p in zip(moved, poses):
            s.set_instance_poses_device(m, p)
    assert upload_counts(P, s) == counts
    assert P.lib.ptrt_refit_tlas(s.ctx) == 0
    busy = not st.query()
    st.synchronize()
    slept = e0.elapsed_time(e1)
    assert slept >= 100.0, f"the sleep took {slept:.1f} ms: the check proves nothing"
    assert busy, "ptrt_set_instance_poses_device / ptrt_refit_tlas returned only after the stream had drained"
    assert upload_counts(P, s) == counts == (1, 0) and s.get_option("tlas_refits") == refits + 1 and s.get_option("inst_pre_ok") == 1
    want = R.compose(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], R.detmath_sincos(O))
    got = s.read_instance_transforms()
    for j, m in enumerate(moved):
        assert same_bits(got["world"][m], want[0][j]) and same_bits(got["inverse"][m], want[1][j])
    s.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    hip = C.CDLL("libamdhip64.so")      # the runtime libptrt_amd.so itself is linked against
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    put, get = P.lib.ptrt_set_instance_poses_device, P.lib.ptrt_read_instance_transforms
    s = P.Scene(32, 32)
    _many_meshes(P, s, n=20)
    good = pose_tensor(np.tile(np.array([1, 2, 3, 0.1, 0.2, 0.3, 1.5, 1.5, 1.5], np.float32), (4, 1)))
    ptr = C.c_void_p(good.data_ptr())
    out = (P.InstanceXform * 64)()
    assert put(s.ctx, 0, 1, ptr) == -4                                          # PTRT_E_NOT_READY
    assert get(s.ctx, 0, 1, C.cast(out, C.c_void_p)) == -4
    s.uploadToGPU()
    n = s.flatten().contents.mesh_count
    assert n == 28
    before = s.read_instance_transforms()
    refits = s.get_option("tlas_refits")

    def refused(*args):
        assert put(s.ctx, *args) == -1, args                                    # PTRT_E_INVALID
        assert b"ptrt_set_instance_poses_device" in P.lib.ptrt_last_error(s.ctx)
        assert s.get_option("inst_pre_ok") == 1, f"{args}: the refused call was noted"

    refused(0, 1, None)
    host = np.tile(np.array([1, 2, 3, 0, 0, 0, 1, 1, 1], np.float32), (4, 1))
    refused(0, 4, C.c_void_p(host.ctypes.data))                                 # host memory
    refused(0, 4, C.c_void_p(torch.from_numpy(host).pin_memory().data_ptr()))   # pinned host memory
    for args in ((n - 1, 2, ptr), (n, 1, ptr), (-1, 1, ptr), (0, -1, ptr), (0, n + 1, ptr)):
        refused(*args)
    # device memory one pose too short for the count.  (torch hands tensors out of larger blocks, inside which a short tensor is
    # still device memory; an allocation of the runtime's own ends where it ends.)
    size = 2 << 20
    dv = C.c_void_p()
    assert hip.hipMalloc(C.byref(dv), size) == 0
    tail = C.c_void_p(dv.value + size - 3 * POSE_BYTES)
    assert hip.hipMemcpy(tail, C.c_void_p(host.ctypes.data), 3 * POSE_BYTES, 1) == 0        # hipMemcpyHostToDevice
    refused(0, 4, tail)
    assert put(s.ctx, 0, 0, C.c_void_p(256)) == 0                               # an empty range is no error and no work
    assert s.get_option("inst_pre_ok") == 1 and s.get_option("tlas_refits") == refits
    assert s.read_instance_transforms().tobytes() == before.tobytes(), "a refused call changed the records"
    assert put(s.ctx, 0, 3, tail) == 0                                          # ... and the three poses that are there are taken
    assert s.get_option("inst_pre_ok") == 0
    assert P.lib.ptrt_refit_tlas(s.ctx) == 0
    after = s.read_instance_transforms()
    assert np.array_equal(after["world"][:3, :, 3], host[:3, :3]) and after[3:].tobytes() == before[3:].tobytes()
    hip.hipFree(dv)
    # the binding checks the tensor before the library sees it
    for bad in (good.cpu(), good[:, :8], good.t(), good.reshape(-1), good.double(), host):
        with pytest.raises(ValueError):
            s.set_instance_poses_device(0, bad)
    with pytest.raises(P.PtrtError, match="ptrt_set_instance_poses_device"):
        s.set_instance_poses_device(n - 1, good)
    # the read-back's own ranges
    vp = C.cast(out, C.c_void_p)
    for args in ((n - 1, 2, vp), (n, 1, vp), (-1, 1, vp), (0, -1, vp), (0, n + 1, vp), (0, 1, None)):
        assert get(s.ctx, *args) == -1, args
        assert b"ptrt_read_instance_transforms" in P.lib.ptrt_last_error(s.ctx)
    assert get(s.ctx, n, 0, vp) == 0 and len(s.read_instance_transforms(n - 2)) == 2
    assert put(None, 0, 1, ptr) == -1 and get(None, 0, 1, vp) == -1
    s.close()
