"""Every box of the bottom-level trees the DEVICE holds (ptrt_read_bvh / Scene.read_bvh), after an upload, ptrt_refit and
ptrt_build_bvh, held to tests/bvh_statement.py -- the min / max of the triangles below each node, no tolerance -- and, where
the host mirror was told the same vertices, to the mirror's nodes bit for bit; and the face order of ptrt_build_bvh
(ptrt_read_prim_order) at the sizes and keys where a radix sort goes wrong, against orders known before any arithmetic of the
builder is restated (bvh_statement.cell_soup) and against the numpy restatement (build_restatement.morton_order).

Which launch shape of the refit a size reaches is asserted from the level widths of the trees as built, not assumed:
tests/test_bvh_statement.py has the same preconditions on the CPU.  No frames are rendered here; frames against the oracle
are tests/test_build_gpu.py's and tests/test_refit.py's."""
import ctypes as C
import time

import numpy as np
import pytest

import bvh_statement as B
from build_restatement import mesh_tree, morton_order
from tlas_reorder_restatement import world_boxes

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
SMALL = (1, 2, 17, 18, 35, 36, 613, 3200)
SORT_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5000)


def device_scene(P, soups, instances=False):
    """one soup mesh per (n, 9) array, uploaded; `instances`: every mesh both moved and scaled as an instance"""
    s = P.Scene(64, 64)
    mat = P.Material((0.7, 0.7, 0.7), 0.5)
    ids = [s.addTriangles(t, mat) for t in soups]
    for k, m in enumerate(ids if instances else ()):
        s.setPosition(m, (1.5 * k - 4.0, 0.25 * k, -3.0 - k))
        s.setInstanceScale(m, (0.5 + 0.25 * k, 1.0 + 0.125 * k, 2.0 - 0.125 * k))
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    return s, ids


def prim_order(P, s, m, n):
    got = np.full(n, -1, np.int32)
    assert P.lib.ptrt_read_prim_order(s.ctx, m, got.ctypes.data_as(C.POINTER(C.c_int)), n) == OK
    return got


def check(P, s, m, tris, mirror, what, order=None):
    """The one assertion of this file, for soup mesh m whose DEVICE vertices are `tris` ((n, 9): face i = vertices 3i .. 3i + 2):
    the device's nodes have the uploaded topology and, node by node, the statement's box over the order the device holds;
    `mirror`: the host copy was told the same vertices -- its order is the device's and its nodes are the device's bit for bit;
    `order`: the face order the device must hold."""
    verts = np.asarray(tris, np.float32).reshape(-1, 3)
    n = len(verts) // 3
    faces = np.arange(3 * n).reshape(-1, 3)
    host, host_prim = mesh_tree(s, m)
    got = s.read_bvh(m)
    assert len(got) == len(host) and all(np.array_equal(got[k], host[k]) for k in ("left", "right", "start", "count")), \
        f"{what}: the topology read back is not the uploaded one"
    dev_order = prim_order(P, s, m, n)
    assert np.array_equal(np.sort(dev_order), np.arange(n)), f"{what}: the device's face order is not a permutation"
    st = B.boxes(host, dev_order, faces, verts)
    B.assert_boxes(got, st, what)
    if order is not None:
        bad = np.flatnonzero(dev_order != order)
        assert bad.size == 0, f"{what}: {bad.size} of {n} leaf positions hold another face, first position {bad[0]}: {dev_order[bad[0]]}, must be {order[bad[0]]}"
    if mirror:
        assert np.array_equal(host_prim, dev_order), f"{what}: the host copy's face order is not the device's"
        assert got.tobytes() == host.tobytes(), f"{what}: device and host nodes differ in bits"
    return got, st


def check_single_leaf_tlas(P, s, what):
    """the root of a one-leaf TLAS is the union of the meshes' world boxes: eight corners of each root box the device holds
    through the world rows, every product and sum rounded to float32 (Transform3D::transformAABB)"""
    d = s.flatten().contents
    assert d.tlas_node_count == 1
    roots = np.zeros((d.mesh_count, 6), np.float32)
    rows = np.zeros((d.mesh_count, 3, 4), np.float32)
    for m in range(d.mesh_count):
        r = s.read_bvh(m)[0]
        roots[m, :3], roots[m, 3:] = r["bmin"], r["bmax"]
        rows[m] = np.array(list(d.meshes[m].world), np.float32).reshape(4, 4)[:3]
    lo, hi = world_boxes(roots, rows)
    t = s.read_tlas()[0]
    assert (t["bmin"] == lo.min(axis=0)).all() and (t["bmax"] == hi.max(axis=0)).all(), \
        f"{what}: TLAS root {t['bmin']} .. {t['bmax']}, the meshes' world boxes span {lo.min(axis=0)} .. {hi.max(axis=0)}"


def test_small_trees_in_one_scene(P):
    """1 to 3,200 faces behind instance transforms: upload, refit far away and back, rebuild, refits that bypass the host copy"""
    import torch
    rng = np.random.RandomState(21)
    home = [B.height_soup(n, rng) for n in SMALL]
    s, ids = device_scene(P, home, instances=True)
    assert all(s.flatten().contents.meshes[m].has_transform == 1 for m in ids)
    first = {}
    for m, n, tris in zip(ids, SMALL, home):
        first[m], st = check(P, s, m, tris, True, f"uploaded, {n} faces")
        assert (len(first[m]) == 1 and st.widths == []) == (n <= 17), f"{n} faces: {len(first[m])} nodes"
    check_single_leaf_tlas(P, s, "uploaded")
    # far outside the built boxes, every mesh its own way; then home again: the boxes must shrink back
    away = [B.height_soup(n, rng, t=0.7, lift=(50.0 if k % 2 else -50.0)) for k, n in enumerate(SMALL)]
    for data, name in ((away, "refitted away"), (home, "refitted home")):
        for m, tris in zip(ids, data):
            s.setVertices(m, tris.reshape(-1, 3))
        s.refitObjectChanges()
        for m, n, tris in zip(ids, SMALL, data):
            got, _ = check(P, s, m, tris, True, f"{name}, {n} faces")
            if data is away:
                assert (got["bmin"][:, 1] > first[m]["bmax"][0, 1]).all() or (got["bmax"][:, 1] < first[m]["bmin"][0, 1]).all()
            else:
                assert got.tobytes() == first[m].tobytes(), f"{n} faces: home again, the boxes are not the uploaded ones"
        check_single_leaf_tlas(P, s, name)
    moved = [B.height_soup(n, rng, t=1.3) for n in SMALL]
    for m, tris in zip(ids, moved):
        s.setVertices(m, tris.reshape(-1, 3))
    s.rebuildObjectChanges()
    for m, n, tris in zip(ids, SMALL, moved):
        check(P, s, m, tris, True, f"rebuilt, {n} faces", morton_order(tris.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3))[0])
    check_single_leaf_tlas(P, s, "rebuilt")
    # positions the host copy never sees: from device memory, then from host memory
    order = {m: prim_order(P, s, m, n) for m, n in zip(ids, SMALL)}
    for how in ("refitFromDevice", "refitFromHost"):
        data = [B.height_soup(n, rng, t=2.1, lift=(9.0 if how == "refitFromHost" else -7.0)) for n in SMALL]
        for m, tris in zip(ids, data):
            buf = torch.from_numpy(tris.copy())
            if how == "refitFromDevice":
                buf = buf.cuda()
                torch.cuda.synchronize()
            getattr(s, how)(m, buf.data_ptr())
            s.sync()                                            # (`buf` goes away with this iteration)
        for m, n, tris in zip(ids, SMALL, data):
            check(P, s, m, tris, False, f"{how}, {n} faces", order[m])
        check_single_leaf_tlas(P, s, how)
    s.close()


def large_soup(P, n, seed):
    """a one-face mesh in front (slot base and vertex base of the large one are not 0) and the n-face soup; the scene's level
    widths, as ptrt_refit walks them"""
    rng = np.random.RandomState(seed)
    s, (tiny, m) = device_scene(P, [B.height_soup(1, rng), B.height_soup(n, rng)])
    faces = np.arange(3 * n).reshape(-1, 3)
    per_mesh = []
    for k, cnt in ((tiny, 1), (m, n)):
        nodes, prim = mesh_tree(s, k)
        per_mesh.append(B.boxes(nodes, prim, faces[:cnt], np.zeros((3 * cnt, 3), np.float32)).widths)
    return s, m, rng, B.scene_widths(per_mesh)


def refits_and_rebuilds(P, s, m, n, rng):
    """refit and rebuild with plain launches, then as captured graphs: captured on one set of positions, replayed on another"""
    faces = np.arange(3 * n).reshape(-1, 3)
    step = 0
    for graphs in (0, 1):
        s.set_option("use_graphs", graphs)
        for rebuild in (False, True):
            for rep in range(1 + graphs):
                step += 1
                tris = B.height_soup(n, rng, t=0.6 * step, lift=(30.0 if step % 2 else -30.0))
                s.setVertices(m, tris.reshape(-1, 3))
                if rebuild:
                    s.rebuildObjectChanges()
                else:
                    s.refitObjectChanges()
                what = f"{n} faces, {'rebuild' if rebuild else 'refit'}, use_graphs {graphs}, {'replayed' if rep else 'first'}"
                check(P, s, m, tris, True, what, morton_order(tris.reshape(-1, 3), faces)[0] if rebuild else None)
    check_single_leaf_tlas(P, s, f"{n} faces")


@pytest.mark.parametrize("n,wide", [(73728, 1), (147456, 2)])
def test_wide_levels_through_their_own_launches(P, n, wide):
    """levels wider than 2,048 nodes: one refit_level_kernel launch each, deepest first, then the one-workgroup kernel over
    the rest -- whose widest level, 2,048 nodes, takes its 1,024 threads twice round"""
    t0 = time.time()
    s, m, rng, widths = large_soup(P, n, 31)
    print(n, "inner levels", widths)
    assert widths[-1] > 2048 and sum(k > 2048 for k in widths) == wide, widths
    assert all(a <= b for a, b in zip(widths, widths[1:])), widths      # (so every wide level does get a launch of its own)
    assert max(k for k in widths if k <= 2048) > 1024, widths
    refits_and_rebuilds(P, s, m, n, rng)
    s.close()
    print(n, "faces: seconds", round(time.time() - t0, 2))


def test_a_partial_deepest_level_sends_a_wide_level_to_the_one_workgroup_kernel(P):
    """139,364 faces: the deepest inner level is narrow, so ptrt_refit hands everything -- the 4,096-node level included -- to
    refit_top_levels_kernel, whose 1,024 threads then stride a level four times"""
    t0 = time.time()
    n = 139364
    s, m, rng, widths = large_soup(P, n, 32)
    print(n, "inner levels", widths)
    assert widths[-1] <= 2048 and max(widths) > 2048, widths
    refits_and_rebuilds(P, s, m, n, rng)
    s.close()
    print(n, "faces: seconds", round(time.time() - t0, 2))


def test_fewer_triangles_pad_no_box(P):
    """updateTriangles with every fifth triangle gone, with one triangle left, and full again: the tail repeats the last real
    vertex, so every box is the statement over the real triangles and that vertex"""
    rng = np.random.RandomState(41)
    n = 3200
    s, (_, w) = device_scene(P, [B.height_soup(5, rng), B.height_soup(n, rng)])
    full = B.height_soup(n, rng, t=0.5)
    for keep, name in ((full[np.arange(n) % 5 != 0], "every fifth gone"), (full[1234:1235], "one triangle"), (full, "full again")):
        s.updateTriangles(w, keep)
        v = keep.reshape(-1, 3)
        padded = np.concatenate([v, np.tile(v[-1], (3 * n - len(v), 1))])
        got, st = check(P, s, w, padded.reshape(-1, 9), True, name, morton_order(padded, np.arange(3 * n).reshape(-1, 3))[0])
        assert (got["bmin"][0] == v.min(axis=0)).all() and (got["bmax"][0] == v.max(axis=0)).all(), f"{name}: the root box is not the real triangles'"
    s.close()


def test_a_hand_made_tree_through_the_raw_abi(P):
    """leaves of 1 and 40 faces, an absent child, a face in no leaf and a node nothing references: after ptrt_refit the boxes
    are the statement's, the node over the absent child has its one child's box (the absent side stayed the inverted 1e30 box),
    the unreferenced node keeps what was uploaded; ptrt_build_bvh and ptrt_read_prim_order refuse the mesh"""
    lib = P.lib
    rng = np.random.RandomState(51)
    nf = 42
    tris0, tris1 = B.height_soup(nf, rng), B.height_soup(nf, rng, t=0.9, lift=12.0)
    faces = np.arange(3 * nf, dtype=np.int32).reshape(-1, 3)
    prim = rng.permutation(nf).astype(np.int32)[:41]                        # one face sits in no leaf
    topo = np.array([[1, 2, 0, 0], [-1, -1, 0, 1], [3, -1, 0, 0], [-1, -1, 1, 40], [-1, -1, 0, 1]])
    st0 = B.boxes(topo, prim, faces, tris0.reshape(-1, 3))
    assert st0.reached.tolist() == [True] * 4 + [False] and st0.widths == [1, 1]
    nodes = (P.BvhNode * 5)()
    for i in range(5):
        lo, hi = (st0.lo[i], st0.hi[i]) if st0.reached[i] else ((-77.0, -78.0, -79.0), (77.0, 78.0, 79.0))
        nodes[i].bmin, nodes[i].bmax = P.Vec3(*map(float, lo)), P.Vec3(*map(float, hi))
        nodes[i].left, nodes[i].right, nodes[i].start, nodes[i].count = (int(v) for v in topo[i])
    v0 = np.ascontiguousarray(tris0.reshape(-1, 3))
    M = (P.MeshDesc * 1)()
    M[0].verts, M[0].vert_count = v0.ctypes.data_as(C.POINTER(P.Vec3)), 3 * nf
    M[0].faces, M[0].face_count = faces.ctypes.data_as(C.POINTER(P.Tri)), nf
    M[0].nodes, M[0].node_count = nodes, 5
    M[0].prim_indices, M[0].prim_count = prim.ctypes.data_as(C.POINTER(C.c_int32)), 41
    for k in (0, 5, 10, 15):
        M[0].world[k] = M[0].inverse[k] = M[0].normal[k] = 1.0
    tlas = (P.BvhNode * 1)()
    tlas[0].bmin, tlas[0].bmax = nodes[0].bmin, nodes[0].bmax
    tlas[0].left, tlas[0].right, tlas[0].start, tlas[0].count = -1, -1, 0, 1
    tids = (C.c_int32 * 1)(0)
    ctx = C.c_void_p()
    assert lib.ptrt_create(16, 16, 0, 0, 0, C.byref(ctx)) == OK
    try:
        assert lib.ptrt_upload_geometry(ctx, M, 1, tlas, 1, tids, 1) == OK, lib.ptrt_last_error(ctx)
        got = np.zeros(5, dtype=P.TLAS_NODE_DTYPE)
        out = got.ctypes.data_as(C.POINTER(P.BvhNode))
        assert lib.ptrt_read_bvh(ctx, 0, out, 5) == OK
        B.assert_boxes(got, st0, "hand-made, uploaded")
        assert np.array_equal(np.stack([got[k] for k in ("left", "right", "start", "count")], axis=1), topo)
        v1 = np.ascontiguousarray(tris1.reshape(-1, 3))
        assert lib.ptrt_update_vertices(ctx, 0, v1.ctypes.data_as(C.POINTER(C.c_float)), 3 * nf, 0) == OK
        assert lib.ptrt_refit(ctx) == OK
        assert lib.ptrt_read_bvh(ctx, 0, out, 5) == OK
        st1 = B.boxes(topo, prim, faces, v1)
        B.assert_boxes(got, st1, "hand-made, refitted")
        assert (got["bmin"][2] == got["bmin"][3]).all() and (got["bmax"][2] == got["bmax"][3]).all()
        assert got["bmin"][0][1] > st0.hi[0][1], "the refit did not move the root"
        assert got["bmin"][4].tolist() == [-77.0, -78.0, -79.0] and got["bmax"][4].tolist() == [77.0, 78.0, 79.0]
        assert lib.ptrt_build_bvh(ctx, 0) == INVALID and b"exactly one" in lib.ptrt_last_error(ctx)
        assert lib.ptrt_read_prim_order(ctx, 0, (C.c_int * nf)(), nf) == INVALID
        assert lib.ptrt_read_bvh(ctx, 0, out, 4) == INVALID and lib.ptrt_read_bvh(ctx, 1, out, 5) == INVALID
        assert lib.ptrt_sync(ctx) == OK
    finally:
        lib.ptrt_destroy(ctx)


# ---- the sort and the Morton code at their edges -----------------------------------------------------------------------
def sized_soup(n, rng):
    """(tris, order): n faces with about n / 8 distinct keys, two of them anchors; a single face has no anchors and no extent"""
    if n == 1:
        tris, _, order = B.cell_soup([[3, 2, 1]], rng, anchors=False)
    else:
        tris, _, order = B.cell_soup(B.key_cells(n - 2, rng)["repeats"], rng)
    return tris, order


def rebuild_and_check(P, s, m, tris, order, what):
    n = len(tris)
    s.setVertices(m, tris.reshape(-1, 3))
    s.rebuildObjectChanges()
    assert np.array_equal(order, morton_order(tris.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3))[0])
    check(P, s, m, tris, True, what, order)


def test_sort_at_every_size_where_its_shape_changes(P):
    """one key per wave round (64), per wave (1,024) and per workgroup (4,096), one less and one more, and 5,000 for the scan's
    uneven last segment.  Smallest first with graphs on: the scratch grows at every mesh and the captured graphs are dropped;
    then every mesh twice more on other data -- a recapture and a replay, in scratch sized for the largest"""
    rng = np.random.RandomState(61)
    a = [sized_soup(n, rng) for n in SORT_SIZES]
    b = [sized_soup(n, rng) for n in SORT_SIZES]
    s, ids = device_scene(P, [t for t, _ in a])
    assert s.flatten().contents.tlas_node_count == 1            # (a TLAS with inner nodes is re-uploaded by a rebuild, which drops every graph)
    s.set_option("use_graphs", 1)
    for m, n, (tris, order) in zip(ids, SORT_SIZES, a):
        rebuild_and_check(P, s, m, tris, order, f"{n} faces, growing")
    for m, n, first, second in zip(ids, SORT_SIZES, b, a):
        for (tris, order), name in ((first, "recaptured"), (second, "replayed")):
            rebuild_and_check(P, s, m, tris, order, f"{n} faces, {name}")
    s.close()


@pytest.mark.parametrize("graphs", [0, 1])
def test_sort_keys_that_repeat_collapse_or_differ_in_few_bits(P, graphs):
    """4,100 faces each -- five waves, two workgroups: equal keys (the identity), two keys alternating face by face (stability
    across rounds, waves and workgroups), keys that differ only in the top pass's or the bottom pass's bits, a plane, a line,
    many repeats, one outlier; and a soup without extent, every key 0"""
    rng = np.random.RandomState(71)
    n = 4100
    soups = {name: B.cell_soup(cells, rng) for name, cells in B.key_cells(n - 2, rng).items()}
    soups["point"] = B.cell_soup(np.tile([[400, 2, 1000]], (n, 1)), rng, anchors=False)
    assert np.array_equal(soups["one_cell"][2], np.arange(n)) and np.array_equal(soups["point"][2], np.arange(n))
    start = B.height_soup(n, rng)
    s, ids = device_scene(P, [start] * len(soups))
    s.set_option("use_graphs", graphs)
    for m, (tris, _, _) in zip(ids, soups.values()):
        s.setVertices(m, tris.reshape(-1, 3))
    s.rebuildObjectChanges()
    faces = np.arange(3 * n).reshape(-1, 3)
    for m, (name, (tris, keys, order)) in zip(ids, soups.items()):
        assert np.array_equal(order, morton_order(tris.reshape(-1, 3), faces)[0]), name
        check(P, s, m, tris, True, f"keys: {name}", order)
    s.close()
