"""TLAS refit over the uploaded topology, the parts that need no GPU: the C ABI declares and exports the three entry points
(ABI still 6), the Python Scene has refitInstanceChanges, and the HOST refit of the TLAS (Scene::refitTLAS, the twin of
pt::refit_tlas_kernel) keeps the topology and gives every node the union of its members' transformAABB boxes, bit for bit."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptrt_set_instance_transforms", "ptrt_refit_tlas", "ptrt_read_tlas")


def test_header_declares_and_library_exports_the_entry_points(P):
    src = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*ptrt_ctx\s*\*" % n, code), f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n), f"{n} is not exported"
    assert re.search(r"typedef\s+struct\s+ptrt_instance_xform\s*\{[^}]*world\[16\][^}]*inverse\[16\][^}]*normal\[16\][^}]*"
                     r"has_transform[^}]*\}\s*ptrt_instance_xform\s*;", code)
    assert C.sizeof(P.InstanceXform) == 3 * 64 + 4
    assert P.lib.ptrt_abi_version() == 6
    assert re.search(r"#define\s+PTRT_ABI_VERSION\s+6\b", src)


def test_python_scene_has_the_methods(P):
    for n in ("refitInstanceChanges", "reseatTLAS", "read_tlas"):
        assert callable(getattr(P.Scene, n, None)), n
    assert P.Scene.POLICIES["GpuRefitAll"] == 3
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    try:
        s.refitInstanceChanges()          # no back end: fails loudly, like refitObjectChanges
    except P.PtrtError:
        pass
    else:
        raise AssertionError("refitInstanceChanges on a host-only scene did not raise")
    s.setDynamicGeometryPolicy("GpuRefitAll")
    s.close()


def tlas_of(d):
    n = d.contents.tlas_node_count
    nodes = np.ctypeslib.as_array(C.cast(d.contents.tlas_nodes, C.POINTER(C.c_int32)), (n, 10)).copy()
    ids = np.ctypeslib.as_array(d.contents.tlas_mesh_indices, (d.contents.tlas_index_count,)).copy()
    return nodes[:, :6].copy().view(np.float32), nodes[:, 6:], ids


def world_boxes(d):
    """Transform3D::transformAABB of every mesh's root box in numpy float32, operation by operation as the host and the device
    evaluate it (-ffp-contract=off on both): corner k takes bmax where bit 0 / 1 / 2 of k is set; each coordinate is
    ((w0 * x + w1 * y) + w2 * z) + w3 with every product and sum rounded to float32 (numpy float32 arrays round each
    elementwise operation); the box is min / max over the eight corners, which no order changes."""
    out = []
    for m in range(d.contents.mesh_count):
        M = d.contents.meshes[m]
        root = M.nodes[0]
        lo = np.array([root.bmin.x, root.bmin.y, root.bmin.z], np.float32)
        hi = np.array([root.bmax.x, root.bmax.y, root.bmax.z], np.float32)
        w = np.array(list(M.world), np.float32).reshape(4, 4)
        k = np.arange(8)
        x = np.where(k & 1, hi[0], lo[0]).astype(np.float32)
        y = np.where(k & 2, hi[1], lo[1]).astype(np.float32)
        z = np.where(k & 4, hi[2], lo[2]).astype(np.float32)
        p = np.stack([((w[r, 0] * x + w[r, 1] * y) + w[r, 2] * z) + w[r, 3] for r in range(3)], axis=1)
        assert p.dtype == np.float32
        out.append((p.min(axis=0), p.max(axis=0)))
    return out


def members(topo, ids, n):
    """mesh indices below node n, from the topology alone"""
    left, right, start, count = (int(v) for v in topo[n])
    if count > 0:
        return [int(i) for i in ids[start:start + count]]
    return members(topo, ids, left) + members(topo, ids, right)


def move_eight(P, s, first=8):
    """moves and rotates eight meshes of scenes.many (instances and baked ones, which become instances); returns them"""
    moved = list(range(first, first + 8))
    for j, m in enumerate(moved):
        s.setPosition(m, (6.0 + 1.5 * j, -2.0 + 0.7 * j, 3.0 - 1.1 * j))
        s.setRotation(m, (0.3 * j, 0.2 + 0.1 * j, -0.25 * j))
    return moved


def test_host_refit_keeps_the_topology_and_unions_the_world_boxes(P):
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.many(s, n=30)
    box0, topo0, ids0 = tlas_of(s.flatten())
    assert len(topo0) > 1, "scenes.many(30) must have a TLAS with inner nodes"
    moved = move_eight(P, s)
    s.refitInstanceChanges(host_only=True)
    d = s.flatten()
    box1, topo1, ids1 = tlas_of(d)
    assert np.array_equal(topo0, topo1) and np.array_equal(ids0, ids1), "the refit changed the TLAS topology"
    assert not np.array_equal(box0.view(np.uint32), box1.view(np.uint32)), "nothing moved"
    world = world_boxes(d)
    for n in range(len(topo1)):
        ms = members(topo1, ids1, n)
        lo = np.min([world[m][0] for m in ms], axis=0)
        hi = np.max([world[m][1] for m in ms], axis=0)
        want = np.concatenate([lo, hi]).astype(np.float32)
        assert np.array_equal(box1[n].view(np.uint32), want.view(np.uint32)), f"TLAS node {n}: {box1[n]} vs {want}"
    assert sorted(members(topo1, ids1, 0)) == list(range(d.contents.mesh_count))
    for m in moved:                                          # the root contains every moved instance
        assert (box1[0, :3] <= world[m][0]).all() and (box1[0, 3:] >= world[m][1]).all()
        assert d.contents.meshes[m].has_transform == 1
    # a host REBUILD over the same meshes gives the same root box and, here, another tree: the refit is not a rebuild
    r = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.many(r, n=30)
    move_eight(P, r)
    box2, topo2, ids2 = tlas_of(r.flatten())
    assert np.array_equal(box2[0].view(np.uint32), box1[0].view(np.uint32))
    s.close()
    r.close()
