"""What pt::reorder_tlas_kernel and Scene::mortonOrderTLAS compute, restated in numpy float32 operation by operation, and the
scenes the TLAS re-order tests share.  No GPU, no library call in the restatement itself."""
import ctypes as C

import numpy as np

BASE = 8            # scenes.many / many_proper: the Cornell box's eight meshes come first


def desc_boxes_and_rows(d):
    """(root boxes (n, 6) float32 lo|hi, world rows (n, 3, 4) float32) of a flattened scene"""
    n = d.contents.mesh_count
    boxes, rows = np.zeros((n, 6), np.float32), np.zeros((n, 3, 4), np.float32)
    for m in range(n):
        M = d.contents.meshes[m]
        r = M.nodes[0]
        boxes[m] = (r.bmin.x, r.bmin.y, r.bmin.z, r.bmax.x, r.bmax.y, r.bmax.z)
        rows[m] = np.array(list(M.world), np.float32).reshape(4, 4)[:3]
    return boxes, rows


def world_boxes(root_boxes, world_rows):
    """Transform3D::transformAABB per mesh: corner k takes bmax where bit 0 / 1 / 2 of k is set, each coordinate is
    ((w0 * x + w1 * y) + w2 * z) + w3 with every product and sum rounded to float32, the box is min / max over the corners."""
    k = np.arange(8)
    lo, hi = root_boxes[:, None, :3], root_boxes[:, None, 3:]
    x = np.where(k & 1, hi[..., 0], lo[..., 0]).astype(np.float32)
    y = np.where(k & 2, hi[..., 1], lo[..., 1]).astype(np.float32)
    z = np.where(k & 4, hi[..., 2], lo[..., 2]).astype(np.float32)
    w = world_rows.astype(np.float32)
    p = np.stack([((w[:, r, 0:1] * x + w[:, r, 1:2] * y) + w[:, r, 2:3] * z) + w[:, r, 3:4] for r in range(3)], axis=2)
    assert p.dtype == np.float32
    return p.min(axis=1), p.max(axis=1)


def spread10(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000ff)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300f00f)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030c30c3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def tlas_morton_codes(root_boxes, world_rows):
    """30-bit Morton code of every mesh's world-box centre: centre (bmin + bmax) * 0.5f (AABB::center()), bounds of all centres,
    one scale (the largest extent), t = (c - lo) / ext clamped to [0, 1], min((int)(t * 1024), 1023), x in the high bit;
    ext == 0: code 0."""
    lo, hi = world_boxes(root_boxes, world_rows)
    c = (lo + hi) * np.float32(0.5)
    assert c.dtype == np.float32
    cmin, cmax = c.min(axis=0), c.max(axis=0)
    ext = np.float32(max(np.float32(0.0), (cmax - cmin).max()))
    if not ext > 0:
        return np.zeros(len(c), np.uint32)
    t = (c - cmin) / ext
    assert t.dtype == np.float32
    t = np.where(t < 0, np.float32(0), np.where(t > 1, np.float32(1), t)).astype(np.float32)
    q = np.minimum((t * np.float32(1024.0)).astype(np.int32), 1023)
    return (spread10(q[:, 0]) << np.uint32(2)) | (spread10(q[:, 1]) << np.uint32(1)) | spread10(q[:, 2])


def tlas_morton_order(root_boxes, world_rows):
    """TLAS index j -> the mesh ranked j: ascending code, ties by mesh index"""
    codes = tlas_morton_codes(root_boxes, world_rows)
    ids = np.arange(len(codes))
    return np.lexsort((ids, codes)).astype(np.int32)


def order_of(s):
    """(numpy order of the scene as flatten() describes it, the TLAS index array flatten() holds)"""
    d = s.flatten()
    ids = np.ctypeslib.as_array(d.contents.tlas_mesh_indices, (d.contents.tlas_index_count,)).copy()
    return tlas_morton_order(*desc_boxes_and_rows(d)), ids


def tlas_nodes(d):
    """(boxes (n, 6) float32, topology (n, 4) int32: left, right, start, count)"""
    n = d.contents.tlas_node_count
    a = np.ctypeslib.as_array(C.cast(d.contents.tlas_nodes, C.POINTER(C.c_int32)), (n, 10)).copy()
    return a[:, :6].copy().view(np.float32), a[:, 6:]


def expected_tlas_boxes(d):
    """every TLAS node's box from the topology and the index array flatten() holds: the union of its members' world boxes"""
    _, topo = tlas_nodes(d)
    ids = np.ctypeslib.as_array(d.contents.tlas_mesh_indices, (d.contents.tlas_index_count,)).copy()
    lo, hi = world_boxes(*desc_boxes_and_rows(d))

    def members(n):
        left, right, start, count = (int(v) for v in topo[n])
        if count > 0:
            return [int(i) for i in ids[start:start + count]]
        return members(left) + members(right)
    out = np.zeros((len(topo), 6), np.float32)
    for n in range(len(topo)):
        ms = members(n)
        out[n, :3], out[n, 3:] = lo[ms].min(axis=0), hi[ms].max(axis=0)
    return out


def leaf_area(d):
    """sum of the TLAS leaf boxes' surface areas, float64"""
    box, topo = tlas_nodes(d)
    e = (box[:, 3:] - box[:, :3]).astype(np.float64)[topo[:, 3] > 0]
    return float((2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])).sum())


def many_transforms(n):
    """{mesh: (position, rotation, scale)} of the instances of scenes.many(n), by replaying its draws"""
    rs = np.random.RandomState(3)
    out = {}
    for k in range(n):
        rs.uniform(0.2, 0.9, 3), rs.uniform(0.05, 0.8)
        pos = (float(rs.uniform(-4, 4)), float(rs.uniform(-4.5, 3.5)), float(rs.uniform(-9, -2)))
        if k % 3 == 0:
            out[BASE + k] = (pos, tuple(rs.uniform(-1, 1, 3)), tuple(rs.uniform(0.2, 0.5, 3)))
        else:
            rs.uniform(0.2, 0.5, 3)
    return out


def scramble(s, transforms, back=False):
    """Every instance to the home of the next instance in the list (a cyclic shift of whole transforms: position, rotation,
    scale -- a rotated home is at x = 0 in many_proper, so every stored inverse stays a true inverse); `back`: all home."""
    inst = sorted(transforms)
    for i, m in enumerate(inst):
        pos, rot, scl = transforms[m if back else inst[(i + 1) % len(inst)]]
        s.setPosition(m, pos)
        s.setRotation(m, rot if rot is not None else (0.0, 0.0, 0.0))
        s.setInstanceScale(m, scl)
    return inst
