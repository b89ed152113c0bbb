"""What ptrt_build_bvh's key and sort compute, restated in numpy float32 operation by operation (pt::morton30 and the stable
radix sort of csrc/pt_build.hip.h), and the arrays of a flattened mesh.  Shared by the tests of the GPU rebuild; no GPU and no
library call in the restatement itself.  tests/bvh_statement.py (cell_soup) supplies keys that need no such restatement."""
import ctypes as C

import numpy as np


def morton_order(verts, faces):
    """The face order ptrt_build_bvh must produce: stable sort by 30-bit Morton code of the fp32 centroid."""
    v = verts.astype(np.float32)
    c = ((v[faces[:, 0]] + v[faces[:, 1]]) + v[faces[:, 2]]) * np.float32(1.0 / 3.0)
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = np.float32((hi - lo).astype(np.float32).max())         # one scale for all axes: the largest extent
    q = np.zeros(c.shape, dtype=np.int64)
    for k in range(3):
        if ext > 0:
            t = ((c[:, k] - lo[k]) / ext).astype(np.float32)
            t = np.clip(t, np.float32(0), np.float32(1))
            q[:, k] = np.minimum((t * np.float32(1024.0)).astype(np.int64), 1023)

    def spread(x):
        out = np.zeros_like(x)
        for b in range(10):
            out |= ((x >> b) & 1) << (3 * b)
        return out
    keys = (spread(q[:, 0]) << 2) | (spread(q[:, 1]) << 1) | spread(q[:, 2])
    return np.argsort(keys, kind="stable").astype(np.int32), keys


def mesh_arrays(P, s, m):
    M = s.flatten().contents.meshes[m]
    verts = np.ctypeslib.as_array(C.cast(M.verts, C.POINTER(C.c_float)), (M.vert_count, 3)).copy()
    faces = np.ctypeslib.as_array(C.cast(M.faces, C.POINTER(C.c_int32)), (M.face_count, 3)).copy()
    return verts, faces


NODE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("start", "<i4"), ("count", "<i4")])


def mesh_tree(s, m):
    """(nodes as the structured array Scene.read_bvh returns, prim indices) of the host copy of mesh m's tree"""
    M = s.flatten().contents.meshes[m]
    nodes = np.ctypeslib.as_array(C.cast(M.nodes, C.POINTER(C.c_int32)), (M.node_count, 10)).copy().view(NODE).reshape(-1)
    prim = np.ctypeslib.as_array(M.prim_indices, (M.prim_count,)).copy()
    return nodes, prim
