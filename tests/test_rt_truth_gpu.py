"""rt_render_kernel against the float64 statement of tests/rt_truth.py: every lab case through Scene.render() and
render_to_device, judged with the CPU's TOL (bytes inside the predicted interval on decided pixels, the whole image with its
partial tiles), and two cases through the public C ABI alone over trees written here, which no host builder has seen."""
import ctypes as C

import numpy as np
import pytest

import rt_truth as T
from test_rt_truth import CASES, lab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(P):
    import ptrt_amd.rt as rt
    return rt


def _judge(st, img, what):
    lo, hi = st.byte_interval(T.TOL["rgb"])
    dec = st.decided_image()
    assert 1.0 - dec.mean() <= T.MAX_UNDECIDED
    assert (lo != hi)[dec].mean() <= T.MAX_UNDECIDED_BYTES
    out = ((img < lo) | (img > hi)) & dec[:, :, None]
    where = np.argwhere(out)[:4].tolist()
    assert not out.any(), f"{what}: {int(out.sum())} bytes of decided pixels outside the predicted interval, first (row, x, c) " \
        f"{where}: gpu {[int(img[tuple(w)]) for w in where]} allowed {[(int(lo[tuple(w)]), int(hi[tuple(w)])) for w in where]}"


@pytest.mark.parametrize("name", CASES)
def test_lab_case_on_the_device(rt, name):
    import torch
    L = lab(name)                                       # the statement, built once per process on the CPU
    s = T.build(rt, L.case, device=0)
    _judge(L.st, s.render(), name + " render()")
    W, H = L.case["W"], L.case["H"]
    t = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda:0")
    s.render_to_device(t)
    _judge(L.st, t.cpu().numpy().reshape(H, W, 3), name + " render_to_device")
    s.close()


def _box(v):
    return tuple(float(x) for x in v.min(axis=0)), tuple(float(x) for x in v.max(axis=0))


def _single_leaf(verts, faces):
    """one node: a leaf with every triangle"""
    return [(*_box(verts), -1, -1, 0, len(faces))], np.arange(len(faces), dtype=np.int32)


def _balanced(verts, faces):
    """the deepest balanced tree: the face list halved in its own order down to one triangle per leaf; boxes are the exact
    float32 bounds of the corners below a node"""
    nodes, prims = [], np.arange(len(faces), dtype=np.int32)

    def make(a, b):
        i = len(nodes)
        nodes.append(None)
        box = _box(verts[faces[a:b]].reshape(-1, 3))
        if b - a == 1:
            nodes[i] = (*box, -1, -1, a, 1)
        else:
            mid = (a + b) // 2
            left = make(a, mid)
            right = make(mid, b)
            nodes[i] = (*box, left, right, -1, 0)
        return i
    make(0, len(faces))
    return nodes, prims


def _vec(Vec3, a):
    return Vec3(*[float(np.float32(x)) for x in a])


def abi_scene(rt, L, tree):
    """the case as the C ABI takes it: per mesh (vertices, faces, node rows, primitive order), the descriptors, lights, view.
    Descriptors, lights and view are the statement's own values rounded to float32."""
    from ptrt_amd import Vec3
    st = L.st
    parts, descs = [], (rt.RtMesh * len(L.meshes))()
    for i, m in enumerate(L.meshes):
        v = np.ascontiguousarray(m["vertices"], np.float32)
        f = np.ascontiguousarray(m["faces"], np.int32)
        nd, pr = (_single_leaf if tree == "single_leaf" else _balanced)(v, f)
        assert int(np.ceil(np.log2(max(len(f), 1)))) + 1 <= 32                       # the walks' stack
        assert all(x[4] >= 0 and x[4] + x[5] <= len(pr) for x in nd if x[5] > 0)
        assert all(-1 <= c < len(nd) for x in nd for c in x[2:4]) and f.min() >= 0 and f.max() < len(v)
        parts.append((v, f, nd, pr))
        mat = rt.Material()
        for k, val in m["material"].items():
            setattr(mat, k, val)
        descs[i].material = mat._m
        R, Ri = T.descriptor(T.F(m["euler"]))
        descs[i].rotation[:] = [float(np.float32(x)) for x in R.reshape(-1)]
        descs[i].inv_rotation[:] = [float(np.float32(x)) for x in Ri.reshape(-1)]
        descs[i].translation = _vec(Vec3, m["position"])
    P, types = st.P, st.held["light_types"]
    lights = (rt.RtLight * max(len(types), 1))()
    for i, ty in enumerate(types):
        lights[i] = rt.RtLight(ty, _vec(Vec3, P["light.position"][i]), _vec(Vec3, T._norm(P["light.direction"][i])),
                               _vec(Vec3, P["light.color"][i]), float(P["light.intensity"][i]), float(P["light.range"][i]),
                               float(np.float32(np.cos(P["light.inner"][i]))), float(np.float32(np.cos(P["light.outer"][i]))))
    view = rt.RtView(_vec(Vec3, P["cam.org"]), _vec(Vec3, P["cam.cmo"]), _vec(Vec3, P["cam.hor"]), _vec(Vec3, P["cam.ver"]),
                     _vec(Vec3, P["ambient"]), _vec(Vec3, P["sky_top"]), _vec(Vec3, P["sky_bottom"]), int(st.held["use_sky"]))
    return parts, descs, lights, len(types), view


@pytest.mark.parametrize("tree", ["single_leaf", "balanced"])
def test_c_abi_with_trees_written_here(rt, tree):
    """the room case through ptrt_rt_upload_mesh / _upload_bvh / _set_scene / _render alone, as test_stack_limit_drops_pushes
    drives it: one leaf per mesh, and the deepest balanced tree (one triangle per leaf); no host builder is involved"""
    from ptrt_amd import BvhNode, Vec3, lib
    L = lab("room")
    W, H = L.case["W"], L.case["H"]
    parts, descs, lights, n_lights, view = abi_scene(rt, L, tree)
    ctx = C.c_void_p()
    assert lib.ptrt_rt_create(W, H, 0, C.byref(ctx)) == 0
    for i, (v, f, nd, pr) in enumerate(parts):
        nodes = (BvhNode * len(nd))()
        for j, row in enumerate(nd):
            nodes[j] = BvhNode(Vec3(*row[0]), Vec3(*row[1]), *[int(x) for x in row[2:6]])
        assert lib.ptrt_rt_upload_mesh(ctx, i, v.ctypes.data, len(v), f.ctypes.data, len(f)) == 0
        assert lib.ptrt_rt_upload_bvh(ctx, i, nodes, len(nd), pr.ctypes.data, len(pr)) == 0, lib.ptrt_rt_last_error(ctx)
    assert lib.ptrt_rt_set_scene(ctx, descs, len(parts), lights, n_lights) == 0
    got = np.zeros((H, W, 3), np.uint8)
    assert lib.ptrt_rt_render(ctx, C.byref(view), got.ctypes.data, 0) == 0, lib.ptrt_rt_last_error(ctx)
    lib.ptrt_rt_destroy(ctx)
    _judge(L.st, got, "C ABI, " + tree)
    assert got.mean() > 10
