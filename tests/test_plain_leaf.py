"""Option "plain_leaf" without a device (csrc/plain_leaf.h).

(a) The implication the option rests on: a mesh box that lies inside the TLAS root box, component by component as fp32
values, cannot be hit by a ray that misses the root box -- pt::slab with pt::make_ray's reciprocal, restated in numpy
float32, over rays aimed at the mesh box.  (b) The derivation the upload runs, through the device-free entry point
ptrt_plain_leaf."""
import ctypes as C

import numpy as np
import pytest

f32 = np.float32
T_FAR = f32(1e30)
N = 1_000_000  # cases per scale


def make_inv(d):
    """pt::make_ray: 1 / d where |d| > 1e-8, else +-1e30 by the sign test d >= 0 (so -0 gives +1e30)"""
    big = np.abs(d) > f32(1e-8)
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(big, f32(1.0) / np.where(big, d, f32(1.0)), np.where(d >= 0, f32(1e30), f32(-1e30))).astype(f32)


def slab(bmin, bmax, o, inv, tmax):
    """pt::slab, one box per ray: every product rounded to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        a = ((bmin - o).astype(f32) * inv).astype(f32)
        b = ((bmax - o).astype(f32) * inv).astype(f32)
    assert not np.isnan(a).any() and not np.isnan(b).any()  # ("operands are never NaN", pt_kernels.hip.h)
    neg = inv < 0
    t0, t1 = np.where(neg, b, a), np.where(neg, a, b)
    tmin, tmx = t0.max(axis=1), t1.min(axis=1)
    return (tmx >= 0) & (tmin <= tmx) & (tmin < tmax)


def cases(scale, seed):
    rs = np.random.RandomState(seed)
    S = np.float64(scale)
    # the mesh box and a second box; the root is the exact min / max of the two, so some of its faces ARE the mesh box's
    lo = (rs.uniform(-1, 1, (N, 3)) * S).astype(f32)
    ext = rs.uniform(0.01, 1, (N, 3))
    ext[rs.rand(N, 3) < 0.03] = 0.0  # flat boxes (a wall's quad)
    hi = np.maximum(lo, (lo.astype(np.float64) + ext * S).astype(f32))
    lo2 = (rs.uniform(-1, 1, (N, 3)) * S).astype(f32)
    hi2 = np.maximum(lo2, (lo2.astype(np.float64) + rs.uniform(0.01, 1, (N, 3)) * S).astype(f32))
    same = rs.rand(N) < 0.1  # the leaf's only mesh: root == mesh box
    lo2[same], hi2[same] = lo[same], hi[same]
    rlo, rhi = np.minimum(lo, lo2), np.maximum(hi, hi2)
    assert (lo >= rlo).all() and (hi <= rhi).all()
    # origins: around the boxes, inside the mesh box, and on a face plane of the mesh box or of the root box
    o = (rs.uniform(-3, 3, (N, 3)) * S).astype(f32)
    inside = rs.rand(N) < 0.2
    u = rs.rand(N, 3)
    o[inside] = (lo + (hi.astype(np.float64) - lo) * u).astype(f32)[inside]
    onface = rs.rand(N) < 0.3
    axis = rs.randint(0, 3, N)
    planes = np.stack([lo, hi, rlo, rhi], axis=0)  # (4, N, 3)
    pick = planes[rs.randint(0, 4, N), np.arange(N), axis]
    rows = np.flatnonzero(onface)
    o[rows, axis[rows]] = pick[rows]
    # directions: at a point of the mesh box (70 %), else anywhere; normalised in float64, stored as float32
    target = lo.astype(np.float64) + (hi.astype(np.float64) - lo) * rs.rand(N, 3)
    d = target - o
    away = rs.rand(N) < 0.3
    d[away] = rs.normal(size=(int(away.sum()), 3))
    dist = np.linalg.norm(d / S, axis=1) * S
    d = d / np.where(dist > 0, dist, 1.0)[:, None]
    d[dist == 0] = (0.0, 0.0, -1.0)
    d = d.astype(f32)
    # components at and below make_ray's threshold, both signs of zero
    special = np.array([0.0, -0.0, 5e-9, -2e-8], f32)
    sp = np.flatnonzero(rs.rand(N) < 0.15)
    d[sp, rs.randint(0, 3, sp.size)] = special[rs.randint(0, 4, sp.size)]
    # limits: T_FAR (closest hit) or a finite one around the distance to the target (shadow rays)
    with np.errstate(over="ignore"):
        tmax = np.where(rs.rand(N) < 0.5, T_FAR, (dist * rs.uniform(0.3, 1.5, N)).astype(f32)).astype(f32)
    return lo, hi, rlo, rhi, o, d, tmax


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e6, 1e30])
def test_a_ray_that_hits_a_box_inside_the_root_box_hits_the_root_box(scale):
    lo, hi, rlo, rhi, o, d, tmax = cases(scale, seed=int(np.log10(scale)) + 40)
    inv = make_inv(d)
    assert (np.abs(d) <= f32(1e-8)).any(axis=1).mean() > 0.1 and np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
    assert ((o == lo) | (o == hi) | (o == rlo) | (o == rhi)).any(axis=1).mean() > 0.25
    assert (tmax != T_FAR).mean() > 0.4  # (at scale 1e30 a finite limit may lie above T_FAR)
    if scale == 1e30:
        with np.errstate(over="ignore"):
            assert np.isinf(((rhi - o).astype(f32) * inv).astype(f32)).any(), "no product overflows at this scale"
    mesh = slab(lo, hi, o, inv, tmax)
    root = slab(rlo, rhi, o, inv, tmax)
    print(f"scale {scale:g}: {mesh.mean():.3f} of the rays hit the mesh box, {root.mean():.3f} the root box, "
          f"{int((mesh & ~root).sum())} hit the mesh box and miss the root box")
    assert mesh.mean() >= 0.2, "the rays are not aimed at the boxes"
    assert (~root).mean() > 0.02, "no ray misses the root box: nothing is tested"
    assert not (mesh & ~root).any()


# ---- (b) the derivation -----------------------------------------------------------------------------------------------------

def _plain_leaf(P, meshes, mesh_count, nodes, node_count, ids, id_count):
    f = P.lib.ptrt_plain_leaf
    f.argtypes = [C.POINTER(P.MeshDesc), C.c_int, C.POINTER(P.BvhNode), C.c_int, C.POINTER(C.c_int32), C.c_int]
    f.restype = C.c_int
    return f(meshes, mesh_count, nodes, node_count, ids, id_count)


@pytest.fixture()
def cornell(P):
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    yield P, s.flatten().contents
    s.close()


def _copy(P, d):
    meshes = (P.MeshDesc * d.mesh_count)()
    for i in range(d.mesh_count):
        C.memmove(C.byref(meshes[i]), C.byref(d.meshes[i]), C.sizeof(P.MeshDesc))
    nodes = (P.BvhNode * d.tlas_node_count)()
    for i in range(d.tlas_node_count):
        C.memmove(C.byref(nodes[i]), C.byref(d.tlas_nodes[i]), C.sizeof(P.BvhNode))
    return meshes, nodes


def test_cornell_is_a_plain_leaf(cornell):
    P, d = cornell
    assert d.mesh_count == 8 and d.tlas_nodes[0].count == 8
    assert _plain_leaf(P, d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == 1
    assert _plain_leaf(P, None, d.mesh_count, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == -1


@pytest.mark.parametrize("mesh", [0, 7])
def test_one_mesh_with_a_transform_is_not(cornell, mesh):
    P, d = cornell
    meshes, nodes = _copy(P, d)
    meshes[mesh].has_transform = 1
    assert _plain_leaf(P, meshes, d.mesh_count, nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == 0


@pytest.mark.parametrize("face", ["bmin.x", "bmin.y", "bmin.z", "bmax.x", "bmax.y", "bmax.z"])
def test_a_root_box_one_ulp_short_on_one_face_is_not(cornell, face):
    P, d = cornell
    meshes, nodes = _copy(P, d)
    side, axis = face.split(".")
    v = getattr(nodes[0], side)
    x = f32(getattr(v, axis))
    # (some mesh box reaches this face of the root box: the root is their union)
    assert any(f32(getattr(getattr(d.meshes[m].nodes[0], side), axis)) == x for m in range(d.mesh_count))
    setattr(v, axis, float(np.nextafter(x, f32(np.inf) if side == "bmin" else f32(-np.inf))))
    assert _plain_leaf(P, meshes, d.mesh_count, nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == 0
    setattr(v, axis, float(x))
    assert _plain_leaf(P, meshes, d.mesh_count, nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == 1
    setattr(v, axis, float("nan"))
    assert _plain_leaf(P, meshes, d.mesh_count, nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == 0


def test_a_tlas_with_inner_nodes_is_not(cornell):
    P, d = cornell
    # the same eight meshes under a root with two leaf children of four
    root = d.tlas_nodes[0]
    nodes = (P.BvhNode * 3)()
    for i in range(3):
        C.memmove(C.byref(nodes[i]), C.byref(root), C.sizeof(P.BvhNode))
    nodes[0].left, nodes[0].right, nodes[0].start, nodes[0].count = 1, 2, 0, 0
    nodes[1].left = nodes[1].right = nodes[2].left = nodes[2].right = -1
    nodes[1].start, nodes[1].count = root.start, 4
    nodes[2].start, nodes[2].count = root.start + 4, 4
    assert _plain_leaf(P, d.meshes, d.mesh_count, nodes, 3, d.tlas_mesh_indices, d.tlas_index_count) == 0
    # ... and a scene whose own TLAS has them
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.many(s, n=12)
    m = s.flatten().contents
    assert m.tlas_node_count > 1 and m.tlas_nodes[0].count == 0
    assert _plain_leaf(P, m.meshes, m.mesh_count, m.tlas_nodes, m.tlas_node_count, m.tlas_mesh_indices, m.tlas_index_count) == 0
    s.close()
