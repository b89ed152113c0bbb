"""Re-ordering the TLAS over its kept shape (ptrt_reorder_tlas, Scene.reorderTLAS), the parts that need no GPU: the host twin
(Scene::reorderTLASOnHost) against a numpy restatement of the arithmetic (tests/tlas_reorder_restatement.py), degenerate keys,
the oracle over the re-ordered tree against the float64 brute force, the leaf boxes' surface area against a refit alone, and
the declarations.  No bound here comes from the code under test: orders and boxes are compared for equality, the brute force
is judged with the constants of tests/test_brute_force.py, and the area check is a strict inequality."""
import os
import re

import numpy as np
import pytest

import brute_force as bf
import tlas_reorder_restatement as R
from test_brute_force import COPLANAR, assert_closest, assert_occluded, many_proper, ray_sets, truth
from test_parity_gpu import _many_meshes
from test_tlas_refit_gpu import many_proper_transforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptrt_reorder_tlas", "ptrt_read_tlas_order", "ptrt_set_instance_transforms_device")


def assert_reordered(s, topo0, what):
    """flatten() after a host re-order: the numpy order, the built topology, the refit's boxes over the new order"""
    want, got = R.order_of(s)
    assert np.array_equal(got, want), f"{what}: host order {got} is not the restatement's {want}"
    assert sorted(got.tolist()) == list(range(len(got)))
    d = s.flatten()
    box, topo = R.tlas_nodes(d)
    assert np.array_equal(topo, topo0), f"{what}: the re-order changed the TLAS topology"
    assert np.array_equal(box.view(np.uint32), R.expected_tlas_boxes(d).view(np.uint32)), f"{what}: boxes are not the refit's"
    return got


# ---- 1. the host twin against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,leaf", [(18, None), (30, None), (48, None), (30, (2, 0))], ids=["n18", "n30", "n48", "n30-leaf(2,0)"])
def test_host_twin_equals_the_numpy_restatement(P, n, leaf):
    """_many_meshes(n) is the Cornell box's 8 meshes and n more: 26, 38 and 56 meshes, each a TLAS with inner nodes."""
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    _many_meshes(P, s, n=n)
    if leaf:
        s.setBVHLeafTarget(*leaf)
    _, topo0 = R.tlas_nodes(s.flatten())
    assert len(topo0) > 1
    _, built = R.order_of(s)
    s.reorderTLAS(host_only=True)
    as_built = assert_reordered(s, topo0, "as built")
    assert not np.array_equal(as_built, built), "the built order already is the Morton order: the case shows nothing"
    R.scramble(s, R.many_transforms(n))
    s.refitInstanceChanges(host_only=True)
    _, kept = R.order_of(s)
    assert np.array_equal(kept, as_built)                    # a refit keeps the order ...
    s.reorderTLAS(host_only=True)
    scrambled = assert_reordered(s, topo0, "scrambled")
    assert not np.array_equal(scrambled, as_built), "the scramble did not change the order"       # ... the re-order follows
    s.close()


# ---- 2. degenerate keys ------------------------------------------------------------------------------------------------------
def test_equal_codes_keep_mesh_order(P):
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    _many_meshes(P, s, n=18)
    a, b = R.BASE + 0, R.BASE + 6                            # two instanced unit cubes
    for m in (b, a):
        s.setPosition(m, (1.25, -0.5, -5.0))
        s.setRotation(m, (0.3, 0.2, -0.1))
        s.setInstanceScale(m, (0.4, 0.3, 0.5))
    _, topo0 = R.tlas_nodes(s.flatten())
    s.reorderTLAS(host_only=True)
    order = assert_reordered(s, topo0, "two instances at one place")
    codes = R.tlas_morton_codes(*R.desc_boxes_and_rows(s.flatten()))
    assert codes[a] == codes[b]
    ja, jb = int(np.flatnonzero(order == a)[0]), int(np.flatnonzero(order == b)[0])
    between = order[min(ja, jb):max(ja, jb) + 1]
    assert ja < jb and (codes[between] == codes[a]).all() and (np.diff(between) > 0).all()
    s.close()


def test_all_instances_at_one_point_keep_mesh_order(P):
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    for k in range(64):
        m = s.addCube(P.Material((0.5, 0.5, 0.5), 0.5))
        s.setPosition(m, (0.5, 1.0, -4.0))
        s.setInstanceScale(m, (0.3, 0.3, 0.3))
    s.setCamera((0, 0, 5), (0, 0, -4), (0, 1, 0), 40.0)
    _, topo0 = R.tlas_nodes(s.flatten())
    assert len(topo0) > 1
    s.reorderTLAS(host_only=True)
    order = assert_reordered(s, topo0, "ext == 0")
    assert not R.tlas_morton_codes(*R.desc_boxes_and_rows(s.flatten())).any()
    assert np.array_equal(order, np.arange(64))
    s.close()


# ---- 3. the re-ordered tree finds the nearest triangle -------------------------------------------------------------------------
def scrambled_many_proper(P, s, then):
    """many_proper, flattened as built, its instances scrambled, then `then`(s); returns the instances"""
    inst = many_proper(P, s)
    home = many_proper_transforms()
    assert sorted(home) == sorted(inst)
    s.flatten()
    R.scramble(s, home)
    then(s)
    return inst


def test_oracle_over_the_reordered_tlas_equals_the_brute_force(P, O):
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    many_proper(P, s)
    _, topo0 = R.tlas_nodes(s.flatten())
    R.scramble(s, many_proper_transforms())
    s.reorderTLAS(host_only=True)
    assert_reordered(s, topo0, "many_proper scrambled")
    desc = s.flatten()
    geom = bf.Geometry.from_desc(desc)
    assert all(m.proper for m in geom.meshes), "the scramble left an instance whose stored inverse is not its inverse"
    assert sum(m.has_transform for m in geom.meshes) >= 20
    for kind, (o, d, mesh, face, small) in ray_sets(geom, "many").items():
        c, tmax, a = truth(geom, o, d, mesh, face, small, ties=COPLANAR["many-proper"])      # (asserts the undecided cap)
        assert_closest(c, O.trace_rays(desc, o, d), geom.radius, f"re-ordered many-proper {kind}")
        assert_occluded(a, O.any_hit(desc, o, d, tmax), f"re-ordered many-proper {kind}")
        assert c["hit"].mean() > 0.2 and 0 < a["occluded"].mean() < 1
    s.close()


# ---- 4. quality without a clock -----------------------------------------------------------------------------------------------
def test_reorder_shrinks_the_leaf_boxes_of_a_scrambled_scene(P):
    """Sum of the TLAS leaf boxes' surface areas of many_proper with every instance at the next one's home: after a refit alone,
    after the re-order, and for a fresh build of the same scene (printed; DESIGN.md 3.17 quotes them).  Asserted: the re-order
    is strictly below the refit.  Nothing is assumed about the fresh build."""
    area = {}
    for name, then in (("refit", lambda s: s.refitInstanceChanges(host_only=True)), ("reorder", lambda s: s.reorderTLAS(host_only=True))):
        s = P.Scene(32, 32, device=P.HOST_ONLY)
        scrambled_many_proper(P, s, then)
        area[name] = R.leaf_area(s.flatten())
        s.close()
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    many_proper(P, s)
    R.scramble(s, many_proper_transforms())                   # before the first flatten(): buildTLAS sees the scrambled scene
    area["build"] = R.leaf_area(s.flatten())
    s.close()
    print(f"TLAS leaf-box surface area, many_proper scrambled: refit {area['refit']:.3f}, re-order {area['reorder']:.3f}, "
          f"fresh build {area['build']:.3f}")
    assert area["reorder"] < area["refit"]


# ---- 5. header and binding -----------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_exposes_the_entry_points(P):
    src = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*ptrt_ctx\s*\*" % n, code), f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n), f"{n} is not exported"
    assert re.search(r"#define\s+PTRT_ABI_VERSION\s+6\b", src) and P.lib.ptrt_abi_version() == 6
    for n in ("reorderTLAS", "read_tlas_order", "set_instance_transforms_device"):
        assert callable(getattr(P.Scene, n, None)), n
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    with pytest.raises(P.PtrtError):
        s.reorderTLAS()                   # no back end: fails loudly, like refitInstanceChanges
    order0 = R.order_of(s)[1]
    s.reorderTLAS(host_only=True)         # a single-leaf TLAS keeps its order
    assert np.array_equal(R.order_of(s)[1], order0)
    s.close()
