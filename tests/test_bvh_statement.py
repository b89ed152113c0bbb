"""tests/bvh_statement.py held to the host side, no GPU: the statement of every box against the host mirror's builder
(Mesh::buildBVH) and its refit (Mesh::refitBVH) on a device=-1 Scene; the level widths the GPU tests rely on, taken from the
host trees as built; the a-priori keys of cell_soup against the numpy restatement of the builder's key (morton_order); and the
new entry point's declaration.  Nothing here assumes the builder's leaf threshold: shapes are read off the trees."""
import os
import re
import time

import numpy as np
import pytest

import bvh_statement as B
from build_restatement import mesh_arrays, mesh_tree, morton_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (1, 17, 18, 35, 36, 3200)
WIDE, WIDER, PARTIAL = 73728, 147456, 139364      # tests/test_bvh_boxes_gpu.py: the launch shapes these reach are asserted below


def soup_scene(P, sizes, seed):
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    rng = np.random.RandomState(seed)
    mat = P.Material((0.7, 0.7, 0.7), 0.5)
    ids = [s.addTriangles(B.height_soup(n, rng), mat) for n in sizes]
    return s, ids, rng


def host_statement(P, s, m):
    nodes, prim = mesh_tree(s, m)
    verts, faces = mesh_arrays(P, s, m)
    return nodes, prim, B.boxes(nodes, prim, faces, verts)


def test_header_declares_and_library_exports_read_bvh(P):
    src = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ptrt_read_bvh\s*\(\s*ptrt_ctx\s*\*\s*ctx\s*,\s*int\s+mesh_index\s*,\s*ptrt_bvh_node\s*\*\s*nodes_out\s*,"
                     r"\s*int\s+node_count\s*\)", code)
    assert hasattr(P.lib, "ptrt_read_bvh") and callable(getattr(P.Scene, "read_bvh", None))
    assert P.lib.ptrt_abi_version() == 6 and re.search(r"#define\s+PTRT_ABI_VERSION\s+6\b", src)     # an addition only


def test_the_statement_on_trees_made_by_hand():
    """two leaves under a root; an absent child; a node nothing references; -0.0 against +0.0"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [3, 2, 2], [2, 5, 2], [-1, -1, -1], [-1, -1, -4], [-0.0, 9, 0]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    nodes = np.array([[1, 2, 0, 0], [-1, -1, 0, 1], [3, -1, 0, 0], [-1, -1, 1, 2], [-1, -1, 0, 3]])   # node 4: referenced by nobody
    st = B.boxes(nodes, [2, 0, 1], faces, verts)
    assert st.reached.tolist() == [True, True, True, True, False] and st.depth.tolist() == [1, 2, 2, 3, 0] and st.widths == [1, 1]
    assert st.lo[1].tolist() == [-1, -1, -4] and st.hi[1].tolist() == [0, 9, 0]                   # face 2 alone
    assert st.lo[3].tolist() == [0, 0, 0] and st.hi[3].tolist() == [3, 5, 2]                      # faces 0 and 1
    assert (st.lo[2] == st.lo[3]).all() and (st.hi[2] == st.hi[3]).all()                          # the absent side adds nothing
    assert st.lo[0].tolist() == [-1, -1, -4] and st.hi[0].tolist() == [3, 9, 2]
    got = np.zeros(5, dtype=[("bmin", "<f4", 3), ("bmax", "<f4", 3)])
    got["bmin"], got["bmax"] = st.lo, st.hi
    got["bmax"][1][0] = -0.0                                                                        # either zero is the same value
    got["bmin"][4] = 77.0                                                                           # no statement there
    B.assert_boxes(got, st)
    got["bmax"][3][1] = np.nextafter(np.float32(5), np.float32(6))                                 # one ulp too large is a difference
    assert B.differing(got, st).tolist() == [3]
    with pytest.raises(AssertionError, match="first node 3 at depth 3"):
        B.assert_boxes(got, st, "by hand")
    assert B.scene_widths([[1, 2, 4], [1], []]) == [2, 2, 4]


def test_host_builder_and_host_refit_equal_the_statement_at_every_node(P):
    s, ids, rng = soup_scene(P, SMALL + (WIDE,), 11)
    for m, n in zip(ids, SMALL + (WIDE,)):
        nodes, prim, st = host_statement(P, s, m)
        assert np.array_equal(np.sort(prim), np.arange(n)) and st.reached.all()
        B.assert_boxes(nodes, st, f"built, {n} faces")
        assert (len(nodes) == 1) == (st.widths == [])
    # new vertices far outside the built boxes, the trees kept: every box follows, and comes back
    before = {m: mesh_tree(s, m)[0] for m in ids}
    for lift in (40.0, 0.0):
        rng = np.random.RandomState(11)
        for m, n in zip(ids, SMALL + (WIDE,)):
            s.setVertices(m, B.height_soup(n, rng, lift=lift).reshape(-1, 3))
            s.refitMeshOnHost(m)
        for m, n in zip(ids, SMALL + (WIDE,)):
            nodes, prim, st = host_statement(P, s, m)
            B.assert_boxes(nodes, st, f"refitted, {n} faces, lift {lift}")
            same = nodes.tobytes() == before[m].tobytes()
            assert same == (lift == 0.0), f"{n} faces, lift {lift}: the refit {'kept' if same else 'did not restore'} the built boxes"
    s.close()


def test_level_widths_of_the_large_soups_reach_the_launch_shapes_the_gpu_tests_name(P):
    """ptrt_refit gives a level wider than 2048 nodes a launch of its own until the first level, deepest first, that is not;
    that one and everything above go to one workgroup.  Read off the host trees."""
    t0 = time.time()
    s, ids, _ = soup_scene(P, (WIDE, WIDER, PARTIAL), 12)
    w = {n: host_statement(P, s, m)[2].widths for m, n in zip(ids, (WIDE, WIDER, PARTIAL))}
    for n, widths in w.items():
        print(n, widths)
        assert widths[0] == 1 and sum(widths) > 0
    assert w[WIDE][-1] > 2048 and sum(k > 2048 for k in w[WIDE]) == 1              # one level through refit_level_kernel
    assert w[WIDER][-1] > 2048 and sum(k > 2048 for k in w[WIDER]) == 2            # two
    assert w[PARTIAL][-1] <= 2048 and max(w[PARTIAL]) > 2048                        # a partial deepest level under a wide one:
    assert max(w[PARTIAL]) > 1024                                                   # ... the one-workgroup loop goes round again
    print("seconds", time.time() - t0)
    s.close()


@pytest.mark.parametrize("n", [2, 65, 1025, 5000])
def test_cell_soup_keys_are_the_restated_builders_keys(n):
    rng = np.random.RandomState(n)
    faces = np.arange(3 * n).reshape(-1, 3)
    for name, cells in B.key_cells(n - 2, rng).items():
        tris, keys, order = B.cell_soup(cells, rng)
        want, mkeys = morton_order(tris.reshape(-1, 3), faces)
        assert np.array_equal(mkeys, keys), name
        assert np.array_equal(want, order), name
        assert keys[0] == 0 and keys[-1] == 2 ** 30 - 1 and order[0] == 0 and order[-1] == n - 1
        if n > 2:
            inner = keys[1:-1]
            if name == "one_cell":
                assert len(np.unique(inner)) == 1 and np.array_equal(order, np.arange(n))
            elif name == "two_cells":
                assert np.array_equal(order[1:-1], np.concatenate([np.arange(2, n - 1, 2), np.arange(1, n - 1, 2)]))
            elif name == "bits_24_29":
                assert not (inner & (2 ** 24 - 1)).any() and len(np.unique(inner)) > 1
            elif name == "bits_0_7":
                assert not (inner >> 8).any() and len(np.unique(inner)) > 1
            elif name == "repeats" and n > 100:
                assert n // 16 < len(np.unique(inner)) <= n // 8
    # no anchors, one point: no extent, every key 0, the identity
    tris, keys, order = B.cell_soup(np.tile([[400, 2, 1000]], (n, 1)), rng, anchors=False)
    want, mkeys = morton_order(tris.reshape(-1, 3), faces)
    assert not mkeys.any() and not keys.any() and np.array_equal(want, np.arange(n)) and np.array_equal(order, want)
