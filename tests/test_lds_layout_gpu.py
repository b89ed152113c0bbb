"""The LDS layouts (csrc/lds_layout.h) at the sizes where a region is at a floor, a clamp or an edge: each case is
a 64x64 frame (72x64 where the workgroups must not divide the tiles), 1 spp, 3 bounces, every buffer, generator state and ray
count against the oracle bit for bit, with the loop shape that ran asserted -- and, where the device queries walk the same
scene, 256 closest-hit and 256 occlusion queries against the float64 brute force over every triangle."""
import pytest

import brute_force as bf
from common import assert_frames_equal, render_both
from test_brute_force import assert_closest, assert_occluded, plain_rays, truth
from test_lds_layout import NODES, PAIR4, PM1, layout  # noqa: F401  (layout: the module fixture over ptrt_lds_layout)
from test_ray_query_gpu import query_both

pytestmark = pytest.mark.gpu

SPP, DEPTH = 1, 3


def blas_depth(desc):
    """the deepest inner node of any mesh's tree, the root at 1 (at least 1): the BLAS stack entries per lane of the upload"""
    d = desc.contents
    best = 1
    for i in range(d.mesh_count):
        M = d.meshes[i]
        todo = [(0, 0)]
        while todo:
            n, depth = todo.pop()
            N = M.nodes[n]
            if N.count > 0:
                continue
            best = max(best, depth + 1)
            todo += [(c, depth + 1) for c in (N.left, N.right) if c >= 0]
    return best


def counts(s):
    """what the upload derives from the scene and the layouts depend on: meshes, triangle slots, BLAS stack entries, lights"""
    d = s.flatten().contents
    return dict(meshes=d.mesh_count, tri_slots=sum(d.meshes[i].face_count for i in range(d.mesh_count)),
                stack_entries=blas_depth(s.flatten()), lights=d.light_count)


def queries(P, s, what, want_pmode):
    geom = bf.Geometry.from_desc(s.flatten())
    o, d = plain_rays("cornell", 256)
    c, tmax, a = truth(geom, o, d, exempt=True)  # (256 rays: the brute force's own statistics are test_brute_force.py's business)
    h, f = query_both(s, o, d, tmax)
    assert s.get_option("query_pmode") == want_pmode, what
    assert c["decided"].sum() >= 128 and a["decided"].sum() >= 128, what
    assert_closest(c, h, geom.radius, what)
    assert_occluded(a, f, what)


def one_cube(P, s):
    m = s.addCube(P.Material((0.8, 0.5, 0.3), 0.4))
    s.scale(m, (4.0, 3.0, 2.0))
    s.rotateSelfEulerXYZ(m, (0.3, 0.5, 0.1))
    s.moveTo(m, (0.3, -0.2, -5.0))
    s.addPointLight((0.5, 4.0, 1.0), (1.0, 0.95, 0.9), 40.0)
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0)


def spheres(segments, leaf):
    """two spheres of `segments` = (left, right) segments, `leaf` = the scene's BVH leaf target"""
    def make(P, s):
        for k, x in enumerate((-1.6, 1.6)):
            m = s.addSphere(segments[k], P.Material((0.7, 0.6, 0.5) if k else (0.3, 0.5, 0.8), 0.4, float(k)))
            s.scale(m, (2.2, 2.2, 2.2))
            s.moveTo(m, (x, 0.3 * x, -5.0 - x))
        s.setBVHLeafTarget(*leaf)
        s.addPointLight((0.5, 4.0, 1.0), (1.0, 0.95, 0.9), 40.0)
        s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0)
    return make


@pytest.mark.parametrize("refill", [0, 2])
def test_pmode1_single_mesh(P, O, blue_noise, refill):
    """One mesh: the pair list is at its 1024-byte floor (128 bytes of entries), the wave's totals sit in the only pad, the dense
    builder's owner table starts 64 bytes into the list, and with lane refill the six parked generator planes take the minima
    and the whole list."""
    s = P.Scene(64, 64)
    one_cube(P, s)
    s.set_option("refill", refill)
    s.set_option("pm1_dense_roots", 1)
    gpu, cpu = render_both(P, O, s, blue_noise, SPP, DEPTH)
    assert s.get_option("pmode") == 1 and s.get_option("pm1_dense_roots_eff") == 1
    assert s.get_option("refilled") == (1 if refill else 0)
    assert_frames_equal(gpu, cpu)
    queries(P, s, "one cube", 1)
    s.close()


def test_pmode1_two_tiles_odd_tile_count(P, O, blue_noise, layout):
    """pm1_wg = 2 on a 72x64 frame: 9 x 8 tiles in rows of nine -- every second workgroup straddles two rows of tiles; then 72x56,
    9 x 7 = 63 tiles: the last workgroup's second wave has no tile.  That the host lays the scene out for two tiles (and does
    not fall back to one) is read from the layout the library states for the scene's counts and the frame's options."""
    for size in ((72, 64), (72, 56)):
        s = P.Scene(*size)
        P.scenes.cornell(s)
        s.set_option("pm1_wg", 2)
        s.set_option("refill", 0)
        gpu, cpu = render_both(P, O, s, blue_noise, SPP, DEPTH)
        assert s.get_option("pmode") == 1 and s.get_option("refilled") == 0 and s.get_option("render_mode") == 0
        n = counts(s)
        _, info = layout(PM1, meshes=n["meshes"], tri_slots=n["tri_slots"], lights=n["lights"], full=0, stage=s.get_option("stage"),
                         lds_pad=s.get_option("lds_pad"), pm1_wg=2, sample_sync=s.get_option("sample_sync_eff"))
        assert info.wg == 2 and info.waves == 2 and info.total > 0
        assert_frames_equal(gpu, cpu)
        s.close()


@pytest.mark.parametrize("make,clamp,ask", [(spheres((6, 6), (2, 0)), "hi", True), (spheres((1030, 6), (2, 0)), "lo", False)], ids=["upper", "lower"])
def test_pmode4_pair_capacity_at_its_clamps(P, O, blue_noise, layout, make, clamp, ask):
    """merged = 1.  Two shallow trees: the 10-KB budget leaves room for every shadow pair, the capacity is 128 entries per mesh.
    A tree of 21 levels (a sphere of 2,121,800 triangles, two per leaf, beside a small one): the stacks alone pass the budget, the capacity is its floor
    of one more batch than the extension pairs need.  Which clamp the scene hits is read from the layout the library states
    for its mesh count and stack depth."""
    s = P.Scene(64, 64)
    make(P, s)
    s.set_option("merged", 1)
    gpu, cpu = render_both(P, O, s, blue_noise, SPP, DEPTH)
    assert s.get_option("pmode") == 4
    n = counts(s)
    stack = n["stack_entries"]
    assert n["meshes"] == 2
    _, info = layout(PAIR4, meshes=2, stack_entries=stack)
    if clamp == "hi":
        assert info.pair_cap == info.pair_cap_hi == 256 and stack <= 8
    else:
        assert stack * 512 > 10240 and info.pair_cap == info.pair_cap_lo == 192
    assert_frames_equal(gpu, cpu)
    if ask:  # (the queries walk this scene in PMODE 2: the one-wave layout without the merged list)
        queries(P, s, "two spheres", 2)
    s.close()


def test_lds_nodes_last_workgroup_short(P, O, blue_noise, layout):
    """PMODE 2 in four-wave workgroups on a 72x64 frame: 72 tiles are 18 workgroups exactly, so a 72x56 frame follows -- 63
    tiles, the last workgroup's fourth wave has none and leaves behind the barrier.  The four-wave shape is the frame's when
    the megakernel renders it in PMODE 2 with the option on, trees with inner nodes and a layout within 64 KB: each is asserted."""
    for size in ((72, 64), (72, 56)):
        s = P.Scene(*size)
        spheres((6, 6), (2, 0))(P, s)
        s.set_option("merged", 0)
        s.set_option("lds_nodes", 1)
        gpu, cpu = render_both(P, O, s, blue_noise, SPP, DEPTH)
        assert s.get_option("pmode") == 2 and s.get_option("lds_nodes") == 1 and s.get_option("render_mode") == 0
        n = counts(s)
        regions, info = layout(NODES, meshes=n["meshes"], stack_entries=n["stack_entries"])
        assert n["stack_entries"] == 6 and info.waves == 4 and 0 < info.total <= 64 * 1024
        assert any(r[0] == "topnodes" for r in regions)
        assert_frames_equal(gpu, cpu)
        s.close()
