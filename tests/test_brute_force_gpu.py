"""The trees on the DEVICE against a float64 brute force over every triangle (tests/brute_force.py): Scene.query_closest /
query_occluded -- the path tracer's own traversals under every loop shape -- over the scene's current description, on every
ray the brute force calls decided: random and camera-like rays and two rays aimed at every triangle.  Built trees, and the
trees nothing ever reads back: after a GPU refit (also from device and host memory, also far beyond the built boxes), after a
GPU rebuild (also with fewer triangles: the padded tail must not be hit), after instance moves behind a real TLAS, behind a
band and an interleaved context.  The constants are those measured on the CPU, oracle against brute force
(tests/test_brute_force.py); nothing here is tuned against the GPU's output."""
import numpy as np
import pytest

import brute_force as bf
from test_brute_force import (COPLANAR, FACE_SCENES, SCENES, assert_closest, assert_occluded, many_proper, plain_rays, ray_sets, truth)
from test_ray_query_gpu import VARIANTS, query_both

pytestmark = pytest.mark.gpu

_cache = {}
_truths = {}


def device_scene(P, name, w=64, h=64, **kw):
    s = P.Scene(w, h, **kw)
    recipe, box = SCENES[name]
    recipe(P, s)
    s.uploadToGPU()
    return s, box


def scene_and_truth(P, name):
    """One Scene per scene and its brute force, once per module: [(kind, o, d, closest, tmax, occluded)]"""
    if name not in _cache:
        s, box = device_scene(P, name)
        geom = bf.Geometry.from_desc(s.flatten())
        assert all(m.proper for m in geom.meshes)
        sets = []
        for kind, (o, d, mesh, face, small) in ray_sets(geom, box, faces=name in FACE_SCENES).items():
            c, tmax, a = truth(geom, o, d, mesh, face, small, ties=COPLANAR.get(name, ()))
            sets.append((kind, o, d, c, tmax, a))
        _cache[name] = (s, geom, sets)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cached():
    yield
    for v in _cache.values():
        v[0].close()
    _cache.clear()
    _truths.clear()


def judge(s, geom, sets, what):
    """All ray sets in one batch through the device queries, each judged against its brute force."""
    o = np.concatenate([x[1] for x in sets])
    d = np.concatenate([x[2] for x in sets])
    tmax = np.concatenate([x[4] for x in sets])
    h, f = query_both(s, np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(tmax))
    at = 0
    for kind, so, sd, c, stm, a in sets:
        n = len(so)
        assert_closest(c, h[at:at + n], geom.radius, f"{what} {kind}")
        assert_occluded(a, f[at:at + n], f"{what} {kind}")
        at += n


@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
@pytest.mark.parametrize("name", list(SCENES))
def test_built_trees(P, name, fg, pt):
    s, geom, sets = scene_and_truth(P, name)
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    try:
        judge(s, geom, sets, f"{name} force_geom={fg} pair_trace={pt}")
        pm = s.get_option("query_pmode")
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)
    # every loop shape is known to have been judged (as tests/test_ray_query_gpu.py asserts it)
    if pt == 0:
        assert pm == 0
    elif name == "cornell":
        assert pm == {-1: 1, 1: 2, 2: 3}[fg]
    elif fg == 2 or name == "many-proper":
        assert pm == 3
    else:
        assert pm in (1, 2, 3)


def fluid_scene(P):
    s = P.Scene(64, 48)
    w, ship = P.scenes.fluid(s, cells=40, t=0.0, ship_segments=24)
    s.uploadToGPU()
    return s, w, ship


def judge_current(s, what, override=None, seed=5, n_plain=4096):
    """Brute force over the scene's current host description (`override`: {mesh: vertices} handed to the device only),
    targeted rays at EVERY triangle and plain rays, against the device queries."""
    if what not in _truths:        # the same vertices under every force_geom: one brute force
        geom = bf.Geometry.from_desc(s.flatten())
        for m, v in (override or {}).items():
            old = geom.meshes[m]
            geom.meshes[m] = bf.Mesh(v, old.faces, old.has_transform, old.world, old.inverse, old.transmission)
        geom = bf.Geometry(geom.meshes)
        assert all(m.proper for m in geom.meshes)
        sets = []
        o, d = plain_rays("fluid", n_plain, seed)
        c, tmax, a = truth(geom, o, d)
        sets.append(("plain", o, d, c, tmax, a))
        o, d, mesh, face, small = bf.targeted_rays(geom, per_mesh=1 << 20)
        c, tmax, a = truth(geom, o, d, mesh, face, small)
        sets.append(("targeted", o, d, c, tmax, a))
        o, d = bf.box_face_rays(geom, per_mesh=1 << 20)
        c, tmax, a = truth(geom, o, d)
        sets.append(("box faces", o, d, c, tmax, a))
        _truths[what] = (geom, sets)
    geom, sets = _truths[what]
    judge(s, geom, sets, what)
    return geom, sets


def tall_water(t, k):
    """water_vertices(40, t) with its heights times k: waves of several units, boxes far beyond the built ones"""
    import ptrt_amd as P
    v = P.scenes.water_vertices(40, t).copy()
    v[:, 1] *= np.float32(k)
    return v


@pytest.mark.parametrize("fg", [-1, 2])
def test_after_gpu_refit(P, fg):
    import torch
    s, w, ship = fluid_scene(P)
    s.set_option("force_geom", fg)
    judge_current(s, "built")
    for t, k in ((0.6, 1.0), (1.9, 9.0), (1.3, 1.0)):          # a step, a large displacement, back to small waves
        s.setVertices(w, tall_water(t, k))
        s.refitObjectChanges()
        geom, _ = judge_current(s, f"refit t={t} x{k}")
        if k > 1:
            assert np.abs(geom.meshes[w].verts[:, 1]).max() > 4.0
    v = tall_water(2.7, 5.0)
    dev = torch.from_numpy(v).cuda()
    s.refitFromDevice(w, dev.data_ptr())
    judge_current(s, "refitFromDevice", {w: v})
    v = tall_water(3.4, 0.5)
    buf = torch.from_numpy(v.copy())
    s.refitFromHost(w, buf.data_ptr())
    judge_current(s, "refitFromHost", {w: v})
    s.close()


@pytest.mark.parametrize("fg", [-1, 2])
def test_after_gpu_rebuild(P, fg):
    import torch
    s, w, ship = fluid_scene(P)
    s.set_option("force_geom", fg)
    s.setVertices(w, tall_water(0.8, 6.0))
    s.rebuildObjectChanges()
    judge_current(s, "rebuildObjectChanges")
    v = tall_water(2.2, 3.0)
    dev = torch.from_numpy(v).cuda()
    s.rebuildFromDevice(w, dev.data_ptr())
    judge_current(s, "rebuildFromDevice", {w: v})
    # fewer triangles: the padded tail must not be hit.  Rays aimed at the REMOVED triangles' old places too; what they
    # find is what the brute force over the kept ones says
    full = tall_water(0.5, 2.0).reshape(-1, 9)
    gone = (np.arange(len(full)) % 5) == 0
    s.updateTriangles(w, full[~gone])
    geom, _ = judge_current(s, "updateTriangles, fewer")
    assert int(bf._usable(geom.meshes[w].triangles()).sum()) == int((~gone).sum())
    ghosts = bf.Geometry([bf.Mesh(full[gone].reshape(-1, 3), np.arange(3 * int(gone.sum())).reshape(-1, 3))])
    ghosts.radius = geom.radius
    o, d, *_ = bf.targeted_rays(ghosts, per_mesh=1 << 20)
    c, tmax, a = truth(geom, o, d)
    h = bf.TARGET_H * geom.radius
    assert (np.abs(c["t"] - h) > 0.5 * h).mean() > 0.9      # the ghost itself is not there
    judge(s, geom, [("at removed triangles", o, d, c, tmax, a)], "updateTriangles, fewer")
    s.close()


def test_after_instance_moves_behind_a_real_tlas(P):
    s = P.Scene(64, 64)
    inst = many_proper(P, s)
    s.uploadToGPU()
    before = bf.Geometry.from_desc(s.flatten())
    assert len(before.meshes) > 17 and s.flatten().contents.tlas_node_count > 1
    moved = inst[:8]
    for j, m in enumerate(moved):
        rotated = before.meshes[m].world[0, 1] != 0.0 or before.meshes[m].world[0, 2] != 0.0
        # far outside the room and the old TLAS boxes; a rotated instance stays at x = 0 (the inverse stays a true inverse)
        s.setPosition(m, (0.0, 9.0 + 2.0 * j, 6.0 + j) if rotated else (11.0 + 2.0 * j, -3.0 + j, 5.0 - 2.0 * j))
        s.setInstanceScale(m, (1.5 + 0.25 * j, 1.0, 2.0))
    geom = bf.Geometry.from_desc(s.flatten())      # the query below commits the moves itself: no sync, no frame in between
    assert all(m.proper for m in geom.meshes) and geom.radius > before.radius + 5.0
    sets = []
    for kind, (o, d, mesh, face, small) in ray_sets(geom, "many", seed=7).items():
        c, tmax, a = truth(geom, o, d, mesh, face, small, ties=COPLANAR["many-proper"])
        sets.append((kind, o, d, c, tmax, a))
    kind, o, d, c, *_ = sets[1]
    assert np.isin(c["mesh"][c["decided"]], moved).sum() >= 8 * 12      # the moved instances are found where they are now
    for fg, pt in VARIANTS:
        s.set_option("force_geom", fg)
        s.set_option("pair_trace", pt)
        judge(s, geom, sets, f"moved instances force_geom={fg} pair_trace={pt}")
    s.close()


@pytest.mark.parametrize("kind", ["band", "interleaved"])
def test_band_and_interleaved_contexts(P, kind):
    _, geom, sets = scene_and_truth(P, "showcase-16")
    s, _ = device_scene(P, "showcase-16", 64, 64, **(dict(tile_y0=16, tile_rows=16) if kind == "band" else dict(interleave=(1, 2))))
    judge(s, geom, sets, kind)
    s.close()
