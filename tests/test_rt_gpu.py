"""The one-bounce ray tracer on the GPU (ptrt_amd.rt.Scene -> ptrt_rt_render -> rt_render_kernel): every image equals
the CPU restatement of tests/rt_restatement.py byte for byte, computed from the scene's own snapshot()."""
import numpy as np
import pytest

import rt_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(P):
    import ptrt_amd.rt as rt
    return rt


def _check(rt, O, s, what=""):
    got = s.render()
    want = R.render(s.snapshot(), s.width, s.height, O)
    bad = np.flatnonzero((got != want).any(axis=2))
    assert bad.size == 0, f"{what}: {bad.size} pixels differ, first {bad[:6]}: gpu {got.reshape(-1, 3)[bad[:3]].tolist()} " \
        f"cpu {want.reshape(-1, 3)[bad[:3]].tolist()}"
    return got


def _scene(rt, W, H, recipe):
    s = rt.Scene(W, H, device=0)
    recipe(s)
    s.uploadToGPU()
    return s


@pytest.mark.parametrize("name", sorted(["cornell", "showcase1", "light_show", "architectural", "material_showcase"]))
def test_demo_scenes_256(rt, O, name):
    s = _scene(rt, 256, 256, rt.scenes.DEMO_SCENES[name])
    img = _check(rt, O, s, name)
    assert img.mean() > 10
    s.close()


@pytest.mark.parametrize("name", ["cornell", "light_show"])
def test_demo_scenes_1080p(rt, O, name):
    s = _scene(rt, 1920, 1080, rt.scenes.DEMO_SCENES[name])
    _check(rt, O, s, name + " 1080p")
    s.close()


def test_lit_test_scene(rt, O):
    s = rt.Scene.createLitTestScene(200, 150, device=0)
    s.uploadToGPU()
    _check(rt, O, s, "Scenes::createLitTestScene")
    s.close()


def test_readme_glass_sphere(rt, O):
    s = _scene(rt, 256, 192, rt.scenes.readme)
    _check(rt, O, s, "readme")
    s.close()


def _lobe_scene(rt, mat, light="point", sphere_mat=None):
    """The material on a rotated cube (mesh 1; the cube's faces point outwards, so lit faces face the camera), a
    sphere beside it (mesh 2; the reference's sphere winding points its normals inwards), a floor (mesh 0)."""
    def recipe(s):
        s.addPlaneXZ(-1.0, 6.0, rt.Material((0.7, 0.7, 0.7), 0.6, 0.0))
        i = s.addCube(mat)
        s.mesh(i).scale(1.6).moveTo((0.0, 0.0, 0.0))           # baked: centred on its own origin
        s.mesh(i).setRotation((0.35, 0.6, 0.15))                # descriptor: rotated about that centre, then moved
        s.mesh(i).setPosition((0.0, -0.4, -4.8))
        j = s.addSphere(16, sphere_mat or rt.Material((0.2, 0.5, 0.9), 0.3, 0.0))
        s.mesh(j).setPosition((1.4, -0.4, -2.5))
        if light == "point":
            s.addPointLight((1.0, 2.5, 0.5), (1.0, 0.9, 0.8), 2.0, 30.0)
            s.addPointLight((-3.5, 0.5, -7.5), (0.6, 0.7, 1.0), 2.0, 30.0)   # behind the cube: what subsurface needs
        elif light == "directional":
            s.addDirectionalLight((-0.3, -1.0, -0.8), (1.0, 1.0, 1.0), 0.5)
        elif light == "spot":
            s.addSpotLight((0.5, 3.0, 0.0), (-0.1, -1.0, -1.0), (1.0, 1.0, 1.0), 3.0, 0.3, 0.6, 50.0)
        elif light == "spot_equal_cones":
            s.addSpotLight((0.5, 3.0, 0.0), (-0.1, -1.0, -1.0), (1.0, 1.0, 1.0), 3.0, 0.5, 0.5, 50.0)
        s.setCamera((0.0, 1.0, 2.0), (0.0, -0.4, -4.8), (0, 1, 0), 50.0)
    return recipe


@pytest.mark.parametrize("light", ["point", "directional", "spot", "spot_equal_cones"])
def test_light_types(rt, O, light):
    s = _scene(rt, 160, 120, _lobe_scene(rt, rt.Material((0.8, 0.3, 0.2), 0.4, 0.0), light))
    _check(rt, O, s, light)
    s.close()


LOBES = {
    "anisotropy": dict(metallic=1.0, roughness=0.35, anisotropy=0.8),
    "anisotropy_neg": dict(metallic=0.5, roughness=0.5, anisotropy=-0.6),
    "clearcoat": dict(clearcoat=1.0, clearcoat_roughness=0.05),
    "sheen": dict(sheen=1.0, sheen_tint=(0.9, 0.2, 0.5)),
    "subsurface": dict(subsurface_radius=0.8, subsurface_color=(1.0, 0.5, 0.3)),
    "iridescence": dict(iridescence=1.0, iridescence_thickness=400.0),
    "glass_smooth": dict(transmission=1.0, roughness=0.0, ior=1.5, albedo=(0.9, 1.0, 0.8)),
    "glass_rough": dict(transmission=1.0, roughness=0.3, transmission_roughness=0.25, ior=1.33),
    "glass_zero_channel": dict(transmission=0.8, roughness=0.0, ior=1.5, albedo=(1.0, 0.0, 0.6)),
    "glass_tir": dict(transmission=1.0, roughness=0.0, ior=2.4),
}


BASE = dict(albedo=(0.8, 0.6, 0.3), roughness=0.4, metallic=0.0)


@pytest.mark.parametrize("lobe", sorted(LOBES))
def test_material_lobes(rt, O, lobe):
    base = rt.Material(BASE["albedo"], BASE["roughness"], BASE["metallic"])
    kw = dict(LOBES[lobe])
    # the lobe alone: the base material with the lobe's fields (anisotropy keeps its metal and roughness)
    s0 = _scene(rt, 160, 120, _lobe_scene(rt, base.replace(**{k: v for k, v in kw.items() if k in ("metallic", "roughness")})))
    without = _check(rt, O, s0, lobe + " without the lobe")
    s0.close()
    # glass also on the sphere: its inward normals make a primary hit an exit (n1 = ior), where ior 2.4 reflects totally
    sphere = base.replace(**kw) if "transmission" in kw else None
    s = _scene(rt, 160, 120, _lobe_scene(rt, base.replace(**kw), sphere_mat=sphere))
    img = _check(rt, O, s, lobe)
    changed = (img != without).any(axis=2).sum()
    assert changed > 200, f"{lobe}: only {changed} pixels depend on the lobe"
    s.close()


def test_sky_off_and_gradient(rt, O):
    s = _scene(rt, 128, 96, _lobe_scene(rt, rt.Materials.Gold()))
    gold = _check(rt, O, s, "sky")
    s.setMeshMaterial(1, rt.Materials.PlasticRed())
    s.uploadToGPU()
    assert (_check(rt, O, s, "plastic") != gold).any(axis=2).sum() > 200   # the cube's material shows
    s.setSkyGradient((0.1, 0.2, 0.9), (0.9, 0.5, 0.1))
    _check(rt, O, s, "gradient")
    s.disableSky()
    _check(rt, O, s, "sky off")
    s.close()


def test_baked_transforms_and_dense_sphere(rt, O):
    def recipe(s):
        i = s.addSphere(256, rt.Material((0.9, 0.9, 0.9), 0.3, 0.0))
        s.mesh(i).scale((2.0, 2.0, 2.0)).moveTo((0.0, 0.0, -4.0)).rotateSelfEulerXYZ((0.2, 0.4, 0.1))
        j = s.addCube(rt.Material((0.9, 0.2, 0.2), 0.5, 0.0))
        s.mesh(j).translate((1.5, 0.0, -1.0))
        s.addPointLight((2, 3, 0), (1, 1, 1), 2.0)
        s.addDirectionalLight((0.2, -1, -0.2), (0.5, 0.6, 1.0), 0.3)
    s = _scene(rt, 192, 192, recipe)
    _check(rt, O, s, "dense sphere")
    s.close()


def test_stale_render_and_render_to_device(rt, O):
    import torch
    s = _scene(rt, 128, 96, _lobe_scene(rt, rt.Material((0.8, 0.3, 0.2), 0.4, 0.0)))
    before = _check(rt, O, s, "before")
    s.mesh(1).setPosition((0.6, 0.2, -2.5))                  # not uploaded: render() keeps the last upload
    stale = s.render()
    assert np.array_equal(stale, before)
    t = torch.zeros(96 * 128 * 3, dtype=torch.uint8, device="cuda:0")
    s.render_to_device(t)                                     # rebuilds descriptors: the moved mesh
    fresh = t.cpu().numpy().reshape(96, 128, 3)
    assert not np.array_equal(fresh, before)
    assert np.array_equal(fresh, R.render(s.snapshot(), 128, 96, O))
    assert np.array_equal(s.render(), fresh)                  # the device path's upload is now the last one
    # a direct vertex edit without bvhDirty is walked with the OLD tree
    old = s.snapshot()["meshes"][1]
    v = s.mesh(1).vertices
    s.mesh(1).vertices = v + np.float32(0.25)
    s.render_to_device(t)
    quirk = t.cpu().numpy().reshape(96, 128, 3)
    assert np.array_equal(quirk, R.render(s.snapshot(), 128, 96, O))
    assert not s.mesh(1).info()["bvhDirty"]
    new = s.snapshot()["meshes"][1]
    assert np.array_equal(new["vertices"], v + np.float32(0.25))
    for k in ("bmin", "bmax", "left", "right", "start", "count", "prims"):
        assert np.array_equal(new[k], old[k]), k                 # the tree that was sent is the old one
    s.mesh(1).setBVHLeafParams(4, 2)                             # bvhDirty: the next send rebuilds over the moved vertices
    s.render_to_device(t)
    rebuilt = t.cpu().numpy().reshape(96, 128, 3)
    assert not np.array_equal(s.snapshot()["meshes"][1]["bmin"], old["bmin"])
    assert not np.array_equal(rebuilt, quirk)                    # the old tree's boxes cut off part of the moved cube
    assert np.array_equal(s.render(), s.render())             # repeated renders are identical
    s.close()


def test_between_path_frames(P, O, rt, blue_noise):
    from common import assert_frames_equal, render_both
    ps = P.Scene(96, 64, device=0)
    P.scenes.cornell(ps)
    gpu1, cpu1 = render_both(P, O, ps, blue_noise, spp=1, depth=3, frames=1)
    s = _scene(rt, 96, 64, rt.scenes.cornell)
    _check(rt, O, s, "between")
    gpu2, cpu2 = render_both(P, O, ps, blue_noise, spp=1, depth=3, frames=1)
    assert_frames_equal(gpu1, cpu1)
    assert_frames_equal(gpu2, cpu2)
    s.close()
    ps.close()


def _chain_mesh(n, leaf_tris, leaf_box, inner_box, dummy_tri):
    """A tree the median split never builds, through the public C ABI: inner node k (index 2k) has leaf k (2k + 1) on
    the left and inner node k + 1 on the right; the last inner node's right child is a leaf with `dummy_tri`."""
    tris = list(leaf_tris) + [dummy_tri]
    verts = np.array([p for t in tris for p in t], np.float32)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    nodes = []
    for k in range(n):
        nodes.append((*inner_box, 2 * k + 1, 2 * k + 2, -1, 0))
        nodes.append((*leaf_box(k), -1, -1, k, 1))
    nodes.append((*inner_box, -1, -1, n, 1))  # the dummy leaf
    nd = np.array([(*b0, *b1, l, r, st, c) for (b0, b1, l, r, st, c) in nodes], dtype=object)
    return verts, faces, nd, np.arange(n + 1, dtype=np.int32)


def test_stack_limit_drops_pushes(rt, O, monkeypatch):
    """Both walks past the 32-entry stack: mesh A's near-first walk pushes its far leaves 0..39 and drops 32..39, so
    leaf 31's triangle is the closest hit found (leaf 39's would be nearer); mesh B's unordered walk drops the inner
    nodes below level 31, so its only occluder (in leaves 32..39) is never reached and A stays lit."""
    import ctypes as C
    from ptrt_amd import BvhNode, Vec3, lib
    n = 40
    big = ((-100.0, -100.0, -70.0), (100.0, 100.0, -1.0))
    # A: triangles facing -z (towards the light behind them) at z = -(3 - 0.02 i); leaf boxes far away at z ~ -(60 - i)
    a_tris = [((-20, -20, -(3 - 0.02 * i)), (0, 30, -(3 - 0.02 * i)), (20, -20, -(3 - 0.02 * i))) for i in range(n)]
    A = _chain_mesh(n, a_tris, lambda k: ((-100.0, -100.0, -(60.5 - k)), (100.0, 100.0, -(59.5 - k))), big,
                    ((500, 500, -2), (501, 500, -2), (500, 501, -2)))
    # B: every box covers the path to the light at z = -10; only leaves 32..39 hold the occluder at z = -5
    occ = ((-50, -50, -5), (0, 60, -5), (50, -50, -5))
    off = ((500, 500, -5), (501, 500, -5), (500, 501, -5))
    b_box = ((-100.0, -100.0, -6.0), (100.0, 100.0, -4.0))
    B = _chain_mesh(n, [occ if i >= 32 else off for i in range(n)], lambda k: b_box, b_box, off)
    mat = rt.Material((0.8, 0.8, 0.8), 0.5, 0.0)
    ctx = C.c_void_p()
    assert lib.ptrt_rt_create(64, 64, 0, C.byref(ctx)) == 0
    snap_meshes, descs = [], (rt.RtMesh * 2)()
    for i, (v, f, nd, pr) in enumerate((A, B)):
        nodes = (BvhNode * len(nd))()
        for j, row in enumerate(nd):
            nodes[j] = BvhNode(Vec3(*row[0:3]), Vec3(*row[3:6]), *[int(x) for x in row[6:10]])
        assert lib.ptrt_rt_upload_mesh(ctx, i, v.ctypes.data, len(v), f.ctypes.data, len(f)) == 0
        assert lib.ptrt_rt_upload_bvh(ctx, i, nodes, len(nd), pr.ctypes.data, len(pr)) == 0, lib.ptrt_rt_last_error(ctx)
        descs[i].material = mat._m
        descs[i].rotation[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        descs[i].inv_rotation[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        arr = np.array([list(r) for r in nd], dtype=np.float64)
        snap_meshes.append({"vertices": v, "faces": f, "bmin": arr[:, 0:3].astype(np.float32),
                            "bmax": arr[:, 3:6].astype(np.float32), "left": arr[:, 6].astype(np.int32),
                            "right": arr[:, 7].astype(np.int32), "start": arr[:, 8].astype(np.int32),
                            "count": arr[:, 9].astype(np.int32), "prims": pr, "translation": np.zeros(3, np.float32),
                            "rotation": np.eye(3, dtype=np.float32), "inv_rotation": np.eye(3, dtype=np.float32),
                            "material": mat})
    light = rt.RtLight(0, Vec3(0, 0, -10), Vec3(0, -1, 0), Vec3(1, 1, 1), 3.0, 20.0, 0.9, 0.8)
    assert lib.ptrt_rt_set_scene(ctx, descs, 2, C.byref(light), 1) == 0
    view = rt.RtView(Vec3(0, 0, 0), Vec3(-1, 1, -1), Vec3(2, 0, 0), Vec3(0, -2, 0), Vec3(0.05, 0.05, 0.05),
                     Vec3(0.6, 0.7, 1.0), Vec3(1, 1, 1), 1)
    got = np.zeros((64, 64, 3), np.uint8)
    assert lib.ptrt_rt_render(ctx, C.byref(view), got.ctypes.data, 0) == 0, lib.ptrt_rt_last_error(ctx)
    lib.ptrt_rt_destroy(ctx)
    snap = {"meshes": snap_meshes, "lights": [light], "view": view}
    want = R.render(snap, 64, 64, O)
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    assert got.mean() > 5
    monkeypatch.setattr(R, "STACK", 64)                           # the same walks with room for every push
    roomy = R.render(snap, 64, 64, O)
    assert (roomy != want).any(axis=2).mean() > 0.9              # so the dropped pushes decide these pixels
