"""The ray tracer's host mirror (host/rt/, ptrt_amd.rt) and the CPU restatement, without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import rt_restatement as R

f32 = np.float32


@pytest.fixture(scope="module")
def rt(P):
    import ptrt_amd.rt as rt
    return rt


def _host(rt, W=64, H=48):
    return rt.Scene(W, H, device=rt.HOST_ONLY)


def test_camera_defaults_and_setters(rt):
    s = _host(rt, 200, 100)
    c = s.getCamera()
    # Camera(aspect, 2, 1): vertical points down, the corner at (-2, 1, -1)
    assert c["horizontal"].tolist() == [4.0, 0.0, 0.0] and c["vertical"].tolist() == [0.0, -2.0, 0.0]
    assert c["lower_left_corner"].tolist() == [-2.0, 1.0, -1.0] and c["corner_minus_origin"].tolist() == [-2.0, 1.0, -1.0]
    s.moveCamera((1, 2, 3))
    c = s.getCamera()
    assert c["origin"].tolist() == [1, 2, 3] and c["lower_left_corner"].tolist() == [-1.0, 3.0, 2.0]
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 90.0)
    c = s.getCamera()
    h = f32(math.tan(f32(90.0) * f32(0.01745329251994329577) * f32(0.5)))
    assert np.allclose(c["vertical"], [0, 2 * h, 0]) and np.allclose(c["horizontal"], [4 * h, 0, 0])
    assert np.allclose(c["forward"], [0, 0, -1])
    s.lookCameraAt((5, 0, 5))
    c = s.getCamera()
    assert np.allclose(c["forward"], [1, 0, 0], atol=1e-6)
    assert math.isclose(float(np.linalg.norm(c["vertical"])), float(2 * h), rel_tol=1e-6)


def test_material_constructor_presets_and_defaults(rt):
    m = rt.Material()
    assert m.albedo == pytest.approx((0.8, 0.8, 0.8)) and m.specular == pytest.approx((0.04,) * 3)
    assert m.clearcoat_roughness == pytest.approx(0.03) and m.iridescence_thickness == 550.0
    m = rt.Material((1.0, 0.5, 0.0), 0.3, 0.5)
    want = [f32(1 - 0.5) * f32(0.04) + f32(0.5) * f32(a) for a in (1.0, 0.5, 0.0)]
    assert list(m.specular) == [float(w) for w in want]
    g = rt.Materials.Gold()
    assert g.metallic == 1.0 and g.roughness == pytest.approx(0.1) and g.specular == pytest.approx((1.0, 0.782, 0.344))
    glass = rt.Materials.Glass()
    assert glass.transmission == 1.0 and glass.ior == pytest.approx(1.5)
    assert rt.Materials.BrushedAluminum().anisotropy == pytest.approx(0.8)


def test_lights_and_scene_defaults(rt):
    s = _host(rt)
    i = s.info()
    assert i["ambient"].tolist() == pytest.approx([0.1] * 3) and i["use_sky"]
    assert i["sky_top"].tolist() == pytest.approx([0.6, 0.7, 1.0])
    s.addSpotLight((0, 3, 0), (0, -2, 0), (1, 1, 1), 2.0, 0.3, 0.6, 40.0)
    s.addDirectionalLight((0, 0, -3), (1, 1, 1))
    sp, dl = s.getLight(0), s.getLight(1)
    assert sp.type == rt.LIGHT_SPOT and sp.inner_cone == pytest.approx(math.cos(0.3)) and sp.outer_cone == pytest.approx(math.cos(0.6))
    assert (sp.direction.x, sp.direction.y, sp.direction.z) == (0.0, -1.0, 0.0)
    assert dl.type == rt.LIGHT_DIRECTIONAL and dl.direction.z == -1.0


def _check_tree(f, nodes, prims, leaf_max, verts):
    assert sorted(prims.tolist()) == list(range(len(f)))          # every face exactly once
    seen = 0
    for i, n in enumerate(nodes):
        if n.count > 0:
            assert n.count <= leaf_max
            seen += n.count
            for p in prims[n.start:n.start + n.count]:
                tri = verts[f[p]]
                assert (tri.min(0) >= [n.bmin.x, n.bmin.y, n.bmin.z]).all()
                assert (tri.max(0) <= [n.bmax.x, n.bmax.y, n.bmax.z]).all()
        else:
            for c in (n.left, n.right):
                assert c > i
                ch = nodes[c]
                assert ch.bmin.x >= n.bmin.x and ch.bmin.y >= n.bmin.y and ch.bmin.z >= n.bmin.z
                assert ch.bmax.x <= n.bmax.x and ch.bmax.y <= n.bmax.y and ch.bmax.z <= n.bmax.z
    assert seen == len(f)


@pytest.mark.parametrize("target,tol", [(4, 2), (1, 0), (8, 3)])
def test_sah_tree_invariants(rt, target, tol):
    s = _host(rt)
    i = s.addSphere(40, rt.Material())
    s.setBVHLeafTarget(target, tol)
    s.uploadToGPU()                                              # host-only: builds the tree, sends nothing
    f, nodes, prims = s.mesh(i).tree()
    _check_tree(f, nodes, prims, target + tol, s.mesh(i).vertices)


def _brute(snap, o, d):
    """Closest hit over every triangle of every mesh, no tree."""
    best_t = np.full(len(o), np.inf)
    for m in snap["meshes"]:
        M = R.MeshData(m)
        lo, ld, _ = M.local(o, d)
        for fi in range(M.face_count):
            ok, t = M.tri(np.full(len(o), fi), lo, ld)
            best_t = np.where(ok & (t < best_t), t, best_t)
    return best_t


def test_walk_equals_brute_force(rt):
    s = _host(rt, 48, 32)
    i = s.addSphere(12, rt.Material())
    s.mesh(i).setPosition((0.2, -0.1, -3.0))
    s.mesh(i).setRotation((0.3, 0.2, 0.1))
    j = s.addCube(rt.Material())
    s.mesh(j).translate((0.9, 0.3, 0.4))
    s.uploadToGPU()
    snap = s.snapshot()
    rng = np.random.default_rng(3)
    o = np.zeros((400, 3), f32)
    d = R.normalize((rng.standard_normal((400, 3)) * [0.4, 0.4, 1] + [0, 0, -1]).astype(f32))
    hit, t, _, _ = R.trace([R.MeshData(m) for m in snap["meshes"]], o, d)
    bt = _brute(snap, o, d)
    assert np.array_equal(hit, np.isfinite(bt)) and hit.sum() > 50
    assert np.array_equal(t[hit], bt[hit].astype(f32))
    # any hit: some triangle closer than tmax
    M = R.MeshData(snap["meshes"][0])
    tmax = np.full(400, f32(3.0))
    ah = R.any_hit(M, o, d, tmax)
    lo, ld, _ = M.local(o, d)
    brute = np.zeros(400, bool)
    for fi in range(M.face_count):
        ok, tt = M.tri(np.full(400, fi), lo, ld)
        brute |= ok & (tt < tmax)
    assert np.array_equal(ah, brute)


def test_hand_checked_pixels(rt, O):
    # nothing in view: the sky lerp, then Reinhard, gamma, * 255
    s = _host(rt, 8, 8)
    i = s.addCube(rt.Material())
    s.mesh(i).setPosition((0, 0, 50))                                 # behind the camera
    s.uploadToGPU()
    img = R.render(s.snapshot(), 8, 8, O)
    d = R.normalize(np.array([[-1 + 2 * 4.5 / 8, -1 + 2 * 4.5 / 8, -1.0]], f32))  # pixel (4, 4): vertical points down
    t = f32(0.5) * (d[0, 1] + f32(1))
    c = (f32(1) - t) * R.V([1, 1, 1]) + t * R.V([0.6, 0.7, 1.0])
    c = c / (c + f32(1))
    want = (np.minimum(O.detmath(4, c, np.full(3, R.GAMMA, f32)), 1) * f32(255)).astype(np.uint8)
    assert img[8 - 1 - 4, 4].tolist() == want.tolist()
    # ambient only (no lights, sky off), roughness 1 and metallic 0: F_ambient = F0 + (max(1 - 1, F0) - F0) x^5 = 0.04
    # at every angle, so every floor pixel is (1 - 0.04) * albedo * ambient
    s2 = _host(rt, 8, 8)
    s2.addPlaneXZ(-1.0, 10.0, rt.Material((0.5, 0.5, 0.5), 1.0, 0.0))
    s2.disableSky()
    s2.uploadToGPU()
    img2 = R.render(s2.snapshot(), 8, 8, O)
    assert (img2[:4] == 0).all()                                      # upper half: the sky is off
    c = (f32(1) - f32(0.04)) * f32(0.5) * f32(0.1)
    c = c / (c + f32(1))
    byte = int(min(float(O.detmath(4, np.array([c], f32), np.array([R.GAMMA], f32))[0]), 1.0) * 255.0)
    assert byte == 62 and (img2[4:] == byte).all()                    # 0.048 -> Reinhard 0.0458 -> gamma 0.2463 -> 62.8
    # one point light above the floor: one pixel recomputed in float64 from the reference's formulas
    s2.addPointLight((0.3, 0.5, -2.0), (1.0, 0.9, 0.8), 1.5, 10.0)
    s2.uploadToGPU()
    snap = s2.snapshot()
    img3 = R.render(snap, 8, 8, O)
    v = snap["view"]
    vec = lambda a: np.array([a.x, a.y, a.z])
    x, y = 5, 1                                                       # a floor pixel (the default camera's vertical points down)
    d = vec(v.corner_minus_origin) + (x + 0.5) / 8 * vec(v.horizontal) + (1 - (y + 0.5) / 8) * vec(v.vertical)
    d /= np.linalg.norm(d)
    t = -1.0 / d[1]
    P = t * d
    N = np.array([0.0, 1.0, 0.0])
    V = -d
    Lv = np.array([0.3, 0.5, -2.0]) - P
    dist = np.linalg.norm(Lv)
    L = Lv / dist
    H = (L + V) / np.linalg.norm(L + V)
    nl, nv, nh, vh = N @ L, max(N @ V, 0.0), max(N @ H, 0.0), max(V @ H, 0.0)
    a2 = 1.0 ** 4
    D = a2 / max(math.pi * (nh * nh * (a2 - 1) + 1) ** 2, 0.001)
    k = (1.0 + 1.0) ** 2 / 8
    G = nv / (nv * (1 - k) + k + 0.001) * nl / (nl * (1 - k) + k + 0.001)
    F = 0.04 + 0.96 * (1 - vh) ** 5
    spec = D * G * F / (4 * nv * nl + 0.001)
    att = (10.0 / (10.0 + dist)) ** 2
    col = np.array([1.0, 0.9, 0.8])
    c = 0.96 * 0.5 * 0.1 + ((1 - F) * 0.5 / math.pi + spec) * col * 1.5 * 20 * nl * att
    want = np.floor(np.clip((c / (c + 1)) ** 0.4545454545, 0, 1) * 255)
    assert np.abs(img3[8 - 1 - y, x].astype(int) - want).max() <= 1, (img3[8 - 1 - y, x], want)
    assert img3[8 - 1 - y, x].min() > byte


def test_ppm_and_obj_round_trip(rt, tmp_path):
    s = _host(rt, 3, 2)
    px = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    p = tmp_path / "a.ppm"
    s.saveAsPPM(p, px)
    lines = p.read_text().splitlines()
    assert lines[:3] == ["P3", "3 2", "255"] and lines[3] == "0 1 2" and len(lines) == 3 + 6
    obj = tmp_path / "q.obj"
    obj.write_text("# quad\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1/1/1 2/2/2 3/3/3 4/4/4\n")
    i = s.addMesh(obj)
    f, _, _ = s.mesh(i).tree()
    assert f.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert s.mesh(i).vertices.tolist()[2] == [1.0, 1.0, 0.0]
    with pytest.raises(rt.RtError):
        s.addMesh(tmp_path / "missing.obj")


def test_c_entries_refuse_null_stale_and_no_device(P, rt):
    L = P.lib
    ctx = C.c_void_p()
    assert L.ptrt_rt_create(64, 64, 0, None) == -1
    assert L.ptrt_rt_create(0, 64, 0, C.byref(ctx)) == -1 and not ctx.value
    buf = C.create_string_buffer(4096)                               # stands in for a dead handle
    before = buf.raw
    fake = C.cast(buf, C.c_void_p)
    assert L.ptrt_rt_upload_mesh(fake, 0, None, 0, None, 0) == -1
    assert L.ptrt_rt_upload_bvh(fake, 0, None, 0, None, 0) == -1
    assert L.ptrt_rt_set_scene(fake, None, 0, None, 0) == -1
    assert L.ptrt_rt_render(fake, None, None, 0) == -1
    assert b"ptrt_rt_render" in L.ptrt_rt_last_error(fake)
    assert L.ptrt_rt_upload_mesh(None, 0, None, 0, None, 0) == -1
    L.ptrt_rt_destroy(fake)
    L.ptrt_rt_destroy(None)
    assert buf.raw == before
    import torch
    if not torch.cuda.is_available():
        assert L.ptrt_rt_create(64, 64, 0, C.byref(ctx)) == -2 and not ctx.value
        with pytest.raises(rt.RtError):
            rt.Scene(64, 64, device=0)
    s = _host(rt)
    s.addCube()
    s.uploadToGPU()
    with pytest.raises(rt.RtError):
        s.render()


def test_hrt_entries_refuse_null_and_stale(P, rt):
    L = P.lib
    buf = C.create_string_buffer(4096)                               # a handle that was never a scene
    before = buf.raw
    fake = C.cast(buf, C.c_void_p)
    f3 = (C.c_float * 3)(1, 2, 3)
    for name, args in [("hrt_upload", ()), ("hrt_disable_sky", ()), ("hrt_add_cube", (None,)),
                       ("hrt_set_ambient_light", (f3,)), ("hrt_mesh_scale", (0, f3)), ("hrt_render", (None,)),
                       ("hrt_snap_counts", (None,)), ("hrt_get_camera", (None,))]:
        assert getattr(L, name)(fake, *args) == -1, name
        assert getattr(L, name)(None, *args) == -1, name
    assert buf.raw == before
    L.hrt_destroy(fake)
    L.hrt_destroy(None)
    assert buf.raw == before
    s = _host(rt)
    i = s.addCube()
    h = s._h
    # NULL outputs and inputs of a live scene: -1 and a message naming the entry, nothing written
    for name, args in [("hrt_get_light", (0, None)), ("hrt_info", (None, None)), ("hrt_get_camera", (None,)),
                       ("hrt_snap_counts", (None,)), ("hrt_snap_view", (None,)), ("hrt_snap_lights", (None,)),
                       ("hrt_mesh_info", (i, None)), ("hrt_snap_mesh", (i, None, None, None, None, None, None)),
                       ("hrt_set_ambient_light", (None,)), ("hrt_mesh_scale", (i, None)), ("hrt_add_mesh", (None, None)),
                       ("hrt_render", (None,)), ("hrt_render_to_device", (None,)), ("hrt_save_ppm", (None, None)),
                       ("hrt_add_point_light", (None, None, 1.0, 1.0)), ("hrt_set_camera", (None, None, None, 45.0, 0.0, 1.0))]:
        assert getattr(L, name)(h, *args) == -1, name
        assert b"NULL" in L.hrt_last_error(), name
    assert L.hrt_material_preset(None, None, 0.0, None) == -1
    assert L.hrt_material_preset(b"NoSuchPreset", None, 0.0, C.byref(rt.RtMaterial())) == -1
    s.close()
    assert L.hrt_upload(h) == -1                                     # closed: stale
    assert b"bad scene handle" in L.hrt_last_error()


def test_presets(rt):
    M = rt.Materials
    names = M.PLAIN + M.COLOURED + M.STONES + ("EmissiveLamp",)
    assert len(names) == 36
    assert M.Diamond().ior == pytest.approx(2.42) and M.Diamond().specular == pytest.approx((0.17,) * 3)
    assert M.Water().transmission == pytest.approx(0.9) and M.Water().roughness == pytest.approx(0.01)
    assert M.FrostedGlass().transmission_roughness == pytest.approx(0.3) and M.FrostedGlass().roughness == pytest.approx(0.3)
    car = M.CarPaint((0.8, 0.1, 0.1))
    assert car.clearcoat == 1.0 and car.metallic == pytest.approx(0.3) and car.specular == pytest.approx((0.05,) * 3)
    pearl = M.PearlescentPaint((0.8, 0.1, 0.1))
    assert pearl.iridescence == pytest.approx(0.8) and pearl.iridescence_thickness == 400.0 and pearl.clearcoat == 1.0
    assert M.Velvet((0.5, 0.1, 0.6)).sheen_tint == pytest.approx((0.6, 0.12, 0.72))
    assert M.Silk((0.1, 0.3, 0.8)).anisotropy == pytest.approx(0.5)
    assert M.Skin().subsurface_radius == pytest.approx(0.5) and M.Wax().subsurface_color == pytest.approx((1.0, 0.9, 0.7))
    assert M.OilSlick().metallic == pytest.approx(0.95) and M.SoapBubble().iridescence_thickness == 380.0
    assert M.NeonLight((0.3, 0.8, 1.0)).emission == pytest.approx((3.0, 8.0, 10.0))
    assert M.NeonLight((0.3, 0.8, 1.0)).albedo == pytest.approx((0.03, 0.08, 0.1))
    assert M.EmissiveLamp((1, 0.5, 0.2)).emission == pytest.approx((5.0, 2.5, 1.0))
    assert M.EmissiveLamp((1, 0.5, 0.2), 2.0).emission == pytest.approx((2.0, 1.0, 0.4))
    assert M.MarbleNero().roughness == pytest.approx(0.12) and M.MarbleNero(False).clearcoat == pytest.approx(0.20)
    assert M.MarbleCarrara().subsurface_radius == 1.0 and M.MarbleVerde().ior == pytest.approx(1.49)
    assert M.WoodCherry().clearcoat == pytest.approx(0.3) and M.WoodCherry().specular == pytest.approx((0.04,) * 3)
    assert M.Ice().transmission == pytest.approx(0.7) and M.Chrome().roughness == pytest.approx(0.02)


def test_demo_scene_recipes(rt):
    counts = {"cornell": (8, 1), "showcase1": (16, 3), "light_show": (14, 5), "architectural": (12, 4),
              "material_showcase": (21, 3)}
    for name, recipe in rt.scenes.DEMO_SCENES.items():
        s = _host(rt)
        recipe(s)
        i = s.info()
        assert (i["meshes"], i["lights"]) == counts[name], name
        s.close()
    s = rt.Scene.createLitTestScene(64, 48, device=rt.HOST_ONLY)
    assert s.info()["meshes"] == 3 and s.info()["lights"] == 3 and s.getLight(2).type == rt.LIGHT_SPOT
    assert s.getMeshMaterial(2).metallic == 1.0


def test_forwarding_header(P, tmp_path):
    """A caller's unchanged `#include "raytracer/RTscene.cuh"` compiles against the mirror with -I host/fwd."""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/llvm/bin/clang++"
    pkg = os.path.dirname(os.path.dirname(P.__file__))
    src = tmp_path / "caller.cpp"
    src.write_text("""
#include "raytracer/RTscene.cuh"
int main() {
    Scene s(32, 24, ptrt_rt::HOST_ONLY);
    Mesh *m = s.addCube(Materials::Glass());
    m->scale(2.0f);
    s.addPointLight(vec3(0, 4, 0), vec3(1.0f));
    s.uploadToGPU();
    auto lit = Scenes::createLitTestScene(16, 16, ptrt_rt::HOST_ONLY);
    return (s.getMeshCount() == 1 && !m->bvhNodes.empty() && lit->getMeshCount() == 3) ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host", "fwd"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0
