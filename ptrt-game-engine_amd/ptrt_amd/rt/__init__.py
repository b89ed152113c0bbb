"""ptrt_amd.rt -- the one-bounce ray tracer of the reference's src/raytracer/ (RTscene.cuh).

``Scene`` is the C++ mirror of host/rt/RTscene.hpp (namespace ptrt_rt) reached through its flat ``hrt_*`` entry
points; it renders with rt_render_kernel through the ``ptrt_rt_*`` C ABI of include/ptrt.h.  ``Scene(w, h,
device=HOST_ONLY)`` builds and inspects scenes without a GPU (its uploadToGPU builds the trees and records what it
would send) but cannot render.  ``snapshot()`` returns exactly what the last upload or render sent.
"""
import ctypes as C

import numpy as np

from .. import Vec3, BvhNode, lib

HOST_ONLY = -1
LIGHT_POINT, LIGHT_DIRECTIONAL, LIGHT_SPOT = 0, 1, 2


class RtMaterial(C.Structure):
    _fields_ = [("albedo", Vec3), ("specular", Vec3), ("metallic", C.c_float), ("roughness", C.c_float),
                ("emission", Vec3), ("ior", C.c_float), ("transmission", C.c_float),
                ("transmission_roughness", C.c_float), ("clearcoat", C.c_float), ("clearcoat_roughness", C.c_float),
                ("subsurface_color", Vec3), ("subsurface_radius", C.c_float), ("anisotropy", C.c_float),
                ("sheen", C.c_float), ("sheen_tint", Vec3), ("iridescence", C.c_float),
                ("iridescence_thickness", C.c_float)]


class RtMesh(C.Structure):
    _fields_ = [("material", RtMaterial), ("translation", Vec3), ("rotation", C.c_float * 9),
                ("inv_rotation", C.c_float * 9)]


class RtLight(C.Structure):
    _fields_ = [("type", C.c_int32), ("position", Vec3), ("direction", Vec3), ("color", Vec3),
                ("intensity", C.c_float), ("range", C.c_float), ("inner_cone", C.c_float), ("outer_cone", C.c_float)]


class RtView(C.Structure):
    _fields_ = [("origin", Vec3), ("corner_minus_origin", Vec3), ("horizontal", Vec3), ("vertical", Vec3),
                ("ambient", Vec3), ("sky_top", Vec3), ("sky_bottom", Vec3), ("use_sky", C.c_int32)]


assert C.sizeof(RtMaterial) == 108 and C.sizeof(RtLight) == 56

_vp, _fp, _ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
_MP = C.POINTER(RtMaterial)


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


for _n, _r, _a in [
    ("ptrt_rt_create", C.c_int, (C.c_int, C.c_int, C.c_int, C.POINTER(_vp))),
    ("ptrt_rt_destroy", None, (_vp,)),
    ("ptrt_rt_last_error", C.c_char_p, (_vp,)),
    ("ptrt_rt_upload_mesh", C.c_int, (_vp, C.c_int, _vp, C.c_int, _vp, C.c_int)),
    ("ptrt_rt_upload_bvh", C.c_int, (_vp, C.c_int, _vp, C.c_int, _vp, C.c_int)),
    ("ptrt_rt_set_scene", C.c_int, (_vp, _vp, C.c_int, _vp, C.c_int)),
    ("ptrt_rt_render", C.c_int, (_vp, _vp, _vp, C.c_int)),
    ("hrt_last_error", C.c_char_p, ()),
    ("hrt_create", _vp, (C.c_int, C.c_int, C.c_int)),
    ("hrt_destroy", None, (_vp,)),
    ("hrt_material_make", C.c_int, (_fp, C.c_float, C.c_float, _MP)),
    ("hrt_material_default", C.c_int, (_MP,)),
    ("hrt_material_preset", C.c_int, (C.c_char_p, _fp, C.c_float, _MP)),
    ("hrt_create_lit_test_scene", _vp, (C.c_int, C.c_int, C.c_int)),
    ("hrt_add_cube", C.c_int, (_vp, _MP)),
    ("hrt_add_plane_xz", C.c_int, (_vp, C.c_float, C.c_float, _MP)),
    ("hrt_add_sphere", C.c_int, (_vp, C.c_int, _MP)),
    ("hrt_add_mesh", C.c_int, (_vp, C.c_char_p, _MP)),
    ("hrt_add_triangles", C.c_int, (_vp, _fp, C.c_int, _MP)),
    ("hrt_add_checkerboard_plane_xz", C.c_int, (_vp, C.c_float, C.c_int, C.c_float, _MP, _MP)),
    ("hrt_set_mesh_material", C.c_int, (_vp, C.c_int, _MP)),
    ("hrt_get_mesh_material", C.c_int, (_vp, C.c_int, _MP)),
    ("hrt_set_bvh_leaf_target", C.c_int, (_vp, C.c_int, C.c_int)),
    ("hrt_mesh_scale", C.c_int, (_vp, C.c_int, _fp)),
    ("hrt_mesh_translate", C.c_int, (_vp, C.c_int, _fp)),
    ("hrt_mesh_move_to", C.c_int, (_vp, C.c_int, _fp)),
    ("hrt_mesh_rotate_self", C.c_int, (_vp, C.c_int, _fp)),
    ("hrt_mesh_set_position", C.c_int, (_vp, C.c_int, _fp)),
    ("hrt_mesh_set_rotation", C.c_int, (_vp, C.c_int, _fp)),
    ("hrt_mesh_set_leaf_params", C.c_int, (_vp, C.c_int, C.c_int, C.c_int)),
    ("hrt_mesh_write_vertices", C.c_int, (_vp, C.c_int, _fp, C.c_int)),
    ("hrt_mesh_info", C.c_int, (_vp, C.c_int, _ip)),
    ("hrt_mesh_read", C.c_int, (_vp, C.c_int, _fp, _ip, _vp, _ip)),
    ("hrt_mesh_build_bvh", C.c_int, (_vp, C.c_int)),
    ("hrt_add_point_light", C.c_int, (_vp, _fp, _fp, C.c_float, C.c_float)),
    ("hrt_add_directional_light", C.c_int, (_vp, _fp, _fp, C.c_float)),
    ("hrt_add_spot_light", C.c_int, (_vp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float, C.c_float)),
    ("hrt_get_light", C.c_int, (_vp, C.c_int, C.POINTER(RtLight))),
    ("hrt_set_ambient_light", C.c_int, (_vp, _fp)),
    ("hrt_set_sky_gradient", C.c_int, (_vp, _fp, _fp)),
    ("hrt_disable_sky", C.c_int, (_vp,)),
    ("hrt_set_camera", C.c_int, (_vp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float)),
    ("hrt_set_camera_simple", C.c_int, (_vp, C.c_float, C.c_float)),
    ("hrt_move_camera", C.c_int, (_vp, _fp)),
    ("hrt_look_camera_at", C.c_int, (_vp, _fp, _fp)),
    ("hrt_get_camera", C.c_int, (_vp, _fp)),
    ("hrt_info", C.c_int, (_vp, _ip, _fp)),
    ("hrt_upload", C.c_int, (_vp,)),
    ("hrt_render", C.c_int, (_vp, _vp)),
    ("hrt_render_to_device", C.c_int, (_vp, _vp)),
    ("hrt_save_ppm", C.c_int, (_vp, C.c_char_p, _vp)),
    ("hrt_snap_counts", C.c_int, (_vp, _ip)),
    ("hrt_snap_mesh", C.c_int, (_vp, C.c_int, _ip, _fp, _ip, _vp, _ip, C.POINTER(RtMesh))),
    ("hrt_snap_lights", C.c_int, (_vp, _vp)),
    ("hrt_snap_view", C.c_int, (_vp, C.POINTER(RtView))),
]:
    _sig(_n, _r, *_a)


class RtError(RuntimeError):
    pass


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _check(rc):
    if rc < 0:
        raise RtError(lib.hrt_last_error().decode())
    return rc


def _vec(v):
    return (v.x, v.y, v.z)


class Material:
    """Material (RTscene.cuh:21-61).  Material() is the default; Material(albedo, roughness, metallic) sets
    specular = lerp(0.04, albedo, metallic), as the reference's constructor does.  Fields are snake_case."""
    _VEC = {"albedo", "specular", "emission", "subsurface_color", "sheen_tint"}

    def __init__(self, albedo=None, roughness=0.5, metallic=0.0):
        self._m = RtMaterial()
        if albedo is None:
            _check(lib.hrt_material_default(C.byref(self._m)))
        else:
            a = albedo if hasattr(albedo, "__len__") else (albedo,) * 3
            _check(lib.hrt_material_make(_f3(a), roughness, metallic, C.byref(self._m)))

    @classmethod
    def _wrap(cls, m):
        o = cls.__new__(cls)
        o._m = m
        return o

    def __getattr__(self, k):
        if k.startswith("_"):
            raise AttributeError(k)
        v = getattr(self._m, k)
        return _vec(v) if k in self._VEC else v

    def __setattr__(self, k, v):
        if k == "_m":
            object.__setattr__(self, k, v)
        elif k in self._VEC:
            setattr(self._m, k, Vec3(*[float(x) for x in (v if hasattr(v, "__len__") else (v,) * 3)]))
        else:
            setattr(self._m, k, float(v))

    def replace(self, **kw):
        m = Material._wrap(RtMaterial.from_buffer_copy(self._m))
        for k, v in kw.items():
            setattr(m, k, v)
        return m


class Materials:
    """The reference's presets (namespace Materials, RTscene.cuh:1297-1590), built by the C++ mirror."""

    @staticmethod
    def preset(name, colour=None, arg=0.0):
        m = RtMaterial()
        _check(lib.hrt_material_preset(name.encode(), _f3(colour) if colour is not None else None, arg, C.byref(m)))
        return Material._wrap(m)

    PLAIN = ("Gold", "Silver", "Copper", "Bronze", "Aluminum", "BrushedAluminum", "Iron", "Chrome", "Glass",
             "FrostedGlass", "Diamond", "Water", "SoapBubble", "Ice", "PlasticRed", "PlasticBlue", "PlasticGreen",
             "RubberBlack", "Concrete", "WoodOak", "WoodCherry", "WoodWalnut", "Skin", "Wax", "Jade", "OilSlick")
    COLOURED = ("CarPaint", "PearlescentPaint", "Velvet", "Silk", "Cotton", "NeonLight")
    STONES = ("MarbleCarrara", "MarbleNero", "MarbleVerde")

    @staticmethod
    def EmissiveLamp(colour, intensity=5.0):
        return Materials.preset("EmissiveLamp", colour, intensity)


for _p in Materials.PLAIN:
    setattr(Materials, _p, staticmethod(lambda _p=_p: Materials.preset(_p)))
for _p in Materials.COLOURED:
    setattr(Materials, _p, staticmethod(lambda colour, _p=_p: Materials.preset(_p, colour)))
for _p in Materials.STONES:
    setattr(Materials, _p, staticmethod(lambda polished=True, _p=_p: Materials.preset(_p, None, 1.0 if polished else 0.0)))


class Scene:
    """class Scene of RTscene.cuh:765-1236 (the C++ mirror ptrt_rt::Scene)."""

    def __init__(self, width, height, device=0, _handle=None):
        self._h = _handle or lib.hrt_create(width, height, device)
        if not self._h:
            raise RtError(lib.hrt_last_error().decode())
        self.width, self.height, self.device = width, height, device

    @classmethod
    def createLitTestScene(cls, width=800, height=600, device=0):
        """Scenes::createLitTestScene (RTscene.cuh:1596-1631), built by the C++ mirror."""
        h = lib.hrt_create_lit_test_scene(width, height, device)
        if not h:
            raise RtError(lib.hrt_last_error().decode())
        return cls(width, height, device, _handle=h)

    def close(self):
        if self._h:
            lib.hrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- meshes
    def addCube(self, mat=None):
        return _check(lib.hrt_add_cube(self._h, C.byref((mat or Material((1.0, 0.0, 0.0)))._m)))

    def addPlaneXZ(self, y, half, mat=None):
        return _check(lib.hrt_add_plane_xz(self._h, y, half, C.byref((mat or Material((0.8, 0.8, 0.8)))._m)))

    def addSphere(self, segments=32, mat=None):
        return _check(lib.hrt_add_sphere(self._h, segments, C.byref((mat or Material((1.0, 0.0, 0.0)))._m)))

    def addMesh(self, path, mat=None):
        return _check(lib.hrt_add_mesh(self._h, str(path).encode(), C.byref((mat or Material())._m)))

    def addTriangles(self, corners, mat=None):
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 9))
        return _check(lib.hrt_add_triangles(self._h, c.ctypes.data_as(_fp), c.shape[0], C.byref((mat or Material())._m)))

    def addCheckerboardPlaneXZ(self, y, tiles, size, white, black):
        _check(lib.hrt_add_checkerboard_plane_xz(self._h, y, tiles, size, C.byref(white._m), C.byref(black._m)))

    def setMeshMaterial(self, i, mat):
        _check(lib.hrt_set_mesh_material(self._h, i, C.byref(mat._m)))

    def getMeshMaterial(self, i):
        m = RtMaterial()
        _check(lib.hrt_get_mesh_material(self._h, i, C.byref(m)))
        return Material._wrap(m)

    def setBVHLeafTarget(self, target, tol=2):
        _check(lib.hrt_set_bvh_leaf_target(self._h, target, tol))

    def mesh(self, i):
        return MeshRef(self, i)

    # -- lights, sky, camera
    def addPointLight(self, pos, color, intensity=1.0, range=100.0):
        _check(lib.hrt_add_point_light(self._h, _f3(pos), _f3(color), intensity, range))

    def addDirectionalLight(self, direction, color, intensity=1.0):
        _check(lib.hrt_add_directional_light(self._h, _f3(direction), _f3(color), intensity))

    def addSpotLight(self, pos, direction, color, intensity=1.0, innerCone=0.5, outerCone=0.7, range=100.0):
        _check(lib.hrt_add_spot_light(self._h, _f3(pos), _f3(direction), _f3(color), intensity, innerCone, outerCone,
                                      range))

    def getLight(self, i):
        light = RtLight()
        _check(lib.hrt_get_light(self._h, i, C.byref(light)))
        return light

    def setAmbientLight(self, a):
        _check(lib.hrt_set_ambient_light(self._h, _f3(a)))

    def setSkyGradient(self, top, bottom):
        _check(lib.hrt_set_sky_gradient(self._h, _f3(top), _f3(bottom)))

    def disableSky(self):
        _check(lib.hrt_disable_sky(self._h))

    def setCamera(self, lookfrom, lookat, vup, vfov, aperture=0.0, focus_dist=1.0):
        _check(lib.hrt_set_camera(self._h, _f3(lookfrom), _f3(lookat), _f3(vup), vfov, aperture, focus_dist))

    def setCameraSimple(self, viewport_height=2.0, focal_length=1.0):
        _check(lib.hrt_set_camera_simple(self._h, viewport_height, focal_length))

    def moveCamera(self, pos):
        _check(lib.hrt_move_camera(self._h, _f3(pos)))

    def lookCameraAt(self, target, vup=(0, 1, 0)):
        _check(lib.hrt_look_camera_at(self._h, _f3(target), _f3(vup)))

    def getCamera(self):
        """{origin, lower_left_corner, horizontal, vertical, corner_minus_origin: float32[3], lens_radius, forward}"""
        o = (C.c_float * 19)()
        _check(lib.hrt_get_camera(self._h, o))
        a = np.array(o[:], dtype=np.float32)
        keys = ["origin", "lower_left_corner", "horizontal", "vertical", "corner_minus_origin"]
        d = {k: a[3 * i:3 * i + 3] for i, k in enumerate(keys)}
        d["lens_radius"], d["forward"] = a[15], a[16:19]
        return d

    def cameraOrigin(self):
        return self.getCamera()["origin"]

    def cameraForward(self):
        return self.getCamera()["forward"]

    def info(self):
        i5, f9 = (C.c_int * 5)(), (C.c_float * 9)()
        _check(lib.hrt_info(self._h, i5, f9))
        f = np.array(f9[:], dtype=np.float32)
        return {"meshes": i5[0], "lights": i5[1], "width": i5[2], "height": i5[3], "use_sky": bool(i5[4]),
                "ambient": f[0:3], "sky_top": f[3:6], "sky_bottom": f[6:9]}

    def getMeshCount(self):
        return self.info()["meshes"]

    # -- upload and render
    def uploadToGPU(self):
        _check(lib.hrt_upload(self._h))

    def render(self):
        """Scene::render: the last upload's meshes and lights, the current camera / ambient / sky -> (H, W, 3) uint8,
        bottom-up as the kernel writes it."""
        out = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        _check(lib.hrt_render(self._h, out.ctypes.data_as(_vp)))
        return out

    def render_to_device(self, tensor):
        """Scene::render_to_device into a contiguous uint8 device tensor of width * height * 3 elements."""
        if not tensor.is_contiguous() or tensor.numel() != self.width * self.height * 3 or str(tensor.dtype) != "torch.uint8":
            raise ValueError("render_to_device needs a contiguous uint8 tensor of width * height * 3 elements")
        _check(lib.hrt_render_to_device(self._h, C.c_void_p(tensor.data_ptr())))
        return tensor

    def saveAsPPM(self, path, pixels):
        p = np.ascontiguousarray(pixels, dtype=np.uint8)
        _check(lib.hrt_save_ppm(self._h, str(path).encode(), p.ctypes.data_as(_vp)))

    def snapshot(self):
        """What the last uploadToGPU / render_to_device sent, and the view the last render used (the current one if
        nothing rendered yet): {"meshes": [{vertices, faces, nodes, prims, translation, rotation, inv_rotation,
        material}], "lights": RtLight array, "view": RtView}."""
        c3 = (C.c_int * 3)()
        _check(lib.hrt_snap_counts(self._h, c3))
        meshes = []
        for i in range(c3[0]):
            n4 = (C.c_int * 4)()
            _check(lib.hrt_snap_mesh(self._h, i, n4, None, None, None, None, None))
            v = np.zeros((n4[0], 3), np.float32)
            f = np.zeros((n4[1], 3), np.int32)
            nodes = (BvhNode * max(n4[2], 1))()
            p = np.zeros(n4[3], np.int32)
            d = RtMesh()
            _check(lib.hrt_snap_mesh(self._h, i, n4, v.ctypes.data_as(_fp), f.ctypes.data_as(_ip), nodes,
                                     p.ctypes.data_as(_ip), C.byref(d)))
            nd = np.ctypeslib.as_array(C.cast(nodes, C.POINTER(C.c_int32)), (max(n4[2], 1) * 10,)).reshape(-1, 10)[:n4[2]]
            meshes.append({"vertices": v, "faces": f, "bmin": nd[:, 0:3].view(np.float32).copy(),
                           "bmax": nd[:, 3:6].view(np.float32).copy(), "left": nd[:, 6].copy(), "right": nd[:, 7].copy(),
                           "start": nd[:, 8].copy(), "count": nd[:, 9].copy(), "prims": p,
                           "translation": np.array(_vec(d.translation), np.float32),
                           "rotation": np.array(d.rotation[:], np.float32).reshape(3, 3),
                           "inv_rotation": np.array(d.inv_rotation[:], np.float32).reshape(3, 3),
                           "material": Material._wrap(RtMaterial.from_buffer_copy(d.material))})
        lights = (RtLight * max(c3[1], 1))()
        _check(lib.hrt_snap_lights(self._h, lights))
        view = RtView()
        _check(lib.hrt_snap_view(self._h, C.byref(view)))
        if not c3[2]:
            view = self.current_view()
        return {"meshes": meshes, "lights": list(lights)[:c3[1]], "view": view}

    def current_view(self):
        """The view a render would send now: camera vectors, ambient, sky."""
        c, i = self.getCamera(), self.info()
        v = RtView()
        for k in ("origin", "corner_minus_origin", "horizontal", "vertical"):
            setattr(v, k, Vec3(*[float(x) for x in c[k]]))
        v.ambient, v.sky_top, v.sky_bottom = (Vec3(*[float(x) for x in i[k]]) for k in ("ambient", "sky_top", "sky_bottom"))
        v.use_sky = int(i["use_sky"])
        return v


class MeshRef:
    """Scene::getMesh(i): the mirror's Mesh methods."""

    def __init__(self, scene, i):
        self.s, self.i = scene, i

    def _call(self, fn, v):
        _check(fn(self.s._h, self.i, _f3(v if hasattr(v, "__len__") else (v,) * 3)))
        return self

    def scale(self, s):
        return self._call(lib.hrt_mesh_scale, s)

    def translate(self, d):
        return self._call(lib.hrt_mesh_translate, d)

    def moveTo(self, p):
        return self._call(lib.hrt_mesh_move_to, p)

    def rotateSelfEulerXYZ(self, r):
        return self._call(lib.hrt_mesh_rotate_self, r)

    def setPosition(self, p):
        return self._call(lib.hrt_mesh_set_position, p)

    def setRotation(self, r):
        return self._call(lib.hrt_mesh_set_rotation, r)

    def setBVHLeafParams(self, target, tol=2):
        _check(lib.hrt_mesh_set_leaf_params(self.s._h, self.i, target, tol))

    def buildBVH(self):
        _check(lib.hrt_mesh_build_bvh(self.s._h, self.i))

    def info(self):
        o = (C.c_int * 5)()
        _check(lib.hrt_mesh_info(self.s._h, self.i, o))
        return {"vertices": o[0], "faces": o[1], "nodes": o[2], "prims": o[3], "bvhDirty": bool(o[4])}

    @property
    def vertices(self):
        n = self.info()
        v = np.zeros((n["vertices"], 3), np.float32)
        _check(lib.hrt_mesh_read(self.s._h, self.i, v.ctypes.data_as(_fp), None, None, None))
        return v

    @vertices.setter
    def vertices(self, v):
        """A direct write of Mesh::vertices: bvhDirty stays as it is (the reference's quirk)."""
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        _check(lib.hrt_mesh_write_vertices(self.s._h, self.i, v.ctypes.data_as(_fp), v.shape[0]))

    def tree(self):
        """The mesh's current (host) tree: faces, nodes (BvhNode array) and primitive indices."""
        n = self.info()
        f = np.zeros((n["faces"], 3), np.int32)
        nodes = (BvhNode * max(n["nodes"], 1))()
        p = np.zeros(n["prims"], np.int32)
        _check(lib.hrt_mesh_read(self.s._h, self.i, None, f.ctypes.data_as(_ip), nodes, p.ctypes.data_as(_ip)))
        return f, list(nodes)[:n["nodes"]], p


from . import scenes  # noqa: E402,F401
