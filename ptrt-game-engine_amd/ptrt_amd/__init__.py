"""ptrt_amd -- Python (ctypes) binding of libptrt_amd.so.

Two layers, both plain C underneath:
  * the C ABI of include/ptrt.h (``lib.ptrt_*``): the drop-in boundary of the
    MI355X path-tracing back end;
  * ``Scene``: the reference's host API (``class Scene`` of
    src/pathtracer/scene/scene.cuh:78-2001) as implemented by the C++ mirror in
    host/ptrt/scene.hpp, reached through its flat ``hs_*`` entry points.

Nothing here computes pixels: if the shared library is missing the import fails,
and if there is no HIP device ``Scene(..., device>=0)`` raises.  A ``device=-1``
scene is host-only (build / flatten / inspect) and cannot render.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTRT_AMD_LIB") or os.path.join(_HERE, "libptrt_amd.so")  # env override: A/B builds
if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C ptrt-game-engine_amd` "
        "(or __graft_entry__.build()); there is no fallback implementation"
    )
lib = C.CDLL(LIB_PATH)


def library_info():
    """Path and SHA-256 (first 16 hex digits) of the shared library this process loaded -- PTRT_AMD_LIB can swap it, so a
    measurement names it."""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        return {"path": os.path.relpath(LIB_PATH, os.path.dirname(os.path.dirname(_HERE))), "sha16": hashlib.sha256(f.read()).hexdigest()[:16],
                "from_env": bool(os.environ.get("PTRT_AMD_LIB"))}


PTRT_OK = 0
BUF_ACCUM, BUF_NORMAL, BUF_DEPTH, BUF_OBJECT_ID, BUF_RGB8, BUF_RNG, BUF_DENOISED, BUF_MOTION, BUF_RENDER_ACCUM = range(9)
DEFAULT_SEED = 12345
HOST_ONLY = -1
QUERY_CLOSEST, QUERY_OCCLUDED = 0, 1  # ptrt_query_rays kinds


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class BvhNode(C.Structure):
    _fields_ = [("bmin", Vec3), ("bmax", Vec3), ("left", C.c_int32), ("right", C.c_int32),
                ("start", C.c_int32), ("count", C.c_int32)]


class Tri(C.Structure):
    _fields_ = [("v0", C.c_int32), ("v1", C.c_int32), ("v2", C.c_int32)]


class MeshDesc(C.Structure):
    _fields_ = [("verts", C.POINTER(Vec3)), ("vert_count", C.c_int32),
                ("faces", C.POINTER(Tri)), ("face_count", C.c_int32),
                ("nodes", C.POINTER(BvhNode)), ("node_count", C.c_int32),
                ("prim_indices", C.POINTER(C.c_int32)), ("prim_count", C.c_int32),
                ("world", C.c_float * 16), ("inverse", C.c_float * 16), ("normal", C.c_float * 16),
                ("has_transform", C.c_int32)]


class InstanceXform(C.Structure):
    _fields_ = [("world", C.c_float * 16), ("inverse", C.c_float * 16), ("normal", C.c_float * 16),
                ("has_transform", C.c_int32)]


class InstancePose(C.Structure):
    _fields_ = [("position", Vec3), ("rotation", Vec3), ("scale", Vec3)]


class Light(C.Structure):
    _fields_ = [("type", C.c_int32), ("position", Vec3), ("direction", Vec3), ("color", Vec3),
                ("intensity", C.c_float), ("range", C.c_float), ("inner_cone", C.c_float),
                ("outer_cone", C.c_float), ("radius", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("origin", Vec3), ("lower_left_corner", Vec3), ("horizontal", Vec3), ("vertical", Vec3),
                ("u", Vec3), ("v", Vec3), ("w", Vec3), ("lens_radius", C.c_float)]


_MAT_FIELDS = ["albedo", "specular", "metallic", "roughness", "emission", "ior", "transmission",
               "transmission_roughness", "clearcoat", "clearcoat_roughness", "subsurface_color",
               "subsurface_radius", "anisotropy", "sheen", "sheen_tint", "iridescence",
               "iridescence_thickness"]
_MAT_VEC = {"albedo", "specular", "emission", "subsurface_color", "sheen_tint"}


class Materials(C.Structure):
    _fields_ = [(n, C.POINTER(Vec3) if n in _MAT_VEC else C.POINTER(C.c_float)) for n in _MAT_FIELDS] + \
               [("count", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("meshes", C.POINTER(MeshDesc)), ("mesh_count", C.c_int32),
                ("tlas_nodes", C.POINTER(BvhNode)), ("tlas_node_count", C.c_int32),
                ("tlas_mesh_indices", C.POINTER(C.c_int32)), ("tlas_index_count", C.c_int32),
                ("materials", Materials),
                ("lights", C.POINTER(Light)), ("light_count", C.c_int32),
                ("camera", Camera), ("sky_top", Vec3), ("sky_bottom", Vec3), ("use_sky", C.c_int32),
                ("env_rgba", C.POINTER(C.c_float)), ("env_width", C.c_int32), ("env_height", C.c_int32)]


class Hit(C.Structure):
    _fields_ = [("hit", C.c_int32), ("t", C.c_float), ("point", Vec3), ("normal", Vec3),
                ("mesh_index", C.c_int32), ("front_face", C.c_int32), ("u", C.c_float), ("v", C.c_float),
                ("face_index", C.c_int32), ("local_point", Vec3)]


class Radiance(C.Structure):
    """`ptrt_radiance`: one ray's answer from ptrt_query_radiance."""
    _fields_ = [("radiance", C.c_float * 3), ("depth", C.c_float), ("normal", C.c_float * 3), ("object_id", C.c_int32)]


class Probe(C.Structure):
    """`ptrt_probe`: one light probe's answer from ptrt_query_probes."""
    _fields_ = [("sh", (C.c_float * 3) * 9), ("mean_distance", C.c_float), ("mean_distance_sq", C.c_float),
                ("hit_fraction", C.c_float), ("reserved", C.c_float * 2)]


class Irradiance(C.Structure):
    """`ptrt_irradiance`: one lightmap texel's answer from ptrt_query_irradiance."""
    _fields_ = [("radiance", C.c_float * 3), ("mean_distance", C.c_float), ("mean_distance_sq", C.c_float),
                ("hit_fraction", C.c_float), ("reserved", C.c_float * 2)]


class Direct(C.Structure):
    """`ptrt_direct`: one lightmap texel's answer from ptrt_query_direct."""
    _fields_ = [("irradiance", C.c_float * 3), ("lit_fraction", C.c_float), ("shadowed_fraction", C.c_float),
                ("reserved", C.c_float * 3)]


class Bounce(C.Structure):
    """`ptrt_bounce`: one lightmap texel's answer from ptrt_query_bounce."""
    _fields_ = [("radiance", C.c_float * 3), ("lit_fraction", C.c_float), ("shadowed_fraction", C.c_float),
                ("hit_fraction", C.c_float), ("reserved", C.c_float * 2)]


class AtlasTexel(C.Structure):
    """`ptrt_atlas_texel`: one texel of a lightmap atlas from ptrt_atlas_texels."""
    _fields_ = [("position", C.c_float * 3), ("face", C.c_int32), ("normal", C.c_float * 3), ("mesh", C.c_int32)]


class ProbeVolumeDesc(C.Structure):
    """`ptrt_probe_volume`: a regular grid of light probes for ptrt_probe_sample / ptrt_query_probe_light (host memory)."""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("counts", C.c_int32 * 3)]


class Stats(C.Structure):
    _fields_ = [("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64),
                ("shadow_rays_walked", C.c_uint64)]


class DenoiserSettings(C.Structure):
    """`ptrt_denoiser_settings` (DenoiserSettings of the non-split path, denoiser.cuh:36-73), filled with the reference's defaults
    by ptrt_denoiser_default_settings; keyword arguments override fields.  Pass to Scene.setDenoiserSettings."""
    _fields_ = [("tau", C.c_float), ("min_alpha", C.c_float), ("max_history", C.c_float), ("sigma_luminance", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("atrous_iterations", C.c_int32),
                ("clamp_scale", C.c_float), ("firefly_threshold", C.c_float), ("depth_reject_absolute", C.c_float),
                ("depth_reject_relative", C.c_float), ("normal_reject_threshold", C.c_float), ("sky_depth_threshold", C.c_float),
                ("edge_depth_threshold", C.c_float), ("edge_normal_threshold", C.c_float), ("use_object_ids", C.c_int32),
                ("enable_firefly_suppression", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib.ptrt_denoiser_default_settings(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise AttributeError(f"ptrt_denoiser_settings has no field {k!r}")
            setattr(self, k, v)


HIT_DTYPE = np.dtype([("hit", "<i4"), ("t", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3),
                      ("mesh_index", "<i4"), ("front_face", "<i4"), ("u", "<f4"), ("v", "<f4"),
                      ("face_index", "<i4"), ("local_point", "<f4", 3)])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) == 64 and C.sizeof(DenoiserSettings) == 68
RADIANCE_DTYPE = np.dtype([("radiance", "<f4", 3), ("depth", "<f4"), ("normal", "<f4", 3), ("object_id", "<i4")])
assert RADIANCE_DTYPE.itemsize == C.sizeof(Radiance) == 32
PROBE_DTYPE = np.dtype([("sh", "<f4", (9, 3)), ("mean_distance", "<f4"), ("mean_distance_sq", "<f4"), ("hit_fraction", "<f4"),
                        ("reserved", "<f4", 2)])
assert PROBE_DTYPE.itemsize == C.sizeof(Probe) == 128
IRRADIANCE_DTYPE = np.dtype([("radiance", "<f4", 3), ("mean_distance", "<f4"), ("mean_distance_sq", "<f4"), ("hit_fraction", "<f4"),
                             ("reserved", "<f4", 2)])
assert IRRADIANCE_DTYPE.itemsize == C.sizeof(Irradiance) == 32
DIRECT_DTYPE = np.dtype([("irradiance", "<f4", 3), ("lit_fraction", "<f4"), ("shadowed_fraction", "<f4"), ("reserved", "<f4", 3)])
assert DIRECT_DTYPE.itemsize == C.sizeof(Direct) == 32
BOUNCE_DTYPE = np.dtype([("radiance", "<f4", 3), ("lit_fraction", "<f4"), ("shadowed_fraction", "<f4"), ("hit_fraction", "<f4"),
                         ("reserved", "<f4", 2)])
assert BOUNCE_DTYPE.itemsize == C.sizeof(Bounce) == 32
ATLAS_TEXEL_DTYPE = np.dtype([("position", "<f4", 3), ("face", "<i4"), ("normal", "<f4", 3), ("mesh", "<i4")])
assert ATLAS_TEXEL_DTYPE.itemsize == C.sizeof(AtlasTexel) == 32
LIGHTMAP_SAMPLE_DTYPE = np.dtype([("rgb", "<f4", 3), ("weight", "<f4"), ("x", "<f4"), ("y", "<f4"), ("face", "<i4"), ("mesh", "<i4")])
assert LIGHTMAP_SAMPLE_DTYPE.itemsize == 32
LIGHTMAP_NEAREST, LIGHTMAP_BILINEAR = 0, 1  # PTRT_LIGHTMAP_*
LIGHTMAP_MODES = dict(nearest=LIGHTMAP_NEAREST, bilinear=LIGHTMAP_BILINEAR)
PROBE_LIGHT_DTYPE = np.dtype([("irradiance", "<f4", 3), ("weight", "<f4"), ("cell", "<i4"), ("used", "<i4"), ("face", "<i4"), ("mesh", "<i4")])
assert PROBE_LIGHT_DTYPE.itemsize == 32 and C.sizeof(ProbeVolumeDesc) == 36
PROBES_TRILINEAR, PROBES_VISIBILITY = 0, 1  # PTRT_PROBES_*
PROBES_MODES = dict(trilinear=PROBES_TRILINEAR, visibility=PROBES_VISIBILITY)
TLAS_NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("start", "<i4"),
                            ("count", "<i4")])
assert TLAS_NODE_DTYPE.itemsize == C.sizeof(BvhNode) == 40
INSTANCE_XFORM_DTYPE = np.dtype([("world", "<f4", 16), ("inverse", "<f4", 16), ("normal", "<f4", 16), ("has_transform", "<i4")])
assert INSTANCE_XFORM_DTYPE.itemsize == C.sizeof(InstanceXform) == 196 and C.sizeof(InstancePose) == 36

_vp = C.c_void_p
_fp = C.POINTER(C.c_float)


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


# ---- include/ptrt.h ------------------------------------------------------------------
_sig("ptrt_abi_version", C.c_int)
_sig("ptrt_last_error", C.c_char_p, _vp)
_sig("ptrt_create", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp))
_sig("ptrt_destroy", None, _vp)
_sig("ptrt_set_blue_noise", C.c_int, _vp, _fp)
_sig("ptrt_reset_rng", C.c_int, _vp, C.c_ulonglong)
_sig("ptrt_upload_geometry", C.c_int, _vp, C.POINTER(MeshDesc), C.c_int, C.POINTER(BvhNode), C.c_int,
     C.POINTER(C.c_int32), C.c_int)
_sig("ptrt_upload_materials", C.c_int, _vp, C.POINTER(Materials))
_sig("ptrt_upload_lights", C.c_int, _vp, C.POINTER(Light), C.c_int)
_sig("ptrt_set_camera", C.c_int, _vp, C.POINTER(Camera))
_sig("ptrt_set_sky", C.c_int, _vp, C.POINTER(Vec3), C.POINTER(Vec3), C.c_int)
_sig("ptrt_upload_scene", C.c_int, _vp, C.POINTER(SceneDesc))
_sig("ptrt_render", C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int)
_sig("ptrt_sync", C.c_int, _vp)
_sig("ptrt_read_buffer", C.c_int, _vp, C.c_int, _vp, C.c_size_t)
_sig("ptrt_device_buffer", _vp, _vp, C.c_int)
_sig("ptrt_write_rng", C.c_int, _vp, C.POINTER(C.c_uint32), C.c_size_t)
_sig("ptrt_trace_rays", C.c_int, _vp, _fp, _fp, C.c_int, _vp)
_sig("ptrt_render_wireframe", C.c_int, _vp, C.c_float, _vp, C.c_int)
_sig("ptrt_query_rays", C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp)
_sig("ptrt_query_radiance", C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("ptrt_query_probes", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_float, _vp)
_sig("ptrt_irradiance_rays", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, _vp, _vp)
_sig("ptrt_query_irradiance", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, _vp, C.c_int, C.c_int, C.c_float, _vp)
_sig("ptrt_direct_rays", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp)
_sig("ptrt_query_direct", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, C.c_int, C.c_int, _vp)
_sig("ptrt_bounce_terms", C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp)
_sig("ptrt_query_bounce", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("ptrt_atlas_texels", C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("ptrt_atlas_dilate", C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int)
_sig("ptrt_atlas_filter", C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int)
_sig("ptrt_atlas_sample", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("ptrt_query_lightmap", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("ptrt_probe_sample", C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_float, _vp)
_sig("ptrt_query_probe_light", C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_float, _vp)
_sig("ptrt_camera_rays", C.c_int, _vp, C.c_int, C.c_int, _vp, _vp)
_sig("ptrt_init_rng_states", C.c_int, _vp, C.c_ulonglong, C.c_ulonglong, C.c_int, _vp)
_sig("ptrt_get_stats", C.c_int, _vp, C.POINTER(Stats))
_sig("ptrt_set_option", C.c_int, _vp, C.c_char_p, C.c_longlong)
_sig("ptrt_get_option", C.c_int, _vp, C.c_char_p, C.POINTER(C.c_longlong))
_sig("ptrt_last_kernel_ms", C.c_int, _vp, _fp, _fp)
_sig("ptrt_set_stream", C.c_int, _vp, _vp)
_sig("ptrt_kernel_ms_history", C.c_int, _vp, _fp, C.c_int)
_sig("ptrt_launch_ms_history", C.c_int, _vp, _fp, _fp, C.c_int)
_sig("ptrt_debug_detmath", C.c_int, _vp, C.c_int, _fp, _fp, C.c_int, _fp)
_sig("ptrt_debug_upload_counts", C.c_int, _vp, C.POINTER(C.c_int))

# ---- Scene mirror (csrc/ptrt_host_capi.cpp) ---------------------------------------------
_sig("hs_last_error", C.c_char_p)
_sig("hs_material_default", None, _fp)
_sig("hs_material_make", None, _fp, C.c_float, C.c_float, _fp)
_sig("hs_scene_create", _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("hs_scene_create_interleaved", _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("hs_tile_rows", C.c_int, _vp)
_sig("hs_farm_create", _vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int)
_sig("hs_farm_scene", _vp, _vp, C.c_int)
_sig("hs_farm_size", C.c_int, _vp)
_sig("hs_farm_transport", C.c_char_p, _vp)
_sig("hs_farm_render", C.c_int, _vp, _vp, C.c_int)
_sig("hs_farm_sync", C.c_int, _vp)
_sig("hs_farm_host_us", C.c_double, _vp)
_sig("hs_farm_set_parallel", C.c_int, _vp, C.c_int)
_sig("hs_farm_destroy", None, _vp)
_sig("ptrt_create_interleaved", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp))
_sig("ptrt_farm_create", C.c_int, C.POINTER(_vp), C.c_int, C.POINTER(_vp))
_sig("ptrt_farm_bands", C.c_int, _vp)
_sig("ptrt_farm_transport", C.c_char_p, _vp)
_sig("ptrt_farm_part_is_local", C.c_int, _vp, C.c_int)
_sig("ptrt_farm_render", C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int)
_sig("ptrt_farm_gather", C.c_int, _vp, _vp, C.c_int)
_sig("ptrt_farm_sync", C.c_int, _vp)
_sig("ptrt_farm_device_frame", _vp, _vp, _vp, C.c_int)
_sig("ptrt_farm_host_us", C.c_double, _vp)
_sig("ptrt_farm_set_option", C.c_int, _vp, C.c_char_p, C.c_longlong)
_sig("ptrt_farm_destroy", None, _vp)
_sig("hs_scene_destroy", None, _vp)
_sig("hs_backend", _vp, _vp)
_sig("hs_init_blue_noise", C.c_int, _vp)
_sig("hs_blue_noise_table", None, _fp)
_sig("hs_blue_noise_generate", None, C.c_int, C.c_int, _fp)
_sig("hs_add_cube", C.c_int, _vp, _fp)
_sig("hs_add_sphere", C.c_int, _vp, C.c_int, _fp)
_sig("hs_add_plane_xz", C.c_int, _vp, C.c_float, C.c_float, _fp)
_sig("hs_add_triangles", C.c_int, _vp, _fp, C.c_int, _fp)
_sig("hs_add_mesh_obj", C.c_int, _vp, C.c_char_p, _fp)
_sig("hs_add_checkerboard", C.c_int, _vp, C.c_float, C.c_int, C.c_float, _fp, _fp)
_sig("hs_mesh_op", C.c_int, _vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float)
_sig("hs_mesh_set_vertices", C.c_int, _vp, C.c_int, _fp, C.c_int)
_sig("hs_mesh_refit_bvh", C.c_int, _vp, C.c_int)
_sig("hs_mesh_set_triangle_soup", C.c_int, _vp, C.c_int, _fp, C.c_int)
_sig("hs_set_dynamic_geometry_policy", C.c_int, _vp, C.c_int)
_sig("hs_commit_counts", C.c_int, _vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong))
_sig("hs_commit_host_us", C.c_int, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("hs_mesh_counts", C.c_int, _vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("hs_add_point_light", None, _vp, _fp, _fp, C.c_float, C.c_float, C.c_float)
_sig("hs_add_directional_light", None, _vp, _fp, _fp, C.c_float)
_sig("hs_add_spot_light", None, _vp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float)
_sig("hs_move_light_to", None, _vp, C.c_int, _fp)
_sig("hs_set_camera", None, _vp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float)
_sig("hs_move_camera", None, _vp, _fp)
_sig("hs_look_camera_at", None, _vp, _fp)
_sig("hs_set_sky_gradient", None, _vp, _fp, _fp)
_sig("hs_disable_sky", None, _vp)
_sig("hs_load_hdri", C.c_int, _vp, C.c_char_p)
_sig("hs_set_environment_map", C.c_int, _vp, _fp, C.c_int, C.c_int)
_sig("hs_free_hdri", None, _vp)
_sig("ptrt_set_env_map", C.c_int, _vp, _fp, C.c_int, C.c_int)
_sig("hs_set_bvh_leaf_target", None, _vp, C.c_int, C.c_int)
_sig("hs_set_max_bounce_depth", None, _vp, C.c_int)
_sig("hs_set_samples_per_pixel", None, _vp, C.c_int)
_sig("hs_set_perf_samples_per_pixel", None, _vp, C.c_int)
_sig("hs_set_max_depth", None, _vp, C.c_int)
_sig("hs_get_samples_per_pixel", C.c_int, _vp)
_sig("hs_serialize_scene", C.c_size_t, _vp, _vp, C.c_size_t)
_sig("hs_set_denoiser_enabled", C.c_int, _vp, C.c_int)
_sig("hs_set_bloom_enabled", None, _vp, C.c_int)
_sig("hs_set_performance_preset", C.c_int, _vp, C.c_char_p)
_sig("hs_set_resolution_scale", C.c_int, _vp, C.c_float)
_sig("hs_get_render_size", None, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("ptrt_set_bloom", C.c_int, _vp, C.c_int)
_sig("ptrt_set_render_size", C.c_int, _vp, C.c_int, C.c_int)
_sig("hs_get_settings", None, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
     C.POINTER(C.c_int), _fp)
_sig("hs_set_mesh_material", C.c_int, _vp, C.c_int, _fp)
_sig("hs_upload", C.c_int, _vp)
_sig("hs_commit_object_changes", C.c_int, _vp)
_sig("hs_get_view_proj", None, _vp, C.c_int, _fp)
_sig("ptrt_denoiser_default_settings", None, _vp)
_sig("ptrt_denoiser_enable", C.c_int, _vp, _vp)
_sig("ptrt_denoiser_disable", C.c_int, _vp)
_sig("ptrt_set_prev_view_proj", C.c_int, _vp, _fp)
_sig("ptrt_post_frame", C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int)
_sig("hs_refit_object_changes", C.c_int, _vp)
_sig("hs_refit_from_device", C.c_int, _vp, C.c_int, _vp)
_sig("hs_refit_from_host", C.c_int, _vp, C.c_int, _vp)
_sig("ptrt_update_vertices", C.c_int, _vp, C.c_int, _fp, C.c_int, C.c_int)
_sig("ptrt_refit", C.c_int, _vp)
_sig("ptrt_build_bvh", C.c_int, _vp, C.c_int)
_sig("ptrt_read_prim_order", C.c_int, _vp, C.c_int, C.POINTER(C.c_int), C.c_int)
_sig("ptrt_read_bvh", C.c_int, _vp, C.c_int, C.POINTER(BvhNode), C.c_int)
_sig("ptrt_update_triangles", C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int)
_sig("ptrt_set_instance_transforms", C.c_int, _vp, C.c_int, C.c_int, C.POINTER(InstanceXform))
_sig("ptrt_set_instance_transforms_device", C.c_int, _vp, C.c_int, C.c_int, _vp)
_sig("ptrt_refit_tlas", C.c_int, _vp)
_sig("ptrt_read_tlas", C.c_int, _vp, C.POINTER(BvhNode), C.c_int)
_sig("hs_refit_instance_changes", C.c_int, _vp, C.c_int)
_sig("ptrt_reorder_tlas", C.c_int, _vp)
_sig("ptrt_read_tlas_order", C.c_int, _vp, C.POINTER(C.c_int32), C.c_int)
_sig("ptrt_set_instance_poses_device", C.c_int, _vp, C.c_int, C.c_int, _vp)
_sig("ptrt_read_instance_transforms", C.c_int, _vp, C.c_int, C.c_int, _vp)
_sig("hs_reseat_tlas", C.c_int, _vp)
_sig("hs_reorder_tlas", C.c_int, _vp, C.c_int)
_sig("hs_rebuild_object_changes", C.c_int, _vp, C.c_int)
_sig("hs_rebuild_from_device", C.c_int, _vp, C.c_int, _vp)
_sig("hs_update_triangles", C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int)
_sig("hs_mesh_prim_indices", C.c_int, _vp, C.c_int, C.POINTER(C.c_int), C.c_int)
_sig("hs_render_to_device", C.c_int, _vp, _vp)
_sig("hs_render_to_host", C.c_int, _vp, _vp)
_sig("hs_render_wireframe_to_device", C.c_int, _vp, _vp, C.c_float)
_sig("hs_render_wireframe_to_host", C.c_int, _vp, _vp, C.c_float)
_sig("hs_query_closest", C.c_int, _vp, _vp, _vp, C.c_int, _vp)
_sig("hs_query_occluded", C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp)
_sig("hs_query_radiance", C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("hs_query_probes", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_float, _vp)
_sig("hs_query_irradiance", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, _vp, C.c_int, C.c_int, C.c_float, _vp)
_sig("hs_irradiance_rays", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, _vp, _vp)
_sig("hs_light_count", C.c_int, _vp)
_sig("hs_query_direct", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, C.c_int, C.c_int, _vp)
_sig("hs_direct_rays", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp)
_sig("hs_query_bounce", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_float, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("hs_bounce_terms", C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp)
_sig("hs_atlas_texels", C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("hs_atlas_dilate", C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int)
_sig("hs_atlas_filter", C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int)
_sig("hs_atlas_sample", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("hs_query_lightmap", C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("hs_probe_sample", C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_float, _vp)
_sig("hs_query_probe_light", C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_float, _vp)
_sig("hs_camera_rays", C.c_int, _vp, C.c_int, C.c_int, _vp, _vp)
_sig("hs_render_baked", C.c_int, _vp, C.c_int, _vp, _vp, C.c_int)
_sig("ptrt_render_baked", C.c_int, _vp, C.c_int, _vp, _vp, C.c_int)
_sig("hs_init_rng_states", C.c_int, _vp, C.c_ulonglong, C.c_ulonglong, C.c_int, _vp)
_sig("hs_post_frame", C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int)
_sig("hs_get_frame_count", C.c_int, _vp)
_sig("hs_set_frame_count", None, _vp, C.c_int)
_sig("hs_trace_single_ray", C.c_int, _vp, _fp, _fp, C.POINTER(Hit))
_sig("hs_save_ppm", C.c_int, _vp, C.c_char_p, _vp)
_sig("hs_view_run", C.c_int, _vp, C.c_int, C.c_int, _vp, C.POINTER(C.c_double), C.c_char_p, C.c_int)
_sig("ptrt_present_create", C.c_int, _vp, C.c_int)
_sig("ptrt_present_map", C.c_int, _vp, C.c_int, C.POINTER(_vp))
_sig("ptrt_present_unmap", C.c_int, _vp, C.c_int)
_sig("ptrt_present_acquire", C.c_int, _vp, C.c_int, C.POINTER(_vp))
_sig("ptrt_present_destroy", C.c_int, _vp)
_sig("ptrt_ring_create", C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(_vp))
_sig("ptrt_ring_map", C.c_int, _vp, C.c_int, C.POINTER(_vp))
_sig("ptrt_ring_unmap", C.c_int, _vp, C.c_int)
_sig("ptrt_ring_acquire", C.c_int, _vp, C.c_int, C.POINTER(_vp))
_sig("ptrt_ring_destroy", None, _vp)
_sig("hs_flatten", C.POINTER(SceneDesc), _vp)


class PtrtError(RuntimeError):
    pass


def _f3(v):
    return (C.c_float * 3)(*[float(a) for a in v])


def _fptr(a):
    return a.ctypes.data_as(_fp)


class Material:
    """`struct Material` (scene/material_lib.cuh:12-105) as 27 floats."""
    NAMES = {"albedo": (0, 3), "specular": (3, 3), "metallic": (6, 1), "roughness": (7, 1), "emission": (8, 3),
             "ior": (11, 1), "transmission": (12, 1), "transmissionRoughness": (13, 1), "clearcoat": (14, 1),
             "clearcoatRoughness": (15, 1), "subsurfaceColor": (16, 3), "subsurfaceRadius": (19, 1),
             "anisotropy": (20, 1), "sheen": (21, 1), "sheenTint": (22, 3), "iridescence": (25, 1),
             "iridescenceThickness": (26, 1)}

    def __init__(self, albedo=None, roughness=0.5, metallic=0.0, **fields):
        self.f = np.zeros(27, dtype=np.float32)
        if albedo is None:
            lib.hs_material_default(_fptr(self.f))
        else:
            lib.hs_material_make(_f3(albedo), float(roughness), float(metallic), _fptr(self.f))
        for k, v in fields.items():
            self.set(k, v)

    def set(self, name, value):
        off, n = self.NAMES[name]
        self.f[off:off + n] = np.asarray(value, dtype=np.float32).reshape(-1) if n == 3 else np.float32(value)
        return self

    def get(self, name):
        off, n = self.NAMES[name]
        return self.f[off:off + n].copy() if n == 3 else float(self.f[off])

    def ptr(self):
        return _fptr(self.f)


def blue_noise_table():
    """The 64x64x2 table `initBlueNoise()` uploads (common/bluenoise.cuh:79-198), libstdc++ build."""
    t = np.zeros(64 * 64 * 2, dtype=np.float32)
    lib.hs_blue_noise_table(_fptr(t))
    return t


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def _named_columns(records, columns, reinterpret=None):
    """{name: view of its columns} for the (n, cols) rows of a query, a tensor or an array, by a `*_COLUMNS` table (name ->
    (first, last + 1, ..)): one column as (n,), several as (n, k).  `reinterpret`: (the other 4-byte type's name, the names of
    the columns that hold its bits), viewed as it."""
    as_type, names = reinterpret or (None, ())
    if names and _is_tensor(records):
        import torch
        as_type = getattr(torch, as_type)
    out = {}
    for name, (a, b, *_) in columns.items():
        col = records[:, a:b]
        if name in names:
            col = col.view(as_type)
        out[name] = col[:, 0] if b - a == 1 else col
    return out


def _flagged(columns, flag):
    """the names of a (first, last + 1, is float) table whose third entry is `flag`"""
    return {name for name, c in columns.items() if c[2] is flag}


# columns of the (n, 16) int32 rows of Scene.query_closest on torch tensors: the fields of ptrt_hit / HIT_DTYPE
HIT_COLUMNS = dict(hit=(0, 1, False), t=(1, 2, True), point=(2, 5, True), normal=(5, 8, True), mesh_index=(8, 9, False),
                   front_face=(9, 10, False), u=(10, 11, True), v=(11, 12, True), face_index=(12, 13, False),
                   local_point=(13, 16, True))


def hit_fields(hits):
    """Named views of query_closest's (n, 16) int32 tensor: float fields reinterpreted as float32, scalars as (n,)."""
    return _named_columns(hits, HIT_COLUMNS, ("float32", _flagged(HIT_COLUMNS, True)))


# columns of the (n, 8) float32 rows of Scene.query_radiance: the fields of ptrt_radiance / RADIANCE_DTYPE
RADIANCE_COLUMNS = dict(radiance=(0, 3, True), depth=(3, 4, True), normal=(4, 7, True), object_id=(7, 8, False))


def radiance_fields(records):
    """Named views of query_radiance's (n, 8) float32 tensor: object_id reinterpreted as int32, scalars as (n,)."""
    return _named_columns(records, RADIANCE_COLUMNS, ("int32", _flagged(RADIANCE_COLUMNS, False)))


# columns of the (n, 32) float32 rows of Scene.query_probes: the fields of ptrt_probe / PROBE_DTYPE
PROBE_COLUMNS = dict(sh=(0, 27), mean_distance=(27, 28), mean_distance_sq=(28, 29), hit_fraction=(29, 30), reserved=(30, 32))


def probe_fields(probes):
    """Named views of query_probes's (n, 32) float32 tensor: sh as (n, 9, 3) -- coefficient, colour channel --, scalars as (n,)."""
    out = _named_columns(probes, PROBE_COLUMNS)
    out["sh"] = out["sh"].reshape(-1, 9, 3)
    return out


# columns of the (n, 8) float32 rows of Scene.query_irradiance: the fields of ptrt_irradiance / IRRADIANCE_DTYPE
IRRADIANCE_COLUMNS = dict(radiance=(0, 3), mean_distance=(3, 4), mean_distance_sq=(4, 5), hit_fraction=(5, 6), reserved=(6, 8))


def irradiance_fields(records):
    """Named views of query_irradiance's (n, 8) float32 rows (a tensor or an array): radiance as (n, 3), scalars as (n,)."""
    return _named_columns(records, IRRADIANCE_COLUMNS)


# columns of the (n, 8) float32 rows of Scene.query_direct: the fields of ptrt_direct / DIRECT_DTYPE
DIRECT_COLUMNS = dict(irradiance=(0, 3), lit_fraction=(3, 4), shadowed_fraction=(4, 5), reserved=(5, 8))


def direct_fields(records):
    """Named views of query_direct's (n, 8) float32 rows (a tensor or an array): irradiance as (n, 3), scalars as (n,)."""
    return _named_columns(records, DIRECT_COLUMNS)


# columns of the (n, 8) float32 rows of Scene.query_bounce: the fields of ptrt_bounce / BOUNCE_DTYPE
BOUNCE_COLUMNS = dict(radiance=(0, 3), lit_fraction=(3, 4), shadowed_fraction=(4, 5), hit_fraction=(5, 6), reserved=(6, 8))


def bounce_fields(records):
    """Named views of query_bounce's (n, 8) float32 rows (a tensor or an array): radiance as (n, 3), scalars as (n,)."""
    return _named_columns(records, BOUNCE_COLUMNS)


# columns of the (n, 8) int32 rows of Scene.atlas_texels: the fields of ptrt_atlas_texel / ATLAS_TEXEL_DTYPE
ATLAS_COLUMNS = dict(position=(0, 3), face=(3, 4), normal=(4, 7), mesh=(7, 8))


def atlas_fields(records):
    """Named views of atlas_texels' (n, 8) int32 rows (a tensor or an array): position and normal reinterpreted as float32,
    (n, 3); face and mesh int32, (n,)."""
    return _named_columns(records, ATLAS_COLUMNS, ("float32", ("position", "normal")))


# columns of the (n, 8) int32 rows of Scene.atlas_sample / query_lightmap: the fields of ptrt_lightmap_sample / LIGHTMAP_SAMPLE_DTYPE
LIGHTMAP_SAMPLE_COLUMNS = dict(rgb=(0, 3, True), weight=(3, 4, True), x=(4, 5, True), y=(5, 6, True), face=(6, 7, False),
                               mesh=(7, 8, False))


def lightmap_sample_fields(records):
    """Named views of atlas_sample's and query_lightmap's (n, 8) int32 rows (a tensor or an array): rgb (n, 3), weight, x and y
    (n,) reinterpreted as float32; face and mesh int32, (n,)."""
    return _named_columns(records, LIGHTMAP_SAMPLE_COLUMNS, ("float32", _flagged(LIGHTMAP_SAMPLE_COLUMNS, True)))


class Scene:
    """The reference's `Scene` host API; see host/ptrt/scene.hpp for per-method citations."""

    def __init__(self, width, height, tile_y0=0, tile_rows=0, device=0, interleave=None):
        """`interleave=(phase, period)`: the scene renders every period-th 8-row strip of the frame from strip `phase`
        (ptrt_create_interleaved) instead of the contiguous rows [tile_y0, tile_y0 + tile_rows)."""
        self.width, self.height = int(width), int(height)
        self.device = device
        self.interleave = interleave
        if interleave is not None:
            phase, period = interleave
            self._h = lib.hs_scene_create_interleaved(self.width, self.height, int(phase), int(period), device)
            if not self._h:
                raise PtrtError(lib.hs_last_error().decode())
            self.tile_y0, self.tile_rows = int(phase) * 8, lib.hs_tile_rows(self._h)
            return
        self.tile_y0 = int(tile_y0)
        self.tile_rows = int(tile_rows) if tile_rows > 0 else self.height
        self._h = lib.hs_scene_create(self.width, self.height, tile_y0, tile_rows, device)
        if not self._h:
            raise PtrtError(lib.hs_last_error().decode())

    @classmethod
    def _borrowed(cls, handle, width, height, device):
        """A Scene owned by someone else (a C++ TileFarm's part): same methods, never destroyed from here."""
        s = cls.__new__(cls)
        s._h, s._owned = handle, False
        s.width, s.height, s.device, s.interleave = int(width), int(height), device, None
        s.tile_y0, s.tile_rows = 0, lib.hs_tile_rows(handle)
        return s

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                lib.hs_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise PtrtError(lib.hs_last_error().decode())
        return rc

    @property
    def ctx(self):
        return lib.hs_backend(self._h)

    def _cchk(self, rc):
        if rc != PTRT_OK:
            raise PtrtError(lib.ptrt_last_error(self.ctx).decode())

    # geometry
    def addCube(self, mat): return self._chk(lib.hs_add_cube(self._h, mat.ptr()))
    def addSphere(self, segments, mat): return self._chk(lib.hs_add_sphere(self._h, segments, mat.ptr()))
    def addPlaneXZ(self, y, half, mat): return self._chk(lib.hs_add_plane_xz(self._h, y, half, mat.ptr()))

    def addTriangles(self, tris, mat):
        a = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        return self._chk(lib.hs_add_triangles(self._h, _fptr(a), a.shape[0], mat.ptr()))

    def addMesh(self, path, mat): return self._chk(lib.hs_add_mesh_obj(self._h, path.encode(), mat.ptr()))

    def addCheckerboardPlaneXZ(self, y, tiles, tile_size, white, black):
        self._chk(lib.hs_add_checkerboard(self._h, y, tiles, tile_size, white.ptr(), black.ptr()))

    def _op(self, mesh, op, v): self._chk(lib.hs_mesh_op(self._h, mesh, op, float(v[0]), float(v[1]), float(v[2])))
    def scale(self, mesh, s): self._op(mesh, 0, (s, s, s) if np.isscalar(s) else s)
    def translate(self, mesh, d): self._op(mesh, 1, d)
    def moveTo(self, mesh, p): self._op(mesh, 2, p)
    def rotateSelfEulerXYZ(self, mesh, r): self._op(mesh, 3, r)
    def setPosition(self, mesh, p): self._op(mesh, 4, p)
    def setRotation(self, mesh, r): self._op(mesh, 5, r)
    def setInstanceScale(self, mesh, s): self._op(mesh, 6, s)

    def setVertices(self, mesh, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._chk(lib.hs_mesh_set_vertices(self._h, mesh, _fptr(a), a.shape[0]))

    def refitMeshOnHost(self, mesh):
        """Mesh::refitBVH alone: the host copy of the mesh keeps its tree and leaf assignment and takes its boxes from the
        current vertices (after setVertices).  No back end needed; the TLAS is not touched."""
        self._chk(lib.hs_mesh_refit_bvh(self._h, int(mesh)))

    def setTriangleSoup(self, mesh, tris):
        """What the reference's updatePTScene does to a `Triangles` mesh (PTRTtransfer.cuh:2249-2270): vertices and faces
        rewritten, bvhDirty / vertsDirty set, local box recomputed; the caller then commits (commitObjectChanges)."""
        a = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        self._chk(lib.hs_mesh_set_triangle_soup(self._h, mesh, _fptr(a), a.shape[0]))

    POLICIES = {"HostRebuild": 0, "GpuRefit": 1, "GpuRebuild": 2, "GpuRefitAll": 3}

    def setDynamicGeometryPolicy(self, policy):
        self._chk(lib.hs_set_dynamic_geometry_policy(self._h, self.POLICIES.get(policy, policy)))

    def commitCounts(self):
        """(commits that took the GPU refit / rebuild path, geometry uploads) so far."""
        a, b = C.c_longlong(), C.c_longlong()
        lib.hs_commit_counts(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def commitHostMicros(self):
        """(caller, mirror, compare): accumulated host microseconds of setTriangleSoup (what updatePTScene does to a `Triangles`
        mesh), of the commits themselves (updateAccelerationStructures) and, within those, of the face-list comparison."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        lib.hs_commit_host_us(self._h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def meshCounts(self, mesh):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(lib.hs_mesh_counts(self._h, mesh, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # lights / camera / sky
    def addPointLight(self, pos, col, intensity=1.0, range=100.0, radius=0.0):
        lib.hs_add_point_light(self._h, _f3(pos), _f3(col), intensity, range, radius)

    def addDirectionalLight(self, direction, col, intensity=1.0):
        lib.hs_add_directional_light(self._h, _f3(direction), _f3(col), intensity)

    def addSpotLight(self, pos, direction, col, intensity=1.0, inner=0.5, outer=0.7, range=100.0, radius=0.0):
        lib.hs_add_spot_light(self._h, _f3(pos), _f3(direction), _f3(col), intensity, inner, outer, range, radius)

    def moveLightTo(self, i, pos): lib.hs_move_light_to(self._h, i, _f3(pos))

    def setCamera(self, lookfrom, lookat, vup, vfov, aperture=0.0, focus_dist=1.0):
        lib.hs_set_camera(self._h, _f3(lookfrom), _f3(lookat), _f3(vup), vfov, aperture, focus_dist)

    def moveCamera(self, pos): lib.hs_move_camera(self._h, _f3(pos))
    def lookCameraAt(self, at): lib.hs_look_camera_at(self._h, _f3(at))
    def setSkyGradient(self, top, bottom): lib.hs_set_sky_gradient(self._h, _f3(top), _f3(bottom))
    def disableSky(self): lib.hs_disable_sky(self._h)
    def loadHDRI(self, path): self._chk(lib.hs_load_hdri(self._h, str(path).encode()))
    def freeHDRI(self): lib.hs_free_hdri(self._h)

    def setEnvironmentMap(self, rgba):
        """(h, w, 4) float32 equirectangular map, row 0 = v 0 (what loadHDRI would hand over)."""
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        assert a.ndim == 3 and a.shape[2] == 4
        self._chk(lib.hs_set_environment_map(self._h, _fptr(a), a.shape[1], a.shape[0]))

    # settings
    def setBVHLeafTarget(self, target, tol=5): lib.hs_set_bvh_leaf_target(self._h, target, tol)
    def setMaxBounceDepth(self, d): lib.hs_set_max_bounce_depth(self._h, d)
    # Scene::setSamplesPerPixel / setMaxDepth (scene.cuh:1248-1255): stored and IGNORED by render_to_device, as in
    # the reference; the sample count a frame uses is perfSettings.samplesPerPixel -> setPerfSamplesPerPixel
    def setSamplesPerPixel(self, n): lib.hs_set_samples_per_pixel(self._h, n)
    def setMaxDepth(self, d): lib.hs_set_max_depth(self._h, d)
    def getSamplesPerPixel(self): return lib.hs_get_samples_per_pixel(self._h)
    def setPerfSamplesPerPixel(self, n): lib.hs_set_perf_samples_per_pixel(self._h, n)
    def setDenoiserEnabled(self, e): self._chk(lib.hs_set_denoiser_enabled(self._h, int(e)))
    def setDenoiserSettings(self, settings):
        """`ptrt_denoiser_enable(ctx, &settings)` on the live context: a new Denoiser with these settings (a `DenoiserSettings`)
        at the current render size; the history starts over.  Whether frames use it stays with setDenoiserEnabled.  Full-frame
        scenes only; a later setResolutionScale re-creates the denoiser with the defaults, as the reference does."""
        if not isinstance(settings, DenoiserSettings):
            raise TypeError("setDenoiserSettings takes a ptrt_amd.DenoiserSettings")
        self._cchk(lib.ptrt_denoiser_enable(self.ctx, C.byref(settings)))

    def setBloomEnabled(self, e): lib.hs_set_bloom_enabled(self._h, int(e))
    def setPerformancePreset(self, name): self._chk(lib.hs_set_performance_preset(self._h, name.encode()))
    def setResolutionScale(self, s): self._chk(lib.hs_set_resolution_scale(self._h, float(s)))

    def renderSize(self):
        """(render_width, render_height): the size the path tracer runs at (perfSettings.resolutionScale)."""
        w, h = C.c_int(), C.c_int()
        lib.hs_get_render_size(self._h, C.byref(w), C.byref(h))
        return w.value, h.value
    def setMeshMaterial(self, mesh, mat): self._chk(lib.hs_set_mesh_material(self._h, mesh, mat.ptr()))

    def settings(self):
        spp, depth, dn, bl, sc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_float()
        lib.hs_get_settings(self._h, C.byref(spp), C.byref(depth), C.byref(dn), C.byref(bl), C.byref(sc))
        return dict(spp=spp.value, depth=depth.value, denoiser=bool(dn.value), bloom=bool(bl.value), scale=sc.value)

    # upload / render
    def initBlueNoise(self): self._chk(lib.hs_init_blue_noise(self._h))
    def uploadToGPU(self): self._chk(lib.hs_upload(self._h))
    def commitObjectChanges(self): self._chk(lib.hs_commit_object_changes(self._h))

    def view_proj(self, current=False):
        """proj*view (16 floats, column-major as mat4 stores them): previous frame's by default."""
        m = np.zeros(16, dtype=np.float32)
        lib.hs_get_view_proj(self._h, 1 if current else 0, _fptr(m))
        return m

    def refitObjectChanges(self):
        """Dynamic vertices, same topology: host + GPU BVH refit instead of the reference's rebuild."""
        self._chk(lib.hs_refit_object_changes(self._h))

    def refitInstanceChanges(self, host_only=False):
        """Moved instances behind the TLAS topology that was uploaded: new matrices (ptrt_set_instance_transforms) and a TLAS
        refit on the device (ptrt_refit_tlas), no host synchronisation; the host TLAS is refitted the same way.
        `host_only`: the host half alone, for a device=-1 scene."""
        self._chk(lib.hs_refit_instance_changes(self._h, int(bool(host_only))))

    def reseatTLAS(self):
        """A fresh TLAS topology: rebuilt on the host over the meshes' current boxes and uploaded (ptrt_update_instances)."""
        self._chk(lib.hs_reseat_tlas(self._h))

    def reorderTLAS(self, host_only=False):
        """refitInstanceChanges with a fresh order: moved instances' matrices go over, the meshes are re-dealt to the TLAS indices
        in Morton order of their world boxes' centres on the device and the TLAS is refitted there (ptrt_reorder_tlas): no
        upload, no host synchronisation; the host TLAS follows through the same arithmetic.
        `host_only`: the host half alone, for a device=-1 scene."""
        self._chk(lib.hs_reorder_tlas(self._h, int(bool(host_only))))

    def set_instance_transforms_device(self, first, tensor):
        """`ptrt_set_instance_transforms_device`: meshes first .. first + count - 1 take their has_transform bit and matrices from
        `tensor`, a contiguous torch tensor on this scene's device whose rows are `ptrt_instance_xform` records (196 bytes:
        world[16], inverse[16], normal[16] as float32 and has_transform as int32 -- shape (count, 49) of a 4-byte dtype or
        (count, 196) of uint8), read in place by one launch on the context's stream: no copy, no synchronisation.  The
        context's stream is ordered behind torch's current stream.  Follow with reorderTLAS / ptrt_reorder_tlas / ptrt_refit_tlas."""
        if not _is_tensor(tensor):
            raise ValueError("set_instance_transforms_device: needs a torch tensor on the scene's device")
        if tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise ValueError(f"set_instance_transforms_device: tensor on {tensor.device}, this scene renders on cuda:{self.device}")
        rec = C.sizeof(InstanceXform)
        if not tensor.is_contiguous() or tensor.dim() != 2 or tensor.shape[1] * tensor.element_size() != rec:
            raise ValueError(f"set_instance_transforms_device: needs a contiguous (count, {rec} bytes) tensor, got "
                             f"{tuple(tensor.shape)} of {tensor.dtype}")
        self._enqueue_between_streams(tensor.device, lambda: self._cchk(lib.ptrt_set_instance_transforms_device(
            self.ctx, int(first), int(tensor.shape[0]), _vp(tensor.data_ptr()))), back=False)

    def set_instance_poses_device(self, first, tensor):
        """`ptrt_set_instance_poses_device`: meshes first .. first + count - 1 take their has_transform bit and matrices from the
        poses in `tensor`, a contiguous (count, 9) float32 torch tensor on this scene's device whose rows are `ptrt_instance_pose`
        records -- position, rotation (Euler radians), scale -- read in place by one launch on the context's stream, which
        derives the matrices as the reference's Transform3D does: no copy, no synchronisation.  The context's stream is ordered
        behind torch's current stream.  Follow with ptrt_refit_tlas / ptrt_reorder_tlas."""
        if not _is_tensor(tensor):
            raise ValueError("set_instance_poses_device: needs a torch tensor on the scene's device")
        if tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise ValueError(f"set_instance_poses_device: tensor on {tensor.device}, this scene renders on cuda:{self.device}")
        import torch
        if not tensor.is_contiguous() or tensor.dim() != 2 or tensor.shape[1] != 9 or tensor.dtype != torch.float32:
            raise ValueError(f"set_instance_poses_device: needs a contiguous (count, 9) float32 tensor, got "
                             f"{tuple(tensor.shape)} of {tensor.dtype}")
        self._enqueue_between_streams(tensor.device, lambda: self._cchk(lib.ptrt_set_instance_poses_device(
            self.ctx, int(first), int(tensor.shape[0]), _vp(tensor.data_ptr()))), back=False)

    def read_instance_transforms(self, first=0, count=None):
        """The has_transform bits and matrices the device's mesh records hold now (ptrt_read_instance_transforms; synchronises):
        a structured array with world, inverse and normal as (3, 4) float32 rows and has_transform (0 or 1), for meshes
        first .. first + count - 1 (count=None: all from `first`)."""
        if count is None:
            count = self.flatten().contents.mesh_count - int(first)
        raw = np.zeros(max(int(count), 0), dtype=INSTANCE_XFORM_DTYPE)
        self._cchk(lib.ptrt_read_instance_transforms(self.ctx, int(first), int(count), raw.ctypes.data_as(_vp)))
        out = np.zeros(len(raw), dtype=[("world", "<f4", (3, 4)), ("inverse", "<f4", (3, 4)), ("normal", "<f4", (3, 4)),
                                        ("has_transform", "<i4")])
        for k in ("world", "inverse", "normal"):
            out[k] = raw[k][:, :12].reshape(-1, 3, 4)
        out["has_transform"] = raw["has_transform"]
        return out

    def read_tlas_order(self):
        """The TLAS index array as the device holds it (ptrt_read_tlas_order; synchronises): int32 mesh indices."""
        n = self.flatten().contents.tlas_index_count
        out = np.zeros(n, dtype=np.int32)
        self._cchk(lib.ptrt_read_tlas_order(self.ctx, out.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return out

    def read_tlas(self):
        """The TLAS as the device holds it (ptrt_read_tlas; synchronises): structured array bmin, bmax, left, right, start, count."""
        n = self.flatten().contents.tlas_node_count
        out = np.zeros(n, dtype=TLAS_NODE_DTYPE)
        self._cchk(lib.ptrt_read_tlas(self.ctx, out.ctypes.data_as(C.POINTER(BvhNode)), n))
        return out

    def read_bvh(self, mesh):
        """Mesh `mesh`'s BVH as the device holds it (ptrt_read_bvh; synchronises): the uploaded nodes, pre-order, with the boxes
        of the last refit / rebuild -- the structured array read_tlas returns."""
        d = self.flatten().contents
        if not 0 <= int(mesh) < d.mesh_count:
            raise PtrtError(f"read_bvh: no mesh {mesh}")
        n = d.meshes[int(mesh)].node_count
        out = np.zeros(n, dtype=TLAS_NODE_DTYPE)
        self._cchk(lib.ptrt_read_bvh(self.ctx, int(mesh), out.ctypes.data_as(C.POINTER(BvhNode)), n))
        return out

    def refitFromDevice(self, mesh, device_ptr):
        """New vertex positions (n x 3 float32) already in device memory -> update + GPU refit, no host sync."""
        self._chk(lib.hs_refit_from_device(self._h, mesh, C.c_void_p(device_ptr)))

    def refitFromHost(self, mesh, host_ptr):
        """New positions from HOST memory (a raw address: pinned memory makes the copy asynchronous) + GPU refit."""
        self._chk(lib.hs_refit_from_host(self._h, mesh, C.c_void_p(host_ptr)))

    def rebuildObjectChanges(self, sync_host_copy=True):
        """commitObjectChanges for unchanged face counts with the BVH rebuilt on the GPU (ptrt_build_bvh)."""
        self._chk(lib.hs_rebuild_object_changes(self._h, int(sync_host_copy)))

    def rebuildFromDevice(self, mesh, device_ptr):
        """New vertex positions already in device memory -> update + GPU BVH rebuild, no host sync."""
        self._chk(lib.hs_rebuild_from_device(self._h, mesh, C.c_void_p(device_ptr)))

    def updateTriangles(self, mesh, verts9, tri_count=None, device_ptr=None):
        """A new triangle list (<= the uploaded count) for a soup mesh + GPU rebuild: numpy (n,9) or a device pointer."""
        if device_ptr is not None:
            self._chk(lib.hs_update_triangles(self._h, mesh, C.c_void_p(device_ptr), int(tri_count), 1))
            return
        a = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 9)
        self._chk(lib.hs_update_triangles(self._h, mesh, a.ctypes.data_as(_vp), a.shape[0], 0))

    def primIndices(self, mesh):
        """Host copy of the mesh's `primIndices` (mesh.cuh:57)."""
        n = self.meshCounts(mesh)[1]
        out = np.zeros(n, dtype=np.int32)
        self._chk(lib.hs_mesh_prim_indices(self._h, mesh, out.ctypes.data_as(C.POINTER(C.c_int)), n))
        return out

    def getFrameCount(self): return lib.hs_get_frame_count(self._h)
    def setFrameCount(self, f): lib.hs_set_frame_count(self._h, f)

    def render_to_device(self, device_ptr):
        """`Scene::render_to_device(unsigned char*)`: asynchronous, RGB8 bottom-up into device memory."""
        self._chk(lib.hs_render_to_device(self._h, C.c_void_p(device_ptr)))

    def render_to_host(self):
        out = np.empty((self.tile_rows, self.width, 3), dtype=np.uint8)
        self._chk(lib.hs_render_to_host(self._h, out.ctypes.data_as(_vp)))
        return out

    def render_to_device_wireframe(self, device_ptr, thickness):
        """`Scene::render_to_device_wireframe(unsigned char*, float)`: the wireframe view (edges of every hit triangle
        closer than `thickness` in barycentrics, the sky elsewhere), RGB8 bottom-up into device memory; synchronises."""
        self._chk(lib.hs_render_wireframe_to_device(self._h, C.c_void_p(device_ptr), float(thickness)))

    def render_wireframe_to_host(self, thickness):
        """The wireframe view into a host array (tile_rows, width, 3), in the buffer's bottom-up order like render_to_host."""
        out = np.empty((self.tile_rows, self.width, 3), dtype=np.uint8)
        self._chk(lib.hs_render_wireframe_to_host(self._h, out.ctypes.data_as(_vp), float(thickness)))
        return out

    def render_baked(self, target=None, *, frame=None, charts=None, chart_first=None, image=None, lightmap_mode="bilinear",
                     volume=None, probes=None, probe_mode="visibility", normal_bias=0.0, hdr=None, gbuffers=False):
        """The baked-light view (ptrt_render_baked): the scene lit by a lightmap atlas -- `charts`, `chart_first`, `image` as for
        query_lightmap --, by a probe volume -- `volume`, `probes` as for query_probe_light --, by both (the atlas where it has a
        sample, the volume elsewhere: moving objects, invalid texels) or by neither (emission and sky), shaded with the scene's
        own materials, in one launch.  `frame`: the frame index whose jitter the primary rays take (None: the one
        render_to_device would use next; it is not advanced).  torch tensors on this scene's device, contiguous, used in place.
        `target`: None -- RGB8 into a host array (tile_rows, width, 3), bottom-up like render_to_host, synchronous; a uint8
        tensor (tile_rows, width, 3) -- this scene's rows on the device; on a band scene a uint8 tensor (height, width, 3) --
        the scene's rows where they belong in the whole frame; False -- no RGB8.  `hdr`: True or an (n, 3) float32 tensor, n =
        tile_rows * width: the linear colour in the order of read(BUF_ACCUM).  `gbuffers`: True or (normal (n, 3) float32, depth
        (n,) float32, object_id (n,) int32): what a frame keeps of a first hit, the layouts post_frame takes.  Returns the host
        array when that is all that was asked for, else a dict of what was filled (rgb8, hdr, normal, depth, object_id).  Only
        a host target synchronises."""
        from . import baked
        import numpy as _np
        if frame is not None and (int(frame) != frame or frame < 0):
            raise ValueError(f"render_baked: frame {frame!r} (None or an integer >= 0)")
        n = self.tile_rows * self.width
        out = {}
        lazy = []  # (key, shape, dtype name) of the tensors to make once the inputs have passed
        if hdr is True:
            lazy.append(("hdr", (n, 3), "float32"))
        elif hdr is not None and hdr is not False:
            out["hdr"] = hdr
        if gbuffers is True:
            lazy += [("normal", (n, 3), "float32"), ("depth", (n,), "float32"), ("object_id", (n,), "int32")]
        elif gbuffers is not False and gbuffers is not None:
            try:
                out["normal"], out["depth"], out["object_id"] = gbuffers
            except (TypeError, ValueError):
                raise ValueError("render_baked: gbuffers: True or the three tensors (normal, depth, object_id)") from None
        mode = 0  # PTRT_OUT_HOST
        if target is not None and target is not False:
            shapes = {(self.tile_rows, self.width, 3): 1, (self.height, self.width, 3): 2}  # PTRT_OUT_DEVICE, _FRAME
            if not hasattr(target, "data_ptr") or tuple(target.shape) not in shapes:
                raise ValueError(f"render_baked: target: None, False or a uint8 tensor of shape {(self.tile_rows, self.width, 3)}" +
                                 (f" or {(self.height, self.width, 3)}" if self.tile_rows != self.height else "") +
                                 f", got {tuple(getattr(target, 'shape', ())) or type(target).__name__}")
            mode = 1 if tuple(target.shape) == (self.tile_rows, self.width, 3) else 2
            baked._tensor(self, "target", target, tuple(target.shape), "torch.uint8")
            out["rgb8"] = target
        if target is False and "hdr" not in out and not any(k == "hdr" for k, _, _ in lazy):
            raise ValueError("render_baked: no target at all: target=False needs hdr")
        view, keep = baked.baked_view(self, charts=charts, chart_first=chart_first, image=image, lightmap_mode=lightmap_mode,
                                      volume=volume, probes=probes, probe_mode=probe_mode, normal_bias=normal_bias,
                                      hdr=out.get("hdr"), normal=out.get("normal"), depth=out.get("depth"),
                                      object_id=out.get("object_id"))
        if mode:
            baked._on_device(self, "target", target)
        if lazy:
            import torch
            if self.device < 0:
                raise ValueError("render_baked: hdr and gbuffers need a device, this scene renders on no device (host-only)")
            for key, shape, dt in lazy:
                out[key] = torch.empty(shape, dtype=getattr(torch, dt), device=torch.device("cuda", self.device))
                setattr(view, "d_" + key, out[key].data_ptr())
        fr = -1 if frame is None else int(frame)
        host = _np.empty((self.tile_rows, self.width, 3), dtype=_np.uint8) if target is None else None
        pixels = host.ctypes.data_as(_vp) if host is not None else _vp(target.data_ptr()) if mode else None
        call = lambda: self._chk(lib.hs_render_baked(self._h, fr, C.byref(view), pixels, mode))  # noqa: E731
        if self.device >= 0 and (keep or out):
            import torch
            self._enqueue_between_streams(torch.device("cuda", self.device), call)
        else:
            call()
        del keep
        if host is not None:
            if not out:
                return host
            out["rgb8"] = host
        return out

    def post_frame(self, accum_ptr, normal_ptr, depth_ptr, object_id_ptr, out_device_ptr=None):
        """Presenting rank of the tile farm: motion vectors + denoiser + bloom + tonemap of this full-frame scene
        over a gathered frame (device pointers, top-down; `ptrt_post_frame`).  RGB8 goes to `out_device_ptr`, or is
        returned as a host array."""
        if out_device_ptr is not None:
            self._chk(lib.hs_post_frame(self._h, accum_ptr, normal_ptr, depth_ptr, object_id_ptr, C.c_void_p(out_device_ptr), 1))
            return None
        out = np.empty((self.tile_rows, self.width, 3), dtype=np.uint8)
        self._chk(lib.hs_post_frame(self._h, accum_ptr, normal_ptr, depth_ptr, object_id_ptr, out.ctypes.data_as(_vp), 0))
        return out

    def view_run(self, frames, slots=2, keep=True, dump_prefix="", dump_every=0):
        """The reference's viewer loop (map_pbo -> render_to_device -> unmap -> blit -> draw) over the HIP
        presentation ring, headless.  Returns (frames as uint8 (n, H, W, 3) or None, wall ms per frame)."""
        out = np.empty((frames, self.tile_rows, self.width, 3), dtype=np.uint8) if keep else None
        ms = C.c_double()
        self._chk(lib.hs_view_run(self._h, frames, slots, out.ctypes.data_as(_vp) if keep else None, C.byref(ms),
                                  dump_prefix.encode(), dump_every))
        return out, ms.value

    def sync(self): self._cchk(lib.ptrt_sync(self.ctx))

    def device_array(self, kind):
        """Zero-copy view of a frame buffer in device memory for array libraries that accept
        `__cuda_array_interface__` (e.g. `torch.as_tensor(scene.device_array(P.BUF_ACCUM), device="cuda")`)."""
        n = self.tile_rows * self.width
        shape, typestr = {BUF_ACCUM: ((n, 3), "<f4"), BUF_NORMAL: ((n, 3), "<f4"), BUF_DEPTH: ((n, 1), "<f4"),
                          BUF_OBJECT_ID: ((n, 1), "<i4")}[kind]
        ptr = lib.ptrt_device_buffer(self.ctx, kind)
        if not ptr:
            raise PtrtError(lib.ptrt_last_error(self.ctx).decode())

        class _View:
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2}
        return _View()

    def read(self, kind):
        n = self.tile_rows * self.width
        rw, rh = self.renderSize()
        r = n if (rw, rh) == (self.width, self.height) else rw * rh   # render-size images (see ptrt.h)
        shape, dt = {BUF_ACCUM: ((n, 3), np.float32), BUF_NORMAL: ((r, 3), np.float32), BUF_DEPTH: ((r,), np.float32),
                     BUF_OBJECT_ID: ((r,), np.int32), BUF_RGB8: ((self.tile_rows, self.width, 3), np.uint8),
                     BUF_RNG: ((n, 6), np.uint32), BUF_DENOISED: ((r, 3), np.float32),
                     BUF_MOTION: ((r, 2), np.float32), BUF_RENDER_ACCUM: ((r, 3), np.float32)}[kind]
        out = np.empty(shape, dtype=dt)
        self._cchk(lib.ptrt_read_buffer(self.ctx, kind, out.ctypes.data_as(_vp), out.nbytes))
        return out

    def write_rng(self, states):
        a = np.ascontiguousarray(states, dtype=np.uint32)
        self._cchk(lib.ptrt_write_rng(self.ctx, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.nbytes))

    def reset_rng(self, seed=DEFAULT_SEED): self._cchk(lib.ptrt_reset_rng(self.ctx, seed))
    def set_option(self, name, value): self._cchk(lib.ptrt_set_option(self.ctx, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_longlong(0)
        self._cchk(lib.ptrt_get_option(self.ctx, name.encode(), C.byref(v)))
        return v.value

    def stats(self):
        s = Stats()
        self._cchk(lib.ptrt_get_stats(self.ctx, C.byref(s)))
        return dict(extension_rays=s.extension_rays, shadow_rays=s.shadow_rays, paths=s.paths,
                    shadow_rays_walked=s.shadow_rays_walked)

    def last_kernel_ms(self):
        a = C.c_float()
        self._cchk(lib.ptrt_last_kernel_ms(self.ctx, C.byref(a), None))
        return a.value

    def set_stream(self, hip_stream):
        self._cchk(lib.ptrt_set_stream(self.ctx, C.c_void_p(hip_stream)))

    def kernel_ms_history(self, max_n=256):
        out = np.zeros(max_n, dtype=np.float32)
        n = lib.ptrt_kernel_ms_history(self.ctx, _fptr(out), max_n)
        if n < 0:
            raise PtrtError(lib.ptrt_last_error(self.ctx).decode())
        return out[:n]

    def launch_ms_history(self, max_n=1024):
        """(trace_ms, tail_ms) of the launches of the last overlapping frames (option time_launches), oldest first."""
        a, b = np.zeros(max_n, dtype=np.float32), np.zeros(max_n, dtype=np.float32)
        n = lib.ptrt_launch_ms_history(self.ctx, _fptr(a), _fptr(b), max_n)
        if n < 0:
            raise PtrtError(lib.ptrt_last_error(self.ctx).decode())
        return a[:n], b[:n]

    def trace_rays(self, origins, directions):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(o.shape[0], dtype=HIT_DTYPE)
        self._cchk(lib.ptrt_trace_rays(self.ctx, _fptr(o), _fptr(d), o.shape[0], out.ctypes.data_as(_vp)))
        return out

    # ---- batched ray queries (ptrt_query_rays through Scene::queryClosestDevice / queryOccludedDevice) ----
    def query_closest(self, origins, directions):
        """Closest hit of every ray.  torch tensors on this scene's device -- float32, contiguous, (n, 3) -- are read in place
        and the answer is an (n, 16) int32 tensor, one 64-byte `ptrt_hit` per row (`hit_fields` names its columns); numpy
        arrays are staged through the device and the answer is a numpy array of HIT_DTYPE, the record of `trace_rays`."""
        return self._query(origins, directions, None)

    def query_occluded(self, origins, directions, tmax):
        """1 where something blocks the ray before `tmax` (the reference's shadow query; glass, transmission > 0.5, never
        blocks), else 0: an (n,) int32 tensor for torch inputs, a numpy array for numpy inputs.  `tmax`: (n,) float32."""
        if tmax is None:
            raise ValueError("query_occluded needs tmax")
        return self._query(origins, directions, tmax)

    def _query(self, origins, directions, tmax):
        arrays = [origins, directions] + ([] if tmax is None else [tmax])
        shapes = [(3,), (3,), ()]
        is_t = [_is_tensor(a) for a in arrays]
        if any(is_t) and not all(is_t):
            raise ValueError("ray query: pass all torch tensors or all numpy arrays")
        n = None
        for a, tail in zip(arrays, shapes):
            if not is_t[0] and not isinstance(a, np.ndarray):
                raise ValueError(f"ray query: expected a numpy array or a torch tensor, got {type(a).__name__}")
            if tuple(a.shape[1:]) != tail or a.ndim != 1 + len(tail):
                raise ValueError(f"ray query: shape {tuple(a.shape)}, expected (n, {tail[0]})" if tail else
                                 f"ray query: tmax shape {tuple(a.shape)}, expected (n,)")
            n = a.shape[0] if n is None else n
            if a.shape[0] != n:
                raise ValueError(f"ray query: {n} origins but {a.shape[0]} rows in another input")
            if (str(a.dtype) != "torch.float32") if is_t[0] else (a.dtype != np.float32):
                raise ValueError(f"ray query: dtype {a.dtype}, expected float32")
        if n >= 2 ** 31:
            raise ValueError(f"ray query: {n} rays (at most 2^31 - 1 per call)")
        closest = tmax is None
        for a in arrays if is_t[0] else []:
            if a.device.type != "cuda" or a.device.index != self.device:
                raise ValueError(f"ray query: tensor on {a.device}, this scene renders on " +
                                 (f"cuda:{self.device}" if self.device >= 0 else "no device (host-only)"))
            if not a.is_contiguous():
                raise ValueError("ray query: tensors must be contiguous")
        if self.device < 0:  # host-only: the mirror refuses (PtrtError) before it looks at the arguments
            self._chk(lib.hs_query_closest(self._h, None, None, n, None) if closest else
                      lib.hs_query_occluded(self._h, None, None, None, n, None))
        import torch
        if not is_t[0]:
            dev = torch.device("cuda", self.device)
            staged = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
            out = self._query_tensors(torch, staged, n, closest).cpu().numpy()
            return out.view(HIT_DTYPE).reshape(n) if closest else out
        return self._query_tensors(torch, arrays, n, closest)

    def _query_tensors(self, torch, arrays, n, closest):
        dev = arrays[0].device
        out = torch.empty((n, 16) if closest else (n,), dtype=torch.int32, device=dev)
        if n == 0:
            return out
        p = [_vp(a.data_ptr()) for a in arrays]
        self._enqueue_between_streams(dev, lambda: self._chk(
            lib.hs_query_closest(self._h, p[0], p[1], n, _vp(out.data_ptr())) if closest else
            lib.hs_query_occluded(self._h, p[0], p[1], p[2], n, _vp(out.data_ptr()))))
        return out

    # ---- path-traced radiance for caller-supplied rays (ptrt_query_radiance through Scene::queryRadiance) ----
    def _device_tensor(self, what, a, cols, dtype):
        if not _is_tensor(a):
            raise ValueError(f"{what}: needs a torch tensor on the scene's device, got {type(a).__name__}")
        if a.device.type != "cuda" or a.device.index != self.device:
            raise ValueError(f"{what}: tensor on {a.device}, this scene renders on " +
                             (f"cuda:{self.device}" if self.device >= 0 else "no device (host-only)"))
        if a.dim() != 2 or a.shape[1] != cols or str(a.dtype) not in dtype.split("|"):
            raise ValueError(f"{what}: shape {tuple(a.shape)} of {a.dtype}, expected (n, {cols}) of {dtype}")
        if not a.is_contiguous():
            raise ValueError(f"{what}: tensors must be contiguous")

    def _out_rows(self, what, out, n, cols, dtype, device, rows_for):
        """The answer's tensor: a new (n, cols) one of `dtype` on `device`, or the caller's `out`, checked.  `rows_for`: how the
        refusal of another row count ends -- "out has .. rows for <rows_for>"."""
        if out is None:
            import torch
            return torch.empty((n, cols), dtype=getattr(torch, dtype.split(".")[1]), device=device)
        self._device_tensor(f"{what}: out", out, cols, dtype)
        if out.shape[0] != n:
            raise ValueError(f"{what}: out has {out.shape[0]} rows for {rows_for}")
        return out

    @staticmethod
    def _ray_rows(rows, device):
        """the (rows, 3), (rows, 3), (rows,), (rows, 3) float32 tensors direct_rays and bounce_terms answer with"""
        import torch
        return tuple(torch.empty(shape, dtype=torch.float32, device=device) for shape in ((rows, 3), (rows, 3), (rows,), (rows, 3)))

    def _phases(self, what, phases, n, noun):
        """`phases` of the texel queries, checked where given: an (n,) float32 tensor, one per texel.  `noun`: what the refusal
        of another count calls the n."""
        if phases is None:
            return
        if not _is_tensor(phases) or phases.dim() != 1:
            raise ValueError(f"{what}: phases: needs a torch tensor of shape (n,) on the scene's device")
        self._device_tensor(f"{what}: phases", phases.unsqueeze(1), 1, "torch.float32")
        if phases.shape[0] != n:
            raise ValueError(f"{what}: {n} {noun}, {phases.shape[0]} phases")

    @staticmethod
    def _atlas_shape(what, image):
        """(w, h) of an (H, W, 4) atlas image, before its device is looked at: a 3-d tensor, 1 x 1 .. 2^28 texels, contiguous"""
        if not _is_tensor(image) or image.dim() != 3:
            raise ValueError(f"{what}: image: needs a torch tensor of shape (H, W, 4) on the scene's device")
        h, w = int(image.shape[0]), int(image.shape[1])
        if h < 1 or w < 1 or h * w > 2 ** 28:
            raise ValueError(f"{what}: a {w} x {h} atlas (1 x 1 .. 2^28 texels)")
        if not image.is_contiguous():
            raise ValueError(f"{what}: image: tensors must be contiguous")
        return w, h

    def _atlas_image(self, what, image):
        """(w, h) of an atlas image, checked: _atlas_shape, then float32 texels of four on the scene's device.  atlas_filter
        checks its numbers between the two, as it always has."""
        w, h = self._atlas_shape(what, image)
        self._device_tensor(f"{what}: image", image.view(h * w, -1), 4, "torch.float32")
        return w, h

    def _enqueue_between_streams(self, dev, call, back=True):
        """`call()` enqueues on the context's stream.  Stream order by events, both ways: the context's stream waits for what
        torch enqueued on its current stream before the call (the inputs), and torch's current stream waits for the call
        (whoever reads the answer there).  `back=False`: the first half only, for a call that leaves nothing to read."""
        import torch
        cur = torch.cuda.current_stream(dev)
        ctx_stream = torch.cuda.ExternalStream(self.get_option("stream"), device=dev)
        other = ctx_stream.cuda_stream != cur.cuda_stream
        if other:
            ctx_stream.wait_stream(cur)
        call()
        if other and back:
            cur.wait_stream(ctx_stream)

    def query_radiance(self, origins, directions, rng_states, samples=1, max_depth=None, out=None):
        """Path-traced radiance along every ray: tracePath with the ray's own generator state, `samples` times, `max_depth`
        bounces (None: the scene's bounce depth).  torch tensors on this scene's device, contiguous, read in place: origins and
        directions (n, 3) float32, rng_states (n, 6) int32 (or uint32) in the canonical order of `read(BUF_RNG)` -- `init_rng_states` makes
        fresh ones -- ADVANCED IN PLACE, so a later call continues each ray's stream.  Returns an (n, 8) float32 tensor, one
        32-byte `ptrt_radiance` per row: radiance 0:3, depth 3, normal 4:7 and the object id's int32 bits in column 7
        (`radiance_fields` names them); `out` takes such a tensor to write into.  No synchronisation."""
        self._device_tensor("query_radiance: origins", origins, 3, "torch.float32")
        self._device_tensor("query_radiance: directions", directions, 3, "torch.float32")
        self._device_tensor("query_radiance: rng_states", rng_states, 6, "torch.int32|torch.uint32")
        n = origins.shape[0]
        if directions.shape[0] != n or rng_states.shape[0] != n:
            raise ValueError(f"query_radiance: {n} origins, {directions.shape[0]} directions, {rng_states.shape[0]} states")
        if n >= 2 ** 31:
            raise ValueError(f"query_radiance: {n} rays (at most 2^31 - 1 per call)")
        out = self._out_rows("query_radiance", out, n, 8, "torch.float32", origins.device, f"{n} rays")
        if n == 0:
            return out
        self._enqueue_between_streams(origins.device, lambda: self._chk(lib.hs_query_radiance(
            self._h, _vp(origins.data_ptr()), _vp(directions.data_ptr()), _vp(rng_states.data_ptr()), n, int(samples),
            0 if max_depth is None else int(max_depth), _vp(out.data_ptr()))))
        return out

    def query_probes(self, positions, directions, rng_states, samples=1, max_depth=None, max_distance=1e30, out=None):
        """Light probes: probe p sends one ray from positions[p] along every direction (one set for all probes, used as given,
        not normalised), ray (p, k) with generator state p * k_dirs + k, `samples` paths of `max_depth` bounces each (None: the
        scene's bounce depth).  torch tensors on this scene's device, contiguous, read in place: positions (n, 3) and
        directions (k, 3) float32, rng_states (n * k, 6) int32 (or uint32) ADVANCED IN PLACE.  Returns an (n, 32) float32
        tensor, one 128-byte `ptrt_probe` per row (`probe_fields` names the columns): the means over the directions of
        Y_i(d) * radiance for the nine spherical harmonics of bands 0-2 (columns 3 * i + channel), of the first-hit distance
        clamped to `max_distance` (27), of its square (28), and the fraction of rays that hit (29); `out` takes such a tensor
        to write into.  `ptrt_amd.probes` has direction sets, grids and the irradiance reconstruction.  No synchronisation."""
        self._device_tensor("query_probes: positions", positions, 3, "torch.float32")
        self._device_tensor("query_probes: directions", directions, 3, "torch.float32")
        self._device_tensor("query_probes: rng_states", rng_states, 6, "torch.int32|torch.uint32")
        n, k = positions.shape[0], directions.shape[0]
        if k < 1:
            raise ValueError("query_probes: no directions")
        if rng_states.shape[0] != n * k:
            raise ValueError(f"query_probes: {n} probes x {k} directions need {n * k} states, got {rng_states.shape[0]}")
        if n >= 2 ** 31 or k >= 2 ** 31:
            raise ValueError(f"query_probes: {n} probes x {k} directions (at most 2^31 - 1 of each per call)")
        out = self._out_rows("query_probes", out, n, 32, "torch.float32", positions.device, f"{n} probes")
        if n == 0:
            return out
        self._enqueue_between_streams(positions.device, lambda: self._chk(lib.hs_query_probes(
            self._h, _vp(positions.data_ptr()), n, _vp(directions.data_ptr()), k, _vp(rng_states.data_ptr()), int(samples),
            0 if max_depth is None else int(max_depth), float(max_distance), _vp(out.data_ptr()))))
        return out

    def _texel_inputs(self, what, positions, normals, samples2, phases):
        """the shared inputs of query_irradiance / irradiance_rays, checked; returns (n texels, k directions)"""
        self._device_tensor(f"{what}: positions", positions, 3, "torch.float32")
        self._device_tensor(f"{what}: normals", normals, 3, "torch.float32")
        self._device_tensor(f"{what}: samples2", samples2, 2, "torch.float32")
        n, k = positions.shape[0], samples2.shape[0]
        if normals.shape[0] != n:
            raise ValueError(f"{what}: {n} positions, {normals.shape[0]} normals")
        if k < 1:
            raise ValueError(f"{what}: no directions")
        if n >= 2 ** 31 or k >= 2 ** 31:
            raise ValueError(f"{what}: {n} texels x {k} directions (at most 2^31 - 1 of each per call)")
        self._phases(what, phases, n, "positions")
        return n, k

    def query_irradiance(self, positions, normals, samples2, rng_states, samples=1, max_depth=None, max_distance=1e30, offset=1e-4,
                         phases=None, out=None):
        """Lightmap texels: texel t gathers one ray per point of `samples2` (k points in [0,1)^2, one set for all texels, used
        as given) from positions[t] + offset * normals[t], along the cosine-distributed direction that point maps to about
        normals[t] (unit normals expected; `phases`, (n,) float32, rotates each texel's set about its normal), ray (t, k) with
        generator state t * k_dirs + k, `samples` paths of `max_depth` bounces each (None: the scene's bounce depth).  torch
        tensors on this scene's device, contiguous, read in place: positions and normals (n, 3), samples2 (k, 2) float32,
        rng_states (n * k, 6) int32 (or uint32) ADVANCED IN PLACE.  Returns an (n, 8) float32 tensor, one 32-byte
        `ptrt_irradiance` per row (`irradiance_fields` names the columns): the means over the directions of the radiance
        (0:3; pi times it is the irradiance), of the first-hit distance clamped to `max_distance` (3), of its square (4), and
        the fraction of rays that hit (5); `out` takes such a tensor to write into.  `ptrt_amd.lightmap` has sample sets,
        phases, quads and the irradiance.  No synchronisation."""
        n, k = self._texel_inputs("query_irradiance", positions, normals, samples2, phases)
        self._device_tensor("query_irradiance: rng_states", rng_states, 6, "torch.int32|torch.uint32")
        if rng_states.shape[0] != n * k:
            raise ValueError(f"query_irradiance: {n} texels x {k} directions need {n * k} states, got {rng_states.shape[0]}")
        out = self._out_rows("query_irradiance", out, n, 8, "torch.float32", positions.device, f"{n} texels")
        if n == 0:
            return out
        self._enqueue_between_streams(positions.device, lambda: self._chk(lib.hs_query_irradiance(
            self._h, _vp(positions.data_ptr()), _vp(normals.data_ptr()), n, _vp(samples2.data_ptr()), k,
            None if phases is None else _vp(phases.data_ptr()), float(offset), _vp(rng_states.data_ptr()), int(samples),
            0 if max_depth is None else int(max_depth), float(max_distance), _vp(out.data_ptr()))))
        return out

    def irradiance_rays(self, positions, normals, samples2, offset=1e-4, phases=None):
        """(origins, directions): (n * k, 3) float32 tensors holding the rays query_irradiance traces for these texels, ray
        (t, k) in row t * k_dirs + k (ptrt_irradiance_rays).  Arguments as for query_irradiance.  No synchronisation."""
        n, k = self._texel_inputs("irradiance_rays", positions, normals, samples2, phases)
        import torch
        o = torch.empty((n * k, 3), dtype=torch.float32, device=positions.device)
        d = torch.empty((n * k, 3), dtype=torch.float32, device=positions.device)
        if n == 0:
            return o, d
        self._enqueue_between_streams(positions.device, lambda: self._chk(lib.hs_irradiance_rays(
            self._h, _vp(positions.data_ptr()), _vp(normals.data_ptr()), n, _vp(samples2.data_ptr()), k,
            None if phases is None else _vp(phases.data_ptr()), float(offset), _vp(o.data_ptr()), _vp(d.data_ptr()))))
        return o, d

    def lightCount(self):
        return lib.hs_light_count(self._h)

    def _direct_inputs(self, what, positions, normals, samples2, phases, lights):
        """the shared inputs of query_direct / direct_rays, checked; returns (n texels, samples2, shadow samples, first light,
        light count)"""
        first, count = self._light_range(what, lights)
        self._device_tensor(f"{what}: positions", positions, 3, "torch.float32")
        if samples2 is None:
            import torch
            samples2 = torch.from_numpy(lightmap.hammersley2(1)).to(positions.device)
        n, k = self._texel_inputs(what, positions, normals, samples2, phases)
        if count * k >= 2 ** 31:
            raise ValueError(f"{what}: {count} lights x {k} shadow samples (at most 2^31 - 1 terms per texel)")
        return n, samples2, k, first, count

    def query_direct(self, positions, normals, samples2=None, phases=None, offset=1e-4, lights=None, out=None):
        """The analytic lights' direct term at lightmap texels: texel t takes one light sample per point of `samples2` (k points
        in [0,1)^2, one set for all texels and lights, the two numbers of a sphere light's cone sample; None: the one point of
        `lightmap.hammersley2(1)`) of each light of `lights` ((first, count) of the scene's lights; None: all) at positions[t]
        with normal normals[t] (used as given), and walks the shadow rays of the samples that can add something from
        positions[t] + offset * normals[t] (`phases`, (n,) float32, rotates each texel's set).  torch tensors on this scene's
        device, contiguous, read in place: positions and normals (n, 3), samples2 (k, 2) float32.  Returns an (n, 8) float32
        tensor, one 32-byte `ptrt_direct` per row (`direct_fields` names the columns): the irradiance (0:3) -- the sum over the
        lights of each light's mean over its samples; a light with a radius contributes radiance * solid angle --, the fraction
        of samples that reached the texel (3) and that were blocked (4); `out` takes such a tensor to write into.
        `ptrt_amd.lightmap` adds it to a gather's rows.  No synchronisation."""
        n, samples2, k, first, count = self._direct_inputs("query_direct", positions, normals, samples2, phases, lights)
        out = self._out_rows("query_direct", out, n, 8, "torch.float32", positions.device, f"{n} texels")
        if n == 0:
            return out
        self._enqueue_between_streams(positions.device, lambda: self._chk(lib.hs_query_direct(
            self._h, _vp(positions.data_ptr()), _vp(normals.data_ptr()), n, _vp(samples2.data_ptr()), k,
            None if phases is None else _vp(phases.data_ptr()), float(offset), first, count, _vp(out.data_ptr()))))
        return out

    def direct_rays(self, positions, normals, samples2=None, phases=None, offset=1e-4, lights=None):
        """(origins, directions, tmax, weights): (n * Q, 3), (n * Q, 3), (n * Q,) and (n * Q, 3) float32 tensors holding the shadow
        rays of query_direct for these texels and what each adds when it is not blocked, term (t, q) in row t * Q + q with
        Q = light count * k and q = light * k + sample (ptrt_direct_rays) -- for the samples query_direct does not walk too
        (weight not positive, NaN included).  Arguments as for query_direct.  No synchronisation."""
        n, samples2, k, first, count = self._direct_inputs("direct_rays", positions, normals, samples2, phases, lights)
        rays = n * count * k
        o, d, t, w = self._ray_rows(rays, positions.device)
        if rays == 0:
            return o, d, t, w
        self._enqueue_between_streams(positions.device, lambda: self._chk(lib.hs_direct_rays(
            self._h, _vp(positions.data_ptr()), _vp(normals.data_ptr()), n, _vp(samples2.data_ptr()), k,
            None if phases is None else _vp(phases.data_ptr()), float(offset), first, count, _vp(o.data_ptr()), _vp(d.data_ptr()),
            _vp(t.data_ptr()), _vp(w.data_ptr()))))
        return o, d, t, w

    def _light_range(self, what, lights):
        """`lights` of the direct and bounce queries, checked; returns (first light, light count)"""
        have = self.lightCount()
        try:
            first, count = (0, have) if lights is None else (int(lights[0]), int(lights[1]))
        except (TypeError, IndexError):
            raise ValueError(f"{what}: lights={lights!r}, expected None or (first, count)") from None
        if first < 0 or count < 0 or first + count > have:
            raise ValueError(f"{what}: lights ({first}, {count}) of the scene's {have}")
        return first, count

    def _shadow_samples(self, what, device, shadow2, count, k):
        """the light samples of query_bounce / bounce_terms, checked; returns (shadow2, shadow samples)"""
        if shadow2 is None:
            import torch
            shadow2 = torch.from_numpy(lightmap.hammersley2(1)).to(device)
        self._device_tensor(f"{what}: shadow2", shadow2, 2, "torch.float32")
        m = shadow2.shape[0]
        if m < 1:
            raise ValueError(f"{what}: no shadow samples")
        if k * count * m >= 2 ** 31:
            raise ValueError(f"{what}: {k} directions x {count} lights x {m} shadow samples (at most 2^31 - 1 terms per texel)")
        return shadow2, m

    def query_bounce(self, positions, normals, samples2, shadow2=None, phases=None, offset=1e-4, lights=None, out=None):
        """The analytic lights' one-bounce term at lightmap texels -- light that reaches the texel after exactly one reflection
        off the surface a gather ray hits first, which neither query_irradiance (its rays take no light sample at their first
        hit) nor query_direct (the lights at the texel itself) sees.  Texel t sends the gather rays of query_irradiance (one
        per point of `samples2`, rotated by `phases`, from positions[t] + offset * normals[t]); at each ray's closest hit it
        takes one light sample per point of `shadow2` (m points in [0,1)^2, rotated by `phases` too; None: the one point of
        `lightmap.hammersley2(1)`) of each light of `lights` ((first, count); None: all), values it by the hit's BSDF as a path
        vertex does (soft clamp kept, no MIS weight) and walks its shadow ray.  torch tensors on this scene's device,
        contiguous, read in place.  Returns an (n, 8) float32 tensor, one 32-byte `ptrt_bounce` per row (`bounce_fields` names
        the columns): the mean radiance (0:3; pi times it is the irradiance, `lightmap.bounce_irradiance`), the fractions of
        the k * Q terms lit (3) and blocked (4), the fraction of gather rays that hit (5); `out` takes such a tensor to write
        into.  `lightmap.full_irradiance` adds it to the direct and gathered terms.  No synchronisation."""
        first, count = self._light_range("query_bounce", lights)
        n, k = self._texel_inputs("query_bounce", positions, normals, samples2, phases)
        shadow2, m = self._shadow_samples("query_bounce", positions.device, shadow2, count, k)
        out = self._out_rows("query_bounce", out, n, 8, "torch.float32", positions.device, f"{n} texels")
        if n == 0:
            return out
        self._enqueue_between_streams(positions.device, lambda: self._chk(lib.hs_query_bounce(
            self._h, _vp(positions.data_ptr()), _vp(normals.data_ptr()), n, _vp(samples2.data_ptr()), k,
            None if phases is None else _vp(phases.data_ptr()), float(offset), _vp(shadow2.data_ptr()), m, first, count,
            _vp(out.data_ptr()))))
        return out

    def bounce_terms(self, hits, directions, n_dirs, shadow2=None, phases=None, lights=None):
        """(origins, L, tmax, values): (r * Q, 3), (r * Q, 3), (r * Q,) and (r * Q, 3) float32 tensors holding the terms
        query_bounce sums, for hits the caller traced: `hits` (r, 16) int32 and `directions` (r, 3) float32 are what
        `query_closest(*irradiance_rays(..))` and `irradiance_rays` return for r = n * n_dirs gather rays, ray (t, k) in row
        t * n_dirs + k; `phases`: (n,) float32 or None.  Term q = light * m + sample of ray i is row i * Q + q, Q = light count
        * m: the path's shadow origin, the direction to the light, the ray's length and the term's value (ptrt_bounce_terms)
        -- for terms query_bounce does not walk too; a miss gives a row of zeros.  No synchronisation."""
        first, count = self._light_range("bounce_terms", lights)
        self._device_tensor("bounce_terms: hits", hits, 16, "torch.int32")
        self._device_tensor("bounce_terms: directions", directions, 3, "torch.float32")
        r, k = hits.shape[0], int(n_dirs)
        if directions.shape[0] != r:
            raise ValueError(f"bounce_terms: {r} hits, {directions.shape[0]} directions")
        if k < 1 or r % k:
            raise ValueError(f"bounce_terms: {r} hits are not a multiple of n_dirs = {k}")
        n = r // k
        self._phases("bounce_terms", phases, n, "texels")
        shadow2, m = self._shadow_samples("bounce_terms", hits.device, shadow2, count, k)
        rows = r * count * m
        o, d, t, v = self._ray_rows(rows, hits.device)
        if rows == 0:
            return o, d, t, v
        self._enqueue_between_streams(hits.device, lambda: self._chk(lib.hs_bounce_terms(
            self._h, _vp(hits.data_ptr()), _vp(directions.data_ptr()), n, k, _vp(shadow2.data_ptr()), m,
            None if phases is None else _vp(phases.data_ptr()), first, count, _vp(o.data_ptr()), _vp(d.data_ptr()),
            _vp(t.data_ptr()), _vp(v.data_ptr()))))
        return o, d, t, v

    def atlas_texels(self, mesh, uv, width, height, out=None, clear=True):
        """The UV charts of mesh `mesh` (the id addCube and its kin return) rasterised into a `width` x `height` lightmap atlas
        (ptrt_atlas_texels).  `uv`: an (F, 6) float32 tensor on this scene's device, contiguous, read in place -- the (x, y) of
        corners v0, v1, v2 of each of the mesh's F faces in TEXEL units (`lightmap.triangle_charts` makes charts for a mesh
        without UVs, `lightmap.uv_to_texels` scales [0, 1] UVs).  Returns an (height * width, 8) int32 tensor, one 32-byte
        `ptrt_atlas_texel` per row, texel (i, j) in row j * width + i (`atlas_fields` names the columns): world position (0:3,
        float32 bits), owning face (3), world geometric normal (4:7, float32 bits), mesh (7; -1 where no face covers the texel's
        centre (i + 0.5, j + 0.5)).  The lowest face covering a centre owns it.  `out` takes such a tensor; with `clear=False`
        its texels with mesh >= 0 are kept, so several meshes can share an atlas (the first call wins).
        `lightmap.atlas_inputs` turns the rows into what query_irradiance and query_direct take.  No synchronisation."""
        self._device_tensor("atlas_texels: uv", uv, 6, "torch.float32")
        width, height = int(width), int(height)
        if width < 1 or height < 1 or width * height > 2 ** 28:
            raise ValueError(f"atlas_texels: a {width} x {height} atlas (1 x 1 .. 2^28 texels)")
        faces = self.meshCounts(int(mesh))[1]
        if uv.shape[0] != faces:
            raise ValueError(f"atlas_texels: uv has {uv.shape[0]} rows, mesh {mesh} has {faces} faces")
        if out is None and not clear:
            raise ValueError("atlas_texels: clear=False needs the atlas of an earlier call as `out`")
        out = self._out_rows("atlas_texels", out, width * height, 8, "torch.int32", uv.device, f"{width} x {height} texels")
        self._enqueue_between_streams(uv.device, lambda: self._chk(lib.hs_atlas_texels(
            self._h, int(mesh), _vp(uv.data_ptr()), width, height, 1 if clear else 0, _vp(out.data_ptr()))))
        return out

    def atlas_dilate(self, image, passes=1):
        """`passes` (1 .. 64) dilation passes over a baked atlas (ptrt_atlas_dilate).  `image`: an (H, W, 4) float32 tensor on
        this scene's device, contiguous, {r, g, b, valid} per texel -- `lightmap.scatter(..).reshape(H, W, 4)` makes one.  Each
        pass gives every invalid texel (valid == 0) that has valid 8-neighbours their mean and marks it valid; texels filled
        in one pass spread in the next.  The passes alternate between `image` and a second buffer allocated here; returns the
        tensor that holds the result -- `image` itself for an even `passes` (it is overwritten from the second pass on).  No
        synchronisation."""
        w, h = self._atlas_image("atlas_dilate", image)
        passes = int(passes)
        if passes < 1 or passes > 64:
            raise ValueError(f"atlas_dilate: {passes} passes (1 .. 64)")
        import torch
        other = torch.empty_like(image)
        where = []
        self._enqueue_between_streams(image.device, lambda: where.append(self._chk(lib.hs_atlas_dilate(
            self._h, _vp(image.data_ptr()), _vp(other.data_ptr()), w, h, passes))))
        return other if where[0] else image

    def atlas_filter(self, texels, image, passes, sigma_distance, sigma_plane, normal_power=2):
        """`passes` (1 .. 8) passes of the edge-aware a-trous filter over a baked atlas (ptrt_atlas_filter), between
        `lightmap.scatter` and `atlas_dilate`.  `texels`: the (H * W, 8) int32 rows of `atlas_texels` for this atlas, read in
        place; `image`: an (H, W, 4) float32 tensor on this scene's device, contiguous, {r, g, b, valid} per texel.  Pass s
        averages the 25 taps of a 5 x 5 B3 kernel at step 2^s, each weighed by its world distance from the centre (nothing
        beyond `sigma_distance` * step), its distance from the centre's tangent plane (nothing beyond `sigma_plane`) and the
        cosine between the two normals squared `normal_power` (0 .. 7) times; invalid texels (valid == 0) and uncovered ones
        (mesh < 0) neither give nor take and are copied.  `lightmap.filter_sigmas(lightmap.texel_pitch(texels, W, H))`
        recommends the sigmas.  The passes alternate between `image` and a second buffer allocated here; returns the tensor
        that holds the result -- `image` itself for an even `passes` (it is overwritten from the second pass on).  No
        synchronisation."""
        w, h = self._atlas_shape("atlas_filter", image)
        passes, normal_power = int(passes), int(normal_power)
        if passes < 1 or passes > 8:
            raise ValueError(f"atlas_filter: {passes} passes (1 .. 8)")
        if normal_power < 0 or normal_power > 7:
            raise ValueError(f"atlas_filter: normal_power {normal_power} (0 .. 7)")
        sigma_distance, sigma_plane = float(sigma_distance), float(sigma_plane)
        for name, v in (("sigma_distance", sigma_distance), ("sigma_plane", sigma_plane)):
            if not (np.isfinite(v) and v > 0.0):
                raise ValueError(f"atlas_filter: {name} {v} (positive and finite)")
        self._device_tensor("atlas_filter: image", image.view(h * w, -1), 4, "torch.float32")
        self._device_tensor("atlas_filter: texels", texels, 8, "torch.int32")
        if texels.shape[0] != h * w:
            raise ValueError(f"atlas_filter: texels has {texels.shape[0]} rows for {w} x {h} texels")
        import torch
        other = torch.empty_like(image)
        where = []
        self._enqueue_between_streams(image.device, lambda: where.append(self._chk(lib.hs_atlas_filter(
            self._h, _vp(texels.data_ptr()), _vp(image.data_ptr()), _vp(other.data_ptr()), w, h, passes, sigma_distance, sigma_plane,
            normal_power))))
        return other if where[0] else image

    def _lightmap_inputs(self, what, n, charts, chart_first, image, mode, out):
        self._device_tensor(f"{what}: charts", charts, 6, "torch.float32")
        if charts.shape[0] < 1:
            raise ValueError(f"{what}: charts has no rows")
        if not _is_tensor(chart_first) or chart_first.dim() != 1:
            raise ValueError(f"{what}: chart_first: needs an (M,) int32 tensor on the scene's device, one entry per uploaded mesh")
        self._device_tensor(f"{what}: chart_first", chart_first.view(-1, 1) if chart_first.is_contiguous() else chart_first[:, None],
                            1, "torch.int32")
        w, h = self._atlas_image(what, image)
        if n >= 2 ** 31:
            raise ValueError(f"{what}: {n} rows (at most 2^31 - 1 per call)")
        return w, h, LIGHTMAP_MODES[mode], self._out_rows(what, out, n, 8, "torch.int32", image.device, f"{n}")

    def atlas_sample(self, hits, charts, chart_first, image, mode="bilinear", out=None):
        """The baked atlas read at ray hits (ptrt_atlas_sample).  torch tensors on this scene's device, contiguous, read in
        place: `hits`, query_closest's (n, 16) int32 rows; `charts`, (F, 6) float32, the `uv` of atlas_texels for every
        lightmapped mesh, concatenated; `chart_first`, (M,) int32, per uploaded mesh the row of `charts` that holds its face 0,
        negative for a mesh without a lightmap (`lightmap.chart_table` makes both); `image`, the (H, W, 4) float32 atlas
        {r, g, b, valid} that atlas_dilate leaves.  `mode`: 'nearest' -- the texel the hit falls in -- or 'bilinear' -- the
        four texels round it, the invalid ones and those outside the atlas skipped and the rest renormalised.  Returns an
        (n, 8) int32 tensor, one 32-byte `ptrt_lightmap_sample` per row (`lightmap_sample_fields` names the columns): rgb (0:3)
        and the weight of the taps used (3; 0: nothing to sample) as float32 bits, the hit in the atlas in texel units (4, 5,
        float32 bits), the hit's face (6) and mesh (7), -1 on a miss; `out` takes such a tensor.  No synchronisation."""
        if mode not in LIGHTMAP_MODES:
            raise ValueError(f"atlas_sample: mode {mode!r} ('nearest' or 'bilinear')")
        self._device_tensor("atlas_sample: hits", hits, 16, "torch.int32")
        n = int(hits.shape[0])
        w, h, mode, out = self._lightmap_inputs("atlas_sample", n, charts, chart_first, image, mode, out)
        if n == 0:
            return out
        self._enqueue_between_streams(image.device, lambda: self._chk(lib.hs_atlas_sample(
            self._h, _vp(hits.data_ptr()), n, _vp(charts.data_ptr()), int(charts.shape[0]), _vp(chart_first.data_ptr()),
            _vp(image.data_ptr()), w, h, mode, _vp(out.data_ptr()))))
        return out

    def query_lightmap(self, origins, directions, charts, chart_first, image, mode="bilinear", out=None):
        """The baked atlas at the closest hit of every ray (ptrt_query_lightmap): what `atlas_sample(query_closest(origins,
        directions), ..)` returns, byte for byte, from one kernel that never writes the hit records.  origins and directions:
        (n, 3) float32 tensors on this scene's device, contiguous; the rest as for atlas_sample.  A lightmapped view of the
        scene is `camera_rays`, then this, then `lightmap.shade_samples`.  No synchronisation."""
        if mode not in LIGHTMAP_MODES:
            raise ValueError(f"query_lightmap: mode {mode!r} ('nearest' or 'bilinear')")
        self._device_tensor("query_lightmap: origins", origins, 3, "torch.float32")
        self._device_tensor("query_lightmap: directions", directions, 3, "torch.float32")
        n = int(origins.shape[0])
        if directions.shape[0] != n:
            raise ValueError(f"query_lightmap: {n} origins, {directions.shape[0]} directions")
        w, h, mode, out = self._lightmap_inputs("query_lightmap", n, charts, chart_first, image, mode, out)
        if n == 0:
            return out
        self._enqueue_between_streams(image.device, lambda: self._chk(lib.hs_query_lightmap(
            self._h, _vp(origins.data_ptr()), _vp(directions.data_ptr()), n, _vp(charts.data_ptr()), int(charts.shape[0]),
            _vp(chart_first.data_ptr()), _vp(image.data_ptr()), w, h, mode, _vp(out.data_ptr()))))
        return out

    @staticmethod
    def _probe_volume(what, volume, mode, normal_bias):
        """what needs no tensor: (ptrt_probe_volume, its row count, the mode's number, the bias)"""
        if mode not in PROBES_MODES:
            raise ValueError(f"{what}: mode {mode!r} ('trilinear' or 'visibility')")
        try:
            desc = ProbeVolumeDesc((C.c_float * 3)(*[float(x) for x in volume.origin]), (C.c_float * 3)(*[float(x) for x in volume.spacing]),
                                   (C.c_int32 * 3)(*[int(x) for x in volume.counts]))
        except (AttributeError, TypeError, IndexError, ValueError) as e:
            raise ValueError(f"{what}: volume: needs a probes.ProbeVolume (origin, spacing, counts): {e}") from None
        counts = [int(x) for x in desc.counts]
        rows = counts[0] * counts[1] * counts[2]
        if min(counts) < 1 or rows > 2 ** 24:
            raise ValueError(f"{what}: volume: counts {counts} (each >= 1, at most 2^24 probes)")
        if not all(math.isfinite(x) and x > 0.0 for x in desc.spacing) or not all(math.isfinite(x) for x in desc.origin):
            raise ValueError(f"{what}: volume: spacing {list(desc.spacing)} (positive and finite), origin {list(desc.origin)} (finite)")
        normal_bias = float(normal_bias)
        if not (normal_bias >= 0.0 and math.isfinite(normal_bias)):
            raise ValueError(f"{what}: normal_bias {normal_bias} (>= 0 and finite)")
        return desc, rows, PROBES_MODES[mode], normal_bias

    def _probe_tensors(self, what, n, rows, probes, out):
        self._device_tensor(f"{what}: probes", probes, 32, "torch.float32")
        if probes.shape[0] != rows:
            raise ValueError(f"{what}: probes has {probes.shape[0]} rows for a volume of {rows} probes")
        if n >= 2 ** 31:
            raise ValueError(f"{what}: {n} rows (at most 2^31 - 1 per call)")
        return self._out_rows(what, out, n, 8, "torch.int32", probes.device, f"{n}")

    def probe_sample(self, positions, normals, volume, probes, mode="visibility", normal_bias=0.0, out=None):
        """A probe volume read at surface points (ptrt_probe_sample).  torch tensors on this scene's device, contiguous, read
        in place: `positions` and `normals`, (n, 3) float32 (normals are used as given: pass unit ones); `probes`, the
        (nx * ny * nz, 32) float32 rows query_probes returns for `volume.positions()`.  `volume`: a `probes.ProbeVolume`.
        `mode`: 'trilinear' -- the eight probes round the point by their trilinear weights -- or 'visibility' -- each weight
        multiplied further by how far the probe faces the normal and by a Chebyshev test of the probe's two distance moments
        against its distance from the point moved `normal_bias` along its normal, so that a probe behind a wall counts for
        little.  Returns an (n, 8) int32 tensor, one 32-byte `ptrt_probe_light` per row (`probes.probe_light_fields` names the
        columns): the irradiance (0:3) and the weight of the corners used (3; 0: nothing to light with) as float32 bits, the
        footprint's first row (4; -1: the point is not finite), the corners used as bits (5), face and mesh (6, 7; -1 here).
        `out` takes such a tensor.  No synchronisation.  Needs no geometry."""
        desc, rows, mode, normal_bias = self._probe_volume("probe_sample", volume, mode, normal_bias)
        self._device_tensor("probe_sample: positions", positions, 3, "torch.float32")
        self._device_tensor("probe_sample: normals", normals, 3, "torch.float32")
        n = int(positions.shape[0])
        if normals.shape[0] != n:
            raise ValueError(f"probe_sample: {n} positions, {normals.shape[0]} normals")
        out = self._probe_tensors("probe_sample", n, rows, probes, out)
        if n == 0:
            return out
        self._enqueue_between_streams(probes.device, lambda: self._chk(lib.hs_probe_sample(
            self._h, _vp(positions.data_ptr()), _vp(normals.data_ptr()), n, C.byref(desc), _vp(probes.data_ptr()), mode, normal_bias,
            _vp(out.data_ptr()))))
        return out

    def query_probe_light(self, origins, directions, volume, probes, mode="visibility", normal_bias=0.0, out=None):
        """The probe volume's irradiance at the closest hit of every ray (ptrt_query_probe_light): what `probe_sample` returns
        for the point and normal columns of `query_closest(origins, directions)`, byte for byte, from one kernel that never
        writes the hit records; face and mesh (columns 6, 7) are the hit's, and a miss is the row (0, 0, 0, 0, -1, 0, -1, -1).
        origins and directions: (n, 3) float32 tensors on this scene's device, contiguous; the rest as for probe_sample.  A
        probe-lit view of the scene is `camera_rays`, then this, then `probes.shade_probe_light`.  No synchronisation."""
        desc, rows, mode, normal_bias = self._probe_volume("query_probe_light", volume, mode, normal_bias)
        self._device_tensor("query_probe_light: origins", origins, 3, "torch.float32")
        self._device_tensor("query_probe_light: directions", directions, 3, "torch.float32")
        n = int(origins.shape[0])
        if directions.shape[0] != n:
            raise ValueError(f"query_probe_light: {n} origins, {directions.shape[0]} directions")
        out = self._probe_tensors("query_probe_light", n, rows, probes, out)
        if n == 0:
            return out
        self._enqueue_between_streams(probes.device, lambda: self._chk(lib.hs_query_probe_light(
            self._h, _vp(origins.data_ptr()), _vp(directions.data_ptr()), n, C.byref(desc), _vp(probes.data_ptr()), mode, normal_bias,
            _vp(out.data_ptr()))))
        return out

    def camera_rays(self, frame, sample=0):
        """(origins, directions): (rows * width, 3) float32 tensors on this scene's device holding the primary rays
        render_to_device gives sample `sample` of frame `frame`, in the order of `read(BUF_ACCUM)` (ptrt_camera_rays; pinhole
        cameras only).  No synchronisation."""
        import torch
        if self.device < 0:
            self._chk(lib.hs_camera_rays(self._h, int(frame), int(sample), None, None))
        dev = torch.device("cuda", self.device)
        rw, rh = self.renderSize()
        n = self.tile_rows * self.width if (rw, rh) == (self.width, self.height) else rw * rh
        o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self._enqueue_between_streams(dev, lambda: self._chk(lib.hs_camera_rays(
            self._h, int(frame), int(sample), _vp(o.data_ptr()), _vp(d.data_ptr()))))
        return o, d

    def init_rng_states(self, seed, first, n):
        """(n, 6) int32 tensor on this scene's device: fresh generator states for subsequences first .. first + n - 1 of
        `seed` in the canonical order (ptrt_init_rng_states) -- what reset_rng(seed) gives pixel `first + i`."""
        import torch
        if self.device < 0:
            self._chk(lib.hs_init_rng_states(self._h, int(seed), int(first), int(n), None))
        dev = torch.device("cuda", self.device)
        st = torch.empty((int(n), 6), dtype=torch.int32, device=dev)
        if n:
            self._enqueue_between_streams(dev, lambda: self._chk(lib.hs_init_rng_states(
                self._h, int(seed), int(first), int(n), _vp(st.data_ptr()))))
        return st

    def traceSingleRay(self, origin, direction):
        h = Hit()
        self._chk(lib.hs_trace_single_ray(self._h, _f3(origin), _f3(direction), C.byref(h)))
        return h

    def saveAsPPM(self, path, pixels):
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        self._chk(lib.hs_save_ppm(self._h, path.encode(), a.ctypes.data_as(_vp)))

    def serialize(self):
        """Canonical byte stream of the flattened scene (host/ptrt/serialize.hpp)."""
        n = lib.hs_serialize_scene(self._h, None, 0)
        if not n:
            raise PtrtError(lib.hs_last_error().decode())
        buf = (C.c_ubyte * n)()
        lib.hs_serialize_scene(self._h, buf, n)
        return bytes(buf)

    def flatten(self):
        """Pointer to the flattened `ptrt_scene_desc` (host arrays owned by the C++ Scene)."""
        p = lib.hs_flatten(self._h)
        if not p:
            raise PtrtError(lib.hs_last_error().decode())
        return p


class TileFarm:
    """host/ptrt/farm.hpp from Python: one C++ Scene per entry of `devices` (bands, or interleaved 8-row strips),
    their images gathered below the C ABI (ptrt_farm_*: device copies on the presenting GPU, RCCL from the others)."""

    def __init__(self, width, height, devices, strips=False):
        self.width, self.height = int(width), int(height)
        arr = (C.c_int * len(devices))(*devices)
        self._f = lib.hs_farm_create(self.width, self.height, arr, len(devices), int(bool(strips)))
        if not self._f:
            raise PtrtError(lib.hs_last_error().decode())
        self.scenes = [Scene._borrowed(lib.hs_farm_scene(self._f, i), width, height, devices[i]) for i in range(len(devices))]

    @property
    def transport(self):
        return lib.hs_farm_transport(self._f).decode()

    def render_to_device(self, ptr):
        if lib.hs_farm_render(self._f, ptr, 1) < 0:
            raise PtrtError(lib.hs_last_error().decode())

    def render_to_host(self):
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        if lib.hs_farm_render(self._f, out.ctypes.data_as(_vp), 0) < 0:
            raise PtrtError(lib.hs_last_error().decode())
        return out

    @property
    def host_us(self):
        """Host time (us) the calling thread spent inside the last render (every part's enqueue + the gather's calls)."""
        return float(lib.hs_farm_host_us(self._f))

    def set_parallel(self, on):
        if lib.hs_farm_set_parallel(self._f, int(bool(on))) < 0:
            raise PtrtError(lib.hs_last_error().decode())

    def sync(self):
        if lib.hs_farm_sync(self._f) < 0:
            raise PtrtError(lib.hs_last_error().decode())

    def close(self):
        if getattr(self, "_f", None):
            for s in self.scenes:
                s.close()
            lib.hs_farm_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


from . import baked, cameras, lightmap, probes, scenes  # noqa: E402,F401
