"""The baked-light view's record (ptrt_baked_view, include/ptrt.h): what Scene.render_baked hands ptrt_render_baked, built from
torch tensors so that callers do not assemble pointers.

    view, keep = baked.baked_view(scene, charts=uv, chart_first=first, image=atlas, volume=vol, probes=rows, hdr=hdr)

`view` is the ctypes record, `keep` the tensors it points into (hold them while the record is in use).  A lightmap is
`charts`, `chart_first` and `image` together (lightmap.chart_table makes the first two, Scene.atlas_dilate leaves the third);
a probe volume is `volume` (a probes.ProbeVolume) and `probes` (Scene.query_probes' rows) together; either half may be absent.
Everything is checked here in the order kind, shape, dtype, layout, device -- so a wrong shape is named as such on a scene without a device too.
"""
import ctypes as C
import math

from . import LIGHTMAP_MODES, PROBES_MODES, ProbeVolumeDesc

_vp = C.c_void_p


class BakedView(C.Structure):
    """`ptrt_baked_view`: the inputs and the optional outputs of ptrt_render_baked (host memory; the pointers are device memory)."""
    _fields_ = [("d_charts", _vp), ("n_chart_faces", C.c_int32), ("d_chart_first", _vp),
                ("d_image", _vp), ("atlas_w", C.c_int32), ("atlas_h", C.c_int32), ("lightmap_mode", C.c_int32),
                ("volume", ProbeVolumeDesc), ("d_probes", _vp), ("probe_mode", C.c_int32), ("normal_bias", C.c_float),
                ("d_hdr", _vp), ("d_normal", _vp), ("d_depth", _vp), ("d_object_id", _vp)]


assert C.sizeof(BakedView) == 128


def _tensor(scene, what, a, shape, dtype):
    """`a` is a contiguous torch tensor of `shape` (None: any extent) and `dtype`, or a ValueError says which of these it is
    not; `_on_device` looks at where it lives, after everything else about the call has passed."""
    if not (hasattr(a, "data_ptr") and hasattr(a, "is_contiguous")):
        raise ValueError(f"render_baked: {what}: needs a torch tensor on the scene's device, got {type(a).__name__}")
    want = "(" + ", ".join("n" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"
    if a.dim() != len(shape) or any(s is not None and int(t) != s for s, t in zip(shape, a.shape)):
        raise ValueError(f"render_baked: {what}: shape {tuple(a.shape)}, expected {want}")
    if str(a.dtype) != dtype:
        raise ValueError(f"render_baked: {what}: dtype {a.dtype}, expected {dtype}")
    if not a.is_contiguous():
        raise ValueError(f"render_baked: {what}: tensors must be contiguous")
    return a


def _on_device(scene, what, a):
    if a.device.type != "cuda" or a.device.index != scene.device:
        raise ValueError(f"render_baked: {what}: tensor on {a.device}, this scene renders on " +
                         (f"cuda:{scene.device}" if scene.device >= 0 else "no device (host-only)"))


def baked_view(scene, *, charts=None, chart_first=None, image=None, lightmap_mode="bilinear", volume=None, probes=None,
               probe_mode="visibility", normal_bias=0.0, hdr=None, normal=None, depth=None, object_id=None):
    """(BakedView, the tensors it points into).  `scene`: the ptrt_amd.Scene that will render -- its device and the pixels of
    its rows (tile_rows * width = n) size the checks.  charts (F, 6) float32, chart_first (M,) int32, image (H, W, 4) float32;
    probes (volume.rows, 32) float32; hdr and normal (n, 3) float32, depth (n,) float32, object_id (n,) int32."""
    v = BakedView()
    keep = []  # (name, tensor)
    if lightmap_mode not in LIGHTMAP_MODES:
        raise ValueError(f"render_baked: lightmap_mode {lightmap_mode!r} ('nearest' or 'bilinear')")
    if probe_mode not in PROBES_MODES:
        raise ValueError(f"render_baked: probe_mode {probe_mode!r} ('trilinear' or 'visibility')")
    half = [charts is not None, chart_first is not None, image is not None]
    if any(half) and not all(half):
        raise ValueError("render_baked: a lightmap is charts, chart_first and image together")
    if (volume is None) != (probes is None):
        raise ValueError("render_baked: a probe volume is volume and probes together")
    n = scene.tile_rows * scene.width
    if image is not None:
        _tensor(scene, "charts", charts, (None, 6), "torch.float32")
        if charts.shape[0] < 1:
            raise ValueError("render_baked: charts has no rows")
        _tensor(scene, "chart_first", chart_first, (None,), "torch.int32")
        _tensor(scene, "image", image, (None, None, 4), "torch.float32")
        h, w = int(image.shape[0]), int(image.shape[1])
        if h < 1 or w < 1 or h * w > 2 ** 28:
            raise ValueError(f"render_baked: a {w} x {h} atlas (1 x 1 .. 2^28 texels)")
        v.d_charts, v.n_chart_faces, v.d_chart_first = charts.data_ptr(), int(charts.shape[0]), chart_first.data_ptr()
        v.d_image, v.atlas_w, v.atlas_h, v.lightmap_mode = image.data_ptr(), w, h, LIGHTMAP_MODES[lightmap_mode]
        keep += [("charts", charts), ("chart_first", chart_first), ("image", image)]
    if probes is not None:
        try:
            desc = ProbeVolumeDesc((C.c_float * 3)(*[float(x) for x in volume.origin]), (C.c_float * 3)(*[float(x) for x in volume.spacing]),
                                   (C.c_int32 * 3)(*[int(x) for x in volume.counts]))
        except (AttributeError, TypeError, IndexError, ValueError) as e:
            raise ValueError(f"render_baked: volume: needs a probes.ProbeVolume (origin, spacing, counts): {e}") from None
        counts = [int(x) for x in desc.counts]
        rows = counts[0] * counts[1] * counts[2]
        if min(counts) < 1 or rows > 2 ** 24:
            raise ValueError(f"render_baked: volume: counts {counts} (each >= 1, at most 2^24 probes)")
        if not all(math.isfinite(x) and x > 0.0 for x in desc.spacing) or not all(math.isfinite(x) for x in desc.origin):
            raise ValueError(f"render_baked: volume: spacing {list(desc.spacing)} (positive and finite), origin {list(desc.origin)} (finite)")
        normal_bias = float(normal_bias)
        if not (normal_bias >= 0.0 and math.isfinite(normal_bias)):
            raise ValueError(f"render_baked: normal_bias {normal_bias} (>= 0 and finite)")
        _tensor(scene, "probes", probes, (rows, 32), "torch.float32")
        v.volume, v.d_probes, v.probe_mode, v.normal_bias = desc, probes.data_ptr(), PROBES_MODES[probe_mode], normal_bias
        keep.append(("probes", probes))
    for name, a, shape, dtype in (("hdr", hdr, (n, 3), "torch.float32"), ("normal", normal, (n, 3), "torch.float32"),
                                  ("depth", depth, (n,), "torch.float32"), ("object_id", object_id, (n,), "torch.int32")):
        if a is not None:
            setattr(v, "d_" + name, _tensor(scene, name, a, shape, dtype).data_ptr())
            keep.append((name, a))
    for name, a in keep:
        _on_device(scene, name, a)
    return v, [a for _, a in keep]
