"""Path-traced radiance for caller-supplied rays, without a GPU: the three entry points are declared and exported, the
record is 32 bytes, the binding checks its arguments and refuses a host-only scene, the mirror's methods compile into a caller
of host/ptrt/scene.hpp, and the panorama camera of ptrt_amd.cameras makes the rays it says it makes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptrt_query_radiance", "ptrt_camera_rays", "ptrt_init_rng_states")


def test_symbols_are_declared_and_exported(P):
    src = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ptrt_[a-z_0-9]+)\s*\(", src))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/ptrt.h"
        assert hasattr(P.lib, name), f"{name} declared in include/ptrt.h but not exported"
    assert re.search(r"typedef struct ptrt_radiance \{[^}]*\} ptrt_radiance;", src)
    assert P.lib.ptrt_abi_version() == 6  # additions only


def test_record_is_32_bytes(P):
    assert C.sizeof(P.Radiance) == 32 and P.RADIANCE_DTYPE.itemsize == 32
    assert (P.Radiance.radiance.offset, P.Radiance.depth.offset, P.Radiance.normal.offset, P.Radiance.object_id.offset) == (0, 12, 16, 28)
    cols = sorted(P.RADIANCE_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b, is_f) in P.RADIANCE_COLUMNS.items():
        assert P.RADIANCE_DTYPE.fields[name][1] == 4 * a == getattr(P.Radiance, name).offset
        assert (P.RADIANCE_DTYPE.fields[name][0].base == np.float32) == is_f


def test_null_context_is_invalid(P):
    buf = (C.c_float * 64)()
    assert P.lib.ptrt_query_radiance(None, buf, buf, buf, 1, 1, 4, buf) == -1
    assert P.lib.ptrt_camera_rays(None, 0, 0, buf, buf) == -1
    assert P.lib.ptrt_init_rng_states(None, 1, 0, 1, buf) == -1
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    assert P.lib.ptrt_query_radiance(stale, buf, buf, buf, 1, 1, 4, buf) == -1
    assert b"ptrt_query_radiance" in P.lib.ptrt_last_error(stale)


def test_binding_checks_arguments_and_host_only_scenes_refuse(P):
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    o = torch.zeros(4, 3)
    st = torch.zeros(4, 6, dtype=torch.int32)
    for args in [(np.zeros((4, 3), np.float32), o, st), (o, o, st),                   # numpy; not on a device
                 (o.double(), o, st), (o, o, st.float()), (o[:, :2], o, st)]:
        with pytest.raises(ValueError):
            s.query_radiance(*args)
    with pytest.raises(P.PtrtError):
        s.camera_rays(0)
    with pytest.raises(P.PtrtError):
        s.init_rng_states(1, 0, 4)
    s.close()


def test_equirect_rays(P):
    import torch
    W, H = 16, 8
    o, d = P.cameras.equirect_rays(W, H, (1.0, 2.0, -3.0), "cpu")
    assert o.shape == d.shape == (H * W, 3) and o.dtype == d.dtype == torch.float32
    assert o.device.type == d.device.type == "cpu" and o.is_contiguous() and d.is_contiguous()
    assert torch.equal(o, torch.tensor([1.0, 2.0, -3.0]).expand(H * W, 3))
    # unit length to float32 precision: three squares of numbers <= 1, each within 2^-24 relative
    assert (d.double().norm(dim=1) - 1.0).abs().max().item() <= 2.0 ** -22
    img = d.reshape(H, W, 3)
    # row 0 looks up, the last row down, rows in between descend; every ray of a row has the row's elevation
    assert (img[0, :, 1] > 0.9).all() and (img[-1, :, 1] < -0.9).all()
    assert (img[:-1, 0, 1] > img[1:, 0, 1]).all()
    assert (img[:, :, 1] - img[:, :1, 1]).abs().max().item() <= 2.0 ** -22
    assert torch.allclose(img[0, :, 1], torch.full((W,), math.cos(math.pi * 0.5 / H)), atol=1e-6)
    # column order: the azimuth atan2(z, x) runs from -pi to pi with x, through the pixel centres
    az = torch.atan2(img[:, :, 2].double(), img[:, :, 0].double())
    want = (torch.arange(W, dtype=torch.float64) + 0.5) * (2.0 * math.pi / W) - math.pi
    assert (az - want[None, :]).abs().max().item() <= 1e-6
    # the inverse of the sky's environment-map lookup: pixel (x, y) looks at texel ((x + 0.5) / W, (y + 0.5) / H)
    u = (az + math.pi) / (2.0 * math.pi)
    v = torch.acos(img[:, :, 1].double().clamp(-1, 1)) / math.pi
    assert (u - ((torch.arange(W) + 0.5) / W)[None, :]).abs().max().item() <= 1e-6
    assert (v - ((torch.arange(H) + 0.5) / H)[:, None]).abs().max().item() <= 1e-6
    # defaults, and a size that is not square or even
    o1, d1 = P.cameras.equirect_rays(5, 3)
    assert o1.shape == (15, 3) and not o1.any() and d1.shape == (15, 3)
    with pytest.raises(ValueError):
        P.cameras.equirect_rays(0, 4)


def test_mirror_methods_compile_and_refuse_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses the three methods; on a host-only Scene they throw (no device to query on)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/llvm/bin/clang++"
    pkg = os.path.dirname(os.path.dirname(P.__file__))
    src = tmp_path / "caller.cpp"
    src.write_text("""
#include "ptrt/scene.hpp"
#include <stdexcept>
static_assert(sizeof(ptrt_radiance) == 32, "ptrt_radiance is 32 bytes");
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.queryRadiance(nullptr, nullptr, nullptr, 0, 1, 4, static_cast<ptrt_radiance *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.cameraRays(0, 0, nullptr, nullptr); } catch (const std::runtime_error &) { ++refused; }
    try { s.initRngStates(12345ull, 0ull, 0, nullptr); } catch (const std::runtime_error &) { ++refused; }
    return refused == 3 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0
