"""Batched ray queries without a GPU: the binding's argument checks, the host-only refusal, the C entry's NULL context, and
the mirror's Scene::queryClosestDevice / queryOccludedDevice compiled into a caller of host/ptrt/scene.hpp."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture
def host_scene(P):
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    yield s
    s.close()


def test_binding_rejects_bad_shapes_and_dtypes(P, host_scene):
    import torch
    s = host_scene
    o = np.zeros((4, 3), np.float32)
    t = np.ones(4, np.float32)
    bad = [((np.zeros((4, 2), np.float32), o), {}), ((o, np.zeros((4, 3, 1), np.float32)), {}), ((o.ravel(), o), {}),
           ((o, o[:3]), {}), ((o.astype(np.float64), o), {}), ((o, o.astype(np.float16)), {}),
           ((torch.zeros(4, 3), o), {}), ((list(o), o), {}),
           ((torch.zeros(4, 3), torch.zeros(4, 3)), {}),                      # not on the scene's device
           ((torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3)), {})]
    for args, _ in bad:
        with pytest.raises(ValueError):
            s.query_closest(*args)
    for tm in (t[:3], t.reshape(4, 1), t.astype(np.float64), None):
        with pytest.raises(ValueError):
            s.query_occluded(o, o, tm)
    with pytest.raises(ValueError):
        s.query_occluded(o, o[:2], t[:2])


def test_host_only_scene_raises(P, host_scene):
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(P.PtrtError):
        host_scene.query_closest(o, o)
    with pytest.raises(P.PtrtError):
        host_scene.query_occluded(o, o, np.ones(4, np.float32))


def test_null_context_is_invalid(P):
    buf = (C.c_float * 12)()
    assert P.lib.ptrt_query_rays(None, P.QUERY_CLOSEST, buf, buf, None, 4, buf) == -1
    assert P.lib.ptrt_query_rays(None, P.QUERY_OCCLUDED, buf, buf, buf, 4, buf) == -1
    assert P.lib.ptrt_query_rays(None, 0, None, None, None, 0, None) == -1
    assert P.QUERY_CLOSEST == 0 and P.QUERY_OCCLUDED == 1


def test_hit_columns_cover_the_record(P):
    cols = sorted(P.HIT_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 16 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b, is_f) in P.HIT_COLUMNS.items():
        assert P.HIT_DTYPE.fields[name][1] == 4 * a
        assert (P.HIT_DTYPE.fields[name][0].base == np.float32) == is_f


def test_mirror_methods_compile_and_refuse_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses both query methods; on a host-only Scene they throw (no device to query on)."""
    import os
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
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.queryClosestDevice(nullptr, nullptr, 0, static_cast<ptrt_hit *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.queryOccludedDevice(nullptr, nullptr, nullptr, 0, static_cast<int32_t *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    return refused == 2 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0
