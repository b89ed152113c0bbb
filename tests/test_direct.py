"""Direct light at lightmap texels (ptrt_query_direct, ptrt_direct_rays; Scene.query_direct; ptrt_amd.lightmap), without a GPU:
the entry points are declared and exported, the record is 32 bytes, the binding checks its arguments, the mirror's methods
compile into a caller of host/ptrt/scene.hpp, the helpers of ptrt_amd.lightmap are what they say, the float32 sum order of
tests/direct_restatement.py stays within its first-order bound of the same sums in float64, the float64 statement decides
(nearly) every sample of the inputs the GPU test compares with it, and the host mirror's traces still build."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import direct_restatement as D
import irradiance_restatement as R
import path_truth as PT
from test_capi_symbols import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported(P):
    names = declared()
    for n in ("ptrt_query_direct", "ptrt_direct_rays"):
        assert n in names, f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n), f"{n} declared in include/ptrt.h but not exported"
    assert hasattr(P.lib, "hs_query_direct") and hasattr(P.lib, "hs_direct_rays")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    for n in ("Direct", "DIRECT_DTYPE", "DIRECT_COLUMNS", "direct_fields"):
        assert hasattr(P, n)
    for n in ("direct_irradiance", "penumbra_texels", "total_irradiance"):
        assert hasattr(P.lightmap, n)


def test_record_is_32_bytes(P):
    assert C.sizeof(P.Direct) == 32 and P.DIRECT_DTYPE.itemsize == 32
    assert (P.Direct.irradiance.offset, P.Direct.lit_fraction.offset, P.Direct.shadowed_fraction.offset,
            P.Direct.reserved.offset) == (0, 12, 16, 20)
    cols = sorted(P.DIRECT_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b) in P.DIRECT_COLUMNS.items():
        assert P.DIRECT_DTYPE.fields[name][1] == 4 * a == getattr(P.Direct, name).offset
    import torch
    f = P.direct_fields(torch.arange(16, dtype=torch.float32).reshape(2, 8))
    assert f["irradiance"].shape == (2, 3) and f["lit_fraction"].tolist() == [3.0, 11.0]
    assert f["shadowed_fraction"].tolist() == [4.0, 12.0] and f["reserved"].shape == (2, 3)


def test_null_context_is_invalid(P):
    buf = (C.c_float * 64)()
    off = C.c_float(1e-4)
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_query_direct(ctx, buf, buf, 1, buf, 1, None, off, 0, 0, buf) == -1
        assert b"ptrt_query_direct" in P.lib.ptrt_last_error(stale)
        assert P.lib.ptrt_direct_rays(ctx, buf, buf, 1, buf, 1, None, off, 0, 0, buf, buf, buf, buf) == -1
        assert b"ptrt_direct_rays" in P.lib.ptrt_last_error(stale)


def test_binding_checks_arguments(P):
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    assert s.lightCount() == 1
    pos, nrm = torch.zeros(2, 3), torch.zeros(2, 3)
    s2 = torch.zeros(4, 2)
    for args in [(np.zeros((2, 3), np.float32), nrm, s2), (pos, nrm, s2), (pos, nrm, None),     # numpy; not on a device
                 (pos.double(), nrm, s2), (pos, nrm.double(), s2), (pos, nrm, s2.double()),
                 (pos, nrm, s2[:, :1]), (pos, nrm[:, :2], s2)]:
        with pytest.raises(ValueError):
            s.query_direct(*args)
        with pytest.raises(ValueError):
            s.direct_rays(*args)
    with pytest.raises(ValueError):
        s.query_direct(pos, nrm, s2, phases=np.zeros(2, np.float32))
    for bad in ((-1, 1), (0, 2), (1, 1), (0, -1), (2, 0), 3, (0,)):
        with pytest.raises(ValueError, match="lights"):
            s.query_direct(pos, nrm, s2, lights=bad)
        with pytest.raises(ValueError, match="lights"):
            s.direct_rays(pos, nrm, s2, lights=bad)
    s.close()


def test_mirror_methods_compile_and_refuse_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses Scene::queryDirect and Scene::directRays; on a host-only Scene they throw."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/llvm/bin/clang++"
    pkg = os.path.dirname(os.path.dirname(P.__file__))
    src = tmp_path / "caller.cpp"
    src.write_text("""
#include "ptrt/scene.hpp"
#include <cstddef>
#include <stdexcept>
static_assert(sizeof(ptrt_direct) == 32, "ptrt_direct is 32 bytes");
static_assert(offsetof(ptrt_direct, lit_fraction) == 12 && offsetof(ptrt_direct, shadowed_fraction) == 16 &&
              offsetof(ptrt_direct, reserved) == 20, "ptrt_direct layout");
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.queryDirect(nullptr, nullptr, 0, nullptr, 1, nullptr, 1e-4f, 0, -1, static_cast<ptrt_direct *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.directRays(nullptr, nullptr, 0, nullptr, 1, nullptr, 1e-4f, 0, 0, nullptr, nullptr, nullptr, nullptr); } catch (const std::runtime_error &) { ++refused; }
    return refused == 2 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0


def test_traces_still_build(P):
    """build/commit_traces links tests/host_mirror/fake_backend.cpp alone: the mirror's new methods live in the class body and
    ask nothing of it.  (tests/test_host_commit_traces.py runs the binary.)"""
    pkg = os.path.dirname(os.path.dirname(P.__file__))
    subprocess.check_call(["make", "-C", pkg, "traces"], stdout=subprocess.DEVNULL)
    assert os.access(os.path.join(pkg, "build", "commit_traces"), os.X_OK)


# ---- ptrt_amd.lightmap -------------------------------------------------------------------------------------------------------
def test_lightmap_helpers(P):
    import torch
    d = np.zeros((4, 8), np.float32)
    d[:, 0:3] = [[1.0, 2.0, 0.5], [0.0, 0.25, 4.0], [3.0, 3.0, 3.0], [0.0, 0.0, 0.0]]
    d[:, 3] = [1.0, 0.5, 0.0, 0.0]     # lit
    d[:, 4] = [0.0, 0.25, 1.0, 0.0]    # shadowed
    E = P.lightmap.direct_irradiance(d)
    assert E.dtype == np.float32 and E.shape == (4, 3) and np.array_equal(E, d[:, 0:3])  # no factor of pi
    assert np.array_equal(P.lightmap.direct_irradiance(torch.from_numpy(d)), E)
    assert P.lightmap.penumbra_texels(d).tolist() == [False, True, False, False]
    g = np.zeros((4, 8), np.float32)
    g[:, 0:3] = [[0.5, 0.5, 0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.125, 0.25, 0.5]]
    total = P.lightmap.total_irradiance(d, g)
    assert total.dtype == np.float32
    assert np.array_equal(total, d[:, 0:3] + np.float32(math.pi) * g[:, 0:3])
    assert np.array_equal(total[2], d[2, 0:3]) and np.array_equal(total[3], P.lightmap.irradiance(g)[3])
    doc = " ".join(P.lightmap.total_irradiance.__doc__.split())
    assert "LACKS" in doc and "one-bounce" in doc and "first hit" in doc
    with pytest.raises(ValueError):
        P.lightmap.total_irradiance(d, g[:3])
    with pytest.raises(ValueError):
        P.lightmap.direct_irradiance(d[:, :6])


# ---- the sum order -----------------------------------------------------------------------------------------------------------
def random_rays(n_shadow, light_count, n=7):
    Q = n_shadow * light_count
    rs = np.random.RandomState(Q)
    w = rs.lognormal(0.0, 2.0, (n * Q, 3)).astype(np.float32)
    dead = rs.uniform(size=n * Q) < 0.2
    w[dead] = 0.0                                            # not walked
    w[rs.uniform(size=n * Q) < 0.05] = np.float32(np.nan)    # nor these
    blocked = (rs.uniform(size=n * Q) < 0.3).astype(np.int32)
    return w, blocked


@pytest.mark.parametrize("n_shadow,light_count", [(1, 1), (1, 3), (2, 3), (4, 6), (16, 4), (16, 6)],
                         ids=["Q=1", "Q=3", "Q=6", "Q=24", "Q=64", "Q=96"])
def test_restatement_stays_within_its_bound_of_float64(n_shadow, light_count):
    """With u = 2^-24, every float32 operation returns its exact result times (1 + e), |e| <= u.  `roundings` = 2: a term is
    an input of the sum as it stands (the weight as ptrt_direct_rays wrote it, or the flag 1.0f) and the total passes through
    one operation behind it (the division); one more is allowed for, as for ptrt_query_irradiance.  The fold adds log2(w)
    levels, each partial sum rounded once and no larger than the sum of the absolute terms below it: log2(w) u per term.
    Adding the chunk sums to the total rounds at most once per chunk: `chunks` u.  Together
        |float32 - exact| <= (2 + log2(w) + chunks) u M_i,   M_i = the sum of the absolute terms under the quantity's divisor,
    and 1.01 covers the second-order terms and the float64 twin's own error."""
    Q = n_shadow * light_count
    w32, blocked = random_rays(n_shadow, light_count)
    got = D.restate(w32, blocked, n_shadow, light_count)
    assert got.shape == (7, 8) and got.dtype == np.float32 and not got[:, 5:].any() and not np.isnan(got).any()
    want = D.restate64(w32, blocked, n_shadow, light_count)
    M = D.magnitudes64(w32, blocked, n_shadow, light_count)
    w = R.width(Q)
    chunks = (Q + w - 1) // w
    bound = (2 + math.log2(w) + chunks) * 2.0 ** -24 * 1.01 * M
    err = np.abs(got[:, :5].astype(np.float64) - want)
    assert (err <= bound).all(), f"worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}"
    if Q >= 3:
        assert (err > 0).any()  # (the comparison is not vacuous: float32 sums do round)
    # the fractions are counts over Q, and together they count the walked samples
    walked = D.walked32(w32).reshape(7, Q)
    assert np.array_equal(got[:, 3] + got[:, 4] > 0, walked.any(axis=1))
    assert np.abs((got[:, 3].astype(np.float64) + got[:, 4]) * Q - walked.sum(axis=1)).max() < 1e-4


def test_restatement_small_cases():
    F = np.float32
    # Q = 3 pads to w = 4 and folds by halves: (v0 + v2) + (v1 + 0); irradiance is over n_shadow, the fractions over Q
    w = np.zeros((3, 3), F)
    w[:, 0] = [1.0, 2.0 ** -24, 2.0 ** -24]
    got = D.restate(w, np.zeros(3, np.int32), 1, 3)
    assert got[0, 0] == (F(1.0) + F(2.0 ** -24)) + (F(2.0 ** -24) + F(0.0)) == F(1.0)
    assert got[0, 3] == F(1.0) and got[0, 4] == F(0.0)
    got = D.restate(w, np.int32([0, 1, 0]), 3, 1)
    assert got[0, 0] == (F(1.0) + F(2.0 ** -24)) / F(3.0) and got[0, 3] == F(2.0) / F(3.0) and got[0, 4] == F(1.0) / F(3.0)
    # a blocked flag on a sample that is not walked counts nowhere; a NaN weight is not walked
    w = np.float32([[0, 0, 0], [np.nan, np.nan, np.nan], [0, 0, 2.0], [-1, 0, 0]])
    got = D.restate(w, np.int32([1, 1, 0, 1]), 4, 1)
    assert got[0].tolist() == [0.0, 0.0, 0.5, 0.25, 0.0, 0.0, 0.0, 0.0]
    assert D.walked32(w).tolist() == [False, False, True, False]


# ---- the float64 statement on the GPU test's inputs ----------------------------------------------------------------------------
def test_statement_decides_the_gpu_tests_inputs(P):
    """tests/test_direct_gpu.py compares ptrt_direct_rays with statement64 on exactly these inputs and leaves out what the
    statement does not decide: at most 2 %."""
    arr, pos, nrm, s2, ph = D.statement_inputs(P)
    nl, k, n = len(D.STATEMENT_LIGHTS), D.STATEMENT_SHADOW, D.STATEMENT_TEXELS
    assert len(s2) == k and len(pos) == n and np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    st, decided = D.statement64(pos, nrm, PT.lights64(arr, nl), 0, nl, s2, ph, k)
    assert decided.shape == (n * nl * k,) and st["L"].shape == st["weight"].shape == (n * nl * k, 3)
    share = 1.0 - decided.mean()
    print(f"statement64: {share:.4f} of {len(decided)} samples undecided")
    assert share <= 0.02
    # the inputs do exercise the statement: walked and not, every kind of light with a positive weight somewhere
    w = st["walked"].reshape(n, nl, k)
    assert 0.3 < w.mean() < 0.95 and w.any(axis=(0, 2)).all() and (~w).any(axis=(0, 2)).all()
    E_L, E_t, E_w = D.margins(st)
    assert np.isfinite(E_L).all() and np.isfinite(E_w).all() and (E_L[~(st["Lt"]["type"] == 1)] > 0).all()
    # a range of lights is the same statement, shifted
    st2, _ = D.statement64(pos, nrm, PT.lights64(arr, nl), 2, 3, s2, ph, k)
    assert np.array_equal(st2["weight"].reshape(n, 3, k, 3), st["weight"].reshape(n, nl, k, 3)[:, 2:5])
