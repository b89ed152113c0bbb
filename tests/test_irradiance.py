"""Lightmap texels (ptrt_query_irradiance, ptrt_irradiance_rays; Scene.query_irradiance; ptrt_amd.lightmap), without a GPU: the
entry points are declared and exported, the record is 32 bytes, the binding checks its arguments, the mirror's methods compile
into a caller of host/ptrt/scene.hpp, the helpers of ptrt_amd.lightmap are what they say, and the float32 sum order of
tests/irradiance_restatement.py stays within its first-order bound of the same sums in float64 and is the probes' order where
the two contracts meet."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import irradiance_restatement as R
import probe_restatement as PR
from test_capi_symbols import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported(P):
    names = declared()
    for n in ("ptrt_query_irradiance", "ptrt_irradiance_rays"):
        assert n in names, f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n), f"{n} declared in include/ptrt.h but not exported"
    assert hasattr(P.lib, "hs_query_irradiance") and hasattr(P.lib, "hs_irradiance_rays")
    assert P.lib.ptrt_abi_version() == 6  # additions only


def test_record_is_32_bytes(P):
    assert C.sizeof(P.Irradiance) == 32 and P.IRRADIANCE_DTYPE.itemsize == 32
    assert (P.Irradiance.radiance.offset, P.Irradiance.mean_distance.offset, P.Irradiance.mean_distance_sq.offset,
            P.Irradiance.hit_fraction.offset, P.Irradiance.reserved.offset) == (0, 12, 16, 20, 24)
    cols = sorted(P.IRRADIANCE_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b) in P.IRRADIANCE_COLUMNS.items():
        assert P.IRRADIANCE_DTYPE.fields[name][1] == 4 * a == getattr(P.Irradiance, name).offset
    import torch
    f = P.irradiance_fields(torch.arange(16, dtype=torch.float32).reshape(2, 8))
    assert f["radiance"].shape == (2, 3) and f["hit_fraction"].tolist() == [5.0, 13.0] and f["reserved"].shape == (2, 2)


def test_null_context_is_invalid(P):
    buf = (C.c_float * 64)()
    off = C.c_float(1e-4)
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_query_irradiance(ctx, buf, buf, 1, buf, 1, None, off, buf, 1, 4, C.c_float(1.0), buf) == -1
        assert b"ptrt_query_irradiance" in P.lib.ptrt_last_error(stale)
        assert P.lib.ptrt_irradiance_rays(ctx, buf, buf, 1, buf, 1, None, off, buf, buf) == -1
        assert b"ptrt_irradiance_rays" in P.lib.ptrt_last_error(stale)


def test_binding_checks_arguments(P):
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    pos, nrm = torch.zeros(2, 3), torch.zeros(2, 3)
    s2 = torch.zeros(4, 2)
    st = torch.zeros(8, 6, dtype=torch.int32)
    for args in [(np.zeros((2, 3), np.float32), nrm, s2, st), (pos, nrm, s2, st),          # numpy; not on a device
                 (pos.double(), nrm, s2, st), (pos, nrm.double(), s2, st), (pos, nrm, s2, st.float()),
                 (pos, nrm, s2[:, :1], st), (pos, nrm[:, :2], s2, st)]:
        with pytest.raises(ValueError):
            s.query_irradiance(*args)
        with pytest.raises(ValueError):
            s.irradiance_rays(*args[:3])
    with pytest.raises(ValueError):
        s.query_irradiance(pos, nrm, s2, st, phases=np.zeros(2, np.float32))
    s.close()


def test_mirror_methods_compile_and_refuse_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses Scene::queryIrradiance and Scene::irradianceRays; on a host-only Scene they throw."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/llvm/bin/clang++"
    pkg = os.path.dirname(os.path.dirname(P.__file__))
    src = tmp_path / "caller.cpp"
    src.write_text("""
#include "ptrt/scene.hpp"
#include <cstddef>
#include <stdexcept>
static_assert(sizeof(ptrt_irradiance) == 32, "ptrt_irradiance is 32 bytes");
static_assert(offsetof(ptrt_irradiance, mean_distance) == 12 && offsetof(ptrt_irradiance, reserved) == 24, "ptrt_irradiance layout");
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.queryIrradiance(nullptr, nullptr, 0, nullptr, 1, nullptr, 1e-4f, nullptr, 1, 4, 1e30f, static_cast<ptrt_irradiance *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.irradianceRays(nullptr, nullptr, 0, nullptr, 1, nullptr, 1e-4f, nullptr, nullptr); } catch (const std::runtime_error &) { ++refused; }
    return refused == 2 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0


# ---- ptrt_amd.lightmap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 16, 64, 130, 4096])
def test_hammersley2_is_in_range_and_without_duplicates(P, n):
    p = P.lightmap.hammersley2(n)
    assert p.shape == (n, 2) and p.dtype == np.float32 and p.flags["C_CONTIGUOUS"]
    assert (p >= 0).all() and (p < 1).all()
    assert len(np.unique(p, axis=0)) == n
    # one point per stratum of width 1 / n in the first coordinate; the second is the base-2 radical inverse
    assert np.array_equal(np.floor(p[:, 0].astype(np.float64) * n).astype(int), np.arange(n))
    assert p[:min(n, 4), 1].tolist() == [0.0, 0.5, 0.25, 0.75][:min(n, 4)]
    with pytest.raises(ValueError):
        P.lightmap.hammersley2(0)


def test_texel_phases(P):
    a, b = P.lightmap.texel_phases(1000, 7), P.lightmap.texel_phases(1000, 7)
    assert a.shape == (1000,) and a.dtype == np.float32 and np.array_equal(a, b)
    assert (a >= 0).all() and (a < 1).all() and len(np.unique(a)) > 990
    assert not np.array_equal(a, P.lightmap.texel_phases(1000, 8)) and P.lightmap.texel_phases(0).shape == (0,)


def test_quad_texels(P):
    pos, nrm = P.lightmap.quad_texels((-5.0, -5.0, -10.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), 4, 2)  # a floor, 4 x 2 texels
    assert pos.shape == nrm.shape == (8, 3) and pos.dtype == nrm.dtype == np.float32
    assert np.array_equal(pos[:4, 0], np.float32([-3.75, -1.25, 1.25, 3.75])) and (pos[:, 1] == -5).all()  # u runs fastest
    assert np.array_equal(pos[::4, 2], np.float32([-7.5, -2.5]))
    assert np.array_equal(nrm, np.tile(np.float32([0, -1, 0]), (8, 1)))  # eu x ev
    pos, nrm = P.lightmap.quad_texels((0, 0, 0), (0.0, 0.0, 10.0), (10.0, 0.0, 0.0), 1, 1)
    assert np.array_equal(pos, np.float32([[5, 0, 5]])) and np.array_equal(nrm, np.float32([[0, 1, 0]]))
    # a tilted quad: a unit normal at right angles to both edges
    eu, ev = np.array([1.0, 2.0, 0.5]), np.array([-0.3, 0.4, 2.0])
    pos, nrm = P.lightmap.quad_texels((1, 2, 3), eu, ev, 3, 5)
    n64 = nrm[0].astype(np.float64)
    assert abs(np.linalg.norm(n64) - 1.0) <= 2.0 ** -22 and abs(n64 @ eu) <= 1e-6 and abs(n64 @ ev) <= 1e-6
    assert np.allclose(pos.astype(np.float64).mean(axis=0), np.array([1, 2, 3]) + 0.5 * eu + 0.5 * ev, atol=1e-6)
    for bad in ((0, 1), (1, 0)):
        with pytest.raises(ValueError):
            P.lightmap.quad_texels((0, 0, 0), eu, ev, *bad)
    with pytest.raises(ValueError):
        P.lightmap.quad_texels((0, 0, 0), eu, 2.0 * eu, 2, 2)


def test_irradiance_and_invalid_texels(P):
    import torch
    rows = np.zeros((3, 8), np.float32)
    rows[:, 0:3] = [[1.0, 2.0, 0.5], [0.0, 0.25, 4.0], [3.0, 3.0, 3.0]]
    rows[:, 3] = [0.01, 5.0, 0.01]
    rows[:, 5] = [1.0, 1.0, 0.75]
    E = P.lightmap.irradiance(rows)
    assert E.dtype == np.float32 and np.array_equal(E, np.float32(math.pi) * rows[:, 0:3])
    assert np.array_equal(P.lightmap.irradiance(torch.from_numpy(rows)), E)
    assert P.lightmap.invalid_texels(rows, 0.1).tolist() == [True, False, False]
    with pytest.raises(ValueError):
        P.lightmap.irradiance(rows[:, :6])


# ---- the sum order -----------------------------------------------------------------------------------------------------------
def random_records(n_dirs, n=7):
    rs = np.random.RandomState(n_dirs)
    L = rs.lognormal(0.0, 2.0, (n * n_dirs, 3)).astype(np.float32)
    L[rs.uniform(size=L.shape) < 0.2] = 0.0
    depth = rs.uniform(0.1, 20.0, n * n_dirs).astype(np.float32)
    oid = rs.randint(-1, 5, n * n_dirs).astype(np.int32)
    depth[oid < 0] = np.float32(1e30)
    return L, depth, oid


@pytest.mark.parametrize("n_dirs", [1, 2, 3, 5, 16, 17, 33, 63, 64, 65, 130, 1000])
def test_restatement_stays_within_its_bound_of_float64(n_dirs):
    """With u = 2^-24, every float32 operation returns its exact result times (1 + e), |e| <= u.  `roundings` = 2: a term
    passes through at most one operation before it is summed (dist * dist; the minimum, the radiance as read from the ray's
    record and the hit flag are exact), and the total through one after (the division).  The fold adds log2(w) levels, each
    partial sum rounded once and no larger than the sum of the absolute terms below it: log2(w) u per term.  Adding the chunk
    sums to the total rounds at most once per chunk: `chunks` u.  Together
        |float32 - exact| <= (roundings + log2(w) + chunks) u M_i,   M_i = the mean over k of the absolute terms,
    and 1.01 covers the second-order terms ((2 + 6 + 16) u is 1.5e-6) and the float64 twin's own error."""
    L, depth, oid = random_records(n_dirs)
    n = 7
    maxd = np.float32(12.3)
    got = R.restate(L, depth, oid, n_dirs, maxd)
    assert got.shape == (n, 8) and got.dtype == np.float32 and not got[:, 6:].any()
    want = R.restate64(L, depth, oid, n_dirs, maxd)
    M = R.magnitudes64(L, depth, n_dirs, maxd)
    w = R.width(n_dirs)
    chunks = (n_dirs + w - 1) // w
    roundings = 2
    bound = (roundings + math.log2(w) + chunks) * 2.0 ** -24 * 1.01 * M
    err = np.abs(got[:, :6].astype(np.float64) - want)
    assert (err <= bound).all(), f"worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}"
    if n_dirs >= 3:
        assert (err > 0).any()  # (the comparison is not vacuous: float32 sums do round)
    if n_dirs >= 33:  # the sums are not the naive left-to-right ones: the fold order is what the kernel computes
        t = R.terms32(L, depth, oid, n_dirs, maxd)
        naive = np.zeros((n, 6), np.float32)
        for k in range(n_dirs):
            naive = naive + t[:, k]
        assert not np.array_equal((naive / np.float32(n_dirs)).view(np.uint32), got[:, :6].view(np.uint32))


def test_widths():
    assert [R.width(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 100000)] == \
        [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64, 64, 64]


@pytest.mark.parametrize("n_dirs", [64, 128, 130])
def test_the_fold_is_the_probes_fold_at_64(n_dirs):
    """For w = 64 the order is ptrt_query_probes's: the same terms through probe_restatement.fold64, chunk by chunk."""
    L, depth, oid = random_records(n_dirs)
    maxd = np.float32(9.0)
    t = R.terms32(L, depth, oid, n_dirs, maxd)
    n = t.shape[0]
    chunks = (n_dirs + 63) // 64
    padded = np.zeros((n, chunks * 64, 6), np.float32)
    padded[:, :n_dirs] = t
    total = np.zeros((n, 6), np.float32)
    for c in range(chunks):
        chunk = padded[:, c * 64:(c + 1) * 64]
        assert np.array_equal(R.fold(chunk).view(np.uint32), PR.fold64(chunk).view(np.uint32))
        total = total + PR.fold64(chunk)
    got = R.restate(L, depth, oid, n_dirs, maxd)
    assert np.array_equal(got[:, :6].view(np.uint32), (total / np.float32(n_dirs)).view(np.uint32))
    # and the three quantities the two records share are the probes' own bits: the distances and the hit fraction
    d = np.zeros((n_dirs, 3), np.float32)
    probe = PR.restate(L, depth, oid, d, n_dirs, maxd)
    assert np.array_equal(got[:, 3:6].view(np.uint32), probe[:, 27:30].view(np.uint32))


def test_small_widths_fold_by_halves():
    """n_dirs = 3 pads to w = 4: (v0 + v2) + (v1 + 0).  With v = (1, 2^-24, 2^-24) every sum that starts at 1 stays 1 (ties to
    even), while v0 + (v1 + v2) -- a fold that paired neighbours -- is 1 + 2^-23."""
    L = np.zeros((3, 3), np.float32)
    L[:, 0] = [1.0, 2.0 ** -24, 2.0 ** -24]
    got = R.restate(L, np.ones(3, np.float32), np.zeros(3, np.int32), 3, 10.0)
    by_halves = (np.float32(1.0) + np.float32(2.0 ** -24)) + (np.float32(2.0 ** -24) + np.float32(0.0))
    in_order = (np.float32(1.0) + np.float32(2.0 ** -24)) + np.float32(2.0 ** -24)
    pairs_first = np.float32(1.0) + (np.float32(2.0 ** -24) + np.float32(2.0 ** -24))
    assert by_halves == in_order == np.float32(1.0) and pairs_first != np.float32(1.0)
    assert got[0, 0] == by_halves / np.float32(3.0)
    assert got[0, 3] == np.float32(1.0) and got[0, 5] == np.float32(1.0)
