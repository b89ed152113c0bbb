"""Light probes (ptrt_query_probes; Scene.query_probes; ptrt_amd.probes), without a GPU: the entry point is declared and
exported, the record is 128 bytes, the binding checks its arguments, the mirror's method compiles into a caller of
host/ptrt/scene.hpp, the helpers of ptrt_amd.probes are what they say -- unit directions, an orthonormal basis, the cosine
lobe's irradiance -- and the float32 sum order of tests/probe_restatement.py stays within its first-order bound of the same
sums in float64."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import probe_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_exported(P):
    src = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ptrt_[a-z_0-9]+)\s*\(", src))
    assert "ptrt_query_probes" in declared, "ptrt_query_probes is not declared in include/ptrt.h"
    assert hasattr(P.lib, "ptrt_query_probes"), "ptrt_query_probes declared in include/ptrt.h but not exported"
    assert hasattr(P.lib, "hs_query_probes")
    assert re.search(r"typedef struct ptrt_probe \{[^}]*\} ptrt_probe;", src)
    assert P.lib.ptrt_abi_version() == 6  # additions only


def test_record_is_128_bytes(P):
    assert C.sizeof(P.Probe) == 128 and P.PROBE_DTYPE.itemsize == 128
    assert (P.Probe.sh.offset, P.Probe.mean_distance.offset, P.Probe.mean_distance_sq.offset, P.Probe.hit_fraction.offset,
            P.Probe.reserved.offset) == (0, 108, 112, 116, 120)
    cols = sorted(P.PROBE_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 32 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b) in P.PROBE_COLUMNS.items():
        assert P.PROBE_DTYPE.fields[name][1] == 4 * a == getattr(P.Probe, name).offset
    import torch
    rows = torch.arange(64, dtype=torch.float32).reshape(2, 32)
    f = P.probe_fields(rows)
    assert f["sh"].shape == (2, 9, 3) and f["sh"][1, 6, 2].item() == 32 + 20 and f["hit_fraction"].tolist() == [29.0, 61.0]
    assert f["mean_distance"].shape == (2,) and f["reserved"].shape == (2, 2)


def test_null_context_is_invalid(P):
    buf = (C.c_float * 64)()
    assert P.lib.ptrt_query_probes(None, buf, 1, buf, 1, buf, 1, 4, 1.0, buf) == -1
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    assert P.lib.ptrt_query_probes(stale, buf, 1, buf, 1, buf, 1, 4, 1.0, buf) == -1
    assert b"ptrt_query_probes" in P.lib.ptrt_last_error(stale)


def test_binding_checks_arguments(P):
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    pos = torch.zeros(2, 3)
    d = torch.zeros(4, 3)
    st = torch.zeros(8, 6, dtype=torch.int32)
    for args in [(np.zeros((2, 3), np.float32), d, st), (pos, d, st),                 # numpy; not on a device
                 (pos.double(), d, st), (pos, d, st.float()), (pos, d[:, :2], st)]:
        with pytest.raises(ValueError):
            s.query_probes(*args)
    s.close()


def test_mirror_method_compiles_and_refuses_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses Scene::queryProbes; on a host-only Scene it throws (no device to query on)."""
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
static_assert(sizeof(ptrt_probe) == 128, "ptrt_probe is 128 bytes");
static_assert(offsetof(ptrt_probe, mean_distance) == 108 && offsetof(ptrt_probe, reserved) == 120, "ptrt_probe layout");
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.queryProbes(nullptr, 0, nullptr, 1, nullptr, 1, 4, 1e30f, static_cast<ptrt_probe *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    return refused == 1 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0


# ---- ptrt_amd.probes ---------------------------------------------------------------------------------------------------------
def product_rule(nz=4, nphi=8):
    """Nodes and weights (summing to 1: a MEAN over the sphere) of Gauss-Legendre in z times equal steps in azimuth: exact for
    polynomials of degree 2 nz - 1 >= 4 in z and trigonometric degree nphi - 1 >= 4 in the azimuth, so for every product of
    two basis functions."""
    z, wz = np.polynomial.legendre.leggauss(nz)
    phi = (np.arange(nphi) + 0.25) * (2.0 * math.pi / nphi)
    r = np.sqrt(1.0 - z * z)
    d = np.stack([(r[:, None] * np.cos(phi)[None, :]).ravel(), (r[:, None] * np.sin(phi)[None, :]).ravel(),
                  np.repeat(z, nphi)], axis=1)
    w = np.repeat(wz / 2.0, nphi) / nphi
    return d, w


@pytest.mark.parametrize("k", [1, 2, 64, 130, 1000])
def test_fibonacci_sphere_gives_unit_directions(P, k):
    d = P.probes.fibonacci_sphere(k)
    assert d.shape == (k, 3) and d.dtype == np.float32 and d.flags["C_CONTIGUOUS"]
    # three squares of numbers <= 1, each rounded to float32 within 2^-24 relative
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    if k >= 64:  # spread over the sphere: the mean direction vanishes like 1 / k
        assert np.abs(d.astype(np.float64).mean(axis=0)).max() <= 2.0 / k
        assert len(np.unique(d, axis=0)) == k
    with pytest.raises(ValueError):
        P.probes.fibonacci_sphere(0)


def test_probe_grid(P):
    g = P.probes.probe_grid((-1.0, 0.0, 2.0), (1.0, 3.0, 2.5), (3, 4, 1))
    assert g.shape == (12, 3) and g.dtype == np.float32
    assert np.array_equal(g[:3, 0], np.float32([-1, 0, 1])) and np.array_equal(g[::3, 1], np.float32([0, 1, 2, 3]))
    assert (g[:, 2] == np.float32(2.25)).all()
    assert np.array_equal(g[4], np.float32([0.0, 1.0, 2.25]))  # x runs fastest
    with pytest.raises(ValueError):
        P.probes.probe_grid((0, 0, 0), (1, 1, 1), (2, 0, 2))


def test_sh9_basis_is_orthonormal(P):
    d, w = product_rule()
    Y = P.probes.sh9_basis(d)
    assert Y.shape == (len(d), 9) and Y.dtype == np.float64
    gram = 4.0 * math.pi * (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(9)).max() <= 1e-12
    # and the kernel's six-digit constants are these functions' normalisations
    got = R.basis32(d.astype(np.float32)).astype(np.float64)
    assert np.abs(got - P.probes.sh9_basis(d.astype(np.float32))).max() <= 2e-6


def test_sh9_irradiance_of_a_linear_radiance(P):
    """L(d) = 1 + d.a has irradiance E(n) = pi + (2 pi / 3) n.a; its coefficient MEANS come from the product rule."""
    d, w = product_rule()
    a = np.array([0.3, -0.5, 0.2])
    L = 1.0 + d @ a
    coeffs = (P.probes.sh9_basis(d) * (w * L)[:, None]).sum(axis=0)  # what query_probes would return, exactly
    n = P.probes.fibonacci_sphere(50).astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    E = P.probes.sh9_irradiance(coeffs[:, None], n)
    assert E.shape == (50, 1)
    assert np.abs(E[:, 0] - (math.pi + (2.0 * math.pi / 3.0) * (n @ a))).max() <= 1e-12
    # three channels, several probes
    c3 = np.stack([coeffs, 2.0 * coeffs, 0.0 * coeffs], axis=1)
    E3 = P.probes.sh9_irradiance(np.stack([c3, 3.0 * c3]), n)
    assert E3.shape == (2, 50, 3) and np.allclose(E3[1, :, 1], 6.0 * E[:, 0], rtol=1e-14) and not E3[:, :, 2].any()
    with pytest.raises(ValueError):
        P.probes.sh9_irradiance(np.zeros((8, 3)), n)


# ---- the sum order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 130, 1000])
def test_restatement_stays_within_its_bound_of_float64(P, n_dirs):
    """With u = 2^-24, every float32 operation returns its exact result times (1 + e), |e| <= u.  A term Y_i(d) * L passes
    through at most 5 of them (Y_6 * L: z * z, 3 *, - 1, c6 *, * L), each acting on a quantity no larger than the term with
    its own terms taken absolute, A_i(d) |L|: the term is off by at most 5 u A_i |L| to first order.  The fold adds 6 levels,
    each partial sum rounded once and no larger than the sum of the absolute terms below it: 6 u per term.  Adding the chunk
    sums to the total rounds once per chunk (`chunks` u), the division once (1 u).  Together
        |float32 - exact| <= (12 + chunks) u M_i,   M_i = mean_k A_i(d_k) |L_k|,
    and 1.01 covers the second-order terms ((12 + 16) u is 2e-6) and the float64 twin's own error.  The distances and the hit
    fraction pass through fewer operations and take the same bound with their own M."""
    rs = np.random.RandomState(n_dirs)
    n = 7
    d = P.probes.fibonacci_sphere(n_dirs)
    L = rs.lognormal(0.0, 2.0, (n * n_dirs, 3)).astype(np.float32)
    L[rs.uniform(size=L.shape) < 0.2] = 0.0
    depth = rs.uniform(0.1, 20.0, n * n_dirs).astype(np.float32)
    oid = rs.randint(-1, 5, n * n_dirs).astype(np.int32)
    depth[oid < 0] = np.float32(1e30)
    maxd = np.float32(12.3)
    got = R.restate(L, depth, oid, d, n_dirs, maxd)
    assert got.shape == (n, 32) and got.dtype == np.float32 and not got[:, 30:].any()
    want = R.restate64(L, depth, oid, d, n_dirs, maxd)
    M = R.magnitudes64(L, depth, d, n_dirs, maxd)
    chunks = (n_dirs + 63) // 64
    bound = (12 + chunks) * 2.0 ** -24 * 1.01 * M
    err = np.abs(got[:, :30].astype(np.float64) - want)
    assert (err <= bound).all(), f"worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}"
    assert (err > 0).any()  # (the comparison is not vacuous: float32 sums do round)
    # the sums are not the naive left-to-right ones: the fold order is what the kernel computes
    if n_dirs >= 63:
        t = R.terms32(L, depth, oid, d, n_dirs, maxd)
        naive = np.zeros((n, 30), np.float32)
        for k in range(n_dirs):
            naive = naive + t[:, k]
        assert not np.array_equal((naive / np.float32(n_dirs)).view(np.uint32), got[:, :30].view(np.uint32))
