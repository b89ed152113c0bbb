"""The analytic lights' one-bounce term at lightmap texels (ptrt_query_bounce, ptrt_bounce_terms; Scene.query_bounce;
ptrt_amd.lightmap), without a GPU: the entry points are declared and exported, the record is 32 bytes, the binding checks its
arguments, the mirror's methods compile into a caller of host/ptrt/scene.hpp, the helpers of ptrt_amd.lightmap are what they
say, tests/bounce_restatement.py folds like tests/irradiance_restatement.py and stays within its first-order bound of the same
sums in float64, its float32 pieces are what they say, and the float64 statement decides (nearly) every term at hits the
oracle's traversal builds on the CPU."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bounce_restatement as B
import irradiance_restatement as R
import path_truth as PT
import shading_truth as T
from test_capi_symbols import declared
from test_irradiance_gpu import texels

F = np.float32


def test_symbols_are_declared_and_exported(P):
    names = declared()
    for n in ("ptrt_query_bounce", "ptrt_bounce_terms"):
        assert n in names, f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n), f"{n} declared in include/ptrt.h but not exported"
    assert hasattr(P.lib, "hs_query_bounce") and hasattr(P.lib, "hs_bounce_terms")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    for n in ("Bounce", "BOUNCE_DTYPE", "BOUNCE_COLUMNS", "bounce_fields"):
        assert hasattr(P, n)
    for n in ("query_bounce", "bounce_terms"):
        assert hasattr(P.Scene, n)
    for n in ("bounce_irradiance", "full_irradiance"):
        assert hasattr(P.lightmap, n)


def test_record_is_32_bytes(P):
    assert C.sizeof(P.Bounce) == 32 and P.BOUNCE_DTYPE.itemsize == 32
    assert (P.Bounce.radiance.offset, P.Bounce.lit_fraction.offset, P.Bounce.shadowed_fraction.offset, P.Bounce.hit_fraction.offset,
            P.Bounce.reserved.offset) == (0, 12, 16, 20, 24)
    cols = sorted(P.BOUNCE_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b) in P.BOUNCE_COLUMNS.items():
        assert P.BOUNCE_DTYPE.fields[name][1] == 4 * a == getattr(P.Bounce, name).offset
    import torch
    f = P.bounce_fields(torch.arange(16, dtype=torch.float32).reshape(2, 8))
    assert f["radiance"].shape == (2, 3) and f["lit_fraction"].tolist() == [3.0, 11.0]
    assert f["shadowed_fraction"].tolist() == [4.0, 12.0] and f["hit_fraction"].tolist() == [5.0, 13.0]
    assert f["reserved"].shape == (2, 2)


def test_null_context_is_invalid(P):
    buf = (C.c_float * 64)()
    off = C.c_float(1e-4)
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_query_bounce(ctx, buf, buf, 1, buf, 1, None, off, buf, 1, 0, 0, buf) == -1
        assert b"ptrt_query_bounce" in P.lib.ptrt_last_error(stale)
        assert P.lib.ptrt_bounce_terms(ctx, buf, buf, 1, 1, buf, 1, None, 0, 0, buf, buf, buf, buf) == -1
        assert b"ptrt_bounce_terms" in P.lib.ptrt_last_error(stale)


def test_binding_checks_arguments(P):
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    pos, nrm = torch.zeros(2, 3), torch.zeros(2, 3)
    s2, sh2 = torch.zeros(4, 2), torch.zeros(2, 2)
    for args in [(np.zeros((2, 3), np.float32), nrm, s2, sh2), (pos, nrm, s2, sh2), (pos, nrm, s2, None),   # numpy; not on a device
                 (pos.double(), nrm, s2, sh2), (pos, nrm, s2.double(), sh2), (pos, nrm, s2, sh2.double()),
                 (pos, nrm, s2[:, :1], sh2), (pos, nrm[:, :2], s2, sh2), (pos, nrm, s2, sh2[:, :1])]:
        with pytest.raises(ValueError):
            s.query_bounce(*args)
    for bad in ((-1, 1), (0, 2), (1, 1), (0, -1), (2, 0), 3, (0,)):
        with pytest.raises(ValueError, match="lights"):
            s.query_bounce(pos, nrm, s2, sh2, lights=bad)
        with pytest.raises(ValueError, match="lights"):
            s.bounce_terms(torch.zeros((8, 16), dtype=torch.int32), torch.zeros(8, 3), 4, sh2, lights=bad)
    for args in [(np.zeros((8, 16), np.int32), torch.zeros(8, 3), 4), (torch.zeros((8, 16), dtype=torch.int32), torch.zeros(8, 3), 4),
                 (torch.zeros((8, 16)), torch.zeros(8, 3), 4), (torch.zeros((8, 16), dtype=torch.int32), torch.zeros(7, 3), 4),
                 (torch.zeros((8, 16), dtype=torch.int32), torch.zeros(8, 3), 3), (torch.zeros((8, 16), dtype=torch.int32), torch.zeros(8, 3), 0)]:
        with pytest.raises(ValueError):
            s.bounce_terms(*args)
    s.close()


def test_mirror_methods_compile_and_refuse_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses Scene::queryBounce and Scene::bounceTerms; on a host-only Scene they throw."""
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
static_assert(sizeof(ptrt_bounce) == 32, "ptrt_bounce is 32 bytes");
static_assert(offsetof(ptrt_bounce, lit_fraction) == 12 && offsetof(ptrt_bounce, shadowed_fraction) == 16 &&
              offsetof(ptrt_bounce, hit_fraction) == 20 && offsetof(ptrt_bounce, reserved) == 24, "ptrt_bounce layout");
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.queryBounce(nullptr, nullptr, 0, nullptr, 1, nullptr, 1e-4f, nullptr, 1, 0, -1, static_cast<ptrt_bounce *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.bounceTerms(nullptr, nullptr, 0, 1, nullptr, 1, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr); } catch (const std::runtime_error &) { ++refused; }
    return refused == 2 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0


# ---- ptrt_amd.lightmap -------------------------------------------------------------------------------------------------------
def test_lightmap_helpers(P):
    import torch
    d = np.zeros((4, 8), np.float32)
    d[:, 0:3] = [[1.0, 2.0, 0.5], [0.0, 0.25, 4.0], [3.0, 3.0, 3.0], [0.0, 0.0, 0.0]]
    g = np.zeros((4, 8), np.float32)
    g[:, 0:3] = [[0.5, 0.5, 0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.125, 0.25, 0.5]]
    b = np.zeros((4, 8), np.float32)
    b[:, 0:3] = [[0.25, 0.125, 1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [0.5, 0.5, 0.5]]
    b[:, 3:6] = [[0.5, 0.25, 1.0]] * 4  # the fractions do not enter
    pi = np.float32(math.pi)
    E = P.lightmap.bounce_irradiance(b)
    assert E.dtype == np.float32 and E.shape == (4, 3) and np.array_equal(E, pi * b[:, 0:3])
    assert np.array_equal(P.lightmap.bounce_irradiance(torch.from_numpy(b)), E)
    full = P.lightmap.full_irradiance(d, g, b)
    assert full.dtype == np.float32
    assert np.array_equal(full, (d[:, 0:3] + pi * g[:, 0:3]) + pi * b[:, 0:3])
    assert np.array_equal(full, P.lightmap.total_irradiance(d, g) + E)
    assert np.array_equal(full[1], P.lightmap.total_irradiance(d, g)[1])       # no bounce light: the two-term sum
    # total_irradiance keeps its two arguments, its result and what its docstring says
    assert np.array_equal(P.lightmap.total_irradiance(d, g), d[:, 0:3] + pi * g[:, 0:3])
    doc = " ".join(P.lightmap.total_irradiance.__doc__.split())
    assert "LACKS" in doc and "one-bounce" in doc and "first hit" in doc and "full_irradiance" in doc
    for bad in ((d, g, b[:3]), (d, g[:3], b), (d[:3], g, b), (d, g, b[:, :6])):
        with pytest.raises(ValueError):
            P.lightmap.full_irradiance(*bad)
    with pytest.raises(ValueError):
        P.lightmap.bounce_irradiance(b[:, :6])


# ---- the sum order -----------------------------------------------------------------------------------------------------------
def random_terms(n_dirs, n_shadow, count, n=5):
    Q = n_shadow * count
    rs = np.random.RandomState(1000 * n_dirs + Q)
    rays = n * n_dirs
    v = rs.lognormal(0.0, 2.0, (rays * Q, 3)).astype(np.float32)
    v[rs.uniform(size=rays * Q) < 0.2] = 0.0                     # not walked
    v[rs.uniform(size=rays * Q) < 0.05] = np.float32(np.nan)     # nor these
    hit = rs.uniform(size=rays) < 0.8
    v.reshape(rays, Q, 3)[~hit] = 0.0                            # a miss: a row of zeros
    blocked = (rs.uniform(size=rays * Q) < 0.3).astype(np.int32)
    return v, blocked, hit


@pytest.mark.parametrize("n_dirs", [1, 3, 4, 16, 17, 64, 65, 130])
def test_restate_folds_like_the_irradiance_restatement(n_dirs):
    """One light, one shadow sample, nothing blocked: B(t, k) is the term itself, and the rows' radiance and hit fraction are
    irradiance_restatement's fold of the same numbers, bit for bit; the lit fraction is the fraction of walked terms."""
    v, _, hit = random_terms(n_dirs, 1, 1)
    v = np.where(np.isnan(v), np.float32(0.0), v)
    got = B.restate(v, np.zeros(len(v), np.int32), hit, n_dirs, 1, 1)
    want = R.restate(v, np.zeros(len(v), np.float32), np.where(hit, 0, -1), n_dirs, 1e30)
    assert got.dtype == np.float32 and got.shape == want.shape == (5, 8)
    assert np.array_equal(got[:, :3].view(np.uint32), want[:, :3].view(np.uint32))
    assert np.array_equal(got[:, 5].view(np.uint32), want[:, 5].view(np.uint32))
    walked = B.walked32(v).reshape(5, n_dirs)
    assert np.abs(got[:, 3].astype(np.float64) * n_dirs - walked.sum(axis=1)).max() < 1e-4 and not got[:, 4].any() and not got[:, 6:].any()


@pytest.mark.parametrize("n_dirs,n_shadow,count", [(1, 1, 1), (3, 2, 1), (4, 2, 5), (17, 1, 3), (64, 2, 2), (130, 1, 5)])
def test_restatement_stays_within_its_bound_of_float64(n_dirs, n_shadow, count):
    """With u = 2^-24, every float32 operation returns its exact result times (1 + e), |e| <= u.  A ray's B is a running sum of
    at most Q terms -- (Q - 1) u per term, first order -- and one division: Q u.  It enters the fold over k as
    irradiance_restatement's terms do: log2(w) levels, one rounding per chunk, the last division and one more allowed for, as
    for ptrt_query_irradiance: (2 + log2(w) + chunks) u.  The counts are whole numbers below 2^24 and their sums exact.
        |float32 - exact| <= (Q + 2 + log2(w) + chunks) u M_i,   M_i = the sum of the absolute terms under the divisors,
    and 1.01 covers the second-order terms and the float64 twin's own error."""
    Q = n_shadow * count
    v, blocked, hit = random_terms(n_dirs, n_shadow, count)
    got = B.restate(v, blocked, hit, n_dirs, n_shadow, count)
    assert got.shape == (5, 8) and got.dtype == np.float32 and not got[:, 6:].any() and not np.isnan(got).any()
    want = B.restate64(v, blocked, hit, n_dirs, n_shadow, count)
    M = B.magnitudes64(np.where(np.isnan(v), np.float32(0.0), v), blocked, hit, n_dirs, n_shadow, count)
    w = R.width(n_dirs)
    chunks = (n_dirs + w - 1) // w
    bound = (Q + 2 + math.log2(w) + chunks) * 2.0 ** -24 * 1.01 * M
    err = np.abs(got[:, :6].astype(np.float64) - want)
    assert (err <= bound).all(), f"worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}"
    if n_dirs * Q >= 6:
        assert (err[:, :3] > 0).any()  # (the comparison is not vacuous: float32 sums do round)
    # the fractions count the walked terms of the rays that hit
    walked = B.walked32(v).reshape(5, n_dirs * Q)
    assert np.abs((got[:, 3].astype(np.float64) + got[:, 4]) * (n_dirs * Q) - walked.sum(axis=1)).max() < 1e-3
    assert np.abs(got[:, 5].astype(np.float64) * n_dirs - hit.reshape(5, n_dirs).sum(axis=1)).max() < 1e-4


def test_restatement_small_cases():
    # one texel, two directions, Q = 3 (three lights, one sample): a ray's sum runs in q order, ((0 + v0) + v1) + v2
    e = np.float32(2.0 ** -24)
    v = np.zeros((6, 3), F)
    v[:, 0] = [1.0, e, e, e, e, 1.0]
    got = B.restate(v, np.zeros(6, np.int32), np.ones(2, bool), 2, 1, 3)
    b0 = (F(0.0) + F(1.0) + e) + e           # 1: each e is lost
    b1 = (F(0.0) + e + e) + F(1.0)           # 1 + 2^-23: the two e arrive together
    assert b0 == F(1.0) and b1 == F(1.0) + F(2.0 ** -23)
    assert got[0, 0] == (b0 / F(1.0) + b1 / F(1.0)) / F(2.0)
    assert got[0, 3] == F(1.0) and got[0, 4] == F(0.0) and got[0, 5] == F(1.0)
    # a miss counts nowhere; a blocked flag on a term that is not walked counts nowhere; a NaN is not walked
    v = np.float32([[0, 0, 0], [0, 0, 0], [np.nan, np.nan, np.nan], [0, 0, 2.0], [0, 0, 4.0], [-1, 0, 0]])
    got = B.restate(v, np.int32([1, 1, 1, 0, 1, 1]), np.array([False, True, True]), 3, 2, 1)
    assert got[0].tolist() == [0.0, 0.0, F(2.0) / F(2.0) / F(3.0), F(1.0) / F(6.0), F(1.0) / F(6.0), F(2.0) / F(3.0), 0.0, 0.0]


def test_float32_pieces():
    # the soft clamp: luminance (0.2126 x + 0.7152 y) + 0.0722 z against 500, the vector times 500 / lum
    v = np.float32([[100.0, 200.0, 300.0], [1000.0, 1000.0, 1000.0], [np.nan, 1.0, 1.0], [-1.0, 0.0, 0.0]])
    c = B.clamp32(v)
    assert np.array_equal(c[0], v[0]) and np.array_equal(c[3], v[3]) and np.isnan(c[2, 0])
    lum = F(0.2126) * F(1000.0) + F(0.7152) * F(1000.0) + F(0.0722) * F(1000.0)
    assert np.array_equal(c[1], v[1] * (F(500.0) / lum)) and abs(float(c[1, 0]) - 500.0) < 1e-3
    val = B.value32(np.float32([[0.25, 0.5, 1.0]]), np.float32([[2.0, 4.0, 8.0]]), np.float32([0.5]), np.float32([0.25]), np.float32([[1.0, 0.5, 0.25]]))
    assert val.tolist() == [[1.0, 2.0, 4.0]]
    # a fused multiply-add rounds once: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 keeps its last bit inside one, and loses it as a product
    x = F(1.0) + F(2.0 ** -12)
    a, b = np.float32([1.0 + 2.0 ** -11, x, 0.0]), np.float32([-1.0, x, 0.0])
    assert B.dot32(a, b) == F(2.0 ** -24)
    assert a[0] * b[0] + a[1] * b[1] == F(0.0)
    assert B._round32(Fraction(1, 3)) == F(1.0) / F(3.0)
    assert B._round32(Fraction(1) + Fraction(1, 2 ** 24)) == F(1.0)                                   # a tie: to even
    assert B._round32(Fraction(1) + Fraction(3, 2 ** 24)) == F(1.0) + F(2.0 ** -22)                   # a tie: to even, upwards


# ---- the float64 statement at hits built on the CPU ----------------------------------------------------------------------------
def add_lab_lights(s):
    """the four lights tests/test_direct_gpu.py's lab adds to Cornell's own (tests/test_bounce_gpu.py checks they are the same)"""
    s.addPointLight((2.0, 3.0, -4.0), (0.8, 0.8, 1.0), 5.0, 15.0, 0.3)
    s.addSpotLight((-3.0, 4.0, -6.0), (0.3, -1.0, 0.1), (1.0, 1.0, 1.0), 12.0, 0.3, 0.3, 30.0, 0.0)
    s.addSpotLight((1.0, 4.5, -7.0), (0.0, -1.0, 0.0), (1.0, 0.7, 0.4), 15.0, 0.2, 0.6, 25.0, 0.2)
    s.addDirectionalLight((-0.4, -1.0, -0.3), (1.0, 0.96, 0.9), 3.0)


def test_statement_decides_the_terms_at_oracle_hits(P, O):
    """The lab's five lights at the hits the oracle's traversal of Cornell gives gather rays built on the CPU: the statement
    leaves at most 2 % of the terms undecided -- a cosine, a cone edge, the clamp's threshold or the walked test within its
    margin of a branch -- and the terms do exercise it."""
    s = P.Scene(64, 64, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    add_lab_lights(s)
    desc = s.flatten()
    nl = int(desc.contents.light_count)
    assert nl == 5
    pos, nrm = texels(P, "cornell", B.STATEMENT_TEXELS)
    s2, sh2, ph, o, d = B.statement_rays(P, pos, nrm)
    hits = O.trace_rays(desc, o, d)
    assert 0.5 < hits["hit"].mean() < 1.0                       # (the box is open towards the camera: some rays leave)
    st, decided = B.statement64(hits, d, PT.lights64(desc.contents.lights, nl), T.load_materials(desc.contents.materials), 0, nl,
                                sh2, ph, B.STATEMENT_DIRS, B.STATEMENT_SHADOW)
    Q = nl * B.STATEMENT_SHADOW
    assert len(decided) == int(hits["hit"].sum()) * Q and st["value"].shape == (len(decided), 3)
    share = 1.0 - decided.mean()
    print(f"statement64: {share:.4f} of {len(decided)} terms undecided")
    assert share <= B.MAX_UNDECIDED
    w = st["walked"].reshape(-1, nl, B.STATEMENT_SHADOW)
    assert 0.2 < w.mean() < 0.98 and w.any(axis=(0, 2)).all()      # walked and not; every light lights some hit
    E = st["E"]
    assert all(np.isfinite(E[k]).all() for k in ("L", "tmax", "value")) and (E["value"][st["walked"] & decided] > 0).any()
    # a range of lights is the same statement, shifted
    st2, _ = B.statement64(hits, d, PT.lights64(desc.contents.lights, nl), T.load_materials(desc.contents.materials), 2, 3, sh2, ph,
                           B.STATEMENT_DIRS, B.STATEMENT_SHADOW)
    assert np.array_equal(st2["value"].reshape(-1, 3, B.STATEMENT_SHADOW, 3), st["value"].reshape(-1, nl, B.STATEMENT_SHADOW, 3)[:, 2:5])
    s.close()
