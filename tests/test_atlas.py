"""Lightmap atlases (ptrt_atlas_texels, ptrt_atlas_dilate; Scene.atlas_texels / atlas_dilate; ptrt_amd.lightmap), without a GPU:
the entry points are declared and exported, the record is 32 bytes, what can be refused without a device is refused, the
mirror's methods compile into a caller of host/ptrt/scene.hpp, `triangle_charts` keeps its promises (judged in float64), the
restatement's dilation (tests/atlas_restatement.py) does what a dilation is for on images made by hand, and the helpers
between the rasteriser and the queries round-trip."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import atlas_restatement as A
from test_capi_symbols import declared

F = np.float32


def test_symbols_are_declared_and_exported(P):
    names = declared()
    for n in ("ptrt_atlas_texels", "ptrt_atlas_dilate"):
        assert n in names, f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n), f"{n} declared in include/ptrt.h but not exported"
    assert hasattr(P.lib, "hs_atlas_texels") and hasattr(P.lib, "hs_atlas_dilate")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    for n in ("AtlasTexel", "ATLAS_TEXEL_DTYPE", "ATLAS_COLUMNS", "atlas_fields"):
        assert hasattr(P, n)
    for n in ("atlas_texels", "atlas_dilate"):
        assert hasattr(P.Scene, n)
    for n in ("triangle_charts", "uv_to_texels", "covered", "atlas_inputs", "scatter"):
        assert hasattr(P.lightmap, n)
    assert "atlas_dilate" in P.lightmap.invalid_texels.__doc__


def test_record_is_32_bytes(P):
    assert C.sizeof(P.AtlasTexel) == 32 and P.ATLAS_TEXEL_DTYPE.itemsize == 32
    assert (P.AtlasTexel.position.offset, P.AtlasTexel.face.offset, P.AtlasTexel.normal.offset, P.AtlasTexel.mesh.offset) == (0, 12, 16, 28)
    cols = sorted(P.ATLAS_COLUMNS.values())
    assert cols[0][0] == 0 and cols[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for name, (a, b) in P.ATLAS_COLUMNS.items():
        assert P.ATLAS_TEXEL_DTYPE.fields[name][1] == 4 * a == getattr(P.AtlasTexel, name).offset
    import torch
    rows = np.arange(16, dtype=np.int32).reshape(2, 8)
    rows[:, 0:3] = np.float32([[1.5, 2.5, 3.5], [4.0, 5.0, 6.0]]).view(np.int32)
    for r in (rows, torch.from_numpy(rows)):
        f = P.atlas_fields(r)
        assert f["face"].tolist() == [3, 11] and f["mesh"].tolist() == [7, 15]
        assert f["position"].shape == (2, 3) and f["position"][1].tolist() == [4.0, 5.0, 6.0] and f["normal"].shape == (2, 3)


def test_refusals_that_need_no_device(P):
    buf = (C.c_float * 64)()
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_atlas_texels(ctx, 0, buf, 1, 1, 1, buf) == -1
        assert b"ptrt_atlas_texels" in P.lib.ptrt_last_error(stale)
        assert P.lib.ptrt_atlas_dilate(ctx, buf, buf, 1, 1, 1) == -1
        assert b"ptrt_atlas_dilate" in P.lib.ptrt_last_error(stale)
    assert not any(buf)
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    uv = torch.zeros(12, 6)
    for args in [(0, np.zeros((12, 6), np.float32), 8, 8), (0, uv, 8, 8), (0, uv.double(), 8, 8), (0, uv[:, :5], 8, 8)]:
        with pytest.raises(ValueError):
            s.atlas_texels(*args)
    for img in (np.zeros((4, 4, 4), np.float32), torch.zeros(4, 4, 4), torch.zeros(16, 4)):
        with pytest.raises(ValueError):
            s.atlas_dilate(img, 1)
    s.close()


def test_mirror_methods_compile_and_refuse_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses Scene::atlasTexels and Scene::atlasDilate; on a host-only Scene they throw."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    pkg = os.path.dirname(os.path.dirname(P.__file__))
    src = tmp_path / "caller.cpp"
    src.write_text("""
#include "ptrt/scene.hpp"
#include <cstddef>
#include <stdexcept>
static_assert(sizeof(ptrt_atlas_texel) == 32, "ptrt_atlas_texel is 32 bytes");
static_assert(offsetof(ptrt_atlas_texel, face) == 12 && offsetof(ptrt_atlas_texel, normal) == 16 &&
              offsetof(ptrt_atlas_texel, mesh) == 28, "ptrt_atlas_texel layout");
int main() {
    Scene s(32, 32, 0, 0, -1);
    Material m;
    s.addCube(m);
    int refused = 0;
    try { s.atlasTexels(0, nullptr, 4, 4, true, static_cast<ptrt_atlas_texel *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.atlasDilate(nullptr, nullptr, 4, 4, 1); } catch (const std::runtime_error &) { ++refused; }
    return refused == 2 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0


# ---- triangle_charts, judged in float64 --------------------------------------------------------------------------------------
def seg_dist(p, a, b):
    """distance of the points p (n, 2) from the segment a b, float64"""
    ab = b - a
    t = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[:, None] * ab), axis=1)


def inside64(p, tri):
    """float64: p (n, 2) inside or on the triangle tri (3, 2), either winding"""
    a, b, c = tri
    area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    b1 = ((p[:, 0] - a[0]) * (c[1] - a[1]) - (p[:, 1] - a[1]) * (c[0] - a[0])) / area
    b2 = ((b[0] - a[0]) * (p[:, 1] - a[1]) - (b[1] - a[1]) * (p[:, 0] - a[0])) / area
    return (b1 >= 0) & (b2 >= 0) & (1.0 - b1 - b2 >= 0)


def linf_point_segment(v, a, b):
    """L-infinity distance of the point v from the segment a b, float64, exact: max(|f1(t)|, |f2(t)|) is convex and piecewise
    linear in t, so its minimum over [0, 1] is at an end or at a breakpoint -- f1 = 0, f2 = 0, f1 = f2 or f1 = -f2."""
    d, r = b - a, v - a
    ts = [0.0, 1.0]
    for num, den in ((r[0], d[0]), (r[1], d[1]), (r[0] - r[1], d[0] - d[1]), (r[0] + r[1], d[0] + d[1])):
        if den != 0:
            ts.append(min(max(num / den, 0.0), 1.0))
    return min(np.abs(r - t * d).max() for t in ts)


def chebyshev_gap(t, u):
    """Chebyshev distance of two convex polygons (k, 2), float64: the L-infinity distance of the origin from their Minkowski
    difference, whose edges are a vertex of one minus an edge of the other -- so the smallest vertex-to-edge distance."""
    return min(linf_point_segment(v, Q[k], Q[(k + 1) % len(Q)]) for Pn, Q in ((t, u), (u, t)) for v in Pn for k in range(len(Q)))


@pytest.mark.parametrize("faces", [1, 2, 3, 12, 128])
@pytest.mark.parametrize("cell,gutter", [(4, 1), (8, 1), (8, 2), (9, 3), (2, 0), (16, 1)])
def test_triangle_charts(P, faces, cell, gutter):
    uv, w, h = P.lightmap.triangle_charts(faces, cell, gutter)
    assert uv.dtype == np.float32 and uv.shape == (faces, 6) and uv.flags["C_CONTIGUOUS"]
    assert w % cell == 0 and h % cell == 0 and (w // cell) * (h // cell) * 2 >= faces
    t = uv.astype(np.float64).reshape(faces, 3, 2)
    assert np.array_equal(t * 2, np.round(t * 2)), "a vertex off the half-texel grid"
    assert t.min() >= 0 and t[:, :, 0].max() <= w and t[:, :, 1].max() <= h, "a chart outside the atlas"
    centres = np.stack(np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5), axis=-1).reshape(-1, 2)
    owners = np.zeros(len(centres), np.int64)
    for f in range(faces):
        for k in range(3):
            d = seg_dist(centres, t[f, k], t[f, (k + 1) % 3])
            assert d.min() > 0.25, f"face {f}: a centre {d.min()} texels from an edge"
        ins = inside64(centres, t[f])
        assert ins.any(), f"face {f} owns no centre"
        owners += ins
    assert owners.max() == 1, "two charts share a centre"
    # the gutter: neighbours only (charts further apart than a cell's neighbours are separated by whole cells)
    cols = w // cell
    for f, g in itertools.combinations(range(faces), 2):
        cf, cg = f // 2, g // 2
        if abs(cf % cols - cg % cols) <= 1 and abs(cf // cols - cg // cols) <= 1:
            gap = chebyshev_gap(t[f], t[g])
            assert gap >= gutter - 1e-9, f"faces {f} and {g} are {gap} texels apart"


def test_triangle_charts_refuses_what_cannot_work(P):
    tc = P.lightmap.triangle_charts
    for args in [(0, 8), (-1, 8), (4, 3), (4, 1, 0), (4, 8, 4), (4, 8, -1), (4.5, 8), (4, 8.5), (1 << 27, 64)]:
        with pytest.raises(ValueError):
            tc(*args)
    assert tc(1, 2, 0)[1:] == (2, 2) and tc(2, 4)[1:] == (4, 4) and tc(3, 4)[1:] == (8, 4)


def test_uv_to_texels(P):
    import torch
    uv = np.float32([[0, 0, 1, 0, 0, 1], [0.5, 0.25, 1, 1, 0.125, 0.75]])
    got = P.lightmap.uv_to_texels(uv, 64, 32)
    assert got.dtype == np.float32 and got.tolist() == [[0, 0, 64, 0, 0, 32], [32, 8, 64, 32, 8, 24]]
    assert np.array_equal(P.lightmap.uv_to_texels(uv.reshape(2, 3, 2), 64, 32), got)
    assert np.array_equal(P.lightmap.uv_to_texels(torch.from_numpy(uv), 64, 32).numpy(), got)
    with pytest.raises(ValueError):
        P.lightmap.uv_to_texels(uv, 0, 4)


# ---- the restatement's dilation on images made by hand -----------------------------------------------------------------------
def image(h, w, valid):
    """(h, w, 4): the texels of `valid` ({(i, j): rgb}) valid, the rest zero"""
    img = np.zeros((h, w, 4), F)
    for (i, j), rgb in valid.items():
        img[j, i] = [*rgb, 1.0]
    return img


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (3, 3), (5, 4)])
def test_dilation_all_invalid_stays_all_invalid(h, w):
    img = np.zeros((h, w, 4), F)
    img[:, :, 0:3] = 7.0  # what an invalid texel holds is kept, not spread
    for passes in (1, 3):
        assert np.array_equal(A.dilate(img, passes), img)


@pytest.mark.parametrize("h,w,at", [(1, 1, (0, 0)), (1, 5, (0, 0)), (1, 5, (2, 0)), (3, 3, (1, 1)), (5, 4, (0, 0)), (5, 4, (3, 4))])
def test_dilation_spreads_one_ring_per_pass(h, w, at):
    rgb = (0.25, 2.0, -3.0)
    img = image(h, w, {at: rgb})
    jj, ii = np.mgrid[0:h, 0:w]
    ring = np.maximum(np.abs(ii - at[0]), np.abs(jj - at[1]))
    for passes in (1, 2, 3, 6):
        out = A.dilate(img, passes)
        assert np.array_equal(out[:, :, 3] != 0, ring <= passes), passes
        assert np.array_equal(out[ring <= passes, 0:3], np.broadcast_to(F(rgb), (int((ring <= passes).sum()), 3)))  # means of equal values
        assert not out[ring > passes].any()
    assert np.array_equal(img, image(h, w, {at: rgb})), "the input was written"


def test_dilation_does_not_read_its_own_pass():
    """1 x 5, valid at the left end only: were pass k to read what pass k wrote, one pass would fill the row."""
    out = A.dilate_pass(image(1, 5, {(0, 0): (1.0, 1.0, 1.0)}))
    assert (out[0, :, 3] != 0).tolist() == [True, True, False, False, False]
    # 3 x 3, two valid corners: the centre is their mean; the texel next to one corner only sees that one
    out = A.dilate_pass(image(3, 3, {(0, 0): (1.0, 0.0, 0.0), (2, 2): (3.0, 0.0, 8.0)}))
    assert out[1, 1].tolist() == [2.0, 0.0, 4.0, 1.0] and out[0, 1].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert out[0, 2].tolist() == [0.0, 0.0, 0.0, 0.0] and out[2, 0].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_dilation_sum_order_and_validity():
    """5 x 4: the fixed neighbour order decides the float32 sum; valid is `!= 0` (a NaN and a negative count, -0.0 does not)."""
    big, one = F(2.0 ** 24), F(1.0)
    img = image(4, 5, {(0, 0): (big, 0, 0), (1, 0): (one, 0, 0), (2, 0): (one, 0, 0), (0, 1): (-big, 0, 0)})
    out = A.dilate_pass(img)
    # texel (1, 1): neighbours in order (0,0) (1,0) (2,0) (0,1): ((2^24 + 1) + 1) - 2^24 = 0 in float32, / 4
    assert out[1, 1].tolist() == [0.0, 0.0, 0.0, 1.0]
    img = np.zeros((1, 3, 4), F)
    img[0, 0] = [5.0, 5.0, 5.0, np.nan]
    img[0, 2] = [9.0, 9.0, 9.0, -0.0]
    out = A.dilate_pass(img)
    assert out[0, 1].tolist() == [5.0, 5.0, 5.0, 1.0] and np.isnan(out[0, 0, 3])
    assert out[0, 2].tolist()[:3] == [9.0, 9.0, 9.0] and out[0, 2, 3] == 0  # -0.0 is invalid and (1, 0) was not valid in this pass


# ---- covered, atlas_inputs, scatter ------------------------------------------------------------------------------------------
def test_helpers_round_trip(P):
    import torch
    L = P.lightmap
    w, h = 5, 3
    rec = A.empty_records(w, h)
    own = [1, 4, 7, 14]
    pos = np.arange(12, dtype=F).reshape(4, 3) + F(0.5)
    nrm = -np.arange(12, dtype=F).reshape(4, 3)
    rec[own, 0:3], rec[own, 4:7] = pos.view(np.int32), nrm.view(np.int32)
    rec[own, 3], rec[own, 7] = [3, 0, 2, 9], [0, 0, 2, 1]
    for r in (rec, torch.from_numpy(rec)):
        idx = L.covered(r)
        assert np.asarray(idx).tolist() == own and str(idx.dtype).endswith("int64")
        p, n = L.atlas_inputs(r)
        assert np.array_equal(np.asarray(p), pos) and np.array_equal(np.asarray(n), nrm)
        assert (p.is_contiguous() and n.is_contiguous()) if hasattr(p, "is_contiguous") else (p.flags["C_CONTIGUOUS"] and n.flags["C_CONTIGUOUS"])
        values = p * 2
        img = L.scatter(values, idx, w, h)
        assert tuple(img.shape) == (h * w, 4) and str(img.dtype).endswith("float32")
        img = np.asarray(img)
        assert np.array_equal(np.flatnonzero(img[:, 3]), own) and np.array_equal(img[own, 0:3], pos * 2)
        assert np.array_equal(img[own, 3], np.ones(4, F)) and not np.delete(img, own, axis=0).any()
    f = P.atlas_fields(rec)
    assert f["mesh"][own].tolist() == [0, 0, 2, 1] and np.array_equal(f["position"][own], pos)
    with pytest.raises(ValueError):
        L.covered(rec.astype(np.float32))
    with pytest.raises(ValueError):
        L.scatter(pos, np.array([0, 1, 2, w * h]), w, h)
    with pytest.raises(ValueError):
        L.scatter(pos, np.array([0, 1, 2]), w, h)
    none = L.atlas_inputs(A.empty_records(2, 2))
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)


# ---- the restatement's own coverage rules ------------------------------------------------------------------------------------
def test_restated_coverage_rules():
    w = h = 8
    ccw, cw = F([1, 1, 6, 1, 1, 6]), F([1, 1, 1, 6, 6, 1])
    a, b = A.face_coverage(ccw, w, h)[0], A.face_coverage(cw, w, h)[0]
    assert np.array_equal(np.sort(a), np.sort(b)) and len(a) == 15  # both windings; centres (1 + a + 0.5, 1 + b + 0.5) with a + b + 1 <= 5: 5+4+3+2+1
    edge = A.face_coverage(F([0.5, 0.5, 4.5, 0.5, 0.5, 4.5]), w, h)[0]
    assert 0 in edge and 4 in edge and 4 * w in edge  # edges and corners are inclusive
    for bad in (F([1, 1, 6, 1, 11, 1]), F([1, 1, np.nan, 1, 1, 6]), F([1, 1, np.inf, 1, 1, 6])):
        assert len(A.face_coverage(bad, w, h)[0]) == 0
    assert len(A.face_coverage(F([-1e30, -1e30, 1e30, -1e30, 0, 1e30]), w, h)[0]) == 0  # products overflow: NaN fails
    assert A.scan_range(F([20, 20, 30, 20, 20, 30]), w, h) is None and A.scan_range(F([-9, -9, -2, -9, -9, -2]), w, h) is None
    assert A.scan_range(F([-1e30, 2, 1e30, 3, 0, 4]), w, h) == (0, 7, 1, 4)
    # ownership: the lower face wins; clear == 0 keeps what is there
    verts = F([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = [[0, 1, 2], [0, 1, 3]]
    uv = np.stack([ccw, F([1, 1, 6, 1, 1, 6])])
    rec = A.atlas_texels(verts, faces, uv, w, h, mesh=4)
    assert set(rec[rec[:, 7] >= 0, 3].tolist()) == {0} and (rec[:, 7] >= 0).sum() == 15
    again = A.atlas_texels(verts, faces[::-1], uv, w, h, mesh=5, clear=False, records=rec)
    assert np.array_equal(again, rec)
    more = A.atlas_texels(verts, faces, F([[0, 0, 8, 0, 0, 8]] * 2), w, h, mesh=6, clear=False, records=rec)
    assert np.array_equal(more[rec[:, 7] >= 0], rec[rec[:, 7] >= 0]) and (more[:, 7] == 6).sum() == 36 - 15
