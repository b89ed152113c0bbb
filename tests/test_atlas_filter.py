"""The lightmap filter (ptrt_atlas_filter; Scene.atlas_filter; lightmap.texel_pitch / filter_sigmas), without a GPU: the entry
point is declared and exported, the binding refuses what it can see, the mirror's method compiles into a caller of
host/ptrt/scene.hpp, the two helpers do what they say on records made by hand, the float32 restatement
(tests/atlas_filter_restatement.py) lies within a derived bound of the same definition in float64, keeps the definition's
exact properties byte for byte, and does what a filter is for: it lowers the error of a noisy signal on the Cornell box's
charts at the recommended sigmas."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import atlas_filter_restatement as R
import atlas_restatement as A
from test_capi_symbols import declared

F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported(P):
    assert "ptrt_atlas_filter" in declared(), "ptrt_atlas_filter is not declared in include/ptrt.h"
    assert hasattr(P.lib, "ptrt_atlas_filter") and hasattr(P.lib, "hs_atlas_filter")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    assert hasattr(P.Scene, "atlas_filter")
    for n in ("texel_pitch", "filter_sigmas"):
        assert hasattr(P.lightmap, n)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ptrt.h")).read()
    assert "atlas_filter_tile" in header and "atlas_filter_tile_eff" in header
    for doc in (P.lightmap.total_irradiance.__doc__, P.lightmap.__doc__):
        assert doc.index("scatter") < doc.index("atlas_filter") < doc.rindex("atlas_dilate")
    assert "CONVENTIONS, not measurements" in P.lightmap.filter_sigmas.__doc__


def test_refusals_that_need_no_device(P):
    buf = (C.c_float * 64)()
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_atlas_filter(ctx, buf, buf, buf, 1, 1, 1, 1.0, 1.0, 2) == -1
        assert b"ptrt_atlas_filter" in P.lib.ptrt_last_error(stale)
    assert not any(buf)
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    rec, img = torch.zeros((16, 8), dtype=torch.int32), torch.zeros(4, 4, 4)
    good = dict(texels=rec, image=img, passes=1, sigma_distance=1.0, sigma_plane=1.0, normal_power=2)
    for change, word in [(dict(passes=0), "passes"), (dict(passes=9), "passes"), (dict(normal_power=-1), "normal_power"),
                         (dict(normal_power=8), "normal_power"), (dict(sigma_distance=0.0), "sigma_distance"),
                         (dict(sigma_distance=-1.0), "sigma_distance"), (dict(sigma_distance=float("nan")), "sigma_distance"),
                         (dict(sigma_plane=float("inf")), "sigma_plane"), (dict(sigma_plane=0.0), "sigma_plane"),
                         (dict(image=np.zeros((4, 4, 4), F)), "image"), (dict(image=torch.zeros(16, 4)), "image"),
                         (dict(image=torch.zeros(4, 4, 8)[:, :, ::2]), "contiguous"),
                         (dict(), "device")]:  # what is left: tensors that are not on a device
        with pytest.raises(ValueError, match=word):
            s.atlas_filter(**dict(good, **change))
    s.close()


def test_mirror_method_compiles_and_refuses_without_a_device(P, tmp_path):
    """A caller of host/ptrt/scene.hpp uses Scene::atlasFilter beside atlasTexels and atlasDilate; host-only they throw."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
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
    const ptrt_atlas_texel *none = nullptr;
    try { s.atlasTexels(0, nullptr, 4, 4, true, static_cast<ptrt_atlas_texel *>(nullptr)); } catch (const std::runtime_error &) { ++refused; }
    try { s.atlasFilter(none, nullptr, nullptr, 4, 4, 3, 0.3f, 0.05f, 2); } catch (const std::runtime_error &) { ++refused; }
    try { float *r = s.atlasFilter(none, nullptr, nullptr, 4, 4, 3, 0.3f, 0.05f); (void)r; } catch (const std::runtime_error &) { ++refused; }
    try { s.atlasDilate(nullptr, nullptr, 4, 4, 1); } catch (const std::runtime_error &) { ++refused; }
    return refused == 4 ? 0 : 1;
}
""")
    exe = tmp_path / "caller"
    lib_dir = os.path.join(pkg, "ptrt_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lptrt_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 0


def test_texel_pitch_and_filter_sigmas(P):
    import torch
    L = P.lightmap
    w, h = 4, 3
    #            texel  position        face mesh
    layout = {(0, 0): ((0, 0, 0), 0, 0), (1, 0): ((1, 0, 0), 0, 0),       # a pair 1 apart
              (2, 0): ((5, 0, 0), 1, 0), (3, 0): ((5, 0, 3), 1, 0),       # another face: (1,0)-(2,0) is no pair; this one is 3 apart
              (0, 1): ((0, 9, 0), 2, 1), (1, 1): ((0, 9, 2), 2, 1), (2, 1): ((2, 9, 2), 2, 1),  # two pairs 2 apart; (3, 1) is empty
              (0, 2): ((0, 0, 0), 0, 0), (1, 2): ((7, 0, 0), 0, 1),       # the same face of another mesh: no pair
              (2, 2): ((0, 0, 0), 5, 0), (3, 2): ((8, 0, 0), 6, 0)}       # two faces: no pair
    rec = A.empty_records(w, h)
    for (i, j), (p, f, m) in layout.items():
        rec[j * w + i, 0:3], rec[j * w + i, 3], rec[j * w + i, 7] = F(p).view(np.int32), f, m
    for r in (rec, torch.from_numpy(rec)):
        assert L.texel_pitch(r, w, h) == 2.0  # of 1, 3, 2, 2
    lonely = rec.copy()
    lonely[[1, 3, 5, 6], 7] = -1   # every pair loses a member
    for r in (lonely, torch.from_numpy(lonely), A.empty_records(w, h)):
        assert L.texel_pitch(r, w, h) == 0.0
    assert L.texel_pitch(rec[:1], 1, 1) == 0.0  # one column: no horizontal neighbour
    with pytest.raises(ValueError):
        L.texel_pitch(rec, 3, 3)
    with pytest.raises(ValueError):
        L.texel_pitch(rec.astype(F), w, h)
    assert L.filter_sigmas(2.0) == (6.0, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            L.filter_sigmas(bad)


# ---- synthetic guides ----------------------------------------------------------------------------------------------------------
def wavy_guides(w, h, seed, pitch=0.25, holes=0.1):
    """records of a gently curved sheet: positions a `pitch` grid with noise, unit normals near +z, one mesh, some holes"""
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:h, 0:w]
    pos = np.stack([ii * pitch, jj * pitch, np.zeros((h, w))], -1) + rng.normal(0, pitch * 0.1, (h, w, 3))
    nrm = np.stack([rng.normal(0, 0.2, (h, w)), rng.normal(0, 0.2, (h, w)), np.ones((h, w))], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    mesh = np.where(rng.random((h, w)) < holes, -1, 0)
    return R.records(pos.reshape(-1, 3), nrm.reshape(-1, 3), mesh.reshape(-1))


def random_image(w, h, seed, invalid=0.1):
    rng = np.random.default_rng(seed + 1000)
    img = (rng.random((h, w, 4)) * 4 - 1).astype(F)
    img[:, :, 3] = rng.random((h, w)) >= invalid
    return img


# ---- float32 against float64 ---------------------------------------------------------------------------------------------------
def pass_bound(sigma_distance, sigma_plane, step, normal_power):
    """First-order bound, in units of U * max|c|, on what one pass's float32 roundings move a channel of a texel whose own
    normal is a unit vector, counted from the definition.  ABSOLUTE errors of a tap's three factors, each in [0, 1]:
      wd:  e 1 rounding (2 in e*e), a product, two sums: d2 to 5 U relative (all terms positive); rr 3 (r, r*r); the quotient 1:
           t = d2 / rr to 9 U, and t <= 1 where wd > 0; the difference 1 - t adds 1:                          10
      wp:  pd = n . e cancels, so its error is absolute: (e 1 + product 1 + sums 2) U |n||e| = 4 U |e|, and |e| <= r where
           wd > 0; pd^2 moves by 2 |pd| * that plus its own rounding; pp 1, the quotient 1; with |pd| <= sigma_plane where
           wp > 0:  8 U r / sigma_plane + 3 U, and 1 for the difference:                                      8 r / sigma_plane + 4
      c:   a dot product of unit vectors, 3 U absolute (a product, two sums); k squarings turn a relative error x into
           2^k x + (2^k - 1) U, and c <= 1:                                                                   4 * 2^k - 1
      the three products of w = ((h * wd) * wp) * c:                                                          3
    A tap's weight is off by at most h times their sum, and the h sum to 1.  The result is num / den with den >= the centre
    tap's weight h00 * c00 = 0.140625 (wd = wp = 1 and c = 1 to 3 U there): d(num / den) = sum dw (c_k - out) / den, and
    |c_k - out| <= 2 max|c|.  The sums themselves: 25 products and 24 + 24 additions and the quotient, relative to
    sum w |c| <= den max|c|:  25 + 24 + 1."""
    r = sigma_distance * step
    weights = 10 + (8 * r / sigma_plane + 4) + (4 * 2 ** normal_power - 1) + 3
    return 2 * weights / 0.140625 + 50


@pytest.mark.parametrize("normal_power", [0, 2, 7])
@pytest.mark.parametrize("passes", [1, 3])
def test_float32_restatement_against_float64(passes, normal_power):
    """A pass is a convex combination of its source, so an error of the source passes through at most as large: the bound of
    several passes is the sum of theirs."""
    w, h = 37, 23
    sd, sp = 0.75, 0.125  # three pitches, half a pitch
    worst = 0.0
    for seed in range(3):
        rec, img = wavy_guides(w, h, seed), random_image(w, h, seed)
        f32, f64 = R.filter(rec, img, passes, sd, sp, normal_power), R.filter64(rec, img, passes, sd, sp, normal_power)
        assert f32.dtype == F and f64.dtype == np.float64
        live = (rec[:, 7].reshape(h, w) >= 0) & (img[:, :, 3] != 0)
        assert np.array_equal(bits(f32)[~live], bits(img)[~live]) and live.sum() > w * h // 2
        assert (np.abs(f32[live, 0:3] - img[live, 0:3]) > 1e-3).mean() > 0.9, "the filter did nothing"
        cmax = np.abs(img[live, 0:3]).max()
        B = sum(pass_bound(sd, sp, 1 << s, normal_power) for s in range(passes)) * U
        err = np.abs(f32[live, 0:3].astype(np.float64) - f64[live, 0:3]).max(axis=0) / cmax
        worst = max(worst, float(err.max()))
        assert (err <= B).all(), (err, B)
    print(f"passes {passes}, normal_power {normal_power}: worst |f32 - f64| / max|c| = {worst:.3e}, bound {B:.3e}")


# ---- exact properties ----------------------------------------------------------------------------------------------------------
def test_a_constant_image_comes_back_constant():
    """num and den are then the same sums (colour 1.0) or num stays 0 (colour 0.0): exact, over any guides whose weights stay
    finite -- random positions, normals of any direction and of lengths up to 1 (longer ones can take c^(2^k) to infinity,
    and infinity / infinity is a NaN by the definition itself)"""
    w, h = 19, 11
    for seed in range(2):
        rng = np.random.default_rng(seed)
        nrm = rng.normal(0, 1, (w * h, 3))
        nrm *= (rng.random(w * h) / np.linalg.norm(nrm, axis=1) * 0.999)[:, None]
        rec = R.records(rng.normal(0, 1, (w * h, 3)), nrm, np.where(rng.random(w * h) < 0.2, -1, rng.integers(0, 2, w * h)))
        img = random_image(w, h, seed, invalid=0.2)
        valid = img[:, :, 3] != 0
        img[valid, 0:3] = F([1.0, 0.0, 1.0])
        for passes, k in ((1, 0), (3, 2), (4, 7)):
            out = R.filter(rec, img, passes, 2.0, 1.5, k)
            assert np.array_equal(bits(out), bits(img)), (seed, passes, k)


def crease(w=8, h=4, pitch=0.25):
    """the left half of the atlas on the plane z = 0 (normal +z), the right half on the plane x = half (normal -x), meeting in a
    right angle under the atlas's middle column boundary"""
    jj, ii = np.mgrid[0:h, 0:w]
    left = ii < w // 2
    half = (w // 2 - 0.5) * pitch
    pos = np.where(left[..., None], np.stack([ii * pitch, jj * pitch, 0 * ii], -1),
                   np.stack([half + 0 * ii, jj * pitch, (ii - w // 2 + 0.5) * pitch], -1))
    nrm = np.where(left[..., None], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0])
    return R.records(pos.reshape(-1, 3), nrm.reshape(-1, 3), np.zeros(w * h, np.int32)), left


@pytest.mark.parametrize("normal_power", [0, 1, 7])
def test_nothing_crosses_a_right_angle(normal_power):
    rec, left = crease()
    img = np.zeros(left.shape + (4,), F)
    img[~left, 0:3] = 1.0
    img[:, :, 3] = 1.0
    out = R.filter(rec, img, 3, 10.0, 10.0, normal_power)  # sigmas that stop nothing: the cosine alone, and it is 0
    assert np.array_equal(bits(out), bits(img))


def test_far_in_the_world_is_far_in_the_filter():
    """two texels adjacent in the atlas, 4 sigma_distance apart in the world: the result is the one without the neighbour"""
    sd = 0.5
    rec = R.records([[0, 0, 0], [4 * sd, 0, 0]], [[0, 0, 1], [0, 0, 1]], [0, 0])
    img = F([[[0.3, 0.7, 1.1, 1.0], [100.0, -50.0, 7.0, 1.0]]])
    alone = rec.copy()
    alone[1, 7] = -1
    for passes in (1, 2):
        out, ref = R.filter(rec, img, passes, sd, 1.0, 0), R.filter(alone, img, passes, sd, 1.0, 0)
        assert np.array_equal(bits(out[0, 0]), bits(ref[0, 0]))
        assert np.abs(out[0, 0, 0:3] - img[0, 0, 0:3]).max() <= 4 * U * 1.1
    near = R.filter(R.records([[0, 0, 0], [0.5 * sd, 0, 0]], [[0, 0, 1], [0, 0, 1]], [0, 0]), img, 1, sd, 1.0, 0)
    assert near[0, 0, 0] > 1.0, "a neighbour inside sigma_distance contributes"


def test_what_is_copied_and_what_reaches_nobody():
    w, h = 13, 9
    rec = wavy_guides(w, h, 5, holes=0.15)
    img = random_image(w, h, 5, invalid=0.15)
    meshed, valid = rec[:, 7].reshape(h, w) >= 0, img[:, :, 3] != 0
    img[2, 3, 3], img[4, 6, 3] = 2.5, -1.0  # valid != 0 is valid, whatever the value
    valid[2, 3] = valid[4, 6] = True
    rec[2 * w + 3, 7] = rec[4 * w + 6, 7] = 0
    meshed[2, 3] = meshed[4, 6] = True
    clean = R.filter(rec, img, 3, 0.75, 0.125, 2)
    live = meshed & valid
    assert np.isfinite(clean).all() and np.array_equal(bits(clean)[~live], bits(img)[~live])
    assert clean[2, 3, 3] == F(2.5) and clean[4, 6, 3] == F(-1.0)
    assert not np.array_equal(clean[2, 3, 0:3], img[2, 3, 0:3])
    # poison everything a skipped tap holds: colours of invalid texels, guides of uncovered ones
    bad_img, bad_rec = img.copy(), rec.copy()
    bad_img[~valid, 0:3] = F([np.nan, np.inf, -np.inf])
    holes = np.flatnonzero(~meshed.reshape(-1))
    bad_rec[holes[0::3], 0:3] = F([np.nan, 1e30, -1e30]).view(np.int32)
    bad_rec[holes[1::3], 4:7] = F([np.nan, np.nan, np.inf]).view(np.int32)
    bad_rec[holes[2::3], 0:3] = F([1e30, 1e30, 1e30]).view(np.int32)
    out = R.filter(bad_rec, bad_img, 3, 0.75, 0.125, 2)
    assert np.array_equal(bits(out)[live], bits(clean)[live]), "a skipped tap reached a live texel"
    assert np.array_equal(bits(out)[~live], bits(bad_img)[~live]), "a texel that is not live was not copied"
    # a zero-normal centre: every weight is 0, den == 0, copied -- and as a tap it gives nothing either
    zero = rec.copy()
    k = int(np.flatnonzero(live.reshape(-1))[7])
    zero[k, 4:7] = 0
    z = R.filter(zero, img, 1, 0.75, 0.125, 2)
    assert np.array_equal(bits(z).reshape(-1, 4)[k], bits(img).reshape(-1, 4)[k])
    gone = rec.copy()
    gone[k, 7] = -1
    g = R.filter(gone, img, 1, 0.75, 0.125, 2)
    others = np.arange(w * h) != k
    assert np.array_equal(bits(z).reshape(-1, 4)[others], bits(g).reshape(-1, 4)[others])
    before = img.copy()  # the filter's input is not written
    R.filter(rec, img, 2, 0.75, 0.125, 2)
    assert np.array_equal(bits(img), bits(before))


# ---- what the filter is for ----------------------------------------------------------------------------------------------------
def test_noise_on_the_cornell_box_goes_down(P):
    """The Cornell scene's 12-face box on triangle_charts(12, 8): a signal linear in world position plus seeded noise of fixed
    amplitude; three passes at filter_sigmas(texel_pitch(..)) lower the RMS error against the clean signal over the covered
    texels."""
    L = P.lightmap
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    box = 6
    M = s.flatten().contents.meshes[box]
    assert M.face_count == 12
    verts = np.ctypeslib.as_array(C.cast(M.verts, C.POINTER(C.c_float)), (M.vert_count, 3)).copy()
    faces = np.ctypeslib.as_array(C.cast(M.faces, C.POINTER(C.c_int32)), (M.face_count, 3)).copy()
    uv, w, h = L.triangle_charts(12, 8)
    rec = A.atlas_texels(verts, faces, uv, w, h, mesh=box, world=F(list(M.world)), normal=F(list(M.normal)),
                         has_transform=bool(M.has_transform))
    s.close()
    idx = L.covered(rec)
    assert len(idx) >= 12 * 10
    pitch = L.texel_pitch(rec, w, h)
    assert pitch > 0
    sd, sp = L.filter_sigmas(pitch)
    pos = L.atlas_inputs(rec)[0].astype(np.float64)
    # The regime the filter is specified for (16 .. 64 directions per texel): a gather's relative noise is about
    # 1 / sqrt(directions), 12.5 % at the quiet end, and an atlas is dense enough that irradiance changes by a few per cent
    # from a texel to the next.  So: values around 2, noise of amplitude 0.25 (12.5 %), a gradient of 0.06 (3 %) per texel
    # pitch, a different direction per channel.  (A signal as steep per texel as the noise is another regime: there three
    # passes, whose footprint is wider than these 5-texel charts, smooth the signal away -- DESIGN.md 3.29 has the figures.)
    dirs = np.float64([[0.5, 0.25, 0.125], [-0.25, 0.5, 0.25], [0.125, -0.125, 0.5]])
    dirs *= (0.06 / pitch) / np.linalg.norm(dirs, axis=1, keepdims=True)
    clean = pos @ dirs.T + 2.0
    noisy = clean + np.random.default_rng(11).uniform(-0.25, 0.25, clean.shape)
    img = L.scatter(noisy.astype(F), idx, w, h).reshape(h, w, 4)
    out = R.filter(rec, img, 3, sd, sp, 2).reshape(-1, 4)
    rms = lambda a: float(np.sqrt(((a[idx, 0:3].astype(np.float64) - clean) ** 2).mean()))  # noqa: E731
    before, after = rms(img.reshape(-1, 4)), rms(out)
    print(f"pitch {pitch:.4f}, sigmas {sd:.4f} / {sp:.4f}: RMS error {before:.4f} -> {after:.4f}")
    assert after < before
    assert np.array_equal(bits(out)[rec[:, 7] < 0], bits(img.reshape(-1, 4))[rec[:, 7] < 0])
