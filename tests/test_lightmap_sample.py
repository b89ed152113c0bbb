"""Baked lightmaps read back at ray hits (ptrt_atlas_sample, ptrt_query_lightmap; Scene.atlas_sample / query_lightmap;
lightmap.chart_table / shade_samples), without a GPU: the entry points are declared and exported and refuse what needs no
device, and the float32 restatement (tests/lightmap_sample_restatement.py) is held against float64 reasoning that does not
share its code -- an affine image comes back as the affine function at the hit within a derived unit, a texel centre returns
its texel, invalid and outside taps are skipped and the rest renormalised with nothing of a skipped texel reaching the
result, and the records without a sample are exactly the ones include/ptrt.h names."""
import ctypes as C
import math

import numpy as np
import pytest

import lightmap_sample_restatement as R
from test_capi_symbols import declared

F = np.float32
EPS = float(np.finfo(np.float32).eps)
NAN, INF = float("nan"), float("inf")


def rows_equal(rows, want):
    """the (n, 8) int32 rows against (r, g, b, weight, x, y, face, mesh) tuples, floats compared by their bits"""
    w = np.zeros((len(want), 8), np.int32)
    for k, rec in enumerate(want):
        w[k, 0:6] = F(rec[0:6]).view(np.int32)
        w[k, 6:8] = rec[6:8]
    return np.array_equal(np.asarray(rows, np.int32), w)


def one_chart(w, h):
    """one face whose chart is the identity on the atlas square scaled by (w, h): a hit at (u, v) lands at (u * w, v * h)"""
    return F([[0, 0, w, 0, 0, h]]), np.int32([0])


def hits_at(x, y, w, h):
    """hits on that face at atlas points (x, y), as far as float32 barycentrics can say them"""
    return R.make_hits(np.zeros(len(x), np.int32), np.zeros(len(x), np.int32), F(x) / F(w), F(y) / F(h))


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported(P):
    names = declared()
    for n in ("ptrt_atlas_sample", "ptrt_query_lightmap"):
        assert n in names, f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n)
    assert hasattr(P.lib, "hs_atlas_sample") and hasattr(P.lib, "hs_query_lightmap")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    assert hasattr(P.Scene, "atlas_sample") and hasattr(P.Scene, "query_lightmap")
    for n in ("chart_table", "sample_rgb", "sample_weight", "shade_samples"):
        assert hasattr(P.lightmap, n)
    assert P.LIGHTMAP_SAMPLE_DTYPE == R.SAMPLE_DTYPE and P.HIT_DTYPE == R.HIT_DTYPE
    assert (P.LIGHTMAP_NEAREST, P.LIGHTMAP_BILINEAR) == (R.NEAREST, R.BILINEAR) == (0, 1)
    for doc in (P.lightmap.__doc__, P.lightmap.shade_samples.__doc__):  # the recipe of a lightmapped view, in its order
        assert doc.rindex("camera_rays") < doc.rindex("query_lightmap") < doc.rindex("shade_samples" if doc is P.lightmap.__doc__ else "then this")


def test_refusals_that_need_no_device(P):
    buf = (C.c_float * 64)()
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    for ctx in (None, stale):
        assert P.lib.ptrt_atlas_sample(ctx, buf, 1, buf, 1, buf, buf, 1, 1, 0, buf) == -1
        assert b"ptrt_atlas_sample" in P.lib.ptrt_last_error(stale)
        assert P.lib.ptrt_query_lightmap(ctx, buf, buf, 1, buf, 1, buf, buf, 1, 1, 0, buf) == -1
        assert b"ptrt_query_lightmap" in P.lib.ptrt_last_error(stale)
    assert not any(buf)
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    hits, rays = torch.zeros((3, 16), dtype=torch.int32), torch.zeros((3, 3))
    good = dict(charts=torch.zeros((2, 6)), chart_first=torch.zeros(1, dtype=torch.int32), image=torch.zeros((4, 4, 4)))
    for change, word in [(dict(mode="trilinear"), "mode"), (dict(mode=1), "mode"),
                         (dict(), "device")]:  # what is left: tensors that are not on a device
        with pytest.raises(ValueError, match=word):
            s.atlas_sample(hits, **dict(good, **change))
        with pytest.raises(ValueError, match=word):
            s.query_lightmap(rays, rays, **dict(good, **change))
    with pytest.raises(ValueError, match="hits"):
        s.atlas_sample(np.zeros((3, 16), np.int32), **good)
    s.close()


# ---- 1. an affine image comes back as the affine function ------------------------------------------------------------------------
def test_bilinear_of_an_affine_image_is_the_affine_function():
    """The image is I(i, j) = a + b (i + 0.5) + c (j + 0.5) per channel, rounded to float32, every texel valid.  In exact
    arithmetic the four weights sum to 1 and reproduce an affine function, so the sample is I at the point the taps are taken
    about, (fl(x - 0.5) + 0.5, fl(y - 0.5) + 0.5).  The float32 result r = (sum w_k I_k) / (sum w_k) differs from that by
    roundings that each multiply a term by (1 + d), |d| <= u = eps / 2.  fx = tx - floor(tx) is exact for tx >= 0.  A computed
    weight carries 3 (gx or gy, which is 1 - fx rounded; the product; and the other factor); a term of the numerator then 1
    for the stored texel, 1 for its evaluation here, 1 for the product w * I and 3 for the three sums: 9 u.  The denominator:
    3 per weight and 3 sums, 6 u.  The quotient: 1 u.  Together 16 u = 8 eps times sum w_k |I_k|.  The shift of the point by
    the rounding of x - 0.5 and y - 0.5 is at most u |x| |b| + u |y| |c|.  So with the unit eps * (sum w_k |I_k| + |b x| +
    |c y|) the error is below 8 units.  Worst observed: 0.91 units."""
    rng = np.random.default_rng(5)
    w, h = 37, 23
    coef = np.array([[3.0, -0.25, 0.125], [-40.0, 1.5, 0.75], [0.001, 0.37, -0.61]])  # per channel a, b, c: signs cancel
    jj, ii = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 4), F)
    for ch in range(3):
        img[:, :, ch] = F(coef[ch, 0] + coef[ch, 1] * (ii + 0.5) + coef[ch, 2] * (jj + 0.5))
    img[:, :, 3] = 1.0
    # authored charts, not the identity: three faces turned and stretched about the atlas, hits all over them
    charts = F([[2, 3, 33, 5, 4, 20], [35.5, 21.5, 3.25, 19, 30, 2.5], [10, 10, 12.5, 10.25, 10.75, 13]])
    first = np.int32([0])
    n = 4000
    u = rng.random(n)
    v = rng.random(n) * (1 - u)
    hits = R.make_hits(np.zeros(n, np.int32), rng.integers(0, 3, n), u, v)
    rows = R.fields(R.sample(hits, charts, first, img, "bilinear"))
    x, y = rows["x"].astype(np.float64), rows["y"].astype(np.float64)
    inner = (x >= 0.5) & (x < w - 0.5) & (y >= 0.5) & (y < h - 0.5)
    assert inner.mean() > 0.9
    assert np.abs(rows["weight"][inner] - 1.0).max() <= 6 * EPS / 2, "four valid taps: the weights sum to 1 within 6 u"
    tx, ty = (F(x) - F(0.5)).astype(np.float64), (F(y) - F(0.5)).astype(np.float64)
    px, py = tx + 0.5, ty + 0.5
    i0, j0 = np.floor(tx), np.floor(ty)
    fx, fy = tx - i0, ty - j0
    worst = 0.0
    for ch in range(3):
        a, b, c = coef[ch]
        truth = a + b * px + c * py
        mag = np.zeros(n)
        for di, dj, wk in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
            mag += wk * np.abs(a + b * (i0 + di + 0.5) + c * (j0 + dj + 0.5))
        unit = EPS * (mag + np.abs(b * x) + np.abs(c * y))
        err = np.abs(rows["rgb"][:, ch].astype(np.float64) - truth) / unit
        worst = max(worst, float(err[inner].max()))
    print(f"bilinear of an affine image: worst error {worst:.3f} units")
    assert worst <= 8.0


# ---- 2. texel centres ------------------------------------------------------------------------------------------------------------
def test_a_texel_centre_returns_that_texel():
    rng = np.random.default_rng(2)
    w, h = 16, 8  # powers of two: (i + 0.5) / w is exact, and so is the way back
    img = (rng.random((h, w, 4)) * 4 - 1).astype(F)
    img[:, :, 3] = 1.0
    charts, first = one_chart(w, h)
    jj, ii = np.mgrid[0:h, 0:w]
    hits = hits_at(ii.reshape(-1) + 0.5, jj.reshape(-1) + 0.5, w, h)
    near = R.fields(R.sample(hits, charts, first, img, "nearest"))
    bil = R.fields(R.sample(hits, charts, first, img, "bilinear"))
    assert np.array_equal(near["x"], F(ii.reshape(-1) + 0.5)) and np.array_equal(near["y"], F(jj.reshape(-1) + 0.5))
    assert np.array_equal(near["rgb"].view(np.int32), img[:, :, 0:3].reshape(-1, 3).view(np.int32)), "nearest: exactly"
    assert (near["weight"] == 1).all()
    # bilinear at a centre: fx = fy = 0, weights 1, 0, 0, 0; the taps with weight 0 are not used: (1 * c) / 1
    assert np.array_equal(bil["rgb"].view(np.int32), img[:, :, 0:3].reshape(-1, 3).view(np.int32)) and (bil["weight"] == 1).all()
    assert (near["face"] == 0).all() and (near["mesh"] == 0).all()


# ---- 3. skipped taps -------------------------------------------------------------------------------------------------------------
def test_invalid_taps_are_skipped_and_the_rest_renormalised():
    w, h = 8, 8
    charts, first = one_chart(w, h)
    img = np.zeros((h, w, 4), F)
    img[:, :, 0:3] = F([1.0, 2.0, 4.0])
    img[:, :, 3] = 1.0
    img[3, 3] = [10.0, 20.0, 40.0, 2.5]     # valid is "not zero", not "one"
    img[3, 4] = [NAN, INF, -INF, 0.0]        # invalid, and poisoned
    img[4, 3] = [INF, NAN, 1e38, -0.0]       # minus zero is zero
    img[4, 4] = [100.0, 200.0, 400.0, 1.0]
    # the footprint (3..4, 3..4) at fx = 0.25, fy = 0.5: weights 0.375, 0.125, 0.375, 0.125; taps 2 and 3 invalid
    rows = R.fields(R.sample(hits_at([3.75], [4.0], w, h), charts, first, img, "bilinear"))
    assert rows["weight"][0] == F(0.5)
    want = (0.375 * np.float64([10, 20, 40]) + 0.125 * np.float64([100, 200, 400])) / 0.5
    assert np.array_equal(rows["rgb"][0], F(want)), "every step is exact here: 0.375 and 0.125 times small integers"
    # nearest on an invalid texel: nothing, and nothing of the poison
    near = R.sample(hits_at([4.5, 3.5, 3.5], [3.5, 4.5, 3.5], w, h), charts, first, img, "nearest")
    assert rows_equal(near, [(0, 0, 0, 0, 4.5, 3.5, 0, 0), (0, 0, 0, 0, 3.5, 4.5, 0, 0), (10, 20, 40, 1, 3.5, 3.5, 0, 0)])
    # all four invalid: weight 0, rgb 0
    img[3, 3, 3] = img[4, 4, 3] = 0.0
    rows = R.sample(hits_at([3.75], [4.0], w, h), charts, first, img, "bilinear")
    assert rows_equal(rows, [(0, 0, 0, 0, 3.75, 4.0, 0, 0)])
    # poison everywhere it may not matter: every invalid texel NaN, the result of every hit finite
    rng = np.random.default_rng(4)
    img = (rng.random((h, w, 4)) + 1).astype(F)
    bad = rng.random((h, w)) < 0.4
    img[bad] = [NAN, INF, -INF, 0.0]
    n = 500
    hits = hits_at(rng.random(n) * w, rng.random(n) * h, w, h)
    for mode in ("nearest", "bilinear"):
        r = R.fields(R.sample(hits, charts, first, img, mode))
        assert np.isfinite(r["rgb"]).all() and np.isfinite(r["weight"]).all()
        assert ((r["weight"] == 0) == (r["rgb"] == 0).all(1)).all()
        assert (r["rgb"][r["weight"] > 0] >= 1).all() and (r["rgb"][r["weight"] > 0] <= 2).all(), "a mean of texels in [1, 2]"
        assert 0 < (r["weight"] == 0).mean() < 0.5


def test_a_border_hit_uses_the_taps_inside_the_atlas():
    w, h = 4, 3
    charts = F([[-4, -4, 12, -4, -4, 12]])  # a chart that reaches outside the atlas all round
    first = np.int32([0])
    img = np.zeros((h, w, 4), F)
    img[:, :, 0] = np.arange(w)[None, :] + 1
    img[:, :, 1] = np.arange(h)[:, None] + 1
    img[:, :, 3] = 1.0

    def at(x, y, mode):
        hits = R.make_hits([0], [0], [(x + 4) / 16], [(y + 4) / 16])
        r = R.fields(R.sample(hits, charts, first, img, mode))[0]
        assert (r["x"], r["y"]) == (F(x), F(y))
        return r

    r = at(0.25, 1.5, "bilinear")          # left of the first column's centres: taps (-1, 1) and (0, 1); fx = 0.75, fy = 0
    assert r["weight"] == F(0.75) and tuple(r["rgb"]) == (1.0, 2.0, 0.0), "not clamped: skipped, and the rest renormalised"
    r = at(0.25, 0.25, "bilinear")         # the corner: only (0, 0), with fx * fy
    assert r["weight"] == F(0.5625) and tuple(r["rgb"]) == (1.0, 1.0, 0.0)
    r = at(3.75, 2.75, "bilinear")         # the far corner: only (3, 2), with gx * gy
    assert r["weight"] == F(0.5625) and tuple(r["rgb"]) == (4.0, 3.0, 0.0)
    for x, y in ((-0.75, 1.0), (4.75, 1.0), (1.0, -0.75), (1.0, 3.75), (-3.0, -3.0), (9.0, 2.0)):
        for mode in ("nearest", "bilinear"):   # outside by more than half a texel: no tap at all
            r = at(x, y, mode)
            assert r["weight"] == 0 and not r["rgb"].any()
    assert at(4 - 2.0 ** -10, 3 - 2.0 ** -10, "nearest")["weight"] == 1 and at(4.0, 1.0, "nearest")["weight"] == 0
    assert at(-2.0 ** -10, 1.0, "nearest")["weight"] == 0 and at(0.0, 0.0, "nearest")["weight"] == 1
    # a 1 x 1 atlas: every bilinear sample inside it is its one texel
    one = np.ones((1, 1, 4), F)
    r = R.fields(R.sample(R.make_hits([0], [0], [0.3], [0.3]), F([[0, 0, 1, 0, 0, 1]]), first, one, "bilinear"))[0]
    assert tuple(r["rgb"]) == (1.0, 1.0, 1.0) and 0 < r["weight"] < 1


def test_the_guard_before_the_conversion():
    """corners far outside the atlas: floor(x) beyond the range of an int reaches no conversion and no tap"""
    img = np.ones((2, 2, 4), F)
    first = np.int32([0])
    for far in (3e9, -3e9, 1e30, -1e30, 2.0 ** 28 + 64):
        charts = F([[far, 0.5, far, 0.5, far, 0.5]])
        for mode in ("nearest", "bilinear"):
            rows = R.sample(R.make_hits([0], [0], [0.25], [0.25]), charts, first, img, mode)
            assert rows_equal(rows, [(0, 0, 0, 0, F(far), 0.5, 0, 0)])


# ---- 4. records without a sample -------------------------------------------------------------------------------------------------
def test_records_without_a_sample():
    img = np.ones((4, 4, 4), F)
    charts = F([[0, 0, 4, 0, 0, 4], [0, 0, 4, 0, 0, 4], [NAN, 0, 4, 0, 0, 4], [0, 0, INF, 0, 0, 4]])
    first = np.int32([0, -1, 2, 3, -7])      # mesh 1: no lightmap; mesh 3: its table ends after one face
    hits = R.make_hits(mesh=[0, 0, 1, 3, 3, 2, 3, 4, 0, 5, -2], face=[0, 9, 0, 0, 1, 0, 0, 0, -1, 0, 0],
                       u=[0.25] * 11, v=[0.5] * 11, hit=[0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    hits["u"][0], hits["mesh_index"][0], hits["face_index"][0] = NAN, 7, 7    # a miss: nothing of the record is looked at
    for mode in ("nearest", "bilinear"):
        rows = R.sample(hits, charts, first, img, mode)
        x3 = F(F(0.25) * F(INF))             # mesh 3's face 0: an infinite corner
        assert rows_equal(rows, [(0, 0, 0, 0, 0, 0, -1, -1),      # a miss
                                 (0, 0, 0, 0, 0, 0, 9, 0),        # first + f beyond the table
                                 (0, 0, 0, 0, 0, 0, 0, 1),        # a negative chart_first
                                 (0, 0, 0, 0, x3, 2.0, 0, 3),     # x not finite: x and y are reported
                                 (0, 0, 0, 0, 0, 0, 1, 3),        # the table ends inside mesh 3
                                 (0, 0, 0, 0, NAN, 2.0, 0, 2),    # a NaN corner
                                 (0, 0, 0, 0, x3, 2.0, 0, 3),
                                 (0, 0, 0, 0, 0, 0, 0, 4),        # chart_first -7
                                 (0, 0, 0, 0, 0, 0, -1, 0),       # a negative face
                                 (0, 0, 0, 0, 0, 0, 0, 5),        # a mesh the table does not have
                                 (0, 0, 0, 0, 0, 0, 0, -2)]), mode
    # query_closest's (n, 16) int32 rows are read as the same records
    as_rows = hits.view(np.int32).reshape(-1, 16)
    assert np.array_equal(R.sample(as_rows, charts, first, img, "bilinear"), R.sample(hits, charts, first, img, "bilinear"))
    # u belongs to corner v1, v to v2
    r = R.fields(R.sample(R.make_hits([0, 0], [0, 0], [1.0, 0.0], [0.0, 1.0]), F([[1, 2, 3, 2.5, 1.5, 3.5]]), first, img, "nearest"))
    assert tuple(r["x"]) == (3.0, 1.5) and tuple(r["y"]) == (2.5, 3.5)


# ---- 5. chart_table and shade_samples --------------------------------------------------------------------------------------------
def test_chart_table(P):
    import torch
    L = P.lightmap
    a, b = L.triangle_charts(12, 8)[0], L.triangle_charts(3, 6)[0]
    charts, first = L.chart_table([None, a, None, b])
    assert isinstance(charts, np.ndarray) and charts.dtype == F and first.dtype == np.int32
    assert np.array_equal(first, [-1, 0, -1, 12]) and np.array_equal(charts, np.concatenate([a, b]))
    tc, tf = L.chart_table([torch.from_numpy(a), None, b.astype(np.float64)])
    assert isinstance(tc, torch.Tensor) and tc.dtype == torch.float32 and tf.dtype == torch.int32
    assert np.array_equal(tf.numpy(), [0, -1, 12]) and np.array_equal(tc.numpy(), np.concatenate([a, b]))
    for bad in ([], [None, None], [a[:, :5]], [a.reshape(-1)], [a[:0]], [a, "charts"]):
        with pytest.raises(ValueError, match="chart_table"):
            L.chart_table(bad)


def test_shade_samples(P):
    import torch
    L = P.lightmap
    rng = np.random.default_rng(8)
    n = 64
    rows = np.zeros((n, 8), np.int32)
    rgb = (rng.random((n, 3)) * 3).astype(F)
    rows[:, 0:3] = rgb.view(np.int32)
    rows[:, 3] = F(1.0).view(np.int32)
    rows[:, 7] = rng.integers(-1, 3, n)
    rows[0, 7], rows[1, 7] = -1, 2
    albedo = F([[0.8, 0.7, 0.6], [0.1, 0.9, 0.2], [0.5, 0.5, 0.5]])
    emission = F([[0, 0, 0], [0, 0, 0], [5.0, 4.0, 3.0]])
    bg = (0.25, 0.5, 0.75)
    got = L.shade_samples(rows, albedo, emission, bg)
    m = rows[:, 7]
    want = np.where((m >= 0)[:, None], (albedo[np.maximum(m, 0)] * rgb) / F(math.pi) + emission[np.maximum(m, 0)], F(bg)[None, :])
    assert got.dtype == F and got.shape == (n, 3) and np.array_equal(got.view(np.int32), want.astype(F).view(np.int32))
    assert np.array_equal(got[0], F(bg)) and (got[1] >= F([5.0, 4.0, 3.0])).all()
    t = L.shade_samples(torch.from_numpy(rows), torch.from_numpy(albedo), torch.from_numpy(emission), bg)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy().view(np.int32), got.view(np.int32))
    assert np.array_equal(L.shade_samples(rows, albedo).view(np.int32),
                          L.shade_samples(rows, albedo, np.zeros_like(albedo), (0, 0, 0)).view(np.int32))
    assert np.array_equal(L.sample_rgb(rows), rgb) and (L.sample_weight(rows) == 1).all()
    assert np.array_equal(L.sample_rgb(torch.from_numpy(rows)).numpy(), rgb)
    f = P.lightmap_sample_fields(rows)
    assert np.array_equal(f["rgb"], rgb) and np.array_equal(f["mesh"], m) and f["weight"].dtype == F
    ft = P.lightmap_sample_fields(torch.from_numpy(rows))
    assert np.array_equal(ft["rgb"].numpy(), rgb) and np.array_equal(ft["face"].numpy(), rows[:, 6])
    for bad in (dict(albedo=albedo[:2]), dict(albedo=albedo[:, :2]), dict(emission=emission[:2]), dict(background=(0, 0)),
                dict(rows=rows.astype(np.float32)), dict(rows=rows[:, :7]), dict(albedo=albedo[:0])):
        with pytest.raises(ValueError):
            L.shade_samples(**dict(dict(rows=rows, albedo=albedo, emission=emission, background=bg), **bad))
