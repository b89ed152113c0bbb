"""Probe volumes read at surface points (ptrt_probe_sample, ptrt_query_probe_light; Scene.probe_sample / query_probe_light;
probes.ProbeVolume / probe_light_fields / shade_probe_light), without a GPU: the entry points are declared and exported and
refuse what needs no device; the float32 restatement (tests/probe_sample_restatement.py) stays within its derived margins of
the float64 statement with the exact constants; and, by reasoning that shares nothing with either, a constant field comes back
as pi L in both modes, a linear field as the linear function at the point, and the record's structure -- one bit on a probe,
no second corner on an axis of one probe, clamped cells, a probe behind its own mean distance, a NaN probe of weight zero, a
point that is not finite -- is the one include/ptrt.h names, in bits."""
import ctypes as C
import math

import numpy as np
import pytest

import probe_sample_restatement as R
from test_capi_symbols import declared

F = np.float32
U = R.U
NAN, INF = float("nan"), float("inf")
MODES = ("trilinear", "visibility")
# the data's own share of an analytic check: a field's band 0 is stored as float32(0.282095f * L) -- the six-digit constant
# against the exact Y_0, and the product's rounding
DATA_REL = abs(float(R.Y32[0]) - R.Y64[0]) / R.Y64[0] + 2 * U


def volume(P, lo, hi, counts):
    return P.probes.ProbeVolume.from_corners(lo, hi, counts)


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def random_probes(vol, rng, sh=(-1.0, 2.0)):
    """synthetic records: sh uniform in `sh`, mean_distance 0.2 .. 2 spacings, mean_distance_sq = mean^2 + |noise|"""
    rec = np.zeros((vol.rows, 32), F)
    rec[:, :27] = rng.uniform(sh[0], sh[1], (vol.rows, 27))
    sp = float(np.mean(vol.spacing))
    rec[:, 27] = rng.uniform(0.2, 2.0, vol.rows) * sp
    rec[:, 28] = rec[:, 27] * rec[:, 27] + np.abs(rng.normal(size=vol.rows)) * F(0.1 * sp * sp)
    rec[:, 29] = 1.0
    return rec


def field_probes(vol, value):
    """records whose band 0 holds the radiance value(Q) (n, 3) at each probe's position, formed in float64 from the float32
    origin and spacing and rounded once, times the kernel's own 0.282095f; every other coefficient 0; distances that never
    reject: mean 1e3 spacings"""
    ax = [vol.origin[a].astype(np.float64) + np.arange(vol.counts[a]) * vol.spacing[a].astype(np.float64) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    Q = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    rec = np.zeros((vol.rows, 32), F)
    rec[:, 0:3] = (float(R.Y32[0]) * value(Q)).astype(F)
    rec[:, 27] = F(1e3 * float(np.max(vol.spacing)))
    rec[:, 28] = rec[:, 27] * rec[:, 27]
    return rec


def light(points, normals, vol, rec, mode, bias=0.0):
    return R.fields(R.sample(points, normals, -1, -1, 1, vol, rec, mode, bias))


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported(P):
    names = declared()
    for n in ("ptrt_probe_sample", "ptrt_query_probe_light"):
        assert n in names, f"{n} is not declared in include/ptrt.h"
        assert hasattr(P.lib, n)
    assert hasattr(P.lib, "hs_probe_sample") and hasattr(P.lib, "hs_query_probe_light")
    assert P.lib.ptrt_abi_version() == 6  # additions only
    assert hasattr(P.Scene, "probe_sample") and hasattr(P.Scene, "query_probe_light")
    for n in ("ProbeVolume", "probe_light_fields", "shade_probe_light"):
        assert hasattr(P.probes, n)
    assert P.PROBE_LIGHT_DTYPE == R.LIGHT_DTYPE and P.PROBE_DTYPE == R.PROBE_DTYPE
    assert (P.PROBES_TRILINEAR, P.PROBES_VISIBILITY) == (R.TRILINEAR, R.VISIBILITY) == (0, 1)
    assert C.sizeof(P.ProbeVolumeDesc) == 36
    # the restatement's exact constants are the ones the package's float64 helpers use
    assert np.allclose(P.probes.sh9_basis([[0.0, 0.0, 1.0]])[0, [0, 2, 6]], [R.Y64[0], R.Y64[1], 2.0 * R.Y64[3]], rtol=1e-15)
    assert np.allclose(4.0 * math.pi * P.probes.COSINE_LOBE[[0, 1, 4]], R.K64, rtol=1e-15)
    doc = P.probes.shade_probe_light.__doc__
    assert doc.rindex("camera_rays") < doc.rindex("query_probe_light") < doc.rindex("then this")


def test_refusals_that_need_no_device(P):
    buf = (C.c_float * 64)()
    stale = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never a live context
    desc = P.ProbeVolumeDesc((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(1, 1, 1))
    for ctx in (None, stale):
        assert P.lib.ptrt_probe_sample(ctx, buf, buf, 1, C.byref(desc), buf, 0, 0.0, buf) == -1
        assert b"ptrt_probe_sample" in P.lib.ptrt_last_error(stale)
        assert P.lib.ptrt_query_probe_light(ctx, buf, buf, 1, C.byref(desc), buf, 0, 0.0, buf) == -1
        assert b"ptrt_query_probe_light" in P.lib.ptrt_last_error(stale)
    assert not any(buf)
    import torch
    s = P.Scene(32, 32, device=P.HOST_ONLY)
    pts = torch.zeros((3, 3))
    vol = P.probes.ProbeVolume((0, 0, 0), (1, 1, 1), (2, 1, 1))
    good = dict(volume=vol, probes=torch.zeros((2, 32)))
    for change, word in [(dict(mode="nearest"), "mode"), (dict(mode=1), "mode"), (dict(volume=None), "volume"),
                         (dict(volume=(0, 0, 0)), "volume"), (dict(normal_bias=-0.1), "normal_bias"), (dict(normal_bias=NAN), "normal_bias"),
                         (dict(normal_bias=INF), "normal_bias"),
                         (dict(), "device")]:  # what is left: tensors that are not on a device
        for fn in (s.probe_sample, s.query_probe_light):
            with pytest.raises(ValueError, match=word):
                fn(pts, pts, **dict(good, **change))
    with pytest.raises(ValueError, match="positions"):
        s.probe_sample(np.zeros((3, 3), F), pts, **good)
    s.close()
    for bad in (dict(counts=(0, 1, 1)), dict(counts=(1, 1)), dict(counts=(4096, 4096, 2)), dict(spacing=(1, 0, 1)), dict(spacing=(1, -1, 1)),
                dict(spacing=(1, INF, 1)), dict(spacing=(NAN, 1, 1)), dict(origin=(0, NAN, 0)), dict(origin=(INF, 0, 0))):
        with pytest.raises(ValueError):
            P.probes.ProbeVolume(**dict(dict(origin=(0, 0, 0), spacing=(1, 1, 1), counts=(2, 2, 2)), **bad))
    assert P.probes.ProbeVolume((0, 0, 0), (1, 1, 1), (4096, 4096, 1)).rows == 2 ** 24


# ---- the restatement against the float64 statement ------------------------------------------------------------------------------
def statement_case(P, seed=1, n=20000):
    """points in and round a 4 x 3 x 2 volume, unit normals, synthetic probes"""
    rng = np.random.default_rng(seed)
    vol = volume(P, (-1.0, -0.5, 0.25), (1.5, 1.0, 1.0), (4, 3, 2))
    lo, hi = vol.corners()
    pts = (lo + (rng.random((n, 3)) * 1.2 - 0.1) * (hi - lo)).astype(F)
    return vol, pts, unit_normals(rng, n), random_probes(vol, rng)


@pytest.mark.parametrize("bias", [0.0, 0.05])
@pytest.mark.parametrize("mode", MODES)
def test_the_restatement_stays_within_its_margins_of_the_statement(P, mode, bias):
    vol, pts, nrm, rec = statement_case(P)
    e32, e64 = R.evaluate(pts, nrm, vol, rec, mode, bias), R.statement64(pts, nrm, vol, rec, mode, bias)
    und = R.undecided(e32, e64)
    assert und.mean() <= 0.02, f"{und.mean():.4f} of the samples are undecided"
    ok = ~und
    assert np.array_equal(e32["used"][ok], e64["used"][ok]) and np.array_equal(e32["cell"][ok], e64["cell"][ok])
    m = R.margins(e64, vol, rec, bias)
    err = np.abs(e32["irradiance"].astype(np.float64) - e64["irradiance"])
    lit = ok & (e64["weight"] > 0)
    assert lit.mean() > 0.9 and np.isfinite(m[lit]).all()
    ratio = np.where(err[lit] > 0, err[lit] / m[lit], 0.0)
    print(f"{mode}, bias {bias}: undecided {und.mean():.5f}, worst error / bound {ratio.max():.3f}, largest bound {m[lit].max():.2e}")
    assert (err[lit] <= m[lit]).all(), f"worst error / bound {ratio.max():.3f}"
    wrel = np.abs(e32["weight"].astype(np.float64) - e64["weight"])[lit] / e64["weight"][lit]
    assert wrel.max() < 1e-3


# ---- the analytic checks (shared with the device's test) ---------------------------------------------------------------------
CONSTANT_L = np.array([0.75, 2.0, 0.125])


def constant_case(P, n=4000, seed=3):
    rng = np.random.default_rng(seed)
    vol = volume(P, (-1.0, 0.0, -2.0), (1.0, 3.0, 0.5), (3, 4, 2))
    lo, hi = vol.corners()
    pts = (lo + (rng.random((n, 3)) * 1.4 - 0.2) * (hi - lo)).astype(F)
    rec = random_probes(vol, rng)
    rec[:, :27] = 0
    rec[:, 0:3] = (R.Y32[0] * CONSTANT_L.astype(F)).astype(F)
    return vol, pts, unit_normals(rng, n), rec


def check_constant(rows, vol, pts, nrm, rec, mode, bias):
    """every record with weight > 0 holds pi L within the margin and the data's share; returns how many had weight > 0"""
    f = R.fields(rows)
    m = R.margins(R.statement64(pts, nrm, vol, rec, mode, bias), vol, rec, bias)
    want = math.pi * CONSTANT_L
    lit = f["weight"] > 0
    err = np.abs(f["irradiance"][lit].astype(np.float64) - want)
    bound = m[lit] + want * DATA_REL
    assert (err <= bound).all(), f"{mode}: off pi L by up to {np.max(err / bound):.2f} bounds"
    assert not f["irradiance"][~lit].any()
    return int(lit.sum())


@pytest.mark.parametrize("mode", MODES)
def test_a_constant_field_is_pi_L(P, mode):
    vol, pts, nrm, rec = constant_case(P)
    lit = check_constant(R.sample(pts, nrm, -1, -1, 1, vol, rec, mode, 0.05), vol, pts, nrm, rec, mode, 0.05)
    assert lit == len(pts) if mode == "trilinear" else lit > len(pts) // 2


LINEAR_A, LINEAR_B = np.array([3.0, 2.0, 4.0]), np.array([[0.5, -0.25, 0.125], [0.0, 0.3, -0.2], [-0.4, 0.1, 0.6]])


def linear_field(Q):
    """radiance per channel, linear in the position and positive over linear_case's volume"""
    return LINEAR_A[None, :] + np.asarray(Q, np.float64) @ LINEAR_B.T


def linear_case(P, n=4000, seed=5):
    rng = np.random.default_rng(seed)
    vol = volume(P, (-1.0, 0.0, -2.0), (2.0, 1.5, -1.0), (4, 3, 2))
    lo, hi = vol.corners()
    pts = (lo + rng.random((n, 3)) * (hi - lo)).astype(F)
    pts = np.clip(pts, lo, hi)
    assert linear_field(np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])).min() > 0.5
    return vol, pts, unit_normals(rng, n), field_probes(vol, linear_field)


def check_linear(rows, vol, pts, nrm, rec):
    """TRILINEAR over a field whose band 0 is linear in the probe position gives pi times that function at P (trilinear weights
    reproduce a linear function exactly), within the margin and the data's share"""
    f = R.fields(rows)
    m = R.margins(R.statement64(pts, nrm, vol, rec, "trilinear", 0.0), vol, rec, 0.0)
    want = math.pi * linear_field(pts)
    assert (f["weight"] > 0).all()
    err = np.abs(f["irradiance"].astype(np.float64) - want)
    bound = m + want * DATA_REL
    assert (err <= bound).all(), f"off the linear function by up to {np.max(err / bound):.2f} bounds"


def test_a_linear_field_is_the_linear_function(P):
    vol, pts, nrm, rec = linear_case(P)
    check_linear(R.sample(pts, nrm, -1, -1, 1, vol, rec, "trilinear", 0.0), vol, pts, nrm, rec)


# ---- structure, in bits --------------------------------------------------------------------------------------------------------
def test_a_point_on_a_probe_uses_that_probe_alone(P):
    vol = volume(P, (-1.0, 0.0, 2.0), (0.5, 3.0, 4.0), (4, 3, 2))
    rng = np.random.default_rng(7)
    rec = random_probes(vol, rng)
    rec[:, 27] = 1e3  # never rejected
    rec[:, 28] = 1e6
    pts = vol.positions()
    nrm = unit_normals(rng, len(pts))
    for mode in MODES:
        f = light(pts, nrm, vol, rec, mode)
        assert (f["weight"] > 0).all()
        assert all(bin(int(u)).count("1") == 1 for u in f["used"]), "more than one corner at a probe's own position"
        # the footprint's corner 0, or -- on the last probe of an axis with more than one -- its neighbour of weight 1
        e = R.evaluate(pts, nrm, vol, rec, mode, 0.0)
        rows = e["row"][np.arange(len(pts)), np.log2(f["used"]).astype(int)]
        assert np.array_equal(rows, np.arange(len(pts)))
        want = np.maximum(0.0, np.einsum("ni,nic->nc", e["B"].astype(np.float64), rec[:, :27].reshape(-1, 9, 3).astype(np.float64)))
        assert np.allclose(f["irradiance"], want, rtol=1e-5, atol=1e-4)


def test_an_axis_of_one_probe_never_uses_its_second_corner(P):
    rng = np.random.default_rng(8)
    pts = (rng.random((500, 3)) * 4 - 1).astype(F)
    nrm = unit_normals(rng, len(pts))
    for counts, never in (((1, 3, 2), 0b10101010), ((3, 1, 2), 0b11001100), ((3, 2, 1), 0b11110000), ((1, 1, 1), 0b11111110)):
        vol = volume(P, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0), counts)
        rec = random_probes(vol, rng)
        for mode in MODES:
            f = light(pts, nrm, vol, rec, mode)
            assert not (f["used"] & never).any() and (f["cell"] >= 0).all(), (counts, mode)
            assert f["used"].any()


def test_points_outside_take_the_clamped_cell(P):
    vol = volume(P, (0.0, 0.0, 0.0), (3.0, 2.0, 1.0), (4, 3, 2))
    rng = np.random.default_rng(9)
    rec = random_probes(vol, rng)
    pts = F([[-5, 0.5, 0.5], [9, 0.5, 0.5], [1.5, -3, 0.5], [1.5, 7, 0.5], [1.5, 0.5, -2], [1.5, 0.5, 4], [-1e30, 1e30, -1e30], [1e38, -1e38, 1e38]])
    inside = np.clip(pts, *vol.corners())
    nrm = unit_normals(rng, len(pts))
    f, g = light(pts, nrm, vol, rec, "trilinear"), light(inside, nrm, vol, rec, "trilinear")
    assert np.array_equal(f["cell"], g["cell"]) and np.array_equal(f["used"], g["used"])
    assert np.array_equal(f["irradiance"].view(np.int32), g["irradiance"].view(np.int32))
    assert f["cell"].tolist() == [0, 3, 1, 1 + 4 * 2, 1, 1 + 12, 0 + 4 * 2, 3 + 12]
    assert f["used"][0] == 0b01010101 and f["used"][1] == 0b01010101  # x clamped onto a probe's plane: the x neighbours have weight 0


def test_a_probe_behind_its_own_mean_distance_is_absent(P):
    vol = volume(P, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2))
    rng = np.random.default_rng(10)
    rec = random_probes(vol, rng)
    rec[:, 27] = 10.0
    rec[:, 28] = 101.0
    blind = 5  # sees 0.1 spacing, with no variance
    rec[blind, 27], rec[blind, 28] = F(0.1), F(0.1) * F(0.1)
    assert rec[blind, 28] - rec[blind, 27] * rec[blind, 27] == 0
    pts = (rng.random((2000, 3))).astype(F)
    nrm = unit_normals(rng, len(pts))
    far = np.linalg.norm(pts.astype(np.float64) - vol.positions()[blind], axis=1) > 0.11
    f = light(pts, nrm, vol, rec, "visibility")
    assert far.sum() > 1500 and not (f["used"][far] & (1 << blind)).any()
    assert (f["used"][far] | (1 << blind) == 255).all() and (f["weight"] > 0).all()
    assert (light(pts, nrm, vol, rec, "trilinear")["used"] == 255).all()


def test_a_nan_probe_of_weight_zero_changes_nothing(P):
    vol = volume(P, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0), (3, 3, 3))
    rng = np.random.default_rng(11)
    rec = random_probes(vol, rng)
    nan_rec = rec.copy()
    centre = 13
    nan_rec[centre] = NAN
    # points on the faces x = 0, y = 2 and z = 0 of the cells: the centre probe is a corner of their footprints, with weight 0
    pts = rng.random((900, 3)).astype(F)
    pts[:300, 0], pts[300:600, 1], pts[600:, 2] = 0.0, 2.0, 0.0
    pts[300:600, 0] += 1.0
    nrm = unit_normals(rng, len(pts))
    for mode in MODES:
        e = R.evaluate(pts, nrm, vol, nan_rec, mode, 0.0)
        touched = ((e["row"] == centre) & ~(e["wt"] > 0)).any(axis=1)
        assert touched.sum() >= 600 and not ((e["row"] == centre) & (e["wt"] > 0)).any()
        a, b = R.sample(pts, nrm, -1, -1, 1, vol, rec, mode, 0.0), R.sample(pts, nrm, -1, -1, 1, vol, nan_rec, mode, 0.0)
        assert np.array_equal(a, b) and np.isfinite(R.fields(b)["irradiance"]).all()
    # and where its weight is positive, visibility skips the NaN by selection; trilinear has no such test
    inner = (rng.random((200, 3)) * 0.9 + 0.55).astype(F)
    f = light(inner, unit_normals(rng, 200), vol, nan_rec, "visibility")
    assert np.isfinite(f["irradiance"]).all() and (f["weight"] > 0).all() and (f["used"] != 255).all()
    assert np.isnan(light(inner, unit_normals(rng, 200), vol, nan_rec, "trilinear")["irradiance"]).all()


def test_records_without_a_cell(P):
    vol = volume(P, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2))
    rec = random_probes(vol, np.random.default_rng(12))
    pts = F([[NAN, 0, 0], [0, INF, 0], [0, 0, -INF], [NAN, NAN, NAN], [0.5, 0.5, 0.5]])
    nrm = F([[0, 0, 1]] * 5)
    for mode in MODES:
        rows = R.sample(pts, nrm, np.int32([4, 5, 6, 7, 8]), np.int32([1, 2, 3, 0, 2]), [1, 1, 1, 1, 0], vol, rec, mode, 0.0)
        assert np.array_equal(rows[:4], np.int32([[0, 0, 0, 0, -1, 0, 4, 1], [0, 0, 0, 0, -1, 0, 5, 2], [0, 0, 0, 0, -1, 0, 6, 3],
                                                  [0, 0, 0, 0, -1, 0, 7, 0]]))
        assert np.array_equal(rows[4], R.MISS) and R.MISS.tolist() == [0, 0, 0, 0, -1, 0, -1, -1]
    # a normal that is not finite is no reason: the cell is found, the colours may be anything
    f = light(F([[0.5, 0.5, 0.5]]), F([[NAN, 0, 1]]), vol, rec, "trilinear")
    assert f["cell"][0] == 0 and f["used"][0] == 255


# ---- the helpers ---------------------------------------------------------------------------------------------------------------
def test_probe_volume_positions_are_the_samplers_q(P):
    V = P.probes.ProbeVolume
    vol = V((0.1, -7.3, 1e3), (0.3, 1.7, 0.01), (5, 3, 4))
    pos = vol.positions()
    assert pos.dtype == F and pos.shape == (60, 3) and vol.rows == 60
    o, sp = F(vol.origin), F(vol.spacing)
    for row in (0, 1, 7, 23, 59):
        i, j, k = row % 5, row // 5 % 3, row // 15
        want = F([o[0] + F(F(i) * sp[0]), o[1] + F(F(j) * sp[1]), o[2] + F(F(k) * sp[2])])
        assert np.array_equal(pos[row].view(np.int32), want.view(np.int32))
    # what the restatement's VISIBILITY branch forms as Q: a point at a probe's position finds that probe among its corners (g
    # may round to either side of the integer) at distance exactly 0
    e = R.evaluate(pos, F([[0, 0, 1]] * 60), vol, np.zeros((60, 32), F), "visibility", 0.0)
    own = e["row"] == np.arange(60)[:, None]
    assert own.any(axis=1).all() and (e["r"][own] == 0).all()
    # from_corners: the corners come back, the order is probe_grid's
    lo, hi = (-2.0, 0.5, 1.0), (2.0, 3.0, 1.75)
    vol = V.from_corners(lo, hi, (5, 6, 4))
    a, b = vol.corners()
    assert np.array_equal(a, F(lo)) and np.allclose(b, hi, rtol=0, atol=4 * float(np.finfo(F).eps) * 3)
    assert np.allclose(vol.positions(), P.probes.probe_grid(lo, hi, (5, 6, 4)), rtol=0, atol=1e-6)
    again = V.from_corners(*vol.corners(), vol.counts)
    assert np.allclose(again.spacing, vol.spacing, rtol=1e-6) and np.array_equal(again.origin, vol.origin) and again.counts == vol.counts
    one = V.from_corners((1, 2, 3), (1, 4, 3), (1, 1, 1))
    assert one.rows == 1 and np.array_equal(one.positions(), F([[1, 2, 3]])) and (one.spacing > 0).all()


def test_fields_and_shading(P):
    import torch
    L = P.probes
    rows = np.zeros((4, 8), np.int32)
    rows[:, 0:3] = F([[1, 2, 3], [0.5, 0.25, 4], [0, 0, 0], [7, 8, 9]]).view(np.int32)
    rows[:, 3] = F([1, 0.5, 0, 2]).view(np.int32)
    rows[:, 4:8] = [[5, 255, 3, 0], [6, 1, 2, 1], [-1, 0, -1, -1], [0, 17, 9, 1]]
    for r in (rows, torch.from_numpy(rows)):
        f = L.probe_light_fields(r)
        assert tuple(f["irradiance"].shape) == (4, 3) and f["weight"].tolist() == [1, 0.5, 0, 2]
        assert f["cell"].tolist() == [5, 6, -1, 0] and f["used"].tolist() == [255, 1, 0, 17] and f["mesh"].tolist() == [0, 1, -1, 1]
    albedo = F([[0.5, 0.5, 0.5], [1.0, 0.25, 0.0]])
    got = L.shade_probe_light(rows, albedo, background=(0.1, 0.2, 0.3))
    irr = rows[:, 0:3].view(F)
    want = (albedo[[0, 1, 0, 1]] * irr) / F(math.pi)
    want[2] = F([0.1, 0.2, 0.3])
    assert got.dtype == F and np.array_equal(got.view(np.int32), want.astype(F).view(np.int32))
    t = L.shade_probe_light(torch.from_numpy(rows), torch.from_numpy(albedo), background=(0.1, 0.2, 0.3))
    assert np.array_equal(t.numpy().view(np.int32), got.view(np.int32)), "arrays and tensors shade alike"
    one = L.shade_probe_light(rows, (0.5, 0.5, 0.5))
    assert np.array_equal(one.view(np.int32), ((F([0.5, 0.5, 0.5]) * irr) / F(math.pi)).view(np.int32))
    for bad in (dict(albedo=albedo[:1]), dict(albedo=albedo[:, :2]), dict(background=(0, 0))):
        with pytest.raises(ValueError):
            L.shade_probe_light(rows, **dict(dict(albedo=albedo), **bad))
    with pytest.raises(ValueError):
        L.probe_light_fields(rows.astype(np.float32))
