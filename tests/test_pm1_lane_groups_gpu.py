"""ptrt_set_option "pm1_lane_groups": with every staged leaf full (pm1_full_leaf), the tail of a PMODE 1 pair list gives each
pair g lanes, g a divisor of the leaf size, in the sub-batches of the upload's plan (csrc/pm1_plan.h) instead
of the 2^sh lanes of one batch.  The same (ray, triangle) tests merged by the same 64-bit min and occlusion flag: option 0
and option 1 must agree bit for bit on every buffer, the generator states and the ray counts, and both with the committed
goldens, the CPU oracle and, for the ray queries, the float64 brute force.  The ray queries are where the pair count of a call
is set exactly: ray sets in which every ray meets the root box of one mesh (or of two), confirmed here by the kernels' slab
test restated in numpy, at ray counts on both sides of every capacity 64 / g and with tails behind a full batch."""
import ctypes as C
import os

import numpy as np
import pytest

import brute_force as bf
from common import assert_frames_equal, bits, render_both
from test_brute_force import assert_closest, assert_occluded
from test_ray_query_gpu import assert_hits_equal, query_both

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SETTINGS = (0, 1)
BUFFERS = ("accum", "normal", "depth", "object_id", "rgb8", "rng")


def _frames(P, s, spp, depth, frame0, frames):
    """the GPU half of common.render_both from frame number `frame0`"""
    s.setPerfSamplesPerPixel(spp)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(P.DEFAULT_SEED)
    s.set_option("count_rays", 1)
    s.setFrameCount(frame0)
    out = []
    for f in range(frames):
        rgb = s.render_to_host()
        out.append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                        object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats()))
    return out


def _assert_same(a, b, what):
    for f, (x, y) in enumerate(zip(a, b)):
        assert x["stats"] == y["stats"], f"{what} frame {f}: ray counts {x['stats']} vs {y['stats']}"
        for k in BUFFERS:
            assert np.array_equal(bits(x[k]), bits(y[k])), f"{what} frame {f}: {k} differs between pm1_lane_groups 0 and 1"


@pytest.mark.parametrize("name", ["cornell_64x64_1spp_d4_f0", "cornell_64x64_4spp_d2_f3"])
def test_cornell_frames_equal_the_goldens_either_way(P, name):
    import make_oracle_golden as M
    scene, w, h, spp, depth, frame = M.CASES[name]
    assert scene == "cornell" and (w, h) == (64, 64)
    g = np.load(os.path.join(GOLD, f"oracle_{name}.npz"))
    got = {}
    for lg in SETTINGS:
        s = P.Scene(w, h)
        P.scenes.cornell(s)
        s.set_option("pm1_lane_groups", lg)
        got[lg] = _frames(P, s, spp, depth, frame, 1)
        assert s.get_option("pmode") == 1 and s.get_option("pm1_full_leaf_eff") == 1
        assert s.get_option("pm1_lane_groups_eff") == lg
        s.close()
        x = got[lg][0]
        assert np.array_equal(x["object_id"], g["object_id"]), lg
        assert np.array_equal(bits(x["accum"]), bits(g["accum"])), lg
        assert np.array_equal(bits(x["depth"]), bits(g["depth"])), lg
        assert np.array_equal(x["rgb8"], g["rgb8"]), lg
    _assert_same(got[0], got[1], name)


def _strip(origin, u, v, tris):
    """`tris` triangles zigzagging over the parallelogram origin + [0, 1] u + [0, 1] v: one mesh, one leaf (<= 17 triangles)"""
    o, u, v = (np.asarray(a, np.float64) for a in (origin, u, v))
    k = tris + 2  # strip vertices: even ones on the v = 0 edge, odd ones on the v = 1 edge
    pts = [o + u * (i // 2) / ((k - 1) // 2) + v * (i % 2) for i in range(k)]
    out = []
    for i in range(tris):
        a, b, c = pts[i], pts[i + 1], pts[i + 2]
        out.append(tuple(a) + tuple(b) + tuple(c) if i % 2 == 0 else tuple(b) + tuple(a) + tuple(c))
    return out


def _strips_scene(tris):
    def make(P, s):
        """a floor, a back wall, a tilted sheet and a small roof under the light, each a strip of `tris` triangles"""
        grey, red, blue = P.Material((0.7, 0.7, 0.7), 0.6), P.Material((0.7, 0.2, 0.1), 0.5), P.Material((0.2, 0.3, 0.8), 0.3)
        s.addTriangles(_strip((-4, -2, -1), (8, 0, 0), (0, 0, -8), tris), grey)
        s.addTriangles(_strip((-4, -2, -9), (8, 0, 0), (0, 6, 0), tris), red)
        s.addTriangles(_strip((-2.5, -1.5, -4), (3, 1.5, -1), (0.5, 2, -2), tris), blue)
        s.addTriangles(_strip((0.5, 1.0, -3), (2, 0, 0), (0, 0.3, -2.5), tris), grey)
        s.addPointLight((1.0, 3.5, -4.0), (1.0, 0.95, 0.9), 3.0, 20.0)
        s.setCamera((0, 0.5, 4), (0, 0, -5), (0, 1, 0), 45.0)
    make.__name__ = f"strips{tris}"
    return make


def _cornell_quads(P, s):
    P.scenes.cornell(s, quads=True)


def _cornell_instance(P, s):
    """the Cornell box plus a cube that keeps its instance transform: closest-hit batches stay at one lane per pair
    (pair_split is off with an instanced mesh), the shadow trace takes the plan"""
    P.scenes.cornell(s)
    m = s.addCube(P.Material((0.8, 0.6, 0.3), 0.4, 0.0))
    s.setPosition(m, (1.2, -1.0, -3.5))
    s.setRotation(m, (0.3, 0.7, -0.2))
    s.setInstanceScale(m, (0.8, 1.3, 0.6))


def _both_settings_against_the_oracle(P, O, blue_noise, make, size, spp, depth, eff):
    got, oracle = {}, None
    for lg in SETTINGS:
        s = P.Scene(*size)
        make(P, s)
        s.set_option("pm1_lane_groups", lg)
        if oracle is None:
            got[lg], oracle = render_both(P, O, s, blue_noise, spp, depth, 1)
        else:
            got[lg] = _frames(P, s, spp, depth, 0, 1)
        assert s.get_option("pmode") == 1, "the scene does not run PMODE 1"
        assert s.get_option("pm1_lane_groups_eff") == (lg if eff else 0), (lg, s.get_option("pm1_lane_groups_eff"))
        s.close()
        assert_frames_equal(got[lg], oracle)
    _assert_same(got[0], got[1], make.__name__)


@pytest.mark.parametrize("tris", [7, 16, 17])
def test_single_leaves_of_other_sizes(P, O, blue_noise, tris):
    """7 and 17: primes, whose plans hand some tails back to the 2^sh rule (entries with g = 0); 16: every power of two divides"""
    _both_settings_against_the_oracle(P, O, blue_noise, _strips_scene(tris), (32, 32), 2, 3, eff=True)


def test_mixed_leaves_have_no_plan(P, O, blue_noise):
    _both_settings_against_the_oracle(P, O, blue_noise, _cornell_quads, (32, 32), 2, 3, eff=False)


def test_instanced_cube(P, O, blue_noise):
    _both_settings_against_the_oracle(P, O, blue_noise, _cornell_instance, (40, 24), 2, 4, eff=True)


# ---- ray queries with the pair count of every call known -------------------------------------------------------------------

COUNTS = [1, 5, 6, 10, 11, 16, 17, 21, 22, 32, 33, 37, 43, 53, 63, 64, 65, 75]
POOL = 160  # rays kept per set; a call of n rays takes n consecutive ones from an offset that moves with n


def _slab_f32(bmin, bmax, o, d, tmax):
    """pt::slab with pt::make_ray's reciprocal, in float32: (rays, boxes) bool"""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        big = np.abs(d) > f(1e-8)
        inv = np.where(big, f(1.0) / np.where(big, d, f(1.0)), np.where(d >= 0, f(1e30), f(-1e30))).astype(f)
        a = ((bmin[None, :, :] - o[:, None, :]) * inv[:, None, :]).astype(f)
        b = ((bmax[None, :, :] - o[:, None, :]) * inv[:, None, :]).astype(f)
        neg = (inv < 0)[:, None, :]
        t0, t1 = np.where(neg, b, a), np.where(neg, a, b)
        tmin, tmx = t0.max(axis=2), t1.min(axis=2)
    return (tmx >= 0) & (tmin <= tmx) & (tmin < f(tmax))


def _root_boxes(desc):
    d = desc.contents
    lo = np.array([[getattr(d.meshes[i].nodes[0].bmin, k) for k in "xyz"] for i in range(d.mesh_count)], np.float32)
    hi = np.array([[getattr(d.meshes[i].nodes[0].bmax, k) for k in "xyz"] for i in range(d.mesh_count)], np.float32)
    return lo, hi


def _rays_meeting(lo, hi, boxes, seed):
    """POOL rays from inside the room that meet the root boxes of exactly `boxes` meshes -- also when every box is grown or
    shrunk by 1e-3, so that the count does not hang on the last bit of a slab product"""
    rs = np.random.RandomState(seed)
    n = 40000
    o = np.stack([rs.uniform(-4.5, 4.5, n), rs.uniform(-4.5, 4.5, n), rs.uniform(-9.5, 4.0, n)], axis=1).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    e = np.float32(1e-3)
    cnt = [_slab_f32(lo - k * e, hi + k * e, o, d, 1e30).sum(axis=1) for k in (0, 1, -1)]
    keep = np.flatnonzero((cnt[0] == boxes) & (cnt[1] == boxes) & (cnt[2] == boxes))
    assert keep.size >= POOL, f"only {keep.size} of {n} candidate rays meet exactly {boxes} root boxes"
    keep = keep[:POOL]
    return np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])


@pytest.mark.parametrize("boxes", [1, 2])
def test_queries_with_known_pair_counts(P, O, boxes):
    s = P.Scene(32, 32)
    P.scenes.cornell(s)
    s.uploadToGPU()
    desc = s.flatten()
    lo, hi = _root_boxes(desc)
    assert len(lo) == 8
    o, d = _rays_meeting(lo, hi, boxes, seed=20 + boxes)
    assert (_slab_f32(lo, hi, o, d, 1e30).sum(axis=1) == boxes).all()  # a call of n <= 64 rays builds n * boxes pairs
    geom = bf.Geometry.from_desc(desc)
    c_bf = bf.closest(geom, o, d)
    far = np.full(len(o), 1e30, np.float32)                 # every box a ray meets is accepted: the shadow trace's P is the same
    near = bf.tmax_multiples(c_bf["t"], geom.radius)         # limits around the hit: fewer pairs, both answers occur
    a_bf = {k: bf.occluded(geom, o, d, t) for k, t in (("far", far), ("near", near))}
    c_or = O.trace_rays(desc, o, d)
    a_or = {k: O.any_hit(desc, o, d, t) for k, t in (("far", far), ("near", near))}
    assert c_bf["decided"].mean() > 0.9 and c_or["hit"].mean() > 0.9
    assert 0 < a_or["near"].mean() < 1 and a_or["far"].mean() > 0.9
    for n in COUNTS:
        at = (7 * n) % (POOL - n + 1)
        sl = slice(at, at + n)
        got = {}
        for lg in SETTINGS:
            s.set_option("pm1_lane_groups", lg)
            h, f_far = query_both(s, o[sl], d[sl], far[sl])
            assert s.get_option("query_pmode") == 1 and s.get_option("pm1_lane_groups_eff") == lg
            _, f_near = query_both(s, o[sl], d[sl], near[sl])
            got[lg] = (h, f_far, f_near)
            what = f"{boxes} boxes per ray, {n} rays, pm1_lane_groups {lg}"
            assert_hits_equal(h, c_or[sl], what + ": closest vs oracle")
            assert np.array_equal(f_far, a_or["far"][sl]) and np.array_equal(f_near, a_or["near"][sl]), what
            assert_closest({k: v[sl] for k, v in c_bf.items()}, h, geom.radius, what)
            assert_occluded({k: v[sl] for k, v in a_bf["far"].items()}, f_far, what + " far")
            assert_occluded({k: v[sl] for k, v in a_bf["near"].items()}, f_near, what + " near")
        assert_hits_equal(got[0][0], got[1][0], f"{boxes} boxes per ray, {n} rays: closest, option 0 vs 1")
        assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
    s.close()
