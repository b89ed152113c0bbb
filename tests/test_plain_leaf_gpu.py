"""ptrt_set_option "plain_leaf" on the device: where the upload finds a single-leaf TLAS whose meshes carry no
transform and whose boxes lie inside the root box, the pair builder of PMODE 1 and 2 leaves out the TLAS root-box test and PMODE
1's pair batches the instance arithmetic (PMODE 4 does not read the flag and reports 0).  The pair lists and merge keys are the same, so with the option at 0 and at -1 every buffer, the
generator states and the ray counts must equal the oracle's, bit for bit -- from the stock cameras, where every ray meets the
root box, and from cameras beside the scene, where a good part of the primary rays miss it."""
import numpy as np
import pytest

from common import assert_frames_equal, bits, render_both
from test_ray_query_gpu import assert_hits_equal, query_both

pytestmark = pytest.mark.gpu

SIZE, SPP, DEPTH, FRAMES = (40, 24), 2, 4, 2  # 40 x 24: ragged tiles in both directions
BUFFERS = ("accum", "normal", "depth", "object_id", "rgb8", "rng")
# stock: the scene builder's camera.  beside: picked on the CPU so that 20 .. 80 % of the oracle's object ids at this size are
# -1 (Cornell 40.5 %, the water scene 68 %); asserted below on the oracle's output.
CAMERAS = {
    "cornell": {"stock": None, "beside": ((9, 0, 6), (5, 0, -5), (0, 1, 0), 40.0)},
    "water": {"stock": None, "beside": ((30, 4, 10), (10, 3, 0), (0, 1, 0), 45.0)},
}


def _cornell(P, s):
    P.scenes.cornell(s)


def _cornell_quads(P, s):
    P.scenes.cornell(s, quads=True)


def _water(P, s):
    """the fluid scene at a small grid (32 water triangles over a 4-segment ship: both BLASes are real trees), water at rest"""
    P.scenes.fluid(s, cells=4, t=0.0, ship_segments=4)


def _cornell_short_box_instanced(P, s):
    P.scenes.cornell(s)
    short = 7  # (the last slab of scenes.cornell)
    s.setPosition(short, (0.4, 0.0, 0.3))
    s.setRotation(short, (0.0, 0.5, 0.1))


def _gpu_frames(P, s):
    """The GPU half of common.render_both: same calls, same order."""
    s.setPerfSamplesPerPixel(SPP)
    s.setMaxBounceDepth(DEPTH)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(P.DEFAULT_SEED)
    s.set_option("count_rays", 1)
    out = []
    for f in range(FRAMES):
        rgb = s.render_to_host()
        out.append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                        object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats()))
    return out


_oracle = {}  # (scene builder, camera) -> the oracle's frames: computed once, shared by the cases, never written to


def _both_settings(P, O, blue_noise, make, family, cam, opts, pmode, eff):
    """`eff`: plain_leaf_eff expected with the option at -1 (at 0 it is 0)"""
    got = {}
    for setting in (0, -1):
        s = P.Scene(*SIZE)
        make(P, s)
        if CAMERAS[family][cam] is not None:
            s.setCamera(*CAMERAS[family][cam])
        for k, v in opts.items():
            s.set_option(k, v)
        s.set_option("plain_leaf", setting)
        if (make, cam) not in _oracle:
            got[setting], _oracle[(make, cam)] = render_both(P, O, s, blue_noise, SPP, DEPTH, FRAMES)
        else:
            got[setting] = _gpu_frames(P, s)
        assert s.get_option("pmode") == pmode, (s.get_option("pmode"), pmode)
        assert s.get_option("plain_leaf_eff") == (eff if setting else 0), (setting, s.get_option("plain_leaf_eff"))
        if "refill" in opts:
            assert s.get_option("refilled") == (1 if opts["refill"] else 0)
        if "pm1_dense_roots" in opts:
            assert s.get_option("pm1_dense_roots_eff") == opts["pm1_dense_roots"]
        s.close()
    cpu = _oracle[(make, cam)]
    miss = float((cpu[0]["object_id"] == -1).mean())
    print(f"{make.__name__} / {cam}: {miss:.3f} of the oracle's object ids are -1")
    if cam == "beside":
        assert 0.2 <= miss <= 0.8, f"the camera beside the scene sees {miss:.3f} of its pixels empty"
    for setting in (0, -1):
        assert_frames_equal(got[setting], cpu)
    for f, (a, b) in enumerate(zip(got[0], got[-1])):
        assert a["stats"] == b["stats"], f"frame {f}: ray counts {a['stats']} vs {b['stats']}"
        for k in BUFFERS:
            assert np.array_equal(bits(a[k]), bits(b[k])), f"frame {f}: {k} differs between plain_leaf 0 and -1"


PM1 = {
    "one-tile": (_cornell, dict(refill=0)),
    "refill": (_cornell, dict(refill=2)),
    "lockstep-roots": (_cornell, dict(refill=2, pm1_dense_roots=0)),
    "dense-roots": (_cornell, dict(refill=0, pm1_dense_roots=1)),
    "wg2": (_cornell, dict(pm1_wg=2)),
    "quads": (_cornell_quads, dict(refill=2)),  # mixed leaves: the guarded triangle loop
}


@pytest.mark.parametrize("cam", ["stock", "beside"])
@pytest.mark.parametrize("kernel", sorted(PM1))
def test_cornell_pmode1(P, O, blue_noise, kernel, cam):
    make, opts = PM1[kernel]
    _both_settings(P, O, blue_noise, make, "cornell", cam, opts, pmode=1, eff=1)


@pytest.mark.parametrize("cam", ["stock", "beside"])
@pytest.mark.parametrize("merged", [0, 1])
def test_water_pmode2_and_pmode4(P, O, blue_noise, merged, cam):
    """PMODE 2 builds its lists with build_pairs and takes the flag.  PMODE 4 (merged=1) runs root tests of its own ahead of
    build_pairs_merged and does not read it: plain_leaf_eff reports 0 there, and the option must not change a bit of the frame."""
    _both_settings(P, O, blue_noise, _water, "water", cam, dict(merged=merged), pmode=4 if merged else 2, eff=0 if merged else 1)


@pytest.mark.parametrize("cam", ["stock", "beside"])
def test_an_instanced_short_box_keeps_the_root_test(P, O, blue_noise, cam):
    _both_settings(P, O, blue_noise, _cornell_short_box_instanced, "cornell", cam, dict(refill=2), pmode=1, eff=0)


def test_a_device_refit_turns_it_off_until_the_next_upload(P, O, blue_noise):
    import torch
    from test_tlas_refit_gpu import upload_counts
    s = P.Scene(*SIZE)
    w, _ = P.scenes.fluid(s, cells=4, t=0.0, ship_segments=4)
    s.set_option("merged", 0)
    gpu, cpu = render_both(P, O, s, blue_noise, SPP, DEPTH, 1)
    assert_frames_equal(gpu, cpu)
    assert s.get_option("pmode") == 2 and s.get_option("plain_leaf_eff") == 1
    v = P.scenes.water_vertices(4, 0.9)
    dev = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    s.refitFromDevice(w, dev.data_ptr())
    s.render_to_host()
    assert s.get_option("plain_leaf_eff") == 0, "the device moved the boxes: nobody compared them with the root box"
    s.set_option("plain_leaf", 1)  # (1 does not force it)
    s.render_to_host()
    assert s.get_option("plain_leaf_eff") == 0
    # the same positions through the host: a full upload, which derives the flag again; the frame is the oracle's
    s.stats()  # (read and cleared: the two frames above are not the oracle's to count)
    uploads = upload_counts(P, s)[0]
    s.setVertices(w, v)
    s.commitObjectChanges()
    assert upload_counts(P, s)[0] == uploads + 1
    s.setFrameCount(0)
    gpu, cpu = render_both(P, O, s, blue_noise, SPP, DEPTH, 1)
    assert s.get_option("plain_leaf_eff") == 1
    assert_frames_equal(gpu, cpu)
    s.close()


def test_ray_queries_from_outside_the_root_box(P, O):
    """4,096 rays through ray_query_kernel's PMODE 1, closest hit and occlusion: about half start outside the root box and point
    away from it (they miss the root), the rest start inside the room."""
    n = 4096
    rs = np.random.RandomState(77)
    s = P.Scene(32, 32)
    P.scenes.cornell(s)
    s.uploadToGPU()
    d0 = s.flatten().contents
    lo = np.array([getattr(d0.tlas_nodes[0].bmin, k) for k in "xyz"], np.float64)
    hi = np.array([getattr(d0.tlas_nodes[0].bmax, k) for k in "xyz"], np.float64)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    o = rs.uniform(lo + 0.2, hi - 0.2, (n, 3))
    d = rs.normal(size=(n, 3))
    outside = rs.rand(n) < 0.5
    k = int(outside.sum())
    away = rs.normal(size=(k, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    o[outside] = centre + away * (np.linalg.norm(half) * rs.uniform(1.2, 3.0, (k, 1)))  # beyond the box's corners
    d[outside] = away + 0.3 * rs.normal(size=(k, 3))
    keep = np.einsum("ij,ij->i", d[outside], away) > 0  # (pointing away from the centre of a convex box: a miss)
    d[np.flatnonzero(outside)[~keep]] = away[~keep]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    tmax = np.where(rs.rand(n) < 0.5, 1e30, rs.uniform(0.5, 12.0, n)).astype(np.float32)
    want_h = O.trace_rays(s.flatten(), o, d)
    want_f = O.any_hit(s.flatten(), o, d, tmax)
    # (a sixth of the room is open: about five rays in six from inside meet a wall or a box)
    assert not want_h["hit"][outside].any() and want_h["hit"][~outside].mean() > 0.75
    assert 0.4 < outside.mean() < 0.6
    got = {}
    for setting in (0, -1):
        s.set_option("plain_leaf", setting)
        got[setting] = query_both(s, o, d, tmax)
        assert s.get_option("query_pmode") == 1
        assert s.get_option("plain_leaf_eff") == (1 if setting else 0)
        assert_hits_equal(got[setting][0], want_h, f"closest hit, plain_leaf {setting}, against the oracle")
        assert np.array_equal(got[setting][1], want_f), f"occlusion, plain_leaf {setting}, against the oracle"
    assert_hits_equal(got[-1][0], got[0][0], "closest hit, plain_leaf -1 against 0")
    assert np.array_equal(got[-1][1], got[0][1])
    s.close()
