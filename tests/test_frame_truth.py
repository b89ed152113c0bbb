"""The host mirror's Camera and the oracle's frames (oracle.render, oracle.primary_rays) against tests/frame_truth.py, the float64
statement of the camera, the primary ray and what a frame keeps of a sample, made from the reference's text alone:
the lab is what the statement says it is, the mirror's camera after every constructor and call, every frame case quantity by
quantity, the measured table, the seventeen seeded misreadings, and three identities on the statement alone.  CPU only; the device
meets the same statement in tests/test_frame_truth_gpu.py."""
import itertools

import numpy as np
import pytest

import frame_truth as FT

CASES = FT.cases() + FT.cases(far=True)
IDS = [FT.case_name(k) for k in CASES]


@pytest.fixture(scope="module")
def lab(P, O):
    lab = FT.Lab(P, O)
    lab.oracle = {}
    yield lab
    lab.close()


def oracle_of(P, O, lab, key):
    if key not in lab.oracle:
        lab.oracle[key] = FT.oracle_case(P, O, lab, key)
    return lab.oracle[key]


# ---------------------------------------------------------------------------------------------------- the lab
def test_the_lab_is_the_room_the_statement_describes(P, O):
    closed, opened = FT.lab_walls(False), FT.lab_walls(True)
    assert len(closed) == 6 and len(opened) == 5 and FT.OPEN_SIDE not in [w[0] for w in opened]
    tris = np.concatenate([t for _, t, _ in closed]).astype(np.float64)
    assert len(tris) == 24 <= 64
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert ((n * -tris[:, 0]).sum(axis=1) > 0.5).all(), "every face is wound to face the room's centre"
    for i, j in itertools.combinations(range(len(tris)), 2):                       # no two faces in one plane
        parallel = abs(n[i] @ n[j]) > 1.0 - 1e-6
        assert not (parallel and abs(n[i] @ (tris[j, 0] - tris[i, 0])) < 1e-3), (i, j)
    emissions = [e for _, _, e in closed]
    assert len(set(emissions)) == 6 and max(max(e) for e in emissions) <= 2.0       # names the wall; far below the soft clamp
    # turned about three axes: no wall's axis within 15 degrees of a world axis
    assert (np.abs(FT._turn()) < np.cos(np.radians(15.0))).all()
    # closed, the room lets no ray out; opened, the cases see walls and sky
    shut = FT.Lab(P, O, open_side=False)
    try:
        assert shut.world.geom.face_count() == 24 and not shut.world.sky.use
        for name in ("pinhole", "lens"):
            fr = shut.frame((name, 70, 33, "whole", 0, 1), units=False)
            assert fr["hit"].all() and fr["samples"][0]["first"]["front_face"].all(), name
    finally:
        shut.close()


def test_the_open_lab_shows_walls_and_sky_to_every_case(lab):
    assert lab.world.geom.face_count() == 20 and lab.world.sky.use
    for key in FT.cases():
        fr = lab.frame(key)
        assert 0.5 < fr["hit"].mean() < 0.95, FT.case_name(key)
        first = fr["samples"][0]["first"]
        faces = set(zip(first["mesh"][fr["hit"]], first["face"][fr["hit"]]))
        assert len(faces) >= 3, "at least three faces of different slopes in view"
        for r in fr["samples"]:
            assert r["first"]["front_face"][r["first"]["hit"]].all()
    seen = np.unique(np.concatenate([lab.frame(k)["object_id"] for k in FT.cases() if k[3] == "whole"]))
    assert len(seen) >= 3, "two walls and the sky between the views"
    for key in FT.cases(far=True):
        assert not lab.frame(key)["hit"].any(), "the far views see nothing"


def test_depth_sees_a_256th_of_a_pixel_and_of_the_lens(lab):
    """From the statement alone.  1/256 pixel of jitter on either axis, and 1/256 lens_radius along u and v, move the predicted
    depth by at least 8 units at 90 % of the decided hit pixels of every case."""
    for key in FT.cases():
        fr = lab.frame(key)
        for what in ("jitter_x", "jitter_y") + (("lens_u", "lens_v") if key[0] == "lens" else ()):
            share = (FT.moved_depth(fr, what, 1.0 / 256.0) >= 8.0).mean()
            assert share >= 0.9, f"{FT.case_name(key)}: {what} moves the depth by 8 units at only {100 * share:.1f} % of the hit pixels"


def test_the_undecided_share_is_within_the_cap(lab):
    """From the statement alone: no output of the code under test enters."""
    for key in CASES:
        und = 1.0 - lab.frame(key)["decided"].mean()
        assert und <= FT.MAX_UNDECIDED, f"{FT.case_name(key)}: {100 * und:.2f} % of the pixels undecided"


def test_rows_of_a_band_and_of_strips():
    assert np.array_equal(FT.band_rows(16, 24), np.arange(16, 40))
    assert np.array_equal(FT.strip_rows(48, 1, 3), np.r_[8:16, 32:40])
    assert np.array_equal(FT.strip_rows(33, 0, 2), np.r_[0:8, 16:24, 32:33])       # the last strip is cut at the frame's edge
    assert np.array_equal(FT.strip_rows(48, 0, 1), np.arange(48))


# ---------------------------------------------------------------------------------------------------- the host mirror
@pytest.mark.parametrize("case", FT.HOST_CAMERAS, ids=[c[0] for c in FT.HOST_CAMERAS])
def test_host_camera_is_the_statements(P, case):
    name, W, H, calls = case
    cam, vp = FT.judge_host_camera(P, name, W, H, calls)
    print(f"{name}: camera {cam:.3g} units, view_proj {vp:.3g} units")
    assert cam <= FT.TOL["camera"], f"{name}: a camera vector is {cam:.3g} units off (allowed {FT.TOL['camera']})"
    assert vp <= FT.TOL["view_proj"], f"{name}: a view_proj entry is {vp:.3g} units off (allowed {FT.TOL['view_proj']})"


def test_the_focus_distance_follows_the_camera(P):
    """camera.cuh:268-324: set_position keeps the point looked at (origin - w x the old focus distance) and takes the new
    distance to it; look_at takes the distance to its target."""
    name, W, H, calls = next(c for c in FT.HOST_CAMERAS if c[0] == "move-look-move")
    for k in range(1, len(calls) + 1):
        cam, _ = FT.host_camera(P, W, H, calls[:k])
        focus = np.linalg.norm(cam["origin"] - (cam["lower_left_corner"] + 0.5 * cam["horizontal"] + 0.5 * cam["vertical"]))
        st = FT.host_camera_fn(calls[:k])(FT.host_camera_inputs(W, H, calls[:k]))
        want = np.linalg.norm(st["origin"][0] - (st["lower_left_corner"][0] + 0.5 * st["horizontal"][0] + 0.5 * st["vertical"][0]))
        assert abs(focus - want) <= 1e-5 * want, (k, focus, want)
        if calls[k - 1][0] == "look":
            assert abs(want - np.linalg.norm(st["origin"][0] - FT._v(calls[k - 1][1]))) < 1e-12
    # the first call's 7.5, then the distance from the new position to the point that was in focus, ...
    st = FT.host_camera_fn(calls[:2])(FT.host_camera_inputs(W, H, calls[:2]))
    lookfrom, lookat = FT._v(calls[0][1]), FT._v(calls[0][2])
    kept = lookfrom + 7.5 * (lookat - lookfrom) / np.linalg.norm(lookat - lookfrom)
    centre = st["lower_left_corner"][0] + 0.5 * st["horizontal"][0] + 0.5 * st["vertical"][0]
    assert np.abs(centre - kept).max() < 1e-6


# ---------------------------------------------------------------------------------------------------- the oracle's frames
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_oracle_frame_is_the_statements(P, O, lab, key):
    got = oracle_of(P, O, lab, key)
    row, bad = FT.measure_case(P, O, lab, key, got=got)
    print(FT.case_name(key), " ".join(f"{q} {v:.3g}" for q, v in row.items()))
    for q, n in bad.items():
        assert n == 0, f"{FT.case_name(key)}: {q} differs at {n} decided pixels"
    for q, v in row.items():
        assert v <= FT.TOL[q], f"{FT.case_name(key)}: {q} is {v:.3g} units off (allowed {FT.TOL[q]})"


@pytest.mark.parametrize("key", FT.cases(far=True), ids=[FT.case_name(k) for k in FT.cases(far=True)])
def test_an_all_miss_view_leaves_the_states_the_statement_says(P, O, lab, key):
    got, fr = oracle_of(P, O, lab, key), lab.frame(key)
    states = FT.case_states(O, key)
    dec = fr["decided"]
    assert (got["object_id"] == -1).all() and (got["depth"] == np.float32(1e30)).all() and not got["normal"].any()
    if key[0] == "far_pinhole":
        assert dec.all() and not fr["draws"].any() and np.array_equal(got["rng"], states), "a pinhole draws nothing"
    else:
        assert dec.mean() > 0.99 and (fr["draws"] >= 2 * key[5]).all() and (fr["draws"] % 2 == 0).all() and (fr["draws"] > 2 * key[5]).any()
        assert np.array_equal(got["rng"][dec], FT.states_after(O, states, fr["draws"])[dec]), "two uniforms per turn of the lens's loop"


def test_the_table_is_what_the_oracle_measures(P, O):
    """The maxima recorded in frame_truth.py, re-measured on the case that attains each."""
    worst = FT.measure(P, O, which={n for n, _ in FT.MEASURED.values()})
    for q, (name, value) in FT.MEASURED.items():
        assert abs(worst[q][1] - value) <= 0.02 * value, f"{q} on {name}: {worst[q][1]:.4g}, table says {value}"
        assert FT.TOL[q] == 4 * value


def test_the_named_terms_are_needed(P, O):
    """With the named cancellation terms left out of the units the same comparison gives the figures recorded beside them."""
    FT.NAMED_TERMS = False
    try:
        worst = FT.measure(P, O, which={n for n, _ in FT.WITHOUT_TERMS})
    finally:
        FT.NAMED_TERMS = True
    for (name, q), value in FT.WITHOUT_TERMS.items():
        assert abs(worst[q][1] - value) <= 0.02 * value, f"{q} on {name} without the terms: {worst[q][1]:.4g}, recorded {value}"
        assert value > 2 * FT.TOL[q]


# misreading -> (case, a quantity that must differ)
_P0, _P15, _P3 = "pinhole-70x33-whole-f0-s1", "pinhole-70x33-whole-f15-s1", "pinhole-70x33-whole-f14-s3"
_L0, _L15 = "lens-70x33-whole-f0-s1", "lens-70x33-whole-f15-s1"
SEEDED = dict(v_unflipped=(_P0, "depth"), no_pixel_centre=(_P0, "depth"), bn_unscaled=(_P0, "depth"), bn_uncentred=(_P0, "depth"),
              bn_transposed=(_P15, "depth"), bn_no_wrap=(_P15, "depth"),              # (frame 0's shift is 0: nothing wraps there)
              frame_not_plus_s=(_P3, "accum"), halton15_fixed=(_L15, "depth"), height_for_u=(_P0, "depth"),
              aperture_unhalved=(_L0, "depth"), lens_dir_unshifted=(_L0, "depth"), lens_uv_swapped=(_L0, "depth"),
              lens_one_draw=("far_lens-70x33-whole-f14-s3", "states"), gbuffer_last_sample=(_P3, "depth"), sum_not_mean=(_P3, "accum"),
              fov_full_angle=(_P0, "depth"), vertical_from_vup=(_P0, "depth"))


def test_every_misreading_has_a_case():
    assert set(SEEDED) == set(FT.MISREADINGS) and len(SEEDED) == 17


@pytest.mark.parametrize("mis", FT.MISREADINGS)
def test_a_seeded_misreading_is_caught(P, O, lab, mis):
    """The statement, misread on purpose, must disagree with the unchanged oracle on decided pixels beyond the table."""
    name, want = SEEDED[mis]
    key = CASES[IDS.index(name)]
    row, bad = FT.measure_case(P, O, lab, key, mis=mis, got=oracle_of(P, O, lab, key))
    caught = [q for q, v in row.items() if v > FT.TOL[q]] + [q for q, n in bad.items() if n]
    print(mis, name, caught)
    assert want in caught, f"{mis} on {name}: only {caught} differ"


# ---------------------------------------------------------------------------------------------------- identities (statement alone)
def test_a_pinholes_centre_ray_passes_through_its_point_of_the_viewport(lab):
    """Zero jitter (the entry 0.5 of both tables: taa 0, blue noise centred): the ray of pixel (x, y) passes through
    llc + (x + .5) / W h + (1 - (y + .5) / H) v."""
    W, H = 70, 33
    cam = FT.case_camera(("pinhole", W, H, "whole", 0, 1))
    x, y = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    n = len(x)
    X = {k: np.repeat(cam[k][None], n, axis=0) for k in FT.CAMERA_VECTORS if k != "w"}
    X.update(lens_radius=np.zeros(n), val=np.full((n, 2), 0.5), acc=np.zeros((n, 2)))
    held = dict(x=x, y=y, W=W, H=H, taa=np.zeros(2), shift=np.zeros(2), wrap=np.zeros((n, 2), bool), lens=False)
    r = FT._ray_fn(X, held)
    point = cam["lower_left_corner"] + ((x + 0.5) / W)[:, None] * cam["horizontal"] + (1.0 - (y + 0.5) / H)[:, None] * cam["vertical"]
    along = ((point - r["origin"]) * r["direction"]).sum(axis=1)
    assert np.abs(r["origin"] + along[:, None] * r["direction"] - point).max() < 1e-12 and (along > 0).all()
    assert np.abs(r["jitter"]).max() == 0.0


def test_rays_through_a_lens_meet_on_the_focus_plane():
    """Every lens sample's ray of one (u, v) passes through llc + u h + v vert, 7.5 in front of the camera."""
    cam = FT.case_camera(("lens", 96, 48, "whole", 0, 1))
    rs = np.random.RandomState(3)
    n = 4096
    uni = rs.random_sample((n, 2 * FT.TURNS)).astype(np.float32).astype(np.float64)
    table = np.full(64 * 64 * 2, 0.5, np.float32)
    o, d, draws = FT.primary_ray(cam, np.full(n, 40), np.full(n, 11), 96, 48, 3, 0, uni, table)
    one = FT.primary_ray_detail(cam, [40], [11], 96, 48, 3, 0, uni[:1], table)
    point = cam["lower_left_corner"] + one["u"][0] * cam["horizontal"] + one["v"][0] * cam["vertical"]
    along = ((point - o) * d).sum(axis=1)
    assert np.abs(o + along[:, None] * d - point).max() < 1e-12
    assert abs(((point - cam["origin"]) * -cam["w"]).sum() - 7.5) < 1e-5 and (draws % 2 == 0).all() and draws.max() > 2
    assert np.linalg.norm(o - cam["origin"], axis=1).max() <= cam["lens_radius"] and len(np.unique(o, axis=0)) > n // 2


def test_the_mean_lens_offset_is_zero():
    """65,536 pixels' first accepted pairs: the offset is uniform on the disk of radius lens_radius -- mean 0 within 5 sigma
    (sigma = r / 2 / sqrt(n) per axis), and a quarter of the samples in each quadrant."""
    cam = FT.case_camera(("lens", 96, 48, "whole", 0, 1))
    rs = np.random.RandomState(4)
    n = 65536
    uni = rs.random_sample((n, 2 * FT.TURNS)).astype(np.float32).astype(np.float64)
    o, _, _ = FT.primary_ray(cam, np.arange(n) % 96, (np.arange(n) // 96) % 48, 96, 48, 0, 0, uni, np.full(64 * 64 * 2, 0.5, np.float32))
    off = o - cam["origin"]
    a, b = off @ cam["u"], off @ cam["v"]
    sigma = cam["lens_radius"] / 2.0 / np.sqrt(n)
    assert abs(a.mean()) <= 5 * sigma and abs(b.mean()) <= 5 * sigma
    assert np.abs(off @ cam["w"]).max() < 1e-7                                     # (the stored u, v, w are rounded to float32)
    quad = np.bincount((a > 0) * 2 + (b > 0), minlength=4)
    assert np.abs(quad - n / 4).max() <= 5 * np.sqrt(n * 0.25 * 0.75)
