"""The analytic lights' one-bounce term at lightmap texels on the device (ptrt_query_bounce, ptrt_bounce_terms;
Scene.query_bounce).  Everything about the sums and the visibility at tolerance 0, compared as bytes: a texel's row must be the
numpy restatement (tests/bounce_restatement.py) of the values bounce_terms writes at the hits query_closest gives
irradiance_rays' rays, and of what query_occluded answers for bounce_terms' shadow rays -- under every traversal and both
material sets, for every segment width and group size at which padding, a partial last group, a group boundary and the chunked
path can go wrong, on a one-wave grid.  The terms are pinned by their parts: the light sample by direct_rays at the hit, the
value by a float32 composition of the device's own BSDF (ptrt_debug_shade); and against a float64 statement.  Exact properties;
the hole in a bake that the term closes; no trace left in the frames around a call; what must be refused is refused with
everything untouched."""
import ctypes as C

import numpy as np
import pytest

import bounce_restatement as B
import irradiance_restatement as R
import path_truth as PT
import shading_truth as T
from test_bounce import add_lab_lights
from test_direct_gpu import lab, slabs
from test_irradiance_gpu import PATTERN, assert_rows_equal, buffers, dev, texels
from test_ray_query_gpu import VARIANTS, as_hits, build

pytestmark = pytest.mark.gpu

W = H = 64
F = np.float32
OFFSET = F(1e-3)

_cache = {}


def scene(P, name):
    if name not in _cache:
        _cache[name] = lab(P) if name == "lab" else slabs(P) if name == "slabs" else build(P, name, W, H)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cached():
    yield
    for s in _cache.values():
        s.close()
    _cache.clear()


def chain(s, pos, nrm, s2, sh2, ph=None, lights=None, offset=OFFSET):
    """the unfused chain: irradiance_rays, query_closest, bounce_terms, query_occluded on the walked terms (a term that is not
    walked is replaced by a ray of length 0, which nothing blocks) -> (hits, directions, origins, L, tmax, values, flags)"""
    import torch
    k = len(s2)
    o, d = s.irradiance_rays(dev(pos), dev(nrm), dev(s2), offset=offset, phases=dev(ph))
    hits = s.query_closest(o, d)
    to, tl, tt, tv = s.bounce_terms(hits, d, k, dev(sh2), phases=dev(ph), lights=lights)
    walked = (tv > 0).any(dim=1)
    wo = torch.where(walked[:, None], to, torch.zeros_like(to)).contiguous()
    wd = torch.where(walked[:, None], tl, torch.tensor([0.0, 1.0, 0.0], device="cuda").expand_as(tl)).contiguous()
    wt = torch.where(walked, tt, torch.zeros_like(tt)).contiguous()
    flags = s.query_occluded(wo, wd, wt).cpu().numpy()
    assert not flags[~walked.cpu().numpy()].any()
    return as_hits(hits), d.cpu().numpy(), to.cpu().numpy(), tl.cpu().numpy(), tt.cpu().numpy(), tv.cpu().numpy(), flags


def unfused(s, pos, nrm, s2, sh2, ph=None, lights=None, offset=OFFSET):
    count = s.lightCount() if lights is None else lights[1]
    hits, d, to, tl, tt, tv, flags = chain(s, pos, nrm, s2, sh2, ph, lights, offset)
    assert tv.shape == (len(pos) * len(s2) * count * len(sh2), 3)
    return B.restate(tv, flags, hits, len(s2), len(sh2), count)


def fused(s, pos, nrm, s2, sh2, ph=None, lights=None, offset=OFFSET):
    return s.query_bounce(dev(pos), dev(nrm), dev(s2), dev(sh2), phases=dev(ph), offset=offset, lights=lights).cpu().numpy()


def slab_texels(P, n):
    """texels on the plane y = 0 under the three slabs, facing up: their gather rays meet the slabs' undersides or leave"""
    pos, nrm = P.lightmap.quad_texels((-5.0, 0.0, 2.0), (10.0, 0, 0), (0, 0, -10.0), 7, 6)
    assert np.array_equal(nrm[0], F([0, 1, 0]))
    return np.ascontiguousarray(pos[:n]), np.ascontiguousarray(nrm[:n])


def scene_texels(P, name, n):
    return slab_texels(P, n) if name == "slabs" else texels(P, "cornell" if name == "lab" else name, n)


# ---- 1. the restatement, as bytes ---------------------------------------------------------------------------------------------
def check_restatement(P, s, name):
    n, k, m = 37, 4, 2
    pos, nrm = scene_texels(P, name, n)
    s2, sh2, ph = P.lightmap.hammersley2(k), P.lightmap.hammersley2(m), P.lightmap.texel_phases(n, 3)
    want = unfused(s, pos, nrm, s2, sh2, ph)
    got = fused(s, pos, nrm, s2, sh2, ph)
    pm = s.get_option("query_pmode")
    assert_rows_equal(got, want, name)
    assert not got[:, 6:].any()
    f = P.bounce_fields(got)
    assert (f["lit_fraction"] >= 0).all() and (f["lit_fraction"] + f["shadowed_fraction"] <= 1).all()
    assert (f["hit_fraction"] > 0).any() and (f["hit_fraction"] <= 1).all()
    return pm, got


@pytest.mark.parametrize("full", [0, 1], ids=["force_full=0", "force_full=1"])
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
def test_cornell_equals_the_restatement_under_every_variant(P, fg, pt, full):
    s = scene(P, "cornell")
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    s.set_option("force_full", full)
    try:
        pm, got = check_restatement(P, s, "cornell")
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)
        s.set_option("force_full", 0)
    assert pm == (0 if pt == 0 else {-1: 1, 1: 2, 2: 3}[fg])
    assert got[:, :3].any() and (got[:, 3] > 0).any()


@pytest.mark.parametrize("name", ["showcase", "many", "fluid", "lab", "slabs"])
def test_scenes_equal_the_restatement(P, name):
    s = scene(P, name)
    pm, got = check_restatement(P, s, name)
    if name == "many":
        assert pm == 3
    if name != "slabs":
        assert got[:, :3].any() and (got[:, 3] > 0).any()


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------
# Q -> ((first light, light count), shadow samples) on the lab's five lights
TERMS = {1: ((0, 1), 1), 5: ((0, 5), 1), 10: ((0, 5), 2)}


@pytest.mark.parametrize("Q", sorted(TERMS))
@pytest.mark.parametrize("n_dirs", [1, 3, 4, 16, 17, 33, 64, 65, 130])
def test_shapes(P, n_dirs, Q):
    """Per direction count, with g = 64 / w texels per wave (1 beyond 64 directions): 1, g - 1, g, g + 1 and 2 g + 1 texels --
    segment padding, a partial last group, a full one, a group boundary, and more than two groups -- at 1, 5 and 10 terms per
    ray."""
    s = scene(P, "lab")
    lights, m = TERMS[Q]
    assert lights[1] * m == Q
    g = 64 // R.width(n_dirs) if n_dirs <= 64 else 1
    s2, sh2 = P.lightmap.hammersley2(n_dirs), P.lightmap.hammersley2(m)
    lit = False
    for n in sorted({1, g - 1, g, g + 1, 2 * g + 1} - {0}):
        pos, nrm = texels(P, "cornell", n)
        ph = P.lightmap.texel_phases(n, n_dirs)
        want = unfused(s, pos, nrm, s2, sh2, ph, lights)
        got = fused(s, pos, nrm, s2, sh2, ph, lights)
        assert_rows_equal(got, want, f"{n} x {n_dirs} x {Q}")
        lit = lit or bool(got[:, :3].any())
    assert lit


def test_a_grid_of_one_wave_per_cu(P):
    """Option persist = 1 sizes the grid to one one-wave workgroup per CU; a batch of three more groups than the chip has CUs
    makes three of them stride twice, and the rows stay the restatement's."""
    import torch
    s = scene(P, "lab")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k, m, lights = 16, 1, (0, 2)    # four texels per wave
    n = 4 * (cus + 3)               # n_cus + 3 groups: with persist 1 the grid is one wave per CU, three of them stride twice
    pos, nrm = texels(P, "cornell", n)
    rs = np.random.RandomState(5)
    pos = (pos + rs.uniform(-0.04, 0.04, pos.shape) * (1 - np.abs(nrm))).astype(np.float32)  # (moved within their planes)
    s2, sh2 = P.lightmap.hammersley2(k), P.lightmap.hammersley2(m)
    want = unfused(s, pos, nrm, s2, sh2, None, lights)
    s.set_option("persist", 1)
    try:
        narrow = fused(s, pos, nrm, s2, sh2, None, lights)
    finally:
        s.set_option("persist", 0)
    wide = fused(s, pos, nrm, s2, sh2, None, lights)
    assert_rows_equal(narrow, want, "persist 1 vs the restatement")
    assert_rows_equal(wide, want, "the default grid vs the restatement")
    assert len(np.unique(wide[:, :3], axis=0)) > n // 2  # other places, other texels


# ---- 3. the terms are pinned by their parts -------------------------------------------------------------------------------------
def lights_of(P, s):
    desc = s.flatten()
    nl = int(desc.contents.light_count)
    return PT.lights64(desc.contents.lights, nl), nl, desc


def test_the_lab_is_the_cpu_tests_lab(P):
    """tests/test_bounce.py measures the statement's undecided share on a host-only Cornell with add_lab_lights: the same lights"""
    got, nl, _ = lights_of(P, scene(P, "lab"))
    h = P.Scene(W, H, device=P.HOST_ONLY)
    P.scenes.cornell(h)
    add_lab_lights(h)
    want, nl2, _ = lights_of(P, h)
    assert nl == nl2 == 5 and all(np.array_equal(got[k], want[k]) for k in want)
    h.close()


@pytest.mark.parametrize("full", [0, 1], ids=["force_full=0", "force_full=1"])
def test_terms_are_pinned_by_their_parts(P, O, full):
    """L and tmax of bounce_terms are direct_rays' at (hit.point, hit.normal) with the texel's phase repeated per ray (the
    sample is sample_light's in both); the origin is the path's; the value is value32 of the device's own evaluateBSDF
    (ptrt_debug_shade op 0 for (mesh, N, V, L, front_face)) and the light's radiance, attenuation and density restated in
    float32, times the Beer-Lambert factor behind a back face; a miss is a row of zeros."""
    s = scene(P, "lab")
    n, k, m = 23, 4, 2
    pos, nrm = texels(P, "cornell", n)
    s2, sh2, ph = P.lightmap.hammersley2(k), P.lightmap.hammersley2(m), P.lightmap.texel_phases(n, 11)
    lights, nl, desc = lights_of(P, s)
    albedo = T.load_materials(desc.contents.materials)["albedo"]
    Q = nl * m
    s.set_option("force_full", full)
    try:
        hits, d, to, tl, tt, tv, _ = chain(s, pos, nrm, s2, sh2, ph)
        struck = hits["hit"] != 0
        assert struck.any() and (~struck).any()
        point, normal = np.ascontiguousarray(hits["point"]), np.ascontiguousarray(hits["normal"])
        ro, rl, rt, _ = s.direct_rays(dev(point), dev(normal), dev(sh2), phases=dev(np.repeat(ph, k)), offset=1e-4)
        rows = np.repeat(struck, Q)
        assert np.array_equal(tl[rows].view(np.uint32), rl.cpu().numpy()[rows].view(np.uint32))
        assert np.array_equal(tt[rows].view(np.uint32), rt.cpu().numpy()[rows].view(np.uint32))
        # the path's shadow origin: the hit's point plus or minus normal * 1e-4f by the side of the light
        N, Pt = np.repeat(normal, Q, axis=0), np.repeat(point, Q, axis=0)
        side = np.array([B.dot32(a, b) for a, b in zip(N[rows], tl[rows])]) > 0
        want_o = np.where(side[:, None], Pt[rows] + N[rows] * F(1e-4), Pt[rows] + (-N[rows]) * F(1e-4))
        assert want_o.dtype == np.float32 and np.array_equal(to[rows].view(np.uint32), want_o.view(np.uint32))
        assert side.any() and (~side).any()
        # misses: rows of zero bytes
        for a in (to, tl, tv):
            assert not a[~rows].view(np.uint32).any()
        assert not tt[~rows].view(np.uint32).any()
        # the value
        V = np.repeat(-d, Q, axis=0)
        mesh, ff = np.repeat(hits["mesh_index"], Q), np.repeat(hits["front_face"], Q)
        x = np.concatenate([mesh[rows, None].astype(F), N[rows], V[rows], tl[rows], ff[rows, None].astype(F)], axis=1).astype(F)
        out = np.zeros((len(x), 4), F)
        fp = C.POINTER(C.c_float)
        P.lib.ptrt_debug_shade.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, C.c_int, fp]
        s.sync()
        rc = P.lib.ptrt_debug_shade(s.ctx, 0, full, np.ascontiguousarray(x).ctypes.data_as(fp), len(x), out.ctypes.data_as(fp))
        assert rc == 0, P.lib.ptrt_last_error(s.ctx)
    finally:
        s.set_option("force_full", 0)
    q = np.tile(np.arange(Q), n * k)[rows]
    pieces = [B.light_pieces32(lights, int(j), p, L) for j, p, L in zip(q // m, Pt[rows], tl[rows])]
    radiance = np.array([p[0] for p in pieces], F)
    att, pdf, tmax = (np.array([p[i] for p in pieces], F) for i in (1, 2, 3))
    assert np.array_equal(tmax.view(np.uint32), tt[rows].view(np.uint32))
    thr = B.throughput32(O, albedo[mesh[rows]], np.repeat(hits["t"], Q)[rows], ff[rows])
    print(f"terms by their parts: {len(x)} terms, {int((ff[rows] == 0).sum())} of them behind a back face")
    want_v = B.value32(out[:, :3], radiance, att, pdf, thr)
    got_v = tv[rows]
    same = (got_v.view(np.uint32) == want_v.view(np.uint32)) | (np.isnan(got_v) & np.isnan(want_v))
    bad = np.argwhere(~same)
    assert bad.size == 0, f"{len(bad)} of {same.size} words differ, first {bad[:4].tolist()}: {got_v[tuple(bad[0])]!r} vs {want_v[tuple(bad[0])]!r}"
    assert (got_v > 0).any() and B.walked32(got_v).reshape(-1, nl, m).any(axis=(0, 2)).all()  # every light lights some hit


# ---- 4. the terms against float64 -----------------------------------------------------------------------------------------------
def test_terms_against_the_float64_statement(P):
    """bounce_terms on the lab within bounce_restatement.margins of statement64 on the terms it decides; at most 2 % undecided."""
    s = scene(P, "lab")
    n, k, m = B.STATEMENT_TEXELS, B.STATEMENT_DIRS, B.STATEMENT_SHADOW
    pos, nrm = texels(P, "cornell", n)
    s2, sh2, ph, _, _ = B.statement_rays(P, pos, nrm)
    lights, nl, desc = lights_of(P, s)
    hits, d, to, tl, tt, tv, _ = chain(s, pos, nrm, s2, sh2, ph, offset=F(1e-4))
    st, decided = B.statement64(hits, d, lights, T.load_materials(desc.contents.materials), 0, nl, sh2, ph, k, m)
    share = 1.0 - decided.mean()
    print(f"bounce_terms: {share:.4f} of {len(decided)} terms undecided")
    assert share <= B.MAX_UNDECIDED
    E, rows = st["E"], st["rows"]
    light = (rows % (nl * m)) // m
    for name, got, want, bound in (("L", tl[rows], st["L"], E["L"][:, None]), ("tmax", tt[rows], st["tmax"], E["tmax"]),
                                   ("value", tv[rows], st["value"], E["value"])):
        err = np.abs(got.astype(np.float64) - want)
        ok = decided if err.ndim == 1 else decided[:, None]
        ratio = np.where(ok, err / np.maximum(bound, 1e-300), 0.0)
        ratio = np.where(ok & (err == 0), 0.0, ratio)
        worst = np.unravel_index(np.argmax(ratio), ratio.shape)[0]
        print(f"bounce_terms: {name}: worst error / margin {ratio.max():.3f} (light {light[worst]}, error {np.max(err[worst]):.3e}); "
              f"largest error {np.where(ok, err, 0.0).max():.3e}; per light " + ", ".join(f"{ratio[light == j].max():.3f}" for j in range(nl)))
        assert ratio.max() <= 1.0, name
    # walked where the statement says so, on the terms it decides; the origin is on the light's side of the hit
    w = B.walked32(tv[rows])
    assert np.array_equal(w[decided], st["walked"][decided]) and w[decided].any() and (~w[decided]).any()
    err_o = np.abs(to[rows].astype(np.float64) - st["origin"])[decided]
    assert err_o.max() <= 2.0 ** -23 * np.abs(st["origin"][decided]).max() + 1e-4 * 2.0 ** -23


# ---- 5. exact properties --------------------------------------------------------------------------------------------------------
def test_no_lights_asked_for_is_zero_bytes(P):
    import torch
    s = scene(P, "lab")
    pos, nrm = texels(P, "cornell", 9)
    s2, sh2 = dev(P.lightmap.hammersley2(4)), dev(P.lightmap.hammersley2(2))
    out = torch.full((9, 8), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    assert s.query_bounce(dev(pos), dev(nrm), s2, sh2, lights=(0, 0), out=out) is out
    assert not out.view(torch.int32).cpu().numpy().any()
    assert not s.query_bounce(dev(pos), dev(nrm), s2, sh2, lights=(3, 0)).view(torch.int32).cpu().numpy().any()
    o, d = s.irradiance_rays(dev(pos), dev(nrm), s2)
    to, tl, tt, tv = s.bounce_terms(s.query_closest(o, d), d, 4, sh2, lights=(0, 0))
    assert to.shape == tv.shape == (0, 3) and tt.shape == (0,)


def test_per_light_ranges_sum_to_the_full_range(P):
    """n_dirs <= 64, so a texel's radiance is fold(B) / n_dirs with B = S / n_shadow, S a ray's running sum over q.  The full
    range's S and the sum of the per-light S differ by the running sum's roundings: at most (Q - 1) u of the sum of the terms
    taken absolute; each B adds its division (u), each fold log2(w) u, each texel its last division (u), and adding the
    lights' rows in float64 adds nothing: |full - sum of the ranges| <= 1.01 (2 (Q + 1 + log2 w) u) M, M the full range's
    sum of absolute terms under the same divisors -- all terms are >= 0, so M is the row itself in float64.  The counts are
    whole numbers: the fractions times n_dirs * Q add up exactly."""
    s = scene(P, "lab")
    n, k, m = 21, 16, 2
    nl = s.lightCount()
    Q = nl * m
    pos, nrm = texels(P, "cornell", n)
    s2, sh2, ph = P.lightmap.hammersley2(k), P.lightmap.hammersley2(m), P.lightmap.texel_phases(n, 4)
    full = fused(s, pos, nrm, s2, sh2, ph).astype(np.float64)
    parts = [fused(s, pos, nrm, s2, sh2, ph, (j, 1)).astype(np.float64) for j in range(nl)]
    total = sum(p[:, :3] for p in parts)
    u = 2.0 ** -24
    bound = 1.01 * 2 * (Q + 1 + np.log2(R.width(k))) * u * np.maximum(full[:, :3], total)
    err = np.abs(full[:, :3] - total)
    print(f"per-light ranges: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all() and full[:, :3].any()
    for col in (3, 4):
        counts = sum(np.rint(p[:, col] * (k * m)) for p in parts)
        assert np.array_equal(np.rint(full[:, col] * (k * Q)), counts)
    assert all(np.array_equal(p[:, 5], full[:, 5]) for p in parts)


def test_doubling_every_intensity_doubles_every_unclamped_row(P):
    """radiance = colour x intensity, and every later operation of a term is a product, a quotient or a sum: a factor of two
    passes through all of them exactly unless the soft clamp's threshold lies between a term and its double."""
    s = lab(P)
    try:
        n, k, m = 21, 4, 2
        pos, nrm = texels(P, "cornell", n)
        s2, sh2, ph = P.lightmap.hammersley2(k), P.lightmap.hammersley2(m), P.lightmap.texel_phases(n, 6)
        desc = s.flatten()
        nl = int(desc.contents.light_count)
        once = fused(s, pos, nrm, s2, sh2, ph)
        arr = (P.Light * nl)()
        for j in range(nl):
            C.memmove(C.byref(arr[j]), C.byref(desc.contents.lights[j]), C.sizeof(P.Light))
            arr[j].intensity = 2.0 * arr[j].intensity
        s.sync()
        assert P.lib.ptrt_upload_lights(s.ctx, arr, nl) == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        twice = fused(s, pos, nrm, s2, sh2, ph)
        hits, _, _, _, _, tv, _ = chain(s, pos, nrm, s2, sh2, ph)      # the doubled terms
        # in front of a face the throughput is 1 and the value is the clamped product itself; a texel with a ray that ends
        # behind one is left out (its clamp cannot be read off the value)
        front = ((hits["hit"] == 0) | (hits["front_face"] == 1)).reshape(n, -1).all(axis=1)
        lum = F(0.2126) * tv[:, 0] + F(0.7152) * tv[:, 1] + F(0.0722) * tv[:, 2]
        unclamped = front & (np.nan_to_num(lum, nan=0.0).reshape(n, -1) < 499.0).all(axis=1)
        assert unclamped.sum() > n // 2
        assert_rows_equal(twice[unclamped][:, :3], (F(2.0) * once[unclamped][:, :3]).astype(F), "twice the intensity")
        assert_rows_equal(twice[:, 3:], once[:, 3:], "the fractions")
        assert once[unclamped][:, :3].any()
    finally:
        s.close()


def test_a_texel_whose_rays_all_miss_has_a_zero_row(P):
    s = scene(P, "lab")
    # outside the box's open side, looking away from it
    pos, nrm = F([[0.0, 0.0, 6.0], [1.0, 1.0, 8.0]]), F([[0, 0, 1], [0, 0, 1]])
    got = fused(s, pos, nrm, P.lightmap.hammersley2(16), P.lightmap.hammersley2(2))
    assert not got.view(np.uint32).any()


def test_transmission_and_an_opaque_slab(P):
    """The slabs over a floor: a texel hovering above the floor looks down, its gather rays end on the floor, and each hit's
    shadow ray crosses the slab between it and the light -- the slab that transmits 0.9 does not block, the opaque one does."""
    s = slabs(P)
    try:
        a, b, c, d = (-8.0, 0.0, -10.0), (8.0, 0.0, -10.0), (8.0, 0.0, 4.0), (-8.0, 0.0, 4.0)
        s.addTriangles([a + d + c, a + c + b], P.Material((0.7, 0.7, 0.7), 0.6))   # normal +y
        s.uploadToGPU()
        down = [0, -1, 0]
        pos, nrm = F([[-3, 0.02, 0], [1.0, 0.02, -6]]), F([down, down])
        s2, sh2 = P.lightmap.hammersley2(8), P.lightmap.hammersley2(1)
        glass = P.bounce_fields(fused(s, pos[0:1], nrm[0:1], s2, sh2, lights=(0, 1)))
        assert glass["hit_fraction"][0] == 1 and glass["lit_fraction"][0] == 1 and glass["shadowed_fraction"][0] == 0
        assert glass["radiance"][0].all()
        solid = P.bounce_fields(fused(s, pos[1:2], nrm[1:2], s2, sh2, lights=(2, 1)))
        assert solid["hit_fraction"][0] == 1 and solid["lit_fraction"][0] == 0 and solid["shadowed_fraction"][0] == 1
        assert not solid["radiance"][0].any()
        assert_rows_equal(fused(s, pos, nrm, s2, sh2), unfused(s, pos, nrm, s2, sh2), "slabs over a floor")
    finally:
        s.close()


# ---- 6. the hole is closed --------------------------------------------------------------------------------------------------------
def test_the_hole_in_a_bake_is_closed(P):
    """Cornell with its lamp's emission off and no sky, gathered to max_depth 1: a gather ray ends at its first hit, where it
    takes no light sample, so query_irradiance is zero everywhere -- the point light's whole indirect term is missing.
    query_bounce has it: the floor's texels are lit off the walls, and full_irradiance is direct + pi * bounce there."""
    s = P.Scene(W, H)
    P.scenes.cornell(s)
    s.setMeshMaterial(5, P.Material(albedo=(0.0, 0.0, 0.0), roughness=0.0))   # the lamp: no emission
    s.uploadToGPU()
    try:
        n, k = 35, 16
        floor = P.lightmap.quad_texels((-4.95, -4.95, -9.95), (0, 0, 9.0), (9.9, 0, 0), 7, 5)
        pos, nrm = floor
        s2, sh2, ph = P.lightmap.hammersley2(k), P.lightmap.hammersley2(1), P.lightmap.texel_phases(n, 8)
        states = s.init_rng_states(12345, 0, n * k)
        gather = s.query_irradiance(dev(pos), dev(nrm), dev(s2), states, samples=1, max_depth=1, phases=dev(ph), offset=OFFSET).cpu().numpy()
        assert not gather[:, :3].view(np.uint32).any() and (gather[:, 5] > 0).all()
        bounce = fused(s, pos, nrm, s2, sh2, ph)
        # (the boxes stand IN the floor slab: a texel under one lies inside it, every one of its rays ends behind a face, on the
        # box's inside, which no light reaches -- a baker's invalid texels; the floor in the open is what the term lights)
        hits = chain(s, pos, nrm, s2, sh2, ph)[0]
        covered = ((hits["hit"] != 0) & (hits["front_face"] == 0)).reshape(n, k).all(axis=1)
        print(f"the hole: {int(covered.sum())} of {n} floor texels under a box")
        assert 0 < covered.sum() < n // 4
        assert (bounce[~covered][:, :3] > 0).all() and (bounce[~covered][:, 3] > 0).all()
        assert not bounce[covered][:, :4].any() and (bounce[covered][:, 5] == 1).all()   # (walked or not, every sample is blocked)
        direct = s.query_direct(dev(pos), dev(nrm), dev(sh2), phases=dev(ph)).cpu().numpy()
        full = P.lightmap.full_irradiance(direct, gather, bounce)
        assert np.array_equal(full.view(np.uint32), (direct[:, :3] + F(np.pi) * bounce[:, :3]).view(np.uint32))
        assert (full[~covered] > P.lightmap.total_irradiance(direct, gather)[~covered]).all()
        assert_rows_equal(bounce, unfused(s, pos, nrm, s2, sh2, ph), "the unlit Cornell")
    finally:
        s.close()


# ---- 7. no trace ------------------------------------------------------------------------------------------------------------------
def test_guard_rows(P):
    """`d_out` and the four term targets between pattern rows, before and after: the rows stay."""
    import torch
    s = scene(P, "lab")
    vp = C.c_void_p
    for n, k, lights, m in ((5, 12, (0, 3), 2), (3, 70, (1, 2), 1)):  # segments of 16 with a partial group; the chunked path with a tail chunk
        Q = lights[1] * m
        pos, nrm = texels(P, "cornell", n)
        s2, sh2, ph = P.lightmap.hammersley2(k), P.lightmap.hammersley2(m), P.lightmap.texel_phases(n, 2)
        batch = fused(s, pos, nrm, s2, sh2, ph, lights)
        G = 3
        rows = n * k * Q
        out = torch.full((n + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
        ro, rl, rv = (torch.full((rows + 2 * G, 3), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3))
        rt = torch.full((rows + 2 * G,), PATTERN, dtype=torch.int32, device="cuda")
        tp, tn, ts, tsh, tph = dev(pos), dev(nrm), dev(s2), dev(sh2), dev(ph)
        rc = P.lib.ptrt_query_bounce(s.ctx, vp(tp.data_ptr()), vp(tn.data_ptr()), n, vp(ts.data_ptr()), k, vp(tph.data_ptr()),
                                     C.c_float(OFFSET), vp(tsh.data_ptr()), m, lights[0], lights[1], vp(out[G:].data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        o, d = s.irradiance_rays(tp, tn, ts, offset=OFFSET, phases=tph)
        hits = s.query_closest(o, d)
        rc = P.lib.ptrt_bounce_terms(s.ctx, vp(hits.data_ptr()), vp(d.data_ptr()), n, k, vp(tsh.data_ptr()), m, vp(tph.data_ptr()),
                                     lights[0], lights[1], vp(ro[G:].data_ptr()), vp(rl[G:].data_ptr()), vp(rt[G:].data_ptr()),
                                     vp(rv[G:].data_ptr()))
        assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)
        s.sync()
        for name, t, cnt in (("out", out, n), ("origins", ro, rows), ("L", rl, rows), ("tmax", rt, rows), ("values", rv, rows)):
            assert (t[:G] == PATTERN).all() and (t[G + cnt:] == PATTERN).all(), f"{name}: a write outside the batch"
            assert not (t[G:G + cnt] == PATTERN).all(dim=-1).any(), f"{name}: a row not written"
        assert_rows_equal(out[G:G + n].view(torch.float32).cpu().numpy(), batch, "raw call")
        to, tl, tt, tv = s.bounce_terms(hits, d, k, tsh, phases=tph, lights=lights)
        assert torch.equal(ro[G:G + rows], to.view(torch.int32)) and torch.equal(rl[G:G + rows], tl.view(torch.int32))
        assert torch.equal(rt[G:G + rows], tt.view(torch.int32)) and torch.equal(rv[G:G + rows], tv.view(torch.int32))


def test_a_bake_between_frames_changes_nothing(P, O, blue_noise):
    import torch
    from common import render_both
    runs = []
    for with_bake in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        lhist = [x.tobytes() for x in s.launch_ms_history()]
        rng = s.read(P.BUF_RNG)
        stats = s.stats()
        if with_bake:
            pos, nrm = texels(P, "cornell", 70)
            s2, sh2 = dev(P.lightmap.hammersley2(4)), dev(P.lightmap.hammersley2(2))
            rows = s.query_bounce(dev(pos), dev(nrm), s2, sh2)
            o, d = s.irradiance_rays(dev(pos), dev(nrm), s2)
            to, tl, tt, tv = s.bounce_terms(s.query_closest(o, d), d, 4, sh2)
            torch.cuda.synchronize()
            assert rows.shape == (70, 8) and rows[:, :3].any() and to.shape == tl.shape == tv.shape == (70 * 4 * 2, 3)
            assert s.kernel_ms_history().tobytes() == hist
            assert [x.tobytes() for x in s.launch_ms_history()] == lhist
            assert np.array_equal(s.read(P.BUF_RNG), rng) and s.stats() == stats
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), n_hist=len(s.kernel_ms_history()),
                         n_lhist=len(s.launch_ms_history()[0])))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["n_hist"] == b["n_hist"] and a["n_lhist"] == b["n_lhist"]


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    q, terms = P.lib.ptrt_query_bounce, P.lib.ptrt_bounce_terms
    vp, cf = C.c_void_p, C.c_float
    INVALID, NOT_READY = -1, -4
    n, k, m = 3, 8, 2
    pos = torch.tensor([[0.0, -4.95, -5.0], [0.3, -4.95, -2.0], [1.0, -4.95, -3.0]], device="cuda")  # on the Cornell floor
    nrm = torch.tensor([0.0, 1.0, 0.0], device="cuda").repeat(n, 1)
    s2, sh2 = dev(P.lightmap.hammersley2(k)), dev(P.lightmap.hammersley2(m))
    ph = torch.zeros(n, device="cuda")
    rows = n * k * m
    out = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    ro, rl, rv = (torch.full((rows, 3), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3))
    rt = torch.full((rows,), PATTERN, dtype=torch.int32, device="cuda")
    hits = torch.zeros((n * k, 16), dtype=torch.int32, device="cuda")     # (misses, until the scene fills them)
    dirs = torch.zeros((n * k, 3), device="cuda")
    pp, pn, ps2, psh, pph, pout, pro, prl, prt, prv, ph_, pd = (vp(x.data_ptr()) for x in (pos, nrm, s2, sh2, ph, out, ro, rl, rt, rv, hits, dirs))
    off = cf(1e-4)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((x == PATTERN).all()) for x in (out, ro, rl, rt, rv))

    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    assert q(ctx, pp, pn, n, ps2, k, pph, off, psh, m, 0, 0, pout) == NOT_READY          # no geometry, no materials
    assert b"ptrt_query_bounce" in P.lib.ptrt_last_error(ctx)
    assert terms(ctx, ph_, pd, n, k, psh, m, pph, 0, 0, pro, prl, prt, prv) == NOT_READY  # no materials
    assert b"ptrt_bounce_terms" in P.lib.ptrt_last_error(ctx)
    assert q(ctx, pp, pn, n, ps2, k, pph, off, psh, m, 0, 1, pout) == INVALID             # (and no lights: the range is refused first)
    assert terms(ctx, ph_, pd, n, k, psh, m, pph, 0, 1, pro, prl, prt, prv) == INVALID
    assert untouched()
    P.lib.ptrt_destroy(ctx)
    assert q(ctx, pp, pn, n, ps2, k, pph, off, psh, m, 0, 0, pout) == INVALID             # a destroyed context
    assert terms(ctx, ph_, pd, n, k, psh, m, pph, 0, 0, pro, prl, prt, prv) == INVALID
    s = build(P, "cornell", 32, 32)
    c = s.ctx
    host = np.zeros((rows, 16), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((n, 8), dtype=torch.int32).pin_memory()
    # device memory that ends before the call's last element: an allocation of the runtime's own ends where it ends
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    inf, nan = float("inf"), float("nan")
    big = 2 ** 31 - 1
    Qa = dict(c=c, pos=pp, nrm=pn, n=n, s2=ps2, k=k, ph=pph, off=off, sh=psh, m=m, first=0, count=1, out=pout)
    order = ("c", "pos", "nrm", "n", "s2", "k", "ph", "off", "sh", "m", "first", "count", "out")
    bad_q = [dict(n=-1), dict(k=0), dict(k=-3), dict(m=0), dict(m=-1), dict(first=-1), dict(count=-1), dict(count=2), dict(first=1),
             dict(first=big, count=big),
             dict(pos=None), dict(nrm=None), dict(s2=None), dict(sh=None), dict(out=None),                              # NULL
             dict(pos=hp), dict(nrm=hp), dict(s2=hp), dict(ph=hp), dict(sh=hp), dict(out=hp),                          # host memory
             dict(out=vp(pinned.data_ptr())),                                                                          # pinned host memory
             dict(pos=tail(n * 12 - 12)), dict(nrm=tail(n * 12 - 12)), dict(s2=tail(k * 8 - 8)), dict(ph=tail(n * 4 - 4)),
             dict(sh=tail(m * 8 - 8)), dict(out=tail(n * 32 - 4)),                                                     # short buffers
             dict(m=big), dict(k=big, m=2), dict(k=1 << 16, m=1 << 15),                                                # Q, n_dirs * Q beyond 2^31 - 1
             dict(off=cf(nan)), dict(off=cf(inf)), dict(off=cf(-inf)), dict(c=None)]
    for change in bad_q:
        args = dict(Qa, **change)
        assert q(*[args[a] for a in order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_query_bounce" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    Ta = dict(c=c, hits=ph_, d=pd, n=n, k=k, sh=psh, m=m, ph=pph, first=0, count=1, o=pro, l=prl, t=prt, v=prv)
    t_order = ("c", "hits", "d", "n", "k", "sh", "m", "ph", "first", "count", "o", "l", "t", "v")
    h1 = n * k  # rays, and rows with one light and one sample
    bad_t = [dict(n=-1), dict(k=0), dict(m=0), dict(first=-1), dict(count=-1), dict(count=2), dict(first=1),
             dict(hits=None), dict(d=None), dict(sh=None), dict(o=None), dict(l=None), dict(t=None), dict(v=None),
             dict(hits=hp), dict(d=hp), dict(sh=hp), dict(ph=hp), dict(o=hp), dict(l=hp), dict(t=hp), dict(v=hp),
             dict(hits=tail(h1 * 64 - 64)), dict(d=tail(h1 * 12 - 12)), dict(sh=tail(m * 8 - 8)), dict(ph=tail(n * 4 - 4)),
             dict(o=tail(rows * 12 - 12)), dict(l=tail(rows * 12 - 4)), dict(t=tail(rows * 4 - 4)), dict(v=tail(rows * 12 - 4)),
             dict(m=big), dict(k=big, m=2), dict(n=big, k=big, m=1), dict(n=big, k=1 << 20, m=1 << 10), dict(n=big, k=300, m=1),
             # (terms per texel; 2^62 rays; a byte count past size_t; more rows than the grid holds)
             dict(c=None)]
    for change in bad_t:
        args = dict(Ta, **change)
        assert terms(*[args[a] for a in t_order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_bounce_terms" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    hip.hipFree(block)
    assert q(c, pp, pn, 0, ps2, k, pph, off, psh, m, 0, 1, pout) == P.PTRT_OK           # n_texels == 0: nothing launched
    assert terms(c, ph_, pd, 0, k, psh, m, pph, 0, 1, pro, prl, prt, prv) == P.PTRT_OK
    assert untouched()
    assert s.get_option("query_pmode") == -1                                             # (and no refusal set it)
    assert q(c, pp, pn, n, ps2, k, None, off, psh, m, 0, 1, pout) == P.PTRT_OK          # and the calls that are in order run
    assert terms(c, ph_, pd, n, k, psh, m, None, 0, 1, pro, prl, prt, prv) == P.PTRT_OK
    s.sync()
    assert not bool((out == PATTERN).any()) and bool((out[:, 6:] == 0).all())
    assert not any(bool((x == PATTERN).any()) for x in (ro, rl, rt, rv))
    assert bool((rv == 0).all())                                                         # (the records were misses)
    assert s.get_option("query_pmode") == 1

    # the binding
    with pytest.raises(ValueError):
        s.query_bounce(pos.cpu(), nrm.cpu(), s2.cpu(), sh2.cpu())
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm[:2], s2, sh2)
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm, s2[:0], sh2)
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm, s2, sh2[:0])
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm, s2, sh2, phases=ph[:2])
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm, s2, sh2, phases=ph.cpu())
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm, s2, sh2, out=torch.zeros((n + 1, 8), device="cuda"))
    with pytest.raises(ValueError):
        s.query_bounce(pos, nrm, s2, sh2, lights=(0, 2))
    with pytest.raises(ValueError):
        s.bounce_terms(hits, dirs[:5], k, sh2)
    with pytest.raises(ValueError):
        s.bounce_terms(hits, dirs, 5, sh2)
    with pytest.raises(P.PtrtError):
        s.query_bounce(pos, nrm, s2, sh2, offset=nan)
    keep = torch.zeros((n, 8), device="cuda")
    assert s.query_bounce(pos, nrm, s2, sh2, out=keep) is keep
    assert s.query_bounce(pos, nrm, s2).shape == (n, 8)                                  # shadow2=None: one sample per light
    assert s.query_bounce(pos[:0], nrm[:0], s2, sh2).shape == (0, 8)
    to, tl, tt, tv = s.bounce_terms(hits[:0], dirs[:0], k, sh2)
    assert to.shape == tl.shape == tv.shape == (0, 3) and tt.shape == (0,)
    s.close()
