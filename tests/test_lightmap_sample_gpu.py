"""Baked lightmaps read back at ray hits on the device (ptrt_atlas_sample, ptrt_query_lightmap; Scene.atlas_sample /
query_lightmap).  Every comparison with the numpy restatement (tests/lightmap_sample_restatement.py) is words, tolerance 0:
query_lightmap equals atlas_sample over query_closest's records and both equal the restatement, under every traversal the
queries have, at the batch sizes round a wave, in both modes, over atlases smaller and larger than the charts, with chart
tables that lack a mesh, end inside one and hold corners outside the atlas and a NaN, and images whose invalid texels carry
NaN and infinity.  Independently of that statement, a ray shot back at a texel finds that texel, and bilinear over a face's
own texels returns the hit's world point.  Moved geometry is followed; what must be refused is refused with every byte
untouched; frames around a call do not notice it; a whole bake, viewed through the camera, holds together."""
import ctypes as C

import numpy as np
import pytest

import lightmap_sample_restatement as R
from test_atlas_gpu import authored
from test_irradiance_gpu import PATTERN, buffers, dev
from test_ray_query_gpu import RADIUS, VARIANTS, ray_set

pytestmark = pytest.mark.gpu

F = np.float32
EPS = float(np.finfo(np.float32).eps)
ATLASES = [(1, 1), (67, 5), (33, 40)]
NS = (1, 63, 64, 65, 4097)
MODES = ("nearest", "bilinear")
TRI, CUBE, XCUBE, SPHERE, BALL = range(5)  # the lab's meshes
RAY_SEED, IMAGE_SEED = 11, 7               # chosen on the CPU, with the oracle's hits: test_the_lab_is_not_vacuous holds for them

_lab = {}


def build_lab(P, **kw):
    """tests/test_atlas_gpu.py's lab: one triangle, a cube moved by its vertices, a cube with an instance transform (no x
    translation), a sphere of 128 faces and one of 512"""
    s = P.Scene(64, 64, **kw)
    mat = P.Material((0.5, 0.5, 0.5), 0.5)
    assert s.addTriangles(F([[-6.0, 0.5, -3.0, -4.5, 0.25, -3.5, -5.5, 2.0, -2.5]]), mat) == TRI
    assert s.addCube(mat) == CUBE
    s.scale(CUBE, (1.5, 1.0, 2.0))
    s.moveTo(CUBE, (-3.0, 0.0, -4.0))
    assert s.addCube(mat) == XCUBE
    s.setPosition(XCUBE, (0.0, 0.5, -4.0))
    s.setRotation(XCUBE, (0.3, 0.5, 0.1))
    s.setInstanceScale(XCUBE, (1.2, 0.8, 1.5))
    assert s.addSphere(8, mat) == SPHERE
    s.moveTo(SPHERE, (0.0, 3.0, -5.0))
    assert s.addSphere(16, mat) == BALL
    s.moveTo(BALL, (0.0, -3.0, -5.0))
    return s


def scene(P, name):
    if name not in _lab:
        if name == "lab":
            s = build_lab(P)
        else:
            s = P.Scene(64, 64)
            P.scenes.cornell(s)
        s.uploadToGPU()
        _lab[name] = s
    return _lab[name]


@pytest.fixture(scope="module", autouse=True)
def _close_lab():
    yield
    for s in _lab.values():
        s.close()
    _lab.clear()


# where the lab's meshes stand -- centre, half extent -- and the share of the aimed rays each gets
LAB_TARGETS = [((-5.3, 0.9, -3.0), (0.5, 0.6, 0.3), 0.05), ((-3.0, 0.0, -4.0), (0.7, 0.45, 0.9), 0.4), ((0.0, 0.5, -4.0), (0.5, 0.35, 0.6), 0.35),
               ((0.0, 3.0, -5.0), (0.4, 0.4, 0.4), 0.12), ((0.0, -3.0, -5.0), (0.4, 0.4, 0.4), 0.08)]


def lab_rays(n, seed=RAY_SEED, name="lab"):
    """n rays.  For the Cornell box test_ray_query_gpu's ray_set as it is -- half from points in the box in random directions,
    half from a camera-like point, the hostile rays at the end (n counts them).  The lab stands in the open and that set alone
    hits it with 6 rays in 100, so there the first n // 2 rays are aimed instead: from points in front of the lab at points
    inside its meshes' boxes; the other n - n // 2 are ray_set's, hostile rays included."""
    assert name == "lab" or name in RADIUS
    if name != "lab":
        return ray_set(name, n, seed)
    a = n // 2
    o, d = ray_set("cornell", n - a, seed)
    rs = np.random.RandomState(seed + 1000)
    which = rs.choice(len(LAB_TARGETS), a, p=[t[2] for t in LAB_TARGETS])
    centre, half = F([t[0] for t in LAB_TARGETS])[which], F([t[1] for t in LAB_TARGETS])[which]
    to = (centre + rs.uniform(-1.0, 1.0, (a, 3)) * half).astype(F)
    ao = (rs.uniform(-1.0, 1.0, (a, 3)) * [6.0, 4.0, 3.0] + [-1.5, 0.0, 3.0]).astype(F)   # z in 0 .. 6: in front of every mesh
    ad = to - ao
    ad /= np.linalg.norm(ad, axis=1, keepdims=True).astype(F)
    return np.ascontiguousarray(np.concatenate([ao, o])), np.ascontiguousarray(np.concatenate([ad.astype(F), d]))


def face_counts(s):
    return [s.meshCounts(m)[1] for m in range(s.flatten().contents.mesh_count)]


def table_for(P, faces, w, h):
    """the chart table of a scene with these face counts for a w x h atlas: the first mesh without a lightmap (-1), the last
    with a table that ends inside it, the third on authored charts (corners outside the atlas, at +-1e30, a NaN corner, a
    zero-area face), the others on triangle_charts in cells of 4 to 8 texels -- often larger than the atlas"""
    L = P.lightmap
    entries = []
    for m, f in enumerate(faces):
        if m == 0:
            entries.append(None)
        elif m == 2 and f >= 2:
            entries.append(authored(f, w, h, f + w))
        else:
            entries.append(L.triangle_charts(f, 4 + m % 5)[0])
    last = len(faces) - 1
    assert faces[last] >= 2
    entries[last] = entries[last][:max(1, faces[last] // 5)]
    charts, first = L.chart_table(entries)
    assert first[0] == -1 and first[last] + faces[last] > len(charts)
    return charts, first


def lab_table(P, w, h):
    return table_for(P, [1, 12, 12, 128, 512], w, h)


def random_image(w, h, seed=IMAGE_SEED):
    """valid colours in (-1, 3) with `valid` 1.0, 2.5 or -1.0; about a fifth invalid (0.0 or -0.0), NaN and infinities in them"""
    rng = np.random.default_rng(seed * 1000 + w * 50 + h)
    n = w * h
    img = (rng.random((n, 4)) * 4 - 1).astype(F)
    img[:, 3] = rng.choice(F([1.0, 1.0, 1.0, 2.5, -1.0]), n)
    bad = np.flatnonzero(rng.random(n) < 0.2)
    img[bad, 0:3] = F([[np.nan, np.inf, -np.inf], [np.inf, 1.0, np.nan], [3.0, 4.0, 5.0]])[rng.integers(0, 3, len(bad))]
    img[bad, 3] = rng.choice(F([0.0, -0.0]), len(bad))
    return img.reshape(h, w, 4)


def assert_rows_equal(got, want, what):
    g, x = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, np.int32), np.asarray(want, np.int32)
    bad = np.argwhere(g != x)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} words differ, first (row, word) {bad[:6].tolist()}: "
                           f"{R.fields(g[bad[0][0]:bad[0][0] + 1])} vs {R.fields(x[bad[0][0]:bad[0][0] + 1])}")


def check_all(P, s, o, d, charts, first, img, what):
    """both entry points against the restatement over the device's own hit records, both modes; returns (hits, rows by mode)"""
    do, dd, dc, df, di = dev(o), dev(d), dev(charts), dev(first), dev(img)
    hits = s.query_closest(do, dd)
    h = hits.cpu().numpy()
    rows = {}
    for mode in MODES:
        want = R.sample(h, charts, first, img, mode)
        assert_rows_equal(s.atlas_sample(hits, dc, df, di, mode), want, f"{what}, {mode}: atlas_sample")
        assert_rows_equal(s.query_lightmap(do, dd, dc, df, di, mode), want, f"{what}, {mode}: query_lightmap")
        rows[mode] = want
    return R.hit_records(h), rows


# ---- 1. bytes against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg,pt", VARIANTS, ids=[f"force_geom={a},pair_trace={b}" for a, b in VARIANTS])
@pytest.mark.parametrize("name", ["lab", "cornell"])
def test_both_entry_points_equal_the_restatement(P, name, fg, pt):
    s = scene(P, name)
    faces = face_counts(s)
    s.set_option("force_geom", fg)
    s.set_option("pair_trace", pt)
    try:
        for n in NS:
            o, d = lab_rays(n, RAY_SEED + n, name)
            for w, h in ATLASES:
                charts, first = table_for(P, faces, w, h)
                check_all(P, s, o, d, charts, first, random_image(w, h), f"{name}, n {n}, atlas {w} x {h}")
                pm = s.get_option("query_pmode")
                # every traversal runs somewhere: the per-lane walk without pairs, PMODE 1, 2 and 3 on the Cornell box by force_geom
                if pt == 0:
                    assert pm == 0
                elif name == "cornell":
                    assert pm == {-1: 1, 1: 2, 2: 3}[fg]
                elif fg == 2:
                    assert pm == 3
    finally:
        s.set_option("force_geom", -1)
        s.set_option("pair_trace", 1)


def test_the_lab_is_not_vacuous(P):
    """over the lab's 4097 rays the restatement itself samples, skips, lacks charts and misses"""
    s = scene(P, "lab")
    o, d = lab_rays(4097)
    w, h = 33, 40
    charts, first = lab_table(P, w, h)
    assert face_counts(s) == [1, 12, 12, 128, 512]
    hits, rows = check_all(P, s, o, d, charts, first, random_image(w, h), "the lab")
    hit = hits["hit"] != 0
    for mode in MODES:
        r = R.fields(rows[mode])
        wt = r["weight"]
        print(f"{mode}: hits {hit.mean():.3f}, weight > 0 {(wt > 0).mean():.3f}, partly invalid {((wt > 0) & (wt < 0.999)).sum()}")
        assert (wt > 0).mean() >= 0.2, "fewer than a fifth of the rays sample anything"
        assert np.isfinite(r["rgb"]).all() and np.isfinite(wt).all(), "a NaN of an invalid texel came through"
    wt = R.fields(rows["bilinear"])["weight"]
    assert ((wt > 0) & (wt < 0.999)).sum() >= 20, "no footprint is partly invalid"
    no_chart = hit & ((hits["mesh_index"] == TRI) | ((hits["mesh_index"] == BALL) & (hits["face_index"] >= 512 // 5)))
    assert no_chart.sum() >= 20 and not rows["bilinear"][no_chart, 0:6].any(), "no record without a chart"
    assert (~hit).sum() >= 20 and (rows["bilinear"][~hit] == np.int32([0, 0, 0, 0, 0, 0, -1, -1])).all()
    r = R.fields(rows["bilinear"])
    nan = ~(np.isfinite(r["x"]) & np.isfinite(r["y"]))
    assert nan.sum() >= 5 and not rows["bilinear"][nan, 0:4].any() and (np.abs(r["x"][~nan]) > 1e20).any(), "the authored corners were never hit"


# ---- 2. geometry, independent of the restatement --------------------------------------------------------------------------------
def texel_rays(P, s, mesh, uv, w, h):
    """the atlas records of `mesh`, the covered indices, the image whose rgb is the record's world position, and one ray per
    covered texel from position + normal back along the normal"""
    import torch
    L = P.lightmap
    rec = s.atlas_texels(mesh, dev(uv), w, h)
    idx = L.covered(rec)
    p, n = L.atlas_inputs(rec)
    img = L.scatter(p, idx, w, h).reshape(h, w, 4)
    entries = [None] * s.flatten().contents.mesh_count
    entries[mesh] = uv
    charts, first = L.chart_table(entries)
    return rec.cpu().numpy(), idx.cpu().numpy(), img, (p + n).contiguous(), (-n).contiguous(), dev(charts), dev(first), torch


def check_texels_found(P, s, mesh, what):
    uv, w, h = P.lightmap.triangle_charts(12, 8)
    rec, idx, img, o, d, charts, first, torch = texel_rays(P, s, mesh, uv, w, h)
    assert len(idx) >= 120
    near = R.fields(s.query_lightmap(o, d, charts, first, img, "nearest").cpu().numpy())
    assert (near["mesh"] == mesh).all() and np.array_equal(near["face"], rec[idx, 3]), f"{what}: another face was hit"
    assert np.array_equal(near["rgb"].view(np.int32), rec[idx, 0:3]), f"{what}: nearest is not the texel's position bit for bit"
    assert (near["weight"] == 1).all()
    off = max(np.abs(near["x"] - (idx % w + 0.5)).max(), np.abs(near["y"] - (idx // w + 0.5)).max())
    print(f"{what}: worst distance of a hit from its texel's centre {off:.3e} texel")
    assert off < 0.35, "triangle_charts keeps every centre 0.35 texel from a chart's edge: nearer than that, the texel is found"
    return rec, idx, img, o, d, charts, first, near


@pytest.mark.parametrize("mesh", [CUBE, XCUBE], ids=["cube", "transformed cube"])
def test_a_ray_back_at_a_texel_finds_it(P, mesh):
    """Nearest returns the texel's position bit for bit.  Bilinear, where all four taps belong to the hit's own face, returns
    the hit's world point: the image is affine there.  Its tolerance, per component, is 48 eps (P + 1), P the largest
    |component| of a position: 8 eps P is the sampling unit of tests/test_lightmap_sample.py (sum w |I| <= P); each texel's
    position lies within tests/test_atlas_gpu.py's 14 eps of its float64 point, and so does the hit distance; the hit point
    o + t d from o = p + n adds its three roundings at magnitude P + 1, the barycentrics of the hit a few more at the size of
    an edge.  A tap off by one texel is wrong by a texel's pitch, about 0.3."""
    s = scene(P, "lab")
    rec, idx, img, o, d, charts, first, near = check_texels_found(P, s, mesh, f"mesh {mesh}")
    w = img.shape[1]
    bil = R.fields(s.query_lightmap(o, d, charts, first, img, "bilinear").cpu().numpy())
    hits = R.hit_records(s.query_closest(o, d).cpu().numpy())
    assert np.array_equal(bil["face"], hits["face_index"]) and (hits["hit"] != 0).all()
    i0, j0 = np.floor(bil["x"] - F(0.5)).astype(int), np.floor(bil["y"] - F(0.5)).astype(int)
    h = img.shape[0]
    own = np.ones(len(idx), bool)
    for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
        i, j = i0 + di, j0 + dj
        inside = (i >= 0) & (j >= 0) & (i < w) & (j < h)
        t = np.where(inside, j * w + i, 0)
        own &= inside & (rec[t, 7] == mesh) & (rec[t, 3] == hits["face_index"])
    assert own.mean() >= 0.1, "too few footprints lie on the hit's own face"
    scale = np.abs(rec[idx, 0:3].view(F)).max() + 1.0
    err = np.abs(bil["rgb"][own].astype(np.float64) - hits["point"][own].astype(np.float64)).max() / (EPS * scale)
    print(f"mesh {mesh}: {own.sum()} of {len(idx)} footprints on their own face; worst |bilinear - hit point| {err:.2f} eps (P + 1)")
    assert err <= 48.0
    assert np.abs(bil["weight"][own] - 1.0).max() <= 3 * EPS


# ---- 3. geometry that moves -----------------------------------------------------------------------------------------------------
def test_moved_geometry_is_followed(P):
    import torch
    s = build_lab(P)
    s.setDynamicGeometryPolicy("GpuRebuild")
    s.uploadToGPU()
    try:
        o, d = lab_rays(4097)
        w, h = 33, 40
        charts, first = lab_table(P, w, h)
        img = random_image(w, h)
        before, _ = check_all(P, s, o, d, charts, first, img, "as uploaded")
        uv = P.lightmap.triangle_charts(12, 8)
        old = {m: s.atlas_texels(m, dev(uv[0]), uv[1], uv[2]).cpu().numpy() for m in (CUBE, XCUBE)}
        M = s.flatten().contents.meshes[CUBE]
        v = np.ctypeslib.as_array(C.cast(M.verts, C.POINTER(C.c_float)), (M.vert_count, 3)).copy()
        s.setVertices(CUBE, (v * F([1.0, 1.5, 1.0]) + F([0.25, 0.0, -0.5])).astype(F))
        s.refitObjectChanges()                                   # ptrt_update_vertices + ptrt_refit
        pose = torch.tensor([[0.0, 0.8, -4.5, 0.2, 0.6, -0.1, 1.2, 0.8, 1.5]], device="cuda")
        s.set_instance_poses_device(XCUBE, pose)                 # no x translation, as in the lab
        assert P.lib.ptrt_refit_tlas(s.ctx) == 0
        after, _ = check_all(P, s, o, d, charts, first, img, "moved")  # no sync between the edits and the queries
        for m in (CUBE, XCUBE):
            was, now = before["mesh_index"] == m, after["mesh_index"] == m
            assert was.any() and now.any() and not np.array_equal(before["t"][was & now], after["t"][was & now]), f"mesh {m} did not move"
        for m in (CUBE, XCUBE):
            rec, idx, *_ = check_texels_found(P, s, m, f"moved mesh {m}")
            assert np.array_equal(rec[:, 3], old[m][:, 3]) and np.array_equal(rec[:, 7], old[m][:, 7]), "the same texels, the same faces"
            assert not np.array_equal(rec[idx, 0:3], old[m][idx, 0:3]), "at new positions"
    finally:
        s.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    smp, qry = P.lib.ptrt_atlas_sample, P.lib.ptrt_query_lightmap
    vp = C.c_void_p
    OK, INVALID, NOT_READY = P.PTRT_OK, -1, -4
    s = scene(P, "lab")
    c = s.ctx
    n, w, h = 70, 9, 7
    o, d = lab_rays(n)
    charts, first = lab_table(P, w, h)
    img = random_image(w, h)
    do, dd, dc, df, di = dev(o), dev(d), dev(charts), dev(first), dev(img)
    hits = s.query_closest(do, dd)
    out = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    big = torch.full((4096, 8), PATTERN, dtype=torch.int32, device="cuda")  # something every input fits into, to overlap with
    host = np.zeros((4096, 8), np.float32)
    hp = vp(host.ctypes.data)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    def p(t, off=0):
        return vp(t.data_ptr() + off)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == PATTERN).all()) and bool((big == PATTERN).all()) and not host.any()

    common = dict(c=c, n=n, charts=p(dc), faces=len(charts), first=p(df), image=p(di), w=w, h=h, mode=1, out=p(out))
    S = dict(common, hits=p(hits))
    Q = dict(common, o=p(do), d=p(dd))
    s_order = ("c", "hits", "n", "charts", "faces", "first", "image", "w", "h", "mode", "out")
    q_order = ("c", "o", "d", "n", "charts", "faces", "first", "image", "w", "h", "mode", "out")
    shared = [dict(n=-1), dict(faces=0), dict(faces=-5), dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 14, h=(1 << 14) + 1),
              dict(w=2 ** 31 - 1, h=2 ** 31 - 1), dict(mode=2), dict(mode=-1),
              dict(charts=None), dict(first=None), dict(image=None), dict(out=None),
              dict(image=p(di, 4)), dict(image=p(di, 8)), dict(out=p(out, 4)), dict(out=p(big, 8)), dict(charts=p(dc, 2)), dict(first=p(df, 1)),
              dict(charts=hp), dict(first=hp), dict(image=hp), dict(out=hp),
              dict(charts=tail(len(charts) * 24 - 4)), dict(first=tail(5 * 4 - 4)), dict(image=tail(w * h * 16 - 16)),
              dict(out=tail(n * 32 - 32)), dict(faces=(size // 24) + 1, charts=block),
              dict(out=p(dc)), dict(out=p(di)), dict(out=p(di, 16 * (w * h - 1))), dict(out=p(big), charts=p(big, n * 32 - 4)),
              dict(out=p(big, 16), first=p(big)), dict(c=None)]
    only_s = [dict(hits=None), dict(hits=p(hits, 4)), dict(hits=p(hits, 8)), dict(hits=hp), dict(hits=tail(n * 64 - 64)), dict(out=p(hits)),
              dict(out=p(hits, 64 * n - 16)), dict(out=p(big, 64), hits=p(big, 0), n=2)]
    only_q = [dict(o=None), dict(d=None), dict(o=p(do, 2)), dict(d=p(dd, 1)), dict(o=hp), dict(d=hp), dict(o=tail(n * 12 - 4)),
              dict(d=tail(n * 12 - 4)), dict(out=p(big), o=p(big, n * 32 - 4)), dict(out=p(big, 16), d=p(big))]
    for fn, name, D, order, cases in ((smp, b"ptrt_atlas_sample", S, s_order, shared + only_s),
                                      (qry, b"ptrt_query_lightmap", Q, q_order, shared + only_q)):
        for change in cases:
            args = dict(D, **change)
            assert fn(*[args[x] for x in order]) == INVALID, (name, change)
            if "c" not in change:
                assert name in P.lib.ptrt_last_error(c), (name, change)
        assert untouched(), name
        args = dict(D, n=0)
        assert fn(*[args[x] for x in order]) == OK and untouched(), "n == 0 is accepted and does nothing"
        assert fn(*[D[x] for x in order]) == OK
        s.sync()
        want = R.sample(hits.cpu().numpy(), charts, first, img, "bilinear")
        assert_rows_equal(out, want, f"{name}: the call that is in order")
        out.fill_(PATTERN)
    hip.hipFree(block)
    # the calls that are in order write their rows and no others
    G = 3
    for fn, D, order in ((smp, S, s_order), (qry, Q, q_order)):
        guarded = torch.full((n + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
        args = dict(D, out=p(guarded, 32 * G), mode=0)
        assert fn(*[args[x] for x in order]) == OK
        s.sync()
        assert (guarded[:G] == PATTERN).all() and (guarded[G + n:] == PATTERN).all(), "a write outside the rows"
        assert_rows_equal(guarded[G:G + n], R.sample(hits.cpu().numpy(), charts, first, img, "nearest"), "between guard rows")
    # before geometry is uploaded; a destroyed context
    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    for fn, name, D, order in ((smp, b"ptrt_atlas_sample", S, s_order), (qry, b"ptrt_query_lightmap", Q, q_order)):
        args = dict(D, c=ctx)
        assert fn(*[args[x] for x in order]) == NOT_READY and name in P.lib.ptrt_last_error(ctx)
        args = dict(D, c=ctx, mode=7)
        assert fn(*[args[x] for x in order]) == INVALID
    P.lib.ptrt_destroy(ctx)
    for fn, D, order in ((smp, S, s_order), (qry, Q, q_order)):
        args = dict(D, c=ctx)
        assert fn(*[args[x] for x in order]) == INVALID
    assert untouched()
    # the binding
    good = dict(charts=dc, chart_first=df, image=di)
    for change in (dict(mode="cubic"), dict(charts=dc[:, :5]), dict(charts=dc.cpu()), dict(chart_first=df.to(torch.int64)),
                   dict(chart_first=df[:, None]), dict(image=di.reshape(-1, 4)), dict(image=di.to(torch.float64)),
                   dict(out=torch.zeros((n + 1, 8), dtype=torch.int32, device="cuda")),
                   dict(out=torch.zeros((n, 8), dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            s.atlas_sample(hits, **dict(good, **change))
        with pytest.raises(ValueError):
            s.query_lightmap(do, dd, **dict(good, **change))
    with pytest.raises(ValueError):
        s.atlas_sample(hits[:, :15], **good)
    with pytest.raises(ValueError):
        s.query_lightmap(do, dd[:-1], **good)
    mine = torch.full((n, 8), PATTERN, dtype=torch.int32, device="cuda")
    assert s.query_lightmap(do, dd, out=mine, **good) is mine and s.atlas_sample(hits[:0], **good).shape == (0, 8)


# ---- 5. neighbours ---------------------------------------------------------------------------------------------------------------
def test_a_query_between_frames_changes_nothing(P, O, blue_noise):
    import torch
    from common import render_both
    runs = []
    for with_call in (False, True):
        s = P.Scene(96, 64)
        P.scenes.cornell(s)
        s.set_option("time_kernels", 1)
        render_both(P, O, s, blue_noise, 2, 4, 1)
        hist = s.kernel_ms_history().tobytes()
        rng = s.read(P.BUF_RNG)
        stats = s.stats()
        if with_call:
            w, h = 33, 40
            charts, first = table_for(P, face_counts(s), w, h)
            o, d = lab_rays(4097, name="cornell")
            rows = s.query_lightmap(dev(o), dev(d), dev(charts), dev(first), dev(random_image(w, h)))
            again = s.atlas_sample(s.query_closest(dev(o), dev(d)), dev(charts), dev(first), dev(random_image(w, h)))
            torch.cuda.synchronize()
            assert torch.equal(rows, again) and bool((rows[:, 3] != 0).any())
            assert s.kernel_ms_history().tobytes() == hist
            assert np.array_equal(s.read(P.BUF_RNG), rng) and s.stats() == stats
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), hist=s.kernel_ms_history()))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and len(a["hist"]) == len(b["hist"])


# ---- 6. the loop closes ----------------------------------------------------------------------------------------------------------
def test_a_bake_viewed_through_the_camera(P):
    """atlas_texels for every mesh of the Cornell box into one shared atlas, query_direct + query_irradiance at 16 directions,
    scatter, atlas_filter, atlas_dilate -- and then camera_rays, query_lightmap, shade_samples at 64 x 64.  (No comparison
    with the path tracer: the bake lacks the analytic lights' one-bounce term by design.)"""
    import torch
    L = P.lightmap
    s = scene(P, "cornell")
    faces = face_counts(s)
    uv, w, h = L.triangle_charts(sum(faces), 12, gutter=2)
    starts = np.concatenate([[0], np.cumsum(faces)])
    per_mesh = [uv[starts[m]:starts[m + 1]] for m in range(len(faces))]
    rec = None
    for m, c in enumerate(per_mesh):
        rec = s.atlas_texels(m, dev(c), w, h, out=rec, clear=rec is None)
    idx = L.covered(rec)
    pos, nrm = L.atlas_inputs(rec)
    n, k = len(idx), 16
    assert set(rec[idx, 7].cpu().tolist()) == set(range(len(faces)))
    direct = s.query_direct(pos, nrm, dev(L.hammersley2(4)))
    gather = s.query_irradiance(pos, nrm, dev(L.hammersley2(k)), s.init_rng_states(7, 0, n * k), samples=1, max_depth=3)
    img = L.scatter(dev(L.total_irradiance(direct, gather)), idx, w, h).reshape(h, w, 4)
    sd, sp = L.filter_sigmas(L.texel_pitch(rec, w, h))
    baked = s.atlas_dilate(s.atlas_filter(rec, img, 2, sd, sp), 2)
    charts, first = L.chart_table([dev(c) for c in per_mesh])
    assert charts.is_cuda and first.tolist() == starts[:-1].tolist()
    o, d = s.camera_rays(0)
    assert o.shape == (64 * 64, 3)
    rows = s.query_lightmap(o, d, charts, first, baked)
    f = P.lightmap_sample_fields(rows)
    hit = f["mesh"] >= 0
    assert float(hit.float().mean()) > 0.5 and bool((f["weight"][hit] > 0).all()), "a camera hit found nothing baked"
    view = L.shade_samples(rows, torch.full((len(faces), 3), 0.7, device="cuda"), background=(0.0, 0.0, 0.0))
    assert view.shape == (64 * 64, 3) and bool(torch.isfinite(view).all()) and float(view.mean()) > 1e-3, "the view is black"
    assert float(view[hit].min()) >= 0.0
    want = R.sample(s.query_closest(o, d).cpu().numpy(), charts.cpu().numpy(), first.cpu().numpy(), baked.cpu().numpy(), "bilinear")
    assert_rows_equal(rows, want, "the samples of the view")
    assert np.array_equal(L.shade_samples(rows.cpu().numpy(), np.full((len(faces), 3), 0.7, F)).view(np.int32),
                          view.cpu().numpy().view(np.int32)), "arrays and tensors shade alike"
