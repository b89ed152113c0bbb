"""Lightmap atlases on the device (ptrt_atlas_texels, ptrt_atlas_dilate; Scene.atlas_texels / atlas_dilate).  The records are
compared as bytes, tolerance 0, with the numpy restatement (tests/atlas_restatement.py) -- for a single triangle, cubes with
and without a transform and spheres, generated and authored charts with every rule of the coverage definition in them, every
`atlas_lanes`, a grid smaller than the work, across a device rebuild (another leaf order) and a refit (other vertices), and
for two meshes in one atlas.  Independently of that fp32 statement, a cube's owner map equals a float64 coverage test, its
positions lie within a forward-propagated unit of the float64 point, and a ray back along the normal hits the texel's own
mesh and face.  The dilation equals its restatement byte for byte; a bake from atlas to dilated image holds together; what
must be refused is refused with every byte untouched; frames around a call do not notice it."""
import ctypes as C

import numpy as np
import pytest

import atlas_restatement as A
from test_atlas import inside64
from test_irradiance_gpu import PATTERN, buffers, dev

pytestmark = pytest.mark.gpu

F = np.float32
EPS = float(np.finfo(np.float32).eps)
ATLASES = [(1, 1), (67, 5), (33, 40)]
LANES = (1, 4, 16, 64, -1)
TRI, CUBE, XCUBE, SPHERE, BALL = range(5)  # the lab's meshes

_lab = {}


def lab(P):
    """one triangle, a cube moved by its vertices, a cube with an instance transform, a sphere of 128 faces and one of 512"""
    if "s" not in _lab:
        s = P.Scene(64, 64)
        mat = P.Material((0.5, 0.5, 0.5), 0.5)
        assert s.addTriangles(F([[-6.0, 0.5, -3.0, -4.5, 0.25, -3.5, -5.5, 2.0, -2.5]]), mat) == TRI
        assert s.addCube(mat) == CUBE
        s.scale(CUBE, (1.5, 1.0, 2.0))
        s.moveTo(CUBE, (-3.0, 0.0, -4.0))
        assert s.addCube(mat) == XCUBE
        s.setPosition(XCUBE, (0.0, 0.5, -4.0))   # (no x translation: with one, the reference's inverse of a rotated instance is not
                                                 # the world matrix's inverse -- tests/brute_force.py -- and rays and texels disagree)
        s.setRotation(XCUBE, (0.3, 0.5, 0.1))
        s.setInstanceScale(XCUBE, (1.2, 0.8, 1.5))
        assert s.addSphere(8, mat) == SPHERE
        s.moveTo(SPHERE, (0.0, 3.0, -5.0))
        assert s.addSphere(16, mat) == BALL
        s.moveTo(BALL, (0.0, -3.0, -5.0))
        s.uploadToGPU()
        _lab["s"] = s
    return _lab["s"]


@pytest.fixture(scope="module", autouse=True)
def _close_lab():
    yield
    if "s" in _lab:
        _lab.pop("s").close()


def host_mesh(s, m):
    """the mesh as the host holds it (what an upload or a refit sends): vertices, faces, matrices"""
    M = s.flatten().contents.meshes[m]
    v = np.ctypeslib.as_array(C.cast(M.verts, C.POINTER(C.c_float)), (M.vert_count, 3)).copy()
    f = np.ctypeslib.as_array(C.cast(M.faces, C.POINTER(C.c_int32)), (M.face_count, 3)).copy()
    return dict(verts=v, faces=f, world=F(list(M.world)), normal=F(list(M.normal)), has_transform=bool(M.has_transform))


def restate(s, m, uv, w, h, **kw):
    return A.atlas_texels(uv=uv, w=w, h=h, mesh=m, **host_mesh(s, m), **kw)


def assert_records_equal(got, want, what=""):
    g, x = A.comparable(got), A.comparable(want)
    bad = np.argwhere(g != x)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} words differ, first (texel, word) {bad[:6].tolist()}: "
                           f"{g[tuple(bad[0])]} vs {x[tuple(bad[0])]}")


def authored(faces, w, h, seed, only=None):
    """(faces, 6) float32 charts with every rule in them: two faces sharing an edge with opposite windings, two overlapping
    (the lower must win), one partly and one wholly outside, corners at +-1e30, a zero-area face, a NaN corner, random
    triangles in and around the atlas, and -- last, so that it takes only what is left -- one that covers the whole atlas.
    `only`: that special alone, for a mesh of one face."""
    W, H = F(w), F(h)
    special = [[0.25 * W, 0.25 * H, 0.75 * W, 0.25 * H, 0.25 * W, 0.75 * H],
               [0.75 * W, 0.75 * H, 0.75 * W, 0.25 * H, 0.25 * W, 0.75 * H],
               [0, 0, 0.5 * W, 0.1 * H, 0.1 * W, 0.6 * H], [0.05 * W, 0.05 * H, 0.1 * W, 0.7 * H, 0.6 * W, 0.05 * H],
               [0.6 * W, 0.5 * H, 1.7 * W, 0.6 * H, 0.7 * W, 1.4 * H], [W + 3, H + 3, W + 9, H + 4, W + 5, H + 11],
               [-1e30, 0.3 * H, 1e30, 0.2 * H, 0.5 * W, 1e30], [1, 1, 3, 3, 5, 5], [0.5 * W, np.nan, W, 0, 0, H],
               [-1, -1, 2 * W + 1, -1, -1, 2 * H + 1]]
    if only is not None:
        return F([special[only]])
    rng = np.random.default_rng(seed)
    uv = (rng.random((faces, 3, 2)) * 1.4 - 0.2) * [w, h]
    uv = np.round(uv * 4) / 4  # quarter texels: centres ON edges happen
    uv = uv.reshape(faces, 6).astype(F)
    k = min(faces - 1, len(special) - 1)
    uv[:k] = F(special[:k])
    uv[faces - 1] = F(special[-1])
    return uv


def uv_sets(P, faces, w, h):
    if faces == 1:
        return [(f"special {k}", authored(1, w, h, 0, only=k)) for k in range(10)]
    cell = max(4, min(8, int((w * h * 2 // faces) ** 0.5)))
    return [("charts", P.lightmap.triangle_charts(faces, cell)[0]), ("authored", authored(faces, w, h, faces + w))]


# ---- 1. bytes against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
@pytest.mark.parametrize("mesh", [TRI, CUBE, XCUBE, SPHERE], ids=["triangle", "cube", "transformed cube", "sphere"])
def test_records_equal_the_restatement(P, mesh, w, h):
    s = lab(P)
    H = host_mesh(s, mesh)
    assert H["has_transform"] == (mesh == XCUBE) and len(H["faces"]) == {TRI: 1, CUBE: 12, XCUBE: 12, SPHERE: 128}[mesh]
    s.set_option("persist", 1)
    try:
        for name, uv in uv_sets(P, len(H["faces"]), w, h):
            want = restate(s, mesh, uv, w, h)
            for g in LANES:
                s.set_option("atlas_lanes", g)
                got = s.atlas_texels(mesh, dev(uv), w, h).cpu().numpy()
                assert s.get_option("atlas_lanes_eff") in ((1, 4, 16, 64) if g < 0 else (g,))
                assert_records_equal(got, want, f"{name}, atlas_lanes {g}")
            if name in ("authored", "special 9"):
                assert (want[:, 7] == mesh).all(), "the whole-atlas triangle left a texel empty"
    finally:
        s.set_option("atlas_lanes", -1)
        s.set_option("persist", 0)


def test_charts_in_their_own_atlas_and_a_grid_smaller_than_the_work(P):
    import torch
    s = lab(P)
    faces = len(host_mesh(s, BALL)["faces"])
    assert faces == 512 and faces > torch.cuda.get_device_properties(0).multi_processor_count  # lanes 64, persist 1: units > grid
    uv, w, h = P.lightmap.triangle_charts(faces, 6)
    want = restate(s, BALL, uv, w, h)
    assert len(set(want[want[:, 7] >= 0, 3].tolist())) == faces  # every face owns a texel
    s.set_option("persist", 1)
    try:
        for g in LANES:
            s.set_option("atlas_lanes", g)
            assert_records_equal(s.atlas_texels(BALL, dev(uv), w, h).cpu().numpy(), want, f"atlas_lanes {g}")
    finally:
        s.set_option("atlas_lanes", -1)
        s.set_option("persist", 0)
    with pytest.raises(P.PtrtError):
        s.set_option("atlas_lanes", 2)
    with pytest.raises(P.PtrtError):
        s.set_option("atlas_lanes", 0)
    assert s.get_option("atlas_lanes") == -1


def test_rebuild_keeps_the_bytes_and_refit_moves_the_positions(P):
    s = P.Scene(64, 64)
    mat = P.Material((0.5, 0.5, 0.5), 0.5)
    c = s.addCube(mat)
    s.scale(c, (2.0, 1.0, 3.0))
    s.addPlaneXZ(-2.0, 6.0, mat)
    s.setDynamicGeometryPolicy("GpuRebuild")
    s.uploadToGPU()
    w, h = 33, 40
    uv = authored(12, w, h, 5)
    before = s.atlas_texels(c, dev(uv), w, h).cpu().numpy()
    assert_records_equal(before, restate(s, c, uv, w, h), "as uploaded")
    v = host_mesh(s, c)["verts"]
    s.setVertices(c, v)
    s.rebuildObjectChanges()                      # ptrt_build_bvh: Morton order, another leaf order
    assert_records_equal(s.atlas_texels(c, dev(uv), w, h).cpu().numpy(), before, "behind ptrt_build_bvh")
    moved = (v * F([1.0, 1.5, 1.0]) + F([0.25, 0.0, -0.5])).astype(F)
    s.setVertices(c, moved)
    s.refitObjectChanges()                        # ptrt_update_vertices + ptrt_refit, no sync
    after = s.atlas_texels(c, dev(uv), w, h).cpu().numpy()
    assert np.array_equal(host_mesh(s, c)["verts"], moved)
    assert_records_equal(after, restate(s, c, uv, w, h), "behind ptrt_refit")
    assert np.array_equal(after[:, 3], before[:, 3]) and not np.array_equal(after[:, 0:3], before[:, 0:3])
    s.close()


def test_two_meshes_share_an_atlas(P):
    s = lab(P)
    w, h = 33, 40
    uv_a = F(np.tile([2, 2, 24, 3, 4, 30], (12, 1)))          # every face of the cube on one chart: face 0 owns it
    uv_b = authored(128, w, h, 9)                              # ends with the triangle that covers everything
    first = s.atlas_texels(CUBE, dev(uv_a), w, h)
    a = first.cpu().numpy()
    both = s.atlas_texels(SPHERE, dev(uv_b), w, h, out=first, clear=False)
    assert both is first
    got = both.cpu().numpy()
    own = a[:, 7] == CUBE
    assert own.any() and not own.all() and (a[own, 3] == 0).all()
    assert np.array_equal(got[own], a[own]), "the overlap did not keep the first mesh"
    assert (got[~own, 7] == SPHERE).all()
    assert_records_equal(got, restate(s, SPHERE, uv_b, w, h, clear=False, records=a), "clear 1 then 0")
    with pytest.raises(ValueError):
        s.atlas_texels(SPHERE, dev(uv_b), w, h, clear=False)


# ---- 2. geometry, independent of the fp32 restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [CUBE, XCUBE], ids=["cube", "transformed cube"])
def test_geometry_against_float64(P, mesh):
    import torch
    s = lab(P)
    H = host_mesh(s, mesh)
    uv, w, h = P.lightmap.triangle_charts(12, cell=8)
    rec = s.atlas_texels(mesh, dev(uv), w, h)
    r = rec.cpu().numpy()
    centres = np.stack(np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5), axis=-1).reshape(-1, 2)
    t = uv.astype(np.float64).reshape(12, 3, 2)
    owner = np.full(w * h, -1)
    for f in range(11, -1, -1):
        owner[inside64(centres, t[f])] = f
    cov = owner >= 0
    assert np.array_equal(r[:, 7] >= 0, cov) and np.array_equal(r[cov, 3], owner[cov]) and (r[cov, 7] == mesh).all()
    assert len(set(owner[cov].tolist())) == 12
    # the float64 point of every covered centre, and the unit: the roundings on the way -- 4 to a barycentric (two products, a
    # difference, a quotient), 4 to a local component (two products, two sums), 6 to a world component (three products, three
    # sums) -- times eps, times the magnitudes that enter, the barycentrics' taken with their condition (|terms| / |A|)
    V = H["verts"].astype(np.float64)[H["faces"]]
    Wm = H["world"].astype(np.float64).reshape(4, 4) if H["has_transform"] else np.eye(4)
    inv = np.float64(list(s.flatten().contents.meshes[mesh].inverse)).reshape(4, 4) if H["has_transform"] else np.eye(4)
    assert np.abs(Wm @ inv - np.eye(4)).max() <= 1e-5, "the instance's stored inverse is not its world matrix's"
    pos = r[:, 0:3].view(F).astype(np.float64)
    worst = 0.0
    for i in np.flatnonzero(cov):
        a, b, c = t[owner[i]]
        d1, d2, q = b - a, c - a, centres[i] - a
        area = d1[0] * d2[1] - d1[1] * d2[0]
        b1, b2 = (q[0] * d2[1] - q[1] * d2[0]) / area, (d1[0] * q[1] - d1[1] * q[0]) / area
        c1, c2 = (abs(q[0] * d2[1]) + abs(q[1] * d2[0])) / abs(area), (abs(d1[0] * q[1]) + abs(d1[1] * q[0])) / abs(area)
        v0, e1, e2 = V[owner[i], 0], V[owner[i], 1] - V[owner[i], 0], V[owner[i], 2] - V[owner[i], 0]
        local = v0 + b1 * e1 + b2 * e2
        truth = Wm[:3, :3] @ local + Wm[:3, 3]
        mag = np.abs(Wm[:3, :3]) @ (np.abs(v0) + c1 * np.abs(e1) + c2 * np.abs(e2)) + np.abs(Wm[:3, 3])
        unit = (4 + 4 + (6 if H["has_transform"] else 0)) * EPS * mag
        err = np.abs(pos[i] - truth) / unit
        worst = max(worst, float(err.max()))
    print(f"mesh {mesh}: worst position error {worst:.3f} units")
    assert worst <= 1.0
    # a ray from just above every covered texel back along its normal hits that mesh and that face at 1e-3
    idx = P.lightmap.covered(rec)
    p, n = P.lightmap.atlas_inputs(rec)
    assert torch.allclose((n * n).sum(1), torch.ones(len(n), device="cuda"), atol=1e-5)
    hit = P.hit_fields(s.query_closest((p + 1e-3 * n).contiguous(), (-n).contiguous()))
    hm, hf, ht = hit["mesh_index"].cpu().numpy(), hit["face_index"].cpu().numpy(), hit["t"].cpu().numpy().astype(np.float64)
    assert (hit["hit"].cpu().numpy() != 0).all() and (hm == mesh).all()
    assert np.array_equal(hf, r[idx.cpu().numpy(), 3])
    mag = np.abs(Wm[:3, :3]) @ np.abs(V).max(axis=(0, 1)) * 2 + np.abs(Wm[:3, 3])
    unit_t = float(np.linalg.norm(14 * EPS * mag))
    print(f"mesh {mesh}: worst |t - 1e-3| {np.abs(ht - 1e-3).max():.3e}, unit {unit_t:.3e}")
    assert np.abs(ht - 1e-3).max() <= unit_t


# ---- 3. dilation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 1), (67, 5), (33, 40)], ids=["1x1", "1x5", "67x5", "33x40"])
def test_dilation_equals_the_restatement(P, w, h):
    import torch
    s = lab(P)
    rng = np.random.default_rng(w * 100 + h)
    img = (rng.random((h, w, 4)) * 4 - 1).astype(F)
    img[:, :, 3] = rng.random((h, w)) < 0.3
    if w * h > 1:
        img[0, 0, 3], img[-1, -1, 3] = 1.0, 0.0
    for passes in (1, 2, 3, 64):
        a = dev(img)
        out = s.atlas_dilate(a, passes)
        assert (out is a) == (passes % 2 == 0), "the result is in the second buffer for odd pass counts, in the image for even"
        want = A.dilate(img, passes)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{passes} passes"
        if passes == 1:
            assert torch.equal(a, dev(img)), "one pass wrote its source"


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------
def test_a_bake_from_atlas_to_dilated_image(P):
    import torch
    L = P.lightmap
    s = P.Scene(64, 64)
    P.scenes.cornell(s)
    c = s.addCube(P.Material((0.8, 0.8, 0.8), 0.5))
    s.setPosition(c, (0.0, 0.0, -3.0))
    s.setRotation(c, (0.3, 0.5, 0.1))
    s.setInstanceScale(c, (1.2, 1.2, 1.2))
    s.uploadToGPU()
    uv, w, h = L.triangle_charts(12, 12, gutter=3)   # charts 6 texels apart: two passes from each side do not meet
    rec = s.atlas_texels(c, dev(uv), w, h)
    idx = L.covered(rec)
    pos, nrm = L.atlas_inputs(rec)
    n, k = len(idx), 16
    assert n > 12
    s2 = dev(L.hammersley2(k))
    direct = s.query_direct(pos, nrm, dev(L.hammersley2(4)))
    gather = s.query_irradiance(pos, nrm, s2, s.init_rng_states(7, 0, n * k), samples=1, max_depth=3)
    total = L.total_irradiance(direct, gather)
    assert np.isfinite(total).all() and total.shape == (n, 3) and total.any()
    img = L.scatter(dev(total), idx, w, h)
    out = s.atlas_dilate(img.reshape(h, w, 4), 2).cpu().numpy()
    valid = out[:, :, 3] != 0
    assert valid.reshape(-1)[idx.cpu().numpy()].all() and np.isfinite(out).all()
    cov = np.zeros(w * h, bool)
    cov[idx.cpu().numpy()] = True
    cov = cov.reshape(h, w)
    near = np.zeros_like(cov)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= cov[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    assert np.array_equal(valid, near), "two passes reach the texels within 2 of a covered one, and no others"
    # the same positions and normals handed to the queries directly: the same rows
    r = rec.cpu().numpy()[idx.cpu().numpy()]
    p2, n2 = dev(np.ascontiguousarray(r[:, 0:3]).view(F)), dev(np.ascontiguousarray(r[:, 4:7]).view(F))
    assert torch.equal(s.query_direct(p2, n2, dev(L.hammersley2(4))).view(torch.int32), direct.view(torch.int32))
    again = s.query_irradiance(p2, n2, s2, s.init_rng_states(7, 0, n * k), samples=1, max_depth=3)
    assert torch.equal(again.view(torch.int32), gather.view(torch.int32))
    s.close()


# ---- 5. refusals and side effects ---------------------------------------------------------------------------------------------
def test_refusals(P):
    import torch
    tex, dil = P.lib.ptrt_atlas_texels, P.lib.ptrt_atlas_dilate
    vp = C.c_void_p
    INVALID, NOT_READY = -1, -4
    w, h = 9, 7
    uv = dev(P.lightmap.triangle_charts(12, 4)[0])
    out = torch.full((w * h, 8), PATTERN, dtype=torch.int32, device="cuda")
    ia, ib = (torch.full((h, w, 4), PATTERN, dtype=torch.int32, device="cuda") for _ in range(2))
    puv, pout, pa, pb = (vp(x.data_ptr()) for x in (uv, out, ia, ib))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((x == PATTERN).all()) for x in (out, ia, ib))

    ctx = vp()
    assert P.lib.ptrt_create(32, 32, 0, 0, 0, C.byref(ctx)) == P.PTRT_OK
    assert tex(ctx, 0, puv, w, h, 1, pout) == NOT_READY and b"ptrt_atlas_texels" in P.lib.ptrt_last_error(ctx)  # before upload
    assert tex(ctx, 0, puv, 0, h, 1, pout) == INVALID
    assert dil(ctx, pa, pb, w, h, 0) == INVALID and untouched()
    P.lib.ptrt_destroy(ctx)
    assert tex(ctx, 0, puv, w, h, 1, pout) == INVALID and dil(ctx, pa, pb, w, h, 1) == INVALID   # a destroyed context
    s = lab(P)
    c = s.ctx
    host = np.zeros((w * h, 8), np.float32)
    hp = vp(host.ctypes.data)
    pinned = torch.zeros((w * h, 8), dtype=torch.int32).pin_memory()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    size = 2 << 20
    block = vp()
    assert hip.hipMalloc(C.byref(block), size) == 0

    def tail(nbytes):
        return vp(block.value + size - nbytes)

    T = dict(c=c, mesh=CUBE, uv=puv, w=w, h=h, clear=1, out=pout)
    t_order = ("c", "mesh", "uv", "w", "h", "clear", "out")
    bad_t = [dict(mesh=-1), dict(mesh=5), dict(mesh=2 ** 31 - 1), dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 14, h=(1 << 14) + 1),
             dict(w=2 ** 31 - 1, h=2 ** 31 - 1), dict(uv=None), dict(out=None), dict(uv=hp), dict(out=hp),
             dict(out=vp(pinned.data_ptr())), dict(uv=tail(12 * 24 - 16)), dict(out=tail(w * h * 32 - 32)),
             dict(out=vp(out.data_ptr() + 4)), dict(c=None)]
    for change in bad_t:
        args = dict(T, **change)
        assert tex(*[args[a] for a in t_order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_atlas_texels" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    D = dict(c=c, a=pa, b=pb, w=w, h=h, passes=1)
    d_order = ("c", "a", "b", "w", "h", "passes")
    bad_d = [dict(passes=0), dict(passes=65), dict(passes=-1), dict(w=0), dict(h=0), dict(w=1 << 14, h=(1 << 14) + 1), dict(a=None),
             dict(b=None), dict(a=hp), dict(b=hp), dict(b=pa), dict(b=vp(ia.data_ptr() + 16)), dict(a=tail(w * h * 16 - 16)),
             dict(b=tail(w * h * 16 - 16)), dict(a=vp(ia.data_ptr() + 4)), dict(c=None)]
    for change in bad_d:
        args = dict(D, **change)
        assert dil(*[args[a] for a in d_order]) == INVALID, change
        if "c" not in change:
            assert b"ptrt_atlas_dilate" in P.lib.ptrt_last_error(c), change
    assert untouched() and not host.any()
    hip.hipFree(block)
    # between guard rows, the calls that are in order write their rows and no others
    G = 3
    guarded = torch.full((w * h + 2 * G, 8), PATTERN, dtype=torch.int32, device="cuda")
    assert tex(c, CUBE, puv, w, h, 1, vp(guarded[G:].data_ptr())) == P.PTRT_OK
    ga, gb = (torch.full((w * h + 2 * G, 4), PATTERN, dtype=torch.int32, device="cuda") for _ in range(2))
    ga[G:G + w * h] = 0
    ga[G, 3] = 0x3f800000                          # one valid texel, the rest invalid
    assert dil(c, vp(ga[G:].data_ptr()), vp(gb[G:].data_ptr()), w, h, 3) == P.PTRT_OK
    s.sync()
    for t in (guarded, ga, gb):
        assert (t[:G] == PATTERN).all() and (t[G + w * h:] == PATTERN).all(), "a write outside the atlas"
    assert not bool((guarded[G:G + w * h, 7] == PATTERN).any()) and not bool((gb[G:G + w * h] == PATTERN).any())
    # the binding
    with pytest.raises(ValueError):
        s.atlas_texels(CUBE, uv[:11], w, h)
    with pytest.raises(ValueError):
        s.atlas_texels(CUBE, uv.cpu(), w, h)
    with pytest.raises(ValueError):
        s.atlas_texels(CUBE, uv, w, h, out=torch.zeros((w * h + 1, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        s.atlas_texels(CUBE, uv, 0, h)
    with pytest.raises(P.PtrtError):
        s.atlas_texels(17, uv, w, h)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            s.atlas_dilate(torch.zeros((h, w, 4), device="cuda"), bad)


def test_a_call_between_frames_changes_nothing(P, O, blue_noise):
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
            uv, w, h = P.lightmap.triangle_charts(12, 8)
            rec = s.atlas_texels(6, dev(uv), w, h)
            img = s.atlas_dilate(torch.rand((h, w, 4), device="cuda").round(), 2)
            torch.cuda.synchronize()
            assert (rec[:, 7] == 6).any() and img.shape == (h, w, 4)
            assert s.kernel_ms_history().tobytes() == hist
            assert np.array_equal(s.read(P.BUF_RNG), rng) and s.stats() == stats
        rgb = s.render_to_host()
        runs.append(dict(buffers(P, s), rgb8=rgb, stats=s.stats(), n_hist=len(s.kernel_ms_history())))
        s.close()
    a, b = runs
    for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["n_hist"] == b["n_hist"]
