"""The restatement (tests/rt_restatement.py) and the host mirror (ptrt_amd.rt) against the float64 statement of the reference's
one-bounce ray tracer (tests/rt_truth.py), on the CPU: quantity by quantity on every lab case, the host-built trees against
the all-triangles answer, the seeded misreadings, the caps and the identities.  DESIGN.md 5.6."""
import numpy as np
import pytest

import rt_restatement as R
import rt_truth as T

CASES = sorted(T.CASES)
_LAB = {}


def _rt():
    try:                                               # torch first, as conftest's P fixture does and for its reason
        import torch  # noqa: F401
    except ImportError:
        pass
    import ptrt_amd.rt as rt
    return rt


def _oracle():
    import oracle
    return oracle


def _expand(n, idx, a):
    out = np.zeros((n,) + a.shape[1:], a.dtype)
    out[idx] = a
    return out


def restated(snap, W, H, O):
    """the restatement's detail as flat per-pixel arrays under the statement's names, and its image"""
    d = {}
    img = R.render(snap, W, H, O, detail=d)
    n = W * H
    q = dict(dir=d["dir"], Fr=d["Fr"], Rdir=d["Rdir"], Tdir=d["Tdir"], thickness=d["thickness"], linear=d["linear"],
             final=d["final"], rgb=d["rgb"], glass=d["glass"], refr_ok=d["refr_ok"], seed=d["seed"])
    g = np.nonzero(d["glass"])[0]
    for key, idx in (("0", np.arange(n)), ("R", g), ("T", g[d["refr_ok"][g]])):
        seg = d[key]
        for k in ("hit", "t", "mesh", "face", "point", "normal", "linear", "amb", "Lo", "shadow", "D", "G", "Fs", "kD", "dif", "ccB"):
            if seg is None:
                continue
            q[k + key] = _expand(n, idx, seg[k])
    return q, img


class Lab:
    def __init__(self, name):
        rt, O = _rt(), _oracle()
        self.name, self.case = name, T.CASES[name]
        self.scene = T.build(rt, self.case)
        self.snap = self.scene.snapshot()
        W, H = self.case["W"], self.case["H"]
        self.got, self.image = restated(self.snap, W, H, O)
        self.meshes = T.describe(self.case, self.scene)
        self.st = T.Statement(self.case, self.meshes, seeds=self.got["seed"])


def lab(name):
    if name not in _LAB:
        _LAB[name] = Lab(name)
    return _LAB[name]


def _v3(v):
    return np.array([v.x, v.y, v.z], np.float64)


def measure_camera(L):
    case = L.case
    q, unit = T.camera_units(case["camera"], case["W"], case["H"])
    view, cam = L.snap["view"], L.scene.getCamera()
    dev = 0.0
    for k in T.CAMERA_VECTORS:
        dev = max(dev, T.in_units(cam[k], q[k], unit[k]).max())
        if k != "lower_left_corner":
            dev = max(dev, T.in_units(_v3(getattr(view, k)), q[k], unit[k]).max())
    return dev


def measure_descriptor(L, mis=None):
    dev = 0.0
    for m, sm in zip(L.meshes, L.snap["meshes"]):
        q, unit = T.descriptor_units(T.F(m["euler"]))
        if mis:
            q = dict(zip(("rotation", "inv_rotation"), T.descriptor(T.F(m["euler"]), mis)))
        for k in ("rotation", "inv_rotation"):
            dev = max(dev, T.in_units(sm[k], q[k], np.maximum(unit[k], 1e-300)).max())
        assert np.array_equal(sm["translation"], np.asarray(m["position"], np.float32))
    return dev


def _masks(st):
    o = st.out
    return {"0": st.decided & o["hit0"], "R": st.decided & o["glass"], "T": st.decided & o["glass"] & o["refr_ok"],
            "all": st.decided}


def _mask_of(q, m):
    if q in ("dir", "linear", "final", "rgb"):
        return m["all"]
    if q in ("Fr", "Rdir") or q.endswith("R"):
        return m["R"]
    if q in ("Tdir", "thickness") or q.endswith("T"):
        return m["T"]
    return m["0"]


def measure_case(L, st=None, unit=None):
    """largest deviation in units per quantity over the decided pixels; hit-dependent quantities over the pixels both hit"""
    st = st or L.st
    unit = unit or L.st.unit
    m = _masks(st)
    dev = {}
    for q in T.UNIT_QUANTITIES:
        if q not in L.got or q not in st.out or q not in unit:
            continue
        mask = _mask_of(q, m)
        if q == "tR":
            mask = mask & st.out["hitR"]
        if q == "tT":
            mask = mask & st.out["hitT"]
        if q in T.LIGHT_TERMS:                         # per light, where the light faces the surface and its shadow is decided
            mask = mask[:, None] & st.held["shadow0"]["need"]
        if not mask.any() or L.got[q][mask].size == 0:
            continue
        dev[q] = float(T.in_units(L.got[q][mask], st.out[q][mask], unit[q][mask]).max())
    return dev


def discrete_mismatches(L, st=None):
    """pixels (decided) whose hit, mesh, face or needed shadow flags differ, per kind"""
    st = st or L.st
    m = _masks(st)
    bad = dict(hit=0, shadow=0)
    for key, mask in (("0", st.decided), ("R", m["R"]), ("T", m["T"])):
        if "hit" + key not in L.got or "hit" + key not in st.out:
            continue
        for k in ("hit", "mesh", "face"):
            bad["hit"] += int((L.got[k + key][mask] != st.out[k + key][mask]).sum())
        S = st.held["shadow" + key]
        need = S["need"] & (mask & st.out["hit" + key])[:, None]
        bad["shadow"] += int((L.got["shadow" + key][need] != S["blocked"][need]).sum())
    return bad


def byte_check(L, st=None, tol=None, image=None):
    """(bytes of decided pixels outside the interval, share of decided pixels' bytes that are undecided)"""
    st = st or L.st
    lo, hi = L.st.byte_interval(T.TOL["rgb"] if tol is None else tol) if st is L.st else (st.image, st.image)
    img = L.image if image is None else image
    dec = st.decided_image()
    out = ((img < lo) | (img > hi))[dec]
    return int(out.sum()), float((lo != hi)[dec].mean())


def measure_perturb():
    """perturbDirectionGGX alone: the restatement's against the statement's on directions about every axis (both tangent
    frames), the lab's rough object's two roughnesses and the ends of the range, and seeds of every size"""
    rng = np.random.default_rng(5)
    n = 4096
    d = T._norm(rng.normal(size=(n, 3)))
    d[:64] = T._norm(np.array([0.0, 0.0, 1.0]) + 1e-3 * rng.normal(size=(64, 3)))    # |N.z| >= 0.9999: the other frame
    d = d.astype(np.float32)
    d = (d / np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(np.float32)
    rough = rng.choice(np.array([0.021, 0.25, 0.3, 0.7, 1.0], np.float32), n)
    seed = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    got, after = R.perturb(d, rough, seed.copy(), _oracle())
    want, unit = T.perturb_units(d.astype(np.float64), rough.astype(np.float64), seed)
    assert np.array_equal(after, T.pcg_uniforms(seed)[2].astype(np.uint32))
    return float(T.in_units(got, want, unit).max())


def measure_all():
    table = {"perturb": ("isolated", measure_perturb())}
    for name in CASES:
        L = lab(name)
        dev = measure_case(L)
        dev["camera"] = measure_camera(L)
        dev["descriptor"] = measure_descriptor(L)
        for q, v in dev.items():
            if q not in table or v > table[q][1]:
                table[q] = (name, v)
    return table


def print_table():
    table = measure_all()
    print("MEASURED = {")
    for q, (name, v) in table.items():
        print(f'    "{q}": ("{name}", {float("%.4g" % (v * 1.0005)) if v else 0.0}),')
    print("}")
    T.NAMED_TERMS = False
    try:
        for name in CASES:
            L = lab(name)
            unit = T.units(L.st.P, L.st.held, L.st.out, named=False)
            dev = measure_case(L, unit=unit)
            print("without terms", name, {q: float("%.4g" % v) for q, v in dev.items() if v > 1.02 * measure_case(L)[q]})
            print("without terms", name, "camera", "%.4g" % measure_camera(L))
    finally:
        T.NAMED_TERMS = True
    for name in CASES:
        L = lab(name)
        print(name, "undecided %.4f" % (1 - L.st.decided.mean()), "bytes undecided %.4f" % byte_check(L)[1] if T.TOL else "",
              {k: round(float(v), 3) for k, v in L.st.shares().items()})


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", CASES)
def test_passthrough_changes_no_byte(name):
    """rt_restatement.render with and without `detail` gives the same image (two scenes asked for; every lab case done)"""
    L = lab(name)
    assert np.array_equal(R.render(L.snap, L.case["W"], L.case["H"], _oracle()), L.image)


@pytest.mark.parametrize("name", CASES)
def test_shares_and_caps_from_the_statement_alone(name):
    st = lab(name).st
    shares = st.shares()
    for k, least in T.SHARES[name].items():
        assert shares[k] >= least, f"{name}: {k} covers {shares[k]:.3f} of the pixels, {least} asked for"
    assert 1.0 - st.decided.mean() <= T.MAX_UNDECIDED, f"{name}: {1 - st.decided.mean():.4f} undecided"
    lo, hi = st.byte_interval(T.TOL["rgb"])
    assert (lo != hi)[st.decided_image()].mean() <= T.MAX_UNDECIDED_BYTES


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_statement(name):
    L = lab(name)
    bad = discrete_mismatches(L)
    assert bad == dict(hit=0, shadow=0), f"{name}: {bad}"
    dev = measure_case(L)
    dev["camera"], dev["descriptor"] = measure_camera(L), measure_descriptor(L)
    for q, v in dev.items():
        print(f"{name:8s} {q:12s} {v:10.4g} units (TOL {T.TOL[q]:.4g})")
    for q, v in dev.items():
        assert v <= T.TOL[q], f"{name}: {q} deviates by {v:.4g} units, TOL {T.TOL[q]:.4g}"
    outside, _ = byte_check(L)
    assert outside == 0, f"{name}: {outside} bytes of decided pixels outside the predicted interval"


def test_measured_table_is_current():
    table = measure_all()
    assert set(table) == set(T.MEASURED)
    for q, (name, v) in table.items():
        assert T.MEASURED[q][0] == name, (q, name, v)
        assert v == pytest.approx(T.MEASURED[q][1], rel=1e-2, abs=1e-3), (q, name, v)
    assert T.TOL == {q: 4.0 * v for q, (_, v) in T.MEASURED.items()}


def _rays_for(tris_world, cam_rays, rng, radius):
    """random rays, camera rays and two rays aimed at every triangle (one at its centroid, one near an edge), float32"""
    o = rng.uniform(-radius, radius, (256, 3))
    d = rng.normal(size=(256, 3))
    c = tris_world.mean(axis=1)
    n = np.cross(tris_world[:, 1] - tris_world[:, 0], tris_world[:, 2] - tris_world[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1), 1e-30)[:, None]
    edge = 0.9 * tris_world[:, 0] + 0.08 * tris_world[:, 1] + 0.02 * tris_world[:, 2]
    side = rng.normal(size=c.shape) * 0.3
    o2 = np.concatenate([c + n * 1.5 + side, edge - n * 0.7 + side])
    d2 = np.concatenate([c, edge]) - o2
    O_, D_ = np.concatenate([o, cam_rays[0], o2]), np.concatenate([d, cam_rays[1], d2])
    D_ /= np.linalg.norm(D_, axis=1)[:, None]
    return O_.astype(np.float32), D_.astype(np.float32)


def _tree_check(snap, meshes, cam_rays, seed, mis=None, extra=None):
    """the restatement's trace / any_hit over the host-built trees against the all-triangles answer; (rays, undecided,
    mismatches)"""
    world = T.World(meshes, mis)
    tw = np.concatenate([t @ Rm.T + Tm for t, Rm, Tm in zip(world.tris, world.R, world.T) if len(t)])
    o, d = _rays_for(tw, cam_rays, np.random.default_rng(seed), world.radius)
    if extra is not None:
        o, d = np.concatenate([o, extra[0]]), np.concatenate([d, extra[1]])
    md = [R.MeshData(m) for m in snap["meshes"]]
    hit, t, mi, fi = R.trace(md, o, d)
    want = world.closest(o.astype(np.float64), d.astype(np.float64))
    dec = want["decided"]
    bad = int((hit != want["hit"])[dec].sum())
    both = dec & hit & want["hit"]
    bad += int(((mi != want["mesh"]) | (fi != want["face"]))[both].sum())
    tmax = np.where(want["hit"], want["t"] * 0.999, 50.0)                     # shadow rays that stop just before the hit
    tm2 = np.where(want["hit"], want["t"] * 1.001, 50.0)                      # and just behind it
    for tm in (tmax, tm2):
        blocked = np.zeros(len(o), bool)
        for M in md:
            if M.transmission > 0 or not M.ok:
                continue
            blocked |= R.any_hit(M, o, d, tm.astype(np.float32))
        wb, wd = world.any_hit(o.astype(np.float64), d.astype(np.float64), tm)
        bad += int((blocked != wb)[wd].sum())
        dec = dec & wd
    return len(o), float(1.0 - dec.mean()), bad


def _camera_rays(case_or_view, W, H):
    if isinstance(case_or_view, dict):
        cam = T.camera_from(case_or_view["camera"], W, H)
    else:
        cam = dict(origin=_v3(case_or_view.origin), corner_minus_origin=_v3(case_or_view.corner_minus_origin),
                   horizontal=_v3(case_or_view.horizontal), vertical=_v3(case_or_view.vertical))
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    o, d = T.get_ray(cam, (xs.reshape(-1) + 0.5) / W, 1.0 - (ys.reshape(-1) + 0.5) / H)
    return np.array(o), d


def _leaf_sizes(scene):
    out = []
    for i in range(scene.getMeshCount()):
        out.append(sorted(int(nd.count) for nd in scene.mesh(i).tree()[1] if nd.count > 0))
    return out


@pytest.mark.parametrize("name", [n for n in CASES if "leaf_target" in T.CASES[n]])
def test_leaf_target_reaches_the_trees(name):
    """the lab's non-default Scene.setBVHLeafTarget shows in the trees that the restatement and the kernel walk: the leaf
    sizes differ from a default build's, no leaf exceeds target + tolerance, and a mesh's own setBVHLeafParams before the
    upload does not (the scene's values overwrite it, RTscene.cuh:1035), which is why the lab does not use it"""
    rt, case = _rt(), T.CASES[name]
    target, tol = case["leaf_target"]
    got, default = _leaf_sizes(lab(name).scene), None
    plain = T.build(rt, case, leaf_target=False)
    default = _leaf_sizes(plain)
    assert got != default
    big = [i for i, sizes in enumerate(default) if max(sizes) > target + tol]
    assert big, "no mesh of the case has a default leaf beyond the target"
    for i in big:
        assert max(got[i]) <= target + tol < max(default[i]) and len(got[i]) > len(default[i])
    own = rt.Scene(case["W"], case["H"], device=rt.HOST_ONLY)
    own.addSphere(8)
    own.mesh(0).setBVHLeafParams(1, 0)
    own.uploadToGPU()
    ref = rt.Scene(case["W"], case["H"], device=rt.HOST_ONLY)
    ref.addSphere(8)
    ref.uploadToGPU()
    assert _leaf_sizes(own) == _leaf_sizes(ref)
    for s in (plain, own, ref):
        s.close()


@pytest.mark.parametrize("name", CASES)
def test_trees_of_the_lab(name):
    L = lab(name)
    n, und, bad = _tree_check(L.snap, L.meshes, _camera_rays(L.case, L.case["W"], L.case["H"]), 7)
    assert bad == 0, f"{name}: {bad} of {n} decided rays differ between the host-built trees and all triangles"
    assert und <= 0.05


def _identity_meshes(scene, snap):
    """a demo scene's meshes for the statement: public vertices and faces; the demo recipes bake every transform, which the
    descriptors must show (identity rotation, zero translation), so that no pose is taken from the snapshot"""
    out = []
    for i, sm in enumerate(snap["meshes"]):
        assert np.array_equal(sm["rotation"], np.eye(3, dtype=np.float32)) and not sm["translation"].any()
        out.append(dict(vertices=scene.mesh(i).vertices, faces=scene.mesh(i).tree()[0], euler=(0.0,) * 3, position=(0.0,) * 3,
                        material=dict(transmission=sm["material"].transmission)))
    return out


DEMO = ("architectural", "cornell", "light_show", "material_showcase", "showcase1")   # named here: nothing is imported at collection


def test_every_demo_scene_is_named():
    assert sorted(_rt().scenes.DEMO_SCENES) == sorted(DEMO)


@pytest.mark.parametrize("name", DEMO)
def test_trees_of_the_demo_scenes(name):
    rt = _rt()
    s = rt.Scene(64, 48, device=rt.HOST_ONLY)
    rt.scenes.DEMO_SCENES[name](s)
    s.uploadToGPU()
    snap = s.snapshot()
    n, und, bad = _tree_check(snap, _identity_meshes(s, snap), _camera_rays(snap["view"], 64, 48), 11)
    assert bad == 0, f"{name}: {bad} of {n} decided rays differ between the host-built trees and all triangles"
    assert und <= 0.05
    s.close()


def _near_start():
    """The reference's default cube alone, and rays that start before each face and aim at it from a distance that is a
    miss of that face under t > 1e-4, a hit under t > 1e-5 and decided under both: the middle of the window that the
    uncertainty of t (UNC_T x the world's radius, the ray being normal to the face) leaves between the two thresholds."""
    rt = _rt()
    s = rt.Scene(8, 8, device=rt.HOST_ONLY)
    s.addCube(rt.Material((0.8, 0.8, 0.8), 0.5, 0.0))
    s.uploadToGPU()
    meshes = [dict(vertices=s.mesh(0).vertices, faces=s.mesh(0).tree()[0], euler=(0.0,) * 3, position=(0.0,) * 3,
                   material=T.material(base=((0.8, 0.8, 0.8), 0.5, 0.0)))]
    w = T.World(meshes)
    unc = T.UNC_T * w.radius
    lo, hi = 1e-5 + unc, 1e-4 - unc
    assert hi - lo > 4e-5, "the window between the thresholds has closed: use a smaller world"
    tri = w.tris[0]
    c = tri.mean(axis=1)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    return s.snapshot(), meshes, ((c + n * 0.5 * (lo + hi)).astype(np.float32), (-n).astype(np.float32))


@pytest.mark.parametrize("mis", sorted(T.MISREADINGS))
def test_seeded_misreading_is_caught(mis):
    """each one-line misreading of the statement fails against the UNCHANGED restatement on the case and quantity named"""
    case, quantity = T.MISREADINGS[mis]
    if quantity == "hit":
        snap, meshes, extra = _near_start()
        cam = _camera_rays(snap["view"], 8, 8)
        assert _tree_check(snap, meshes, cam, 7, None, extra)[2] == 0
        assert _tree_check(snap, meshes, cam, 7, mis, extra)[2] >= len(extra[0])     # every such ray is decided and differs
        return
    L = lab(case)
    if quantity == "descriptor":
        assert measure_descriptor(L) <= T.TOL["descriptor"] < measure_descriptor(L, mis)
        return
    st = T.Statement(L.case, L.meshes, mis=mis, seeds=L.got["seed"], with_units=False)
    if quantity == "bytes":
        dec = st.decided_image() & L.st.decided_image()
        lo, hi = L.st.byte_interval(T.TOL["rgb"])
        assert (((st.image < lo) | (st.image > hi))[dec]).mean() > 0.2
        return
    if quantity == "shadow":
        assert discrete_mismatches(L, st)["shadow"] > 0
        return
    dev = measure_case(L, st, L.st.unit)
    assert dev[quantity] > T.TOL[quantity], f"{mis}: {quantity} deviates by {dev[quantity]:.4g}, TOL {T.TOL[quantity]:.4g}"


# ------------------------------------------------------------------------------------------- identities, the statement alone
def test_emissive_wall_gives_its_emission_byte():
    st = lab("lamp").st
    e = np.asarray(T.CASES["lamp"]["meshes"][0]["material"]["emission"], np.float32).astype(np.float64)
    want = np.floor(np.clip((e / (e + 1.0)) ** T.GAMMA, 0, 1) * 255.0)
    lo, hi = st.byte_interval(T.TOL["rgb"])
    dec = st.decided_image() & (lo == hi).all(axis=2)
    assert dec.mean() > 0.9
    assert (st.image[dec] == want).all()


def test_reflect_refract_identities():
    rng = np.random.default_rng(3)
    N = T._norm(rng.normal(size=(64, 3)))
    I = T._norm(rng.normal(size=(64, 3)))
    assert np.abs(T.reflect_vec(T.reflect_vec(I, N), N) - I).max() < 1e-14
    Nf = T.face_forward(N, I)
    for eta in (1.0 / 1.5, 1.5, 1.0 / 2.4):
        ok, Tv, _ = T.refract_vec(-Nf, Nf, np.full(64, eta))
        assert ok.all() and np.abs(T._norm(Tv) + Nf).max() < 1e-14          # normal incidence keeps the direction


def test_critical_angle_two_sides():
    ior = T.F(2.4)
    eta = np.array([ior, ior])
    crit = np.arcsin(1.0 / ior)
    N = np.array([[0.0, 0.0, 1.0]] * 2)
    ang = np.array([crit * (1 - 1e-6), crit * (1 + 1e-6)])
    I = np.stack([np.sin(ang), np.zeros(2), -np.cos(ang)], axis=1)
    ok, Tv, k = T.refract_vec(I, N, eta)
    assert ok.tolist() == [True, False] and k[0] > 0 > k[1]
    assert abs(T._norm(Tv[:1])[0, 2]) < 2e-3                                 # the refracted ray grazes the surface
    # the statement's pixels: Fr is exactly 1 where refrOk is false, and below 1 elsewhere (glass case, ior 2.4 from inside)
    o = lab("glass").st.out
    tir = o["glass"] & ~o["refr_ok"]
    assert tir.any() and (o["Fr"][tir] == 1.0).all() and (o["eta"][tir] > 1.0).all()
    assert (o["Fr"][o["glass"] & o["refr_ok"]] < 1.0).all()


def test_simple_constructor_is_the_look_at_constructor_flipped():
    asp = T.aspect_of(70, 33)
    a = T.camera_simple(asp, 1.6, 1.2)
    h = 1.6 / 2.0 / 1.2
    b = T.camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 2.0 * np.arctan(h) / T.DEG, asp, 0.0, 1.2)
    s, t = np.meshgrid(np.linspace(0, 1, 7), np.linspace(0, 1, 5))
    (oa, da), (ob, db) = T.get_ray(a, s, t), T.get_ray(b, s, 1.0 - t)
    assert np.abs(da - db).max() < 1e-14 and np.abs(oa - ob).max() == 0.0


def test_aperture_renders_a_pinhole():
    case = T.CASES["glass"]
    assert case["camera"][0][5] > 0
    c = T.camera_from(case["camera"], case["W"], case["H"])
    assert c["lens_radius"] > 0
    pin = [case["camera"][0][:5] + (0.0,) + case["camera"][0][6:]]
    p = T.camera_from(pin, case["W"], case["H"])
    s, t = np.meshgrid(np.linspace(0, 1, 5), np.linspace(0, 1, 5))
    assert all(np.array_equal(a, b) for a, b in zip(T.get_ray(c, s, t), T.get_ray(p, s, t)))
