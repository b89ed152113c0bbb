"""The oracle's evaluateBSDF, material_pdf and material_scatter against tests/shading_truth.py, the float64 statement made from
the reference's text alone, and the identities a sampler and its pdf must satisfy, checked on the statement
alone -- with the places where the reference's own formulas do not satisfy them asserted as documented cases.  CPU only; the
device functions meet the same statement in tests/test_shading_truth_gpu.py."""
import numpy as np
import pytest

import shading_truth as T


class Lab:
    def __init__(self, P, O):
        self.scene, self.lib, self.mats = T.open_library(P)
        self.names = T.library_names()
        self.states = T.scatter_states(O)
        self.adv = T.advance(O, self.states)

    def one(self, name):
        """The arrays of one material, as a 1-item statement input."""
        return T.gather(self.lib, np.array([self.names.index(name)]))


@pytest.fixture(scope="module")
def lab(P, O):
    lab = Lab(P, O)
    yield lab
    lab.scene.close()


@pytest.fixture(scope="module")
def judged(lab, O):
    """Every item of every material through the oracle, judged by the statement with the table's tolerances."""
    out = {}
    for m, name in enumerate(lab.names):
        x = T.eval_items(lab.lib, [m])
        y = T.scatter_items(m, lab.states)
        out[name] = (T.judge_eval(lab.lib, x, O.eval_bsdf_n(lab.mats, x), tol=T.TOL),
                     T.judge_scatter(lab.lib, y, lab.adv, T.oracle_scatter_got(O.scatter_n(lab.mats, y)), tol=T.TOL))
    return out


def test_library_keeps_the_ids_of_the_function_answers(lab):
    import make_function_kats as M
    assert lab.names[:21] == M.NAMES + ["GlowingNeon"] and len(lab.names) == 21 + len(T.SYNTHETIC) == len(lab.lib["ior"])
    L = lab.lib
    # the classes the synthetic materials are there for
    assert {0.0, 0.02, 0.15, 0.16, 0.5, 1.0} <= set(np.round(L["roughness"][21:], 6))
    assert {0.0, 0.05, 0.1, 1.0} <= set(np.round(L["metallic"][21:], 6))
    tr = L["transmission"][21:] > 0
    assert {1.0, 1.33, 1.5, 2.42} <= set(np.round(L["ior"][21:][tr], 6)) and {0.5, 1.0} <= set(np.round(L["transmission"][21:], 6))
    assert {0.0, 0.3} <= set(np.round(L["transmissionRoughness"][21:][tr], 6))
    cc = L["clearcoat"][21:] > 0
    assert {0.5, 1.0} <= set(np.round(L["clearcoat"][21:], 6)) and {0.0, 0.1, 0.3} <= set(np.round(L["clearcoatRoughness"][21:][cc], 6))
    assert {100.0, 400.0, 800.0} <= set(L["iridescenceThickness"][21:][L["iridescence"][21:] > 0])
    assert (L["sheen"][21:] == 1.0).any() and (L["albedo"][21:] == 0.0).any()
    white = lab.names.index("spec_white")
    assert (L["specular"][white] == 1.0).all() and L["metallic"][white] == 0.0


def test_at_most_two_percent_of_any_material_and_set_is_undecided(lab):
    """From the statement alone: no output of the code under test enters."""
    uni = lab.adv[0]
    seen = dict(eval=0.0, eval_ior1=0.0, scatter=0.0, scatter_both=0.0, scatter_both_ior1=0.0)
    for m, name in enumerate(lab.names):
        ior1 = lab.lib["ior"][m] == 1.0
        x = T.eval_items(lab.lib, [m])
        ids, N, V, L, ff = T.split_eval(x)
        M = T.gather(lab.lib, ids)
        assert len(x) >= 1000
        for what, dec in (("evaluateBSDF", T.evaluateBSDF(M, N, V, L, ff)[1]), ("material_pdf", T.material_pdf(M, N, V, L, ff)[1])):
            assert 1.0 - dec.mean() <= T.MAX_UNDECIDED, f"{name}, {what}: {100 * (1 - dec.mean()):.2f} % undecided"
            seen["eval_ior1" if ior1 else "eval"] = max(seen["eval_ior1" if ior1 else "eval"], 1.0 - dec.mean())
        y = T.scatter_items(m, lab.states)
        ids, N, V, ff = T.split_scatter(y)
        M = T.gather(lab.lib, ids)
        s = T.scatter_sample(M, N, V, ff, uni[:, 0], uni[:, 1], uni[:, 2])
        assert 1.0 - s["decided"].mean() <= T.MAX_UNDECIDED, f"{name}, sampling half of material_scatter"
        seen["scatter"] = max(seen["scatter"], 1.0 - s["decided"].mean())
        full = T.material_scatter(M, N, V, ff, uni[:, 0], uni[:, 1], uni[:, 2])
        key = "scatter_both_ior1" if ior1 else "scatter_both"
        seen[key] = max(seen[key], 1.0 - full["decided"].mean())
        if ior1:
            # DOCUMENTED CASE: at ior 1 the refracted direction is -V, so V x eta + L = 0 and the refraction's half vector
            # (path_logic.cuh:639) is the normalised rounding error of that sum: the value half of every refracted sample, and of
            # nothing else, is undecided
            assert np.array_equal(~full["decided"], s["decided"] & (s["lobe"] == T.LOBE_REFRACT))
            assert (s["lobe"] == T.LOBE_REFRACT).mean() > 0.5
        else:
            assert 1.0 - full["decided"].mean() <= T.MAX_UNDECIDED, f"{name}, material_scatter"
    # the shares recorded in shading_truth.py and DESIGN.md 5.2
    for key, share in T.UNDECIDED.items():
        assert abs(seen[key] - share) <= 1e-9, f"{key}: {seen[key]:.6f}, recorded {share}"


def test_view_in_the_surface_is_undecided_and_finite(lab, O):
    """DOCUMENTED CASE: with NdotV = 0 the early returns (path_logic.cuh:163, pdf.cuh:135) hang on the sign of a rounding error;
    every such item is undecided, and the oracle returns finite numbers for them -- but for one more documented case."""
    x = T.eval_items(lab.lib, nv0=True)
    ids, N, V, L, ff = T.split_eval(x)
    M = T.gather(lab.lib, ids)
    assert not T.evaluateBSDF(M, N, V, L, ff)[1].any() and not T.material_pdf(M, N, V, L, ff)[1].any()
    out = O.eval_bsdf_n(lab.mats, x)
    # DOCUMENTED CASE: material_pdf is 0 / 0 at ior 1 for L = -V, the direction straight through: V x eta + L vanishes, normalize
    # returns the zero vector, and dwh_dwo (pdf.cuh:121) divides LdotH = 0 by (VdotH + LdotH)^2 = 0.  The statement says NaN too.
    nan = np.isnan(T.material_pdf(M, N, V, L, ff)[0])
    assert 0 < nan.sum() <= 8 and (lab.lib["ior"][ids[nan]] == 1.0).all() and (T._dot(V, L)[nan] < -1 + 1e-6).all()
    assert np.isnan(out[nan, 3]).all() and np.isfinite(out[~nan]).all() and np.isfinite(out[:, :3]).all()


def test_oracle_matches_the_statement(lab, judged):
    for name, (e, s) in judged.items():
        for q in ("f", "pdf"):
            i = int(np.argmax(e[q]))
            assert e[q][i] <= T.TOL[q], f"{name}: {q} of eval item {i} is {e[q][i]:.3g} units off (allowed {T.TOL[q]})"
        assert not s["flags_bad"].any(), f"{name}: ok / specular flags differ at items {np.flatnonzero(s['flags_bad'])[:8]}"
        assert not s["draws_bad"].any(), f"{name}: number of uniforms drawn differs at {np.flatnonzero(s['draws_bad'])[:8]}"
        for q in ("direction", "attenuation", "out_pdf"):
            i = int(np.argmax(s[q]))
            assert s[q][i] <= T.TOL[q], f"{name}: {q} of scatter item {i} is {s[q][i]:.3g} units off (allowed {T.TOL[q]})"
    # every lobe was met, on decided items
    lobes = np.concatenate([s["sample"]["lobe"][s["decided"]] for _, s in judged.values()])
    assert set(np.unique(lobes)) == {T.LOBE_COAT, T.LOBE_SPEC, T.LOBE_REFRACT, T.LOBE_TIR, T.LOBE_DIFFUSE}
    # specular (1,1,1) at metallic 0: F = 1, P_opaque_spec = 1 and P_opaque_diff = 0 exactly, so `return false`
    # (path_logic.cuh:712) is reached by u = 1 alone, the largest value curand_uniform returns (2^-24 of the draws): every one of
    # these draws takes the specular lobe.  The false return is not met at this count.
    white = judged["spec_white"][1]["sample"]
    assert white["ok"].all() and (white["lobe"] == T.LOBE_SPEC).all()


def test_scatter_outside_the_integrators_domain(lab, O):
    """V in or below the surface: tracePath never asks, the functions answer all the same.  Judged where decided; no bound."""
    st = T.scatter_states(O, T.OUTSIDE_VIEWS, 256)
    adv = T.advance(O, st)
    for name in ("PlasticRed", "Gold", "CarPaintMidnight", "Glass", "trans1_coat"):
        y = T.scatter_items(lab.names.index(name), st, T.OUTSIDE_VIEWS)
        out = O.scatter_n(lab.mats, y)
        assert np.isfinite(out[:, :8]).all()
        s = T.judge_scatter(lab.lib, y, adv, T.oracle_scatter_got(out), tol=T.TOL)
        assert not s["flags_bad"].any() and not s["draws_bad"].any()
        for q in ("direction", "attenuation", "out_pdf"):
            assert s[q].max() <= T.TOL[q], f"{name}: {q} {s[q].max():.3g} units"


def test_the_table_is_what_the_oracle_measures(P, O):
    """The maxima recorded in shading_truth.py, re-measured on the material that attains each."""
    for q, (name, value) in T.MEASURED.items():
        worst, _ = T.measure(P, O, [name])
        assert abs(worst[q] - value) <= 0.02 * value, f"{q} on {name}: {worst[q]:.3f}, table says {value}"
        assert T.TOL[q] == 4 * value


def test_the_named_terms_are_needed(P, O):
    """The units carry two named cancellation terms.  With the terms left out the same comparison gives the deviations recorded
    beside them, far beyond the table: they are needed, by this much, on these materials."""
    for name in sorted({n for n, _ in T.WITHOUT_TERMS}):
        worst, _ = T.measure(P, O, [name], terms=False)
        for (n, q), value in T.WITHOUT_TERMS.items():
            if n == name:
                assert abs(worst[q] - value) <= 0.02 * value, f"{q} on {name} without the terms: {worst[q]:.4g}, recorded {value}"
                assert q == "direction_rad" or value > 2 * T.TOL[q]
    # the largest distance between the sampled direction and the statement's is the same with the terms: it is no unit
    worst, _ = T.measure(P, O, ["trans1_ior242"])
    value = T.WITHOUT_TERMS["trans1_ior242", "direction_rad"]
    assert abs(worst["direction_rad"] - value) <= 0.02 * value and worst["direction"] <= T.TOL["direction"]


@pytest.mark.parametrize("mis, names", [("fresnel_exp4", ("PlasticRed",)), ("k_over_2", ("PlasticRed",)), ("eta_back", ("Glass",)),
                                        ("basis_sign", ("PlasticRed",)), ("specprob_vdoth", ("PlasticRed",))])
def test_a_seeded_misreading_is_caught(lab, O, mis, names):
    """The statement, misread on purpose, must disagree with the oracle on a decided item by more than the table allows."""
    caught = []
    for name in names:
        m = lab.names.index(name)
        x = T.eval_items(lab.lib, [m])
        e = T.judge_eval(lab.lib, x, O.eval_bsdf_n(lab.mats, x), mis=mis, tol=T.TOL)
        y = T.scatter_items(m, lab.states)
        s = T.judge_scatter(lab.lib, y, lab.adv, T.oracle_scatter_got(O.scatter_n(lab.mats, y)), mis=mis, tol=T.TOL)
        caught += [q for q in ("f", "pdf") if (e[q] > T.TOL[q]).any()]
        caught += [q for q in ("direction", "attenuation", "out_pdf") if (s[q] > T.TOL[q]).any()]
        caught += [q for q in ("flags_bad", "draws_bad") if s[q].any()]
    want = dict(fresnel_exp4="f", k_over_2="f", eta_back="f", basis_sign="direction", specprob_vdoth="pdf")[mis]
    assert want in caught, f"{mis}: only {caught} differ"


# ---------------------------------------------------------------------------------------------------- identities (statement alone)
GL_X, GL_W = np.polynomial.legendre.leggauss(4)


def polar_grid(theta_edges):
    """Gauss-Legendre nodes and weights (4 per cell) of a grid in the polar angle."""
    a, b = theta_edges[:-1, None], theta_edges[1:, None]
    return (0.5 * (a + b) + 0.5 * (b - a) * GL_X).ravel(), (0.5 * (b - a) * GL_W).ravel()


LOG_THETA = np.concatenate([[0.0], np.logspace(-9, np.log10(np.pi / 2), 361)])   # 40 cells per decade: a2 = 1e-12 has theta ~ 1e-6


def half_vectors(N, theta, w_theta, n_phi):
    """H over the hemisphere of N on (theta) x (n_phi midpoints): -> H (n,3), solid-angle weights (n,)."""
    t, b = T._frame(N)
    phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    H = (np.sin(th) * np.cos(ph))[..., None] * t + (np.sin(th) * np.sin(ph))[..., None] * b + np.cos(th)[..., None] * N
    w = (w_theta * np.sin(theta))[:, None] * np.full(n_phi, 2 * np.pi / n_phi)
    return H.reshape(-1, 3), w.ravel()


def rep(M1, n):
    return {k: np.repeat(v, n, axis=0) for k, v in M1.items()}


def pdf_mass(M1, N, V, ff=True, n_phi=48):
    """Integral of material_pdf over the directions L = reflect(-V, H), H over the hemisphere of N with V.H > 0 (that covers
    every L above the surface), in half-vector coordinates: dL = 4 V.H dH."""
    theta, wt = polar_grid(LOG_THETA)
    H, w = half_vectors(N, theta, wt, n_phi)
    n = len(H)
    Vn = np.repeat(V[None], n, axis=0)
    vh = T._dot(Vn, H)
    L = 2.0 * vh[:, None] * H - Vn
    pdf = T.material_pdf(rep(M1, n), np.repeat(N[None], n, axis=0), Vn, L, np.full(n, ff))[0]
    return float((pdf * 4.0 * vh * w)[vh > 0].sum())


def sampler_draws(M1, N, V, ff, n=65536, seed=1):
    rs = np.random.RandomState(seed)
    u = rs.random_sample((n, 3))
    return T.material_scatter(rep(M1, n), np.repeat(N[None], n, axis=0), np.repeat(V[None], n, axis=0), np.full(n, ff),
                              u[:, 0], u[:, 1], u[:, 2])


def lobe_mass(roughness):
    """Integral over the hemisphere of pdf_ggx_reflect in half-vector coordinates at V = N: 2 pi int D cos sin dtheta."""
    theta, wt = polar_grid(LOG_THETA)
    N = np.repeat(np.array([[0.0, 0.0, 1.0]]), len(theta), axis=0)
    H = np.stack([np.sin(theta), 0 * theta, np.cos(theta)], axis=1)
    D = T.distributionGGX(N, H, np.full(len(theta), roughness))
    return float(2 * np.pi * (D * np.cos(theta) * np.sin(theta) * wt).sum())


def test_4a_the_clamped_lobe_loses_its_mass():
    """DOCUMENTED CASE (pbr_utils.cuh:47): `a2 / fmaxf(denom, 1e-6f)` caps D wherever pi d^2 < 1e-6, which is the peak of every
    lobe with roughness below ~0.155, while importance_sample_ggx draws from the uncapped GGX: pdf_ggx_reflect is not the density
    of what is sampled, and integrates to these masses."""
    for rough, mass, tol in ((0.02, 5.7e-4, 0.05e-4), (0.05, 0.0220, 0.00005), (0.1, 0.323, 0.0005), (0.15, 0.9894, 0.00005)):
        assert abs(lobe_mass(T.F(rough)) - mass) <= tol, (rough, lobe_mass(T.F(rough)))
    for rough in (0.16, 0.2, 0.3, 0.5, 1.0):
        assert abs(lobe_mass(T.F(rough)) - 1.0) <= 1e-4, (rough, lobe_mass(T.F(rough)))
    # the edge: the cap bites while pi a2^2 < 1e-6, i.e. below roughness (1e-6 / pi)^(1/8)
    assert abs((T.F(1e-6) / T.PI) ** 0.125 - 0.1541) < 1e-4


MASS_HOLDS = ("rough016", "rough1", "metal1_r016", "metal1_r1", "PlasticRed", "coat1_r03", "coat1_metal", "sheen_tint", "irid400",
              "spec_white", "albedo_zero_channel")


def test_4a_mass_of_the_pdf_is_the_share_of_the_draws_it_accounts_for(lab):
    """Opaque, every sampled GGX roughness >= 0.16: the pdf integrates to the fraction of the sampler's draws that leave above
    the surface (the others get pdf 0 and attenuation 0).  65,536 draws: 4 sigma of the binomial + 2e-3 for the quadrature."""
    nm = T.normals()
    for name in MASS_HOLDS:
        M1 = lab.one(name)
        assert M1["transmission"][0] == 0 and max(M1["roughness"][0], 0.02) >= T.F(0.16)
        assert M1["clearcoat"][0] == 0 or M1["clearcoatRoughness"][0] >= T.F(0.16)
        for c in (1.0, 0.7, 0.3):
            N = nm["rand0"]
            V = T.view(N, c)
            s = sampler_draws(M1, N, V, True)
            p = float((s["ok"] & (T._dot(s["direction"], np.repeat(N[None], len(s["ok"]), axis=0)) > 0)).mean())
            mass = pdf_mass(M1, N, V)
            assert abs(mass - p) <= 4 * np.sqrt(p * (1 - p) / 65536) + 2e-3, f"{name}, NdotV {c}: mass {mass:.4f}, draws {p:.4f}"


def test_4a_mass_of_the_library_metals_is_the_clamped_lobes(lab):
    """DOCUMENTED CASE: the whole pdf of Silver (roughness 0.05) integrates to 0.022, of Gold (0.1) to 0.32, while all of their
    draws leave above the surface at normal incidence: their MIS weights see a BSDF sampler 45 x and 3 x less likely than it is."""
    N = np.array([0.0, 0.0, 1.0])
    for name, mass, tol in (("Silver", 0.0220, 5e-5), ("Gold", 0.323, 5e-4), ("metal1_r002", 5.7e-4, 5e-6), ("metal1_r015", 0.9894, 5e-5)):
        M1 = lab.one(name)
        s = sampler_draws(M1, N, N, True, n=4096)
        assert s["ok"].all() and (s["direction"][:, 2] > 0).mean() > 0.999
        a2 = max(M1["roughness"][0], T.F(0.02)) ** 4
        below = a2 / (1 + a2)         # the share of the GGX lobe beyond 45 degrees, whose reflections leave below the surface
        assert abs(pdf_mass(M1, N, N) + below - mass) <= tol, (name, pdf_mass(M1, N, N))


DENSITY_PAIRS = (("rough016", 1.0), ("rough016", 0.7), ("metal1_r016", 0.7), ("coat1_r03", 0.7), ("spec_white", 0.3),
                 ("sheen_tint", 0.7), ("irid100", 0.7), ("coat1_metal", 1.0))


def test_4b_density_of_the_draws_is_the_pdf(lab):
    """65,536 draws of the statement's sampler, binned by their half vector H = normalize(V + L) in 8 x 8 bins (polar angle about
    N at the octiles of the material's own GGX lobe, azimuth uniform), against the quadrature of material_pdf x 4 V.H over each
    bin (96 x 24 midpoints).  A bin count is binomial(n, p): accepted within 5 sqrt(n p (1 - p)) + 0.5 % of n p + 2 (the last
    two for the quadrature across the horizon cut); seeds are fixed."""
    nm = T.normals()
    n = 65536
    for name, c in DENSITY_PAIRS:
        M1 = lab.one(name)
        N = nm["rand1"]
        V = T.view(N, c)
        t, b = T._frame(N)
        a2 = max(M1["roughness"][0], T.F(0.02)) ** 4
        q = np.arange(9) / 8.0
        edges = np.arccos(np.sqrt((1 - q) / (1 + (a2 - 1) * q)))
        s = sampler_draws(M1, N, V, True, n=n, seed=7)
        L = s["direction"]
        up = s["ok"] & (L @ N > 0)
        H = T._normalize(V[None] + L[up])
        th = np.arccos(np.clip(H @ N, -1, 1))
        ph = np.mod(np.arctan2(H @ b, H @ t), 2 * np.pi)
        it = np.clip(np.searchsorted(edges, th, side="right") - 1, 0, 7)
        ip = np.minimum((ph / (2 * np.pi / 8)).astype(int), 7)
        counts = np.bincount(it * 8 + ip, minlength=64).reshape(8, 8)
        for i in range(8):
            theta = edges[i] + (np.arange(96) + 0.5) * (edges[i + 1] - edges[i]) / 96
            Hq, w = half_vectors(N, theta, np.full(96, (edges[i + 1] - edges[i]) / 96), 8 * 24)
            k = len(Hq)
            Vn = np.repeat(V[None], k, axis=0)
            vh = T._dot(Vn, Hq)
            Lq = 2.0 * vh[:, None] * Hq - Vn
            pdf = T.material_pdf(rep(M1, k), np.repeat(N[None], k, axis=0), Vn, Lq, np.ones(k, bool))[0]
            p = np.where(vh > 0, pdf * 4.0 * vh * w, 0.0).reshape(96, 8, 24).sum(axis=(0, 2))
            bound = 5 * np.sqrt(n * p * (1 - p)) + 0.005 * n * p + 2
            assert (np.abs(counts[i] - n * p) <= bound).all(), f"{name}, NdotV {c}, polar bin {i}: {counts[i]} vs {n * p}"
        assert counts.sum() > 0.5 * n


def test_4c_out_pdf_against_material_pdf(lab):
    """out_pdf of material_scatter and material_pdf(V, scattered direction), both from the statement, over the scatter items."""
    uni = lab.adv[0]
    found = {}
    for m, name in enumerate(lab.names):
        y = T.scatter_items(m, lab.states)
        ids, N, V, ff = T.split_scatter(y)
        M = T.gather(lab.lib, ids)
        s = T.material_scatter(M, N, V, ff, uni[:, 0], uni[:, 1], uni[:, 2])
        mp, dp, _ = T.material_pdf(M, N, V, s["direction"], ff)
        ok = s["ok"] & s["decided"] & dp
        ndl = T._dot(N, s["direction"])
        # (1e-6: `NdotL * (1.0f / PI)` in pdf.cuh:76 and `NdotL / PI` in path_logic.cuh:758 differ by the rounding of a literal)
        agree = np.abs(s["out_pdf"] - mp) <= 1e-6 * np.maximum(s["out_pdf"], mp)
        transmissive = (lab.lib["transmission"][m] > 0) & (lab.lib["metallic"][m] < T.F(0.1))
        if not transmissive:
            # the identity: equal wherever the direction leaves above the surface
            assert agree[ok & (ndl > 0)].all(), name
            # DOCUMENTED CASE: below the surface material_pdf is 0 (pdf.cuh:169, :208 gate every term by NdotL > 0) while
            # material_scatter adds the coat and the specular lobe's pdf unconditionally (path_logic.cuh:722-751)
            below = ok & (ndl < 0)
            assert (mp[below] == 0).all() and (s["out_pdf"][below] >= 0).all(), name
            found[name] = int((s["out_pdf"][below] > 0).sum())
        else:
            lobe = s["lobe"]
            eta = np.where(ff, 1.0 / lab.lib["ior"][m], lab.lib["ior"][m])
            H = T._normalize(V + s["direction"])
            k_half = 1.0 - eta * eta * (1.0 - np.maximum(T._dot(V, H), 0.0) ** 2)
            floor = s["out_pdf"] <= T.F(1e-6) * (1 + 1e-9)               # `fmaxf(pdf_total, 1e-6f)`, path_logic.cuh:687
            # refracted samples and total internal reflections carry the pdf material_pdf gives them
            sel = ok & ~floor & ((lobe == T.LOBE_REFRACT) & (ndl < 0) | (lobe == T.LOBE_TIR))
            assert agree[sel].all(), name
            # coat and reflection samples agree outside the region of total internal reflection ...
            sel = ok & ~floor & (ndl > 0) & ((lobe == T.LOBE_COAT) | (lobe == T.LOBE_SPEC))
            assert agree[sel & (k_half > 1e-4)].all(), name
            # ... DOCUMENTED CASE: inside it (k < 0 at the half vector of V and the direction) material_pdf adds the lobe of the
            # refraction samples that were reflected (pdf.cuh:188-198) whatever lobe the direction came from, material_scatter
            # only when it came from the refraction branch (path_logic.cuh:671): out_pdf is smaller
            inside = sel & (k_half < -1e-4)
            if inside.any():
                assert (s["out_pdf"][inside] < mp[inside]).all(), name
            found[name] = int(inside.sum())
    # the case exists: back faces of the dielectrics, none on a material without total internal reflection
    assert found["Glass"] > 100 and found["Diamond"] > 100 and found["trans1_ior1"] == 0, found
    # and so does the other: draws of the opaque lobes that leave below the surface with a positive out_pdf
    assert found["Silver"] > 100 and found["PlasticRed"] > 100 and found["CarPaintMidnight"] > 100, found


def refraction_jacobian(eta, c, n_theta=24, n_phi=16, theta_max=0.6):
    """The map H -> L of the refraction branch (path_logic.cuh:569-584) around N = z at NdotV = c: -> (ratio, weight D-free):
    ratio = dwh_dwo as pdf_ggx_refract claims it x the solid-angle Jacobian dL/dH measured by central differences -- 1 if the
    claim is the Jacobian of the sampled map -- with the closed form the measurement is held to."""
    N = np.array([0.0, 0.0, 1.0])
    V = np.array([np.sqrt(1 - c * c), 0.0, c])
    theta = (np.arange(n_theta) + 0.5) * theta_max / n_theta
    H, _ = half_vectors(N, theta, np.full(n_theta, theta_max / n_theta), n_phi)

    def refract(H):               # the statement's own refraction branch (path_logic.cuh:569-584)
        n = len(H)
        vh, _, k, _, L = T.refraction_branch(np.repeat(V[None], n, axis=0), H, np.full(n, eta))
        return L, vh, k

    L0, vh, k = refract(H)
    good = (vh > 0.05) & (k > 0.05)
    e1 = np.cross(H, V)
    e1 /= np.linalg.norm(e1, axis=1)[:, None]
    e2 = np.cross(H, e1)
    h = 1e-5

    def moved(e):
        Hp = H + h * e
        Hm = H - h * e
        return (refract(Hp / np.linalg.norm(Hp, axis=1)[:, None])[0] - refract(Hm / np.linalg.norm(Hm, axis=1)[:, None])[0]) / (2 * h)

    jac = np.linalg.norm(np.cross(moved(e1), moved(e2)), axis=1)            # dL / dH
    ldh = np.abs(np.einsum("ij,ij->i", L0, H))
    # dH / dL as the statement's pdf_ggx_refract claims it (pdf.cuh:121): at roughness 1 D = 1 / pi, so pdf = NdotH / pi x dwh_dwo
    n = len(H)
    claimed = T.pdf_ggx_refract(np.repeat(N[None], n, axis=0), np.repeat(V[None], n, axis=0), L0, np.ones(n), np.full(n, eta)) * \
        T.PI / (H @ N)
    closed = eta * eta * (eta * vh - ldh) ** 2 / (eta * vh + ldh) ** 2
    return (claimed * jac)[good], closed[good]


def test_4d_the_refraction_pdf_is_not_the_density_of_the_refracted_draws(lab):
    """DOCUMENTED CASE (pdf.cuh:121, path_logic.cuh:654): dwh_dwo = eta^2 LdotH / (eta VdotH + LdotH)^2 with both cosines taken
    positive.  The Jacobian of the sampled map is LdotH / (eta VdotH - LdotH)^2 (the two cosines have opposite signs, and eta
    is already the ratio), so the claimed density is eta^2 (eta c_i - c_o)^2 / (eta c_i + c_o)^2 times the true one: measured
    here by central differences of the statement's own refraction, for Glass and Water on both faces."""
    seen = {}
    for name in ("Glass", "Water"):
        ior = float(lab.one(name)["ior"][0])
        for front in (True, False):
            eta = 1.0 / ior if front else ior
            r = np.concatenate([refraction_jacobian(eta, c)[0] for c in (1.0, 0.7, 0.9 if not front else 0.3)])
            cl = np.concatenate([refraction_jacobian(eta, c)[1] for c in (1.0, 0.7, 0.9 if not front else 0.3)])
            assert len(r) > 300 and np.allclose(r, cl, rtol=1e-5), (name, front)
            seen[name, front] = (float(r.min()), float(r.max()))
            assert np.median(r) < 0.25, "the claimed density is a fraction of the true one over most of the lobe"
    # at normal incidence and H = N: eta^2 (eta - 1)^2 / (eta + 1)^2
    for (name, front), (lo, hi) in seen.items():
        ior = float(lab.one(name)["ior"][0])
        eta = 1.0 / ior if front else ior
        assert lo <= eta ** 2 * (eta - 1) ** 2 / (eta + 1) ** 2 * 1.3 and hi >= eta ** 2 * (eta - 1) ** 2 / (eta + 1) ** 2 * 0.7
    for key, (lo, hi) in REFRACTION_RATIO.items():
        assert abs(seen[key][0] - lo) <= 0.02 * lo and abs(seen[key][1] - hi) <= 0.02 * hi, (key, seen[key])


# smallest and largest claimed / true density over the grid of the test above
REFRACTION_RATIO = {("Glass", True): (0.01778, 0.3556), ("Glass", False): (0.09004, 1.0116),
                    ("Water", True): (0.011343, 0.4254), ("Water", False): (0.035498, 0.6251)}
