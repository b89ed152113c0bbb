"""Next-event estimation and the integrator of the reference (sample_direct_lighting_with_mat, tracePath) and the sample loop of
ptrt_query_radiance, stated once more in float64 numpy.

TEST INFRASTRUCTURE.  The kernels (pt_render, pt_async, pt_wavefront, pt_radiance.hip.h) and oracle/ptrt_oracle.cpp are ONE
reading of path_logic.cuh:305-393 and :782-899, held to each other at tolerance 0.  This module is a second reading, made from
the reference's text alone (file:line beside each function, relative to the reference's src/pathtracer), vectorised over rays.
It reuses three things that are pinned elsewhere and nothing else of the oracle: `brute_force.closest` / `brute_force.occluded`
for every extension and shadow ray (no tree), `shading_truth` for evaluateBSDF, material_pdf and material_scatter's two halves,
and `oracle_xorwow_draw` for the uniforms of a generator state.  Literals are the float32 values the text spells; everything
else is float64, with one exception that the reused brute force sets: a Ray holds floats, and brute_force takes rays as
float32, so the statement rounds every ray it makes (origin, direction) to float32 before it uses it for anything.

sample_direct_lighting_with_mat is stated in two halves, as shading_truth states material_scatter: `light_sample` maps (hit
point, normal, lights, uniforms) to (index, L, pdf_sample, light_dist, radiance x attenuation, shadow origin, shadow tmax,
uniforms drawn) and `light_value` maps (that sample, V, material, shadowed) to the clamped contribution; the comparison judges
the contribution AT THE L UNDER TEST.  `vertex` is one turn of tracePath's loop from a given ray, hit record, throughput and
uniforms; `trace_path` chains it with the brute force; `query_radiance` is the sample loop as include/ptrt.h words it.

DECIDED.  As in brute_force (DELTA, GAP) and shading_truth (M_DOT, M_K, M_PROB, M_DIFF, M_P0, M_LEN), reused unchanged.  The new
discontinuous decisions and their margins:
    M_PICK  = 1e-6    r x nLights against the nearest integer 1 .. nLights - 1 (the product rounds by 2^-24 x nLights)
    M_CONE  = 1e-6    theta against outerCone on the hard edge; (theta - outerCone) / epsilon against 0 where the soft factor
                      gates "some channel of the contribution > 0"
    M_SOLID = 7.5e-7  solid_angle against 1e-6: float32 keeps 1 - cos_theta_max to about 2^-24 absolute, twice, and 2 pi x 2 x
                      2^-24 = 7.5e-7, so float32's solid angle is one of 0, 3.7e-7, 7.5e-7, 1.12e-6 .. next to the threshold
    M_DOT   = 1e-6    (shading_truth's) the sign of N.L for the shadow offset and of scatter_dir.N for the origin offset
    brute_force's own rule for the shadow ray's occlusion at tmax = light_dist - 1e-3
    M_RR    = 1e-5    u > p of the roulette (p carries the throughput's accumulated rounding)
    M_POS   = 1e-30   "some channel of the contribution > 0": positive beyond float32's underflow, or zero through a gate that
                      is itself decided (the shadow ray, the BSDF's own gates, the hard edge, the soft factor by M_CONE)
    M_TEX   = 1.5e-3  the environment map's 8-bit filter weight: frac x 256 against the next half (oracle/ptrt_oracle.cpp's
                      texture-filter convention -- PARITY UNPINNED there, restated here as it is written, not re-derived);
                      atan2f and acosf to 2 ulp put 2.5e-6 on u x 16 and 8e-7 on v x 8: 6.4e-4 after x 256, doubled
Comparisons of a float32 input with a float32 literal need none: radius <= 0, epsilon <= 1e-6f (innerCone - outerCone, formed in
float32 here, where the difference of two inputs is what both precisions see), emission > 0, light type, front_face.  Continuous
clamps (the soft clamps 500 / 50 / 100, fminf(sin^2, 0.9999f), the roulette's 0.05 / 0.95) need none.  A path is decided when
every vertex on it is.  At most 2 % of the vertices of any (light set, ray set) may be undecided and at most 5 % of the paths
at depth 5 (asserted in tests/test_path_truth.py from this module alone); light set H is outside that bound and says so: its
solid angle crosses 1e-6 inside the scene, and a light sample there is undecided by construction.

SCENE.  `light_lab` (below, not in ptrt_amd.scenes): a floor quad and eight objects floating at least 0.05 above it, nothing
coplanar with anything (coplanar faces are ties); LIGHT_SETS A .. H are applied to the same scene; RAY_SETS
hold at most 2,048 unit rays each with generator states from xorwow_init(SEED).

TOLERANCES.  shading_truth's convention: unit(q) = EPS32 x (|q| + sum_i |x_i dq/dx_i|), x_i over the float32 inputs of the
vertex (ray direction, hit point, normal, t, the picked light's fields, the material's fields, the uniforms, the throughput),
central differences of `vertex` with a relative step of 2^-23, branches held.  Cancelling expressions that lose more than any
input's rounding explains are NAMED and add a term of their own (`terms=False` leaves them out):
  * `1.0f - cos_theta_max` (path_logic.cuh:353 and sampling.cuh:111): kept to 2^-24 absolute twice (the rounding of
    cos_theta_max and of 1 - sin^2 before the root), so solid_angle carries 2 pi x 2^-23 absolute:
        unit(pdf_sample) += pdf_sample x 2 pi 2^-23 / solid_angle, and the same share of the contribution and its weight.
  * `1.0f - cos_theta * cos_theta` in sample_cone_direction (sampling.cuh:112), with cos_theta = 1 - u1 (1 - cos_theta_max)
    itself kept to 2^-24: sin_theta is known to sqrt(sin^2 + 2^-22) - sin:   unit(L) += that.
The measured table is MEASURED below (python tests/path_truth.py prints it); tests/test_path_truth.py re-measures it.
"""
import ctypes as C

import numpy as np

import brute_force as bf
import shading_truth as T
from shading_truth import EPS32, F, PI, TWO_PI, _col, _dot

LIGHT_POINT, LIGHT_DIRECTIONAL, LIGHT_SPOT = 0, 1, 2          # scene/lights.cuh:8-12
M_PICK, M_CONE, M_SOLID, M_RR, M_POS, M_TEX = 1e-6, 1e-6, 7.5e-7, 1e-5, 1e-30, 1.5e-3
M_DOT = T.M_DOT
MAX_UNDECIDED_VERTICES, MAX_UNDECIDED_PATHS = 0.02, 0.05
SEED = 20261019
DEPTH = 5
DRAWS_PER_VERTEX = 7                                          # 3 for the light sample, 3 for the scatter, 1 for the roulette
RR_START, RR_MIN = 2, F(0.05)                                 # rendering/path_logic.cuh:24-25
MAX_BOUNCE_WEIGHT, MAX_NEE, MAX_FINAL = F(50.0), F(500.0), F(100.0)   # :27-29

MISREADINGS = ("nee_primary", "emission_always", "pdf_pick_sphere", "attenuate_linear", "spot_theta_centre", "balance",
               "rr_from_3", "no_div_p", "absorb_front", "pick_round")

# quantity -> (case that attains it, largest deviation of the oracle in units); tests/test_path_truth.py re-measures
MEASURED = dict(L=("E-glass-gradient", 0.9288), pdf_sample=("E-free-gradient", 0.8296), light_dist=("E-emissive-gradient", 0.9501),
                contribution=("F-glass-off", 1.374), w=("G-glass-gradient", 0.8838), throughput_absorbed=("B-glass-off", 0.9048),
                p=("A-glass-gradient", 0.7801), throughput_after=("A-glass-gradient", 0.9999), next_origin=("B-glass-off", 0.43),
                accumulated=("F-glass-off", 1.373), radiance=("A-glass-gradient", 7.762))
# the same measurement with the named terms left out of the units: (case, quantity) -> units
WITHOUT_TERMS = {("D-free-off", "L"): 16.61, ("D-free-off", "pdf_sample"): 41.38, ("D-free-off", "contribution"): 17.18,
                 ("A-emissive-gradient", "radiance"): 69.03, ("H-glass-off", "pdf_sample"): 155140.0,
                 ("H-glass-off", "contribution"): 39697.0}
TOL = {q: 4 * v for q, (_, v) in MEASURED.items()}


# ------------------------------------------------------------------------------------------------------------ small functions
def clamp_vector_soft(v, max_lum):                   # rendering/path_logic.cuh:44-52
    lum = F(0.2126) * v[:, 0] + F(0.7152) * v[:, 1] + F(0.0722) * v[:, 2]
    on = (lum > max_lum) & (lum > 0.0)
    with np.errstate(all="ignore"):
        return np.where(_col(on), v * _col(max_lum / np.where(on, lum, 1.0)), v)


def mis_weight(a, b, mis=None):                      # math/pdf.cuh:26-30
    if mis == "balance":
        return a / (a + b + F(1e-10))
    return a * a / (a * a + b * b + F(1e-10))


def attenuate(distance, rng, mis=None):              # rendering/render_utils.cuh:21-24
    att = rng / (rng + distance)
    return att if mis == "attenuate_linear" else att * att


def sample_cone_direction(axis, cos_theta_max, u1, u2):   # math/sampling.cuh:105-120
    """-> (direction, what float32 may lose in sin_theta; see TOLERANCES)"""
    cos_theta = 1.0 - u1 * (1.0 - cos_theta_max)
    s2 = np.maximum(0.0, 1.0 - cos_theta * cos_theta)
    sin_theta = np.sqrt(s2)
    phi = TWO_PI * u2
    Tn, B = T.createOrthoNormalBasis(axis)
    d = _col(sin_theta * np.cos(phi)) * Tn + _col(sin_theta * np.sin(phi)) * B + _col(cos_theta) * axis
    return d, np.sqrt(s2 + 2.0 * EPS32) - sin_theta


def spot_factor(theta, inner, outer, dec=None, active=None):   # rendering/path_logic.cuh:361-369
    eps = (inner.astype(np.float32) - outer.astype(np.float32)).astype(np.float64)
    hard = eps <= F(1e-6)
    if dec is not None:
        dec.far(theta, outer, M_CONE, active & hard)
    with np.errstate(all="ignore"):
        soft = np.clip((theta - outer) / np.where(hard, 1.0, eps), 0.0, 1.0)
    return np.where(hard, np.where(theta >= outer, 1.0, 0.0), soft), hard, eps


def absorption(albedo, t, back, mis=None):           # rendering/path_logic.cuh:823-829, pbr_utils.cuh:151-162
    coeff = np.maximum(-np.log(np.maximum(F(1e-6), albedo)), 0.0)
    on = np.ones_like(back) if mis == "absorb_front" else back
    return np.where(_col(on), np.exp(-coeff * _col(t)), 1.0)


def roulette_p(thr):                                 # rendering/path_logic.cuh:872-875
    return np.maximum(RR_MIN, np.minimum(F(0.95), thr.max(axis=1)))


class Sky:
    """off, gradient, or an environment map ((h, w, 4) float32, row 0 = v 0)."""

    def __init__(self, use=False, top=(0, 0, 0), bottom=(0, 0, 0), env=None):
        self.use = bool(use)
        self.top = np.asarray(top, np.float32).astype(np.float64)
        self.bottom = np.asarray(bottom, np.float32).astype(np.float64)
        self.env = None if env is None else np.ascontiguousarray(env, np.float32)


def sample_sky(d, sky):                              # rendering/render_utils.cuh:115-137
    """-> (colour (n,3), decided)"""
    n = len(d)
    if not sky.use:
        return np.zeros((n, 3)), np.ones(n, bool)
    if sky.env is None:
        t = 0.5 * (d[:, 1] + 1.0)
        return T._lerp(sky.bottom[None, :], sky.top[None, :], t), np.ones(n, bool)
    # tex2D as oracle/ptrt_oracle.cpp:718-748 words it (normalised coordinates, wrap in u, clamp in v, linear filter with
    # 8 fractional bits rounded to nearest): the oracle's DOCUMENTED convention, parity unpinned, said here and not re-derived
    h, w = sky.env.shape[:2]
    E = sky.env.astype(np.float64)
    phi = np.arctan2(d[:, 2], d[:, 0])
    theta = np.arccos(np.maximum(-1.0, np.minimum(1.0, d[:, 1])))
    u = (phi + PI) * F(1.0 / TWO_PI)
    v = theta * F(1.0 / PI)
    uw = u - np.floor(u)
    vc = np.where(v < 0.0, 0.0, np.where(v >= 1.0, F(1.0 - F(1.0 / h)), v))
    xB, yB = uw * w - 0.5, vc * h - 0.5
    fi, fj = np.floor(xB), np.floor(yB)
    ax, by = (xB - fi) * 256.0, (yB - fj) * 256.0
    dec = (np.abs(ax - np.floor(ax) - 0.5) > M_TEX) & (np.abs(by - np.floor(by) - 0.5) > M_TEX)
    a, b = np.rint(ax) / 256.0, np.rint(by) / 256.0
    i, j = fi.astype(np.int64), fj.astype(np.int64)

    def tex(ii, jj):
        return E[np.clip(jj, 0, h - 1), np.mod(ii, w), :3]

    out = tex(i, j) * _col((1 - a) * (1 - b)) + tex(i + 1, j) * _col(a * (1 - b)) + tex(i, j + 1) * _col((1 - a) * b) + \
        tex(i + 1, j + 1) * _col(a * b)
    return out, dec


# ------------------------------------------------------------------------------------------------------------ lights
LIGHT_FIELDS = ("position", "direction", "color", "intensity", "range", "inner", "outer", "radius")


def make_lights(P, specs):
    """[dict(type, position, direction, color, intensity, range, inner, outer, radius)] -> a ctypes array of ptrt_light"""
    arr = (P.Light * max(len(specs), 1))()
    for k, s in enumerate(specs):
        L = arr[k]
        L.type = s["type"]
        for name in ("position", "direction", "color"):
            v = np.asarray(s.get(name, (0, 0, 0)), np.float64)
            if name == "direction" and np.any(v):
                v = v / np.linalg.norm(v)
            setattr(L, name, P.Vec3(*[float(x) for x in v]))
        L.intensity, L.range, L.radius = s.get("intensity", 1.0), s.get("range", 100.0), s.get("radius", 0.0)
        L.inner_cone, L.outer_cone = s.get("inner", 0.0), s.get("outer", 0.0)
    return arr


def lights64(arr, n):
    """the float32 fields of n ptrt_light as {field: float64 array}"""
    def v3(name):
        return np.array([[getattr(getattr(arr[k], name), c) for c in "xyz"] for k in range(n)], np.float64).reshape(n, 3)
    out = dict(type=np.array([arr[k].type for k in range(n)], np.int64), position=v3("position"), direction=v3("direction"),
               color=v3("color"))
    for f, g in (("intensity", "intensity"), ("range", "range"), ("inner", "inner_cone"), ("outer", "outer_cone"), ("radius", "radius")):
        out[f] = np.array([getattr(arr[k], g) for k in range(n)], np.float64)
    return out


def pick_light(lights, r, mis=None):                 # rendering/path_logic.cuh:320-325
    """-> (index, decided)"""
    n = len(lights["type"])
    x = np.minimum(r, F(0.99999994)) * n
    near = np.rint(x)
    dec = (np.abs(x - near) > M_PICK) | (near < 1) | (near > n - 1)
    idx = near if mis == "pick_round" else np.floor(x)
    return np.clip(idx.astype(np.int64), 0, n - 1), dec


def light_sample(point, N, Lt, r, u1, u2, n_lights, mis=None, index_dec=None):   # rendering/path_logic.cuh:311-381
    """Lt: the PICKED light's fields per item (gather of lights64).  -> dict(L, pdf_sample, light_dist, radiance (colour x
    intensity), attenuation, radatt, shadow_origin, shadow_tmax, draws, solid_angle, sphere, sin_unit, gate (the soft spot
    factor where it is the gate of a zero), decided)."""
    n = len(point)
    dec = T.Decisions(n)
    if index_dec is not None:
        dec.ok &= index_dec
    pdf_pick = 1.0 / float(n_lights)
    directional = Lt["type"] == LIGHT_DIRECTIONAL
    local = ~directional
    toLight = Lt["position"] - point
    d2 = _dot(toLight, toLight)
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2)
        axis = toLight / _col(dist)
        sphere = local & ~(Lt["radius"] <= 0.0)
        sin2 = np.minimum(Lt["radius"] * Lt["radius"] / d2, F(0.9999))
        cos_max = np.sqrt(1.0 - sin2)
        cone, sin_loss = sample_cone_direction(axis, cos_max, u1, u2)
        solid = TWO_PI * (1.0 - cos_max)
        dec.far(solid, F(1e-6), M_SOLID, sphere)
        pdf_sphere = np.where(solid > F(1e-6), pdf_pick / solid, pdf_pick)
        if mis == "pdf_pick_sphere":
            pdf_sphere = np.full(n, pdf_pick)
        L = np.where(_col(directional), -Lt["direction"], np.where(_col(sphere), cone, axis))
        pdf = np.where(sphere, pdf_sphere, pdf_pick)
        light_dist = np.where(directional, F(1e30), dist)
        att = np.where(directional, 1.0, attenuate(dist, Lt["range"], mis))
        spot = local & (Lt["type"] == LIGHT_SPOT)
        theta = _dot(axis if mis == "spot_theta_centre" else L, -Lt["direction"])
        factor, hard, eps = spot_factor(theta, Lt["inner"], Lt["outer"], dec, spot)
        att = np.where(spot, att * factor, att)
        gate = np.where(spot & ~hard, (theta - Lt["outer"]) / np.where(hard, 1.0, eps), 1.0)
    ndl = _dot(N, L)
    dec.far(ndl, 0.0, M_DOT)
    origin = point + np.where(_col(ndl > 0.0), N * F(1e-4), -N * F(1e-4))
    radiance = Lt["color"] * _col(Lt["intensity"])
    return dict(L=L, pdf_sample=pdf, light_dist=light_dist, radiance=radiance, attenuation=att, radatt=radiance * _col(att),
                shadow_origin=origin, shadow_tmax=light_dist - F(1e-3), draws=np.where(sphere, 3, 1), solid_angle=solid,
                sphere=sphere, sin_unit=np.where(sphere, sin_loss, 0.0), gate=gate, decided=dec.ok)


def light_value(s, V, N, ff, M, shadowed, L=None, mis=None):   # rendering/path_logic.cuh:384-392
    """The clamped contribution of light sample s at direction L (default: its own).  -> (contribution (n,3), decided)"""
    L = s["L"] if L is None else L
    f, dec = T.evaluateBSDF(M, N, V, L, ff)
    with np.errstate(all="ignore"):
        direct = f * s["radatt"] / _col(s["pdf_sample"])
    direct = clamp_vector_soft(np.where(_col((s["pdf_sample"] > 0.0) & ~shadowed), direct, 0.0), MAX_NEE)
    return direct, dec | shadowed


# ------------------------------------------------------------------------------------------------------------ the world
class World:
    """What tracePath reads: geometry for the brute force, materials, emission, lights, sky."""

    def __init__(self, P, scene):
        desc = scene.flatten()
        self.desc = desc
        self.geom = bf.Geometry.from_desc(desc)
        m = desc.contents.materials
        self.lib = T.load_materials(m)
        self.emission = np.ctypeslib.as_array(C.cast(m.emission, C.POINTER(C.c_float)), (int(m.count) * 3,)).astype(np.float64).reshape(-1, 3)
        self.lights, self.n_lights, self.light_array = None, 0, None
        self.sky = Sky()

    def set_lights(self, P, specs):
        self.light_array = make_lights(P, specs)
        self.n_lights = len(specs)
        self.lights = lights64(self.light_array, self.n_lights)
        return self

    def oracle_desc(self, P):
        """A copy of the flattened scene with this world's lights and sky, for oracle.trace_paths (keeps what it points to)."""
        d = P.SceneDesc.from_buffer_copy(self.desc.contents)
        d.lights = C.cast(self.light_array, C.POINTER(P.Light)) if self.n_lights else None
        d.light_count = self.n_lights
        d.use_sky = int(self.sky.use)
        d.sky_top, d.sky_bottom = P.Vec3(*self.sky.top), P.Vec3(*self.sky.bottom)
        if self.sky.env is not None:
            d.env_rgba = self.sky.env.ctypes.data_as(C.POINTER(C.c_float))
            d.env_height, d.env_width = self.sky.env.shape[:2]
        else:
            d.env_rgba, d.env_width, d.env_height = None, 0, 0
        self._keep = d
        return C.pointer(d)


def hit_of(world, o, d):
    """brute_force.closest as the hit record `vertex` takes: hit, t, point, normal, mesh, front_face, decided"""
    a = bf.closest(world.geom, o, d)
    t = np.where(a["hit"], a["t"], F(1e30))
    return dict(hit=a["hit"], t=t, point=o + _col(np.where(a["hit"], a["t"], 0.0)) * d, normal=a["normal"],
                mesh=np.where(a["hit"], a["mesh"], -1), front_face=a["front_face"], decided=a["decided"] & ~a["quirk"],
                invcos=a["invcos"], face=a["face"])


# ------------------------------------------------------------------------------------------------------------ one vertex
def _take(uni, cursor, k):
    rows = np.arange(len(uni))
    return uni[rows, np.minimum(cursor + k, uni.shape[1] - 1)]


def _nudged(v, size, sign, axis):
    """v turned by `size` (per item) along one of its two tangents: what a named cancellation may do to a sampled direction"""
    Tn, B = T.createOrthoNormalBasis(v)
    w = v + _col(sign * size) * (Tn if axis == 0 else B)
    return w / _col(np.sqrt(_dot(w, w)))


def vertex(world, bounce, d, spec, hit, thr, acc, prev_spec, uni, mis=None, held=None, sky_dec=True):
    """One turn of tracePath's loop (rendering/path_logic.cuh:795-893) for n rays that HIT: direction d, the ray's specular flag,
    the hit record (t, point, normal, mesh, front_face), throughput and accumulated colour before, prev_was_specular, and the
    next DRAWS_PER_VERTEX uniforms of each ray's stream.  `held`: decisions of an earlier evaluation (index, shadowed, the
    scatter's lobe) to keep while inputs are perturbed.  -> dict, see the end of the function."""
    n = len(d)
    nudge = held.get("nudge") if held else None
    M = held["M"] if held and "M" in held else T.gather(world.lib, hit["mesh"])
    em = held["em"] if held and "em" in held else world.emission[hit["mesh"]]
    N, point, ff = hit["normal"], hit["point"], hit["front_face"]
    V = -d
    dec = np.ones(n, bool)
    # :823-829 Beer-Lambert on back faces
    thr_abs = thr * absorption(M["albedo"], hit["t"], ~ff, mis)
    # :831-836 emission
    emissive = (em > 0.0).any(axis=1)
    em_added = emissive & (((bounce == 0) | prev_spec) if mis != "emission_always" else True)
    acc = acc + np.where(_col(em_added), thr_abs * em, 0.0)
    # :840-857 next-event estimation
    nee = ~spec if mis != "nee_primary" else (~spec | (bounce == 0))
    nee = nee & (world.n_lights > 0)
    cursor = np.zeros(n, np.int64)
    out = dict(light_sampled=nee, light_index=np.full(n, -1))
    contrib, w, pdf_brdf = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    nee_added = np.zeros(n, bool)
    nee_dec = np.ones(n, bool)
    if world.n_lights > 0:
        r, u1, u2 = uni[:, 0], uni[:, 1], uni[:, 2]
        if held:
            idx, idec = held["light_index"], np.ones(n, bool)
        else:
            idx, idec = pick_light(world.lights, r, mis)
        Lt = held["Lt"] if held and "Lt" in held else {k: v[idx] for k, v in world.lights.items()}
        s = light_sample(point, N, Lt, r, u1, u2, world.n_lights, mis, idec)
        if held:
            shadowed, sdec = held["shadowed"], np.ones(n, bool)
        else:
            shadowed, sdec = np.zeros(n, bool), np.ones(n, bool)
            if nee.any():
                k = np.flatnonzero(nee)
                occ = bf.occluded(world.geom, s["shadow_origin"][k], s["L"][k], s["shadow_tmax"][k])
                shadowed[k], sdec[k] = occ["occluded"], occ["decided"] & ~occ["quirk"]
        L_eval = held["L_eval"] if held and held.get("L_eval") is not None else s["L"]
        solid_unit = np.where(s["sphere"] & (s["solid_angle"] > F(1e-6)), TWO_PI * EPS32 / np.maximum(s["solid_angle"], 1e-300), 0.0)
        if nudge and nudge[0] == "L":
            L_eval = _nudged(L_eval, s["sin_unit"], nudge[1], nudge[2])
        if nudge and nudge[0] == "solid":
            s = dict(s, pdf_sample=s["pdf_sample"] * (1.0 + nudge[1] * solid_unit))
        contrib, vdec = light_value(s, V, N, ff, M, shadowed, L_eval, mis)
        pos = contrib.max(axis=1)
        with np.errstate(all="ignore"):
            pdf_brdf, pdec, cancel = T.material_pdf(M, N, V, L_eval, ff)
            if nudge and nudge[0] == "cancel":
                pdf_brdf = pdf_brdf + nudge[1] * cancel
            w = mis_weight(s["pdf_sample"], pdf_brdf, mis)
        nee_added = nee & (pos > 0.0) & (s["pdf_sample"] > 0.0)
        # "some channel > 0": positive beyond underflow, or zero through decided gates (and a soft spot factor away from 0)
        pos_dec = (pos > M_POS) | ((pos == 0.0) & (np.abs(s["gate"]) > M_CONE))
        nee_dec = s["decided"] & sdec & vdec & pos_dec & (pdec | ~nee_added)
        acc = acc + np.where(_col(nee_added), thr_abs * contrib * _col(w), 0.0)
        cursor = np.where(nee, s["draws"], 0)
        out.update(light_index=np.where(nee, idx, -1), L=s["L"], pdf_sample=s["pdf_sample"], light_dist=s["light_dist"],
                   shadowed=shadowed, shadow_decided=sdec, sample_decided=s["decided"], sample=s, Lt=Lt,
                   solid_unit=solid_unit,
                   pdf_cancel=cancel)
        dec &= nee_dec | ~nee
    acc_vertex = acc
    # :859-869 material_scatter
    su, su1, su2 = _take(uni, cursor, 0), _take(uni, cursor, 1), _take(uni, cursor, 2)
    sc = T.scatter_sample(M, N, V, ff, su, su1, su2)
    sdir = held["scatter_dir"] if held and held.get("scatter_dir") is not None else sc["direction"]
    if nudge and nudge[0] == "scatter":
        sdir = _nudged(sdir, sc["sin_unit"], nudge[1], nudge[2])
    att, _, vdec2 = T.scatter_value(M, N, V, ff, sdir, sc["is_refraction"])
    ok = sc["ok"]
    cursor = cursor + sc["draws"]
    dec &= sc["decided"] & (vdec2 | ~ok)
    # :871-880 Russian roulette
    start = RR_START + 1 if mis == "rr_from_3" else RR_START
    rr = ok & (bounce >= start)
    p = roulette_p(thr_abs)
    u_rr = _take(uni, cursor, 0)
    survived = ~rr | ~(u_rr > p)
    dec &= ~rr | (np.abs(u_rr - p) > M_RR)
    cursor = cursor + rr
    thr2 = np.where(_col(rr) & (mis != "no_div_p"), thr_abs / _col(p), thr_abs)
    # :882-892
    thr_after = clamp_vector_soft(thr2 * att, MAX_BOUNCE_WEIGHT)
    sn = _dot(sdir, N)
    alive = held["alive"] if held and held.get("alive") is not None else ok & survived
    dec &= ~alive | (np.abs(sn) > M_DOT)
    origin = np.where(_col(sn > 0.0), point + N * F(1e-4), point - N * F(1e-4))
    out.update(throughput_absorbed=thr_abs, emission_added=em_added, contribution=contrib, w=w, pdf_brdf=pdf_brdf,
               nee_added=nee_added, nee_decided=nee_dec, accumulated=acc_vertex, scatter=sc, scatter_ok=ok, scatter_dir=sdir,
               attenuation=att, scatter_specular=sc["specular"], roulette=rr, p=p, u=u_rr, survived=survived,
               throughput_after=np.where(_col(alive), thr_after, thr_abs), next_origin=origin, alive=alive, draws=cursor,
               decided=dec, M=M, em=em)
    return out


# ------------------------------------------------------------------------------------------------------------ tracePath
def uniforms(O, states, count):
    """(n, count) float64: the next `count` uniforms of every generator state"""
    out = np.zeros((len(states), count))
    for i, s in enumerate(states):
        out[i] = O.xorwow_draw(s, count, uniform=True)[0]
    return out


def states_after(O, states, draws):
    out = np.zeros_like(states)
    for i, (s, k) in enumerate(zip(states, draws)):
        out[i] = O.xorwow_draw(s, int(k))[1]
    return out


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _plane_hit(world, o, d, base):
    """The hit record of rays (o, d) with the triangles a base evaluation found (branches held): t from the triangle's plane."""
    n = len(o)
    t, nrm = np.full(n, F(1e30)), np.zeros((n, 3))
    for mi in np.unique(base["mesh"][base["hit"]]):
        k = np.flatnonzero(base["hit"] & (base["mesh"] == mi))
        tri = world.geom.meshes[mi].world_triangles()[base["face"][k]]
        g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        g /= np.sqrt(_dot(g, g))[:, None]
        t[k] = _dot(tri[:, 0] - o[k], g) / _dot(d[k], g)
        nrm[k] = np.where(_col(_dot(g, base["normal"][k]) > 0.0), g, -g)
    return dict(hit=base["hit"], t=t, point=o + _col(np.where(base["hit"], t, 0.0)) * d, normal=nrm, mesh=base["mesh"],
                front_face=base["front_face"], decided=base["decided"], invcos=base["invcos"], face=base["face"])


def trace_path(world, o, d, uni, max_depth=DEPTH, mis=None, base=None, nudge=None):   # rendering/path_logic.cuh:782-899
    """n paths from float32 rays (o, d) flagged specular as a camera's are (ptrt.h, ptrt_query_radiance), each with its own
    uniform stream uni (n, >= DRAWS_PER_VERTEX x max_depth).  -> dict(vertices: per bounce a dict of (n,) arrays -- `on` says
    which rays reached it --, radiance (max_depth, n, 3): what a path cut at depth k + 1 returns, draws (max_depth, n),
    decided (max_depth, n): every vertex up to there decided, depth, normal, object_id, first_decided, first_invcos)."""
    n = len(o)
    rnd = _f32 if base is None else (lambda a: np.array(a, np.float64))   # `base`: branches held, nothing rounded (conditioning)
    o, d = rnd(o), rnd(d)
    thr, acc = np.ones((n, 3)), np.zeros((n, 3))
    spec, prev_spec = np.ones(n, bool), np.ones(n, bool)
    on = np.ones(n, bool)
    cursor = np.zeros(n, np.int64)
    decided = np.ones(n, bool)
    verts, rad, drw, decs = [], [], [], []
    first = {}
    for bounce in range(max_depth):
        k = np.flatnonzero(on)
        rec = dict(on=on.copy(), index=k)
        if len(k):
            bv = base["vertices"][bounce] if base is not None else None
            h = hit_of(world, o[k], d[k]) if bv is None else _plane_hit(world, o[k], d[k], bv["hit"])
            if bounce == 0:
                first = dict(depth=h["t"], normal=np.where(_col(h["hit"]), h["normal"], 0.0), object_id=h["mesh"], first_decided=h["decided"],
                             first_invcos=h["invcos"])
            decided[k] &= h["decided"]
            miss = ~h["hit"]
            sky, sky_dec = sample_sky(d[k], world.sky)
            acc[k[miss]] += thr[k[miss]] * sky[miss]
            decided[k[miss]] &= sky_dec[miss]
            on[k[miss]] = False
            kh = k[~miss]
            hh = {q: v[~miss] for q, v in h.items()}
            rec.update(hit=h, hit_index=kh)
            if len(kh):
                rows = np.arange(len(kh))[:, None]
                u7 = uni[kh[:, None], np.minimum(cursor[kh][:, None] + np.arange(DRAWS_PER_VERTEX)[None, :], uni.shape[1] - 1)]
                held = None
                if bv is not None:
                    b = bv["v"]
                    held = dict(light_index=np.maximum(b["light_index"], 0), shadowed=b.get("shadowed"), alive=b["alive"],
                                nudge=nudge[1:] if nudge and nudge[0] == bounce else None)
                v = vertex(world, bounce, d[kh], spec[kh], hh, thr[kh], acc[kh], prev_spec[kh], u7, mis, held)
                rec["v"] = v
                acc[kh] = v["accumulated"]
                thr[kh] = v["throughput_after"]
                cursor[kh] += v["draws"]
                decided[kh] &= v["decided"]
                prev_spec[kh] = np.where(v["scatter_ok"], v["scatter_specular"], prev_spec[kh])
                spec[kh] = v["scatter_specular"]
                o[kh] = rnd(v["next_origin"])
                d[kh] = rnd(v["scatter_dir"])
                on[kh] = v["alive"]
        verts.append(rec)
        rad.append(clamp_vector_soft(acc, MAX_FINAL))
        drw.append(cursor.copy())
        decs.append(decided.copy())
    return dict(vertices=verts, radiance=np.array(rad), draws=np.array(drw), decided=np.array(decs), **first)


def query_radiance(world, o, d, uni, samples=1, max_depth=DEPTH, mis=None):
    """The sample loop of ptrt_query_radiance (include/ptrt.h): `samples` paths per ray from one stream, each soft-clamped by
    tracePath, summed in order, divided by `samples`; first hit of sample 0.  -> dict(radiance, depth, normal, object_id,
    draws, decided, first_decided, first_invcos)"""
    n = len(o)
    total, draws, dec = np.zeros((n, 3)), np.zeros(n, np.int64), np.ones(n, bool)
    first = None
    for s in range(samples):
        rows = np.arange(n)[:, None]
        u = uni[rows, np.minimum(draws[:, None] + np.arange(DRAWS_PER_VERTEX * max_depth)[None, :], uni.shape[1] - 1)]
        p = trace_path(world, o, d, u, max_depth, mis)
        total = total + p["radiance"][-1]
        draws = draws + p["draws"][-1]
        dec &= p["decided"][-1]
        first = first or p
    return dict(radiance=total / float(samples), depth=first["depth"], normal=first["normal"], object_id=first["object_id"],
                draws=draws, decided=dec, first_decided=first["first_decided"], first_invcos=first["first_invcos"])


# ------------------------------------------------------------------------------------------------------------ the scene
def light_lab(P, scene):
    """A diffuse floor and eight objects floating above it, none coplanar with another; about 230 triangles within radius 10.
    Returns {name: mesh index}."""
    Mt = P.Material
    ids = {}
    ids["floor"] = scene.addPlaneXZ(-1.0, 8.0, Mt((0.7, 0.7, 0.65), 0.9, 0.0))

    def cube(name, mat, size, pos, rot=None):
        m = scene.addCube(mat)
        scene.scale(m, size)
        if rot is not None:
            scene.rotateSelfEulerXYZ(m, rot)
        scene.moveTo(m, pos)
        ids[name] = m

    cube("diffuse", Mt((0.8, 0.3, 0.2), 0.8, 0.0), (1.2, 1.2, 1.2), (-3.0, -0.3, -1.0), (0.0, 0.4, 0.0))
    cube("rough_metal", Mt((0.9, 0.7, 0.3), 0.3, 1.0), (1.0, 1.6, 1.0), (-0.8, -0.12, -3.2), (0.0, -0.3, 0.0))
    cube("mirror", Mt((0.9, 0.9, 0.95), 0.05, 1.0), (1.8, 1.8, 0.2), (3.0, 0.0, -2.4))           # its front face is z = -2.3
    cube("glass", Mt((0.6, 0.9, 0.7), 0.1, 0.0, transmission=1.0, ior=1.5), (2.0, 2.0, 2.0), (0.6, 0.07, 1.6), (0.0, 0.2, 0.0))
    cube("coated", Mt((0.2, 0.3, 0.8), 0.5, 0.0, clearcoat=1.0, clearcoatRoughness=0.1), (1.0, 1.0, 1.0), (-3.2, -0.4, 2.6), (0.1, 0.7, 0.0))
    cube("emissive", Mt((0.9, 0.9, 0.9), 0.8, 0.0, emission=(4.0, 3.0, 2.0)), (0.8, 0.8, 0.8), (3.4, 0.9, 0.6), (0.2, 0.3, 0.1))
    m = scene.addCube(Mt((0.3, 0.8, 0.4), 0.6, 0.0))             # a proper instance: rotated, scaled, no x translation
    scene.setPosition(m, (0.0, 0.3, -5.5))
    scene.setRotation(m, (0.3, 0.5, 0.1))
    scene.setInstanceScale(m, (1.4, 0.8, 1.1))
    ids["instance"] = m
    m = scene.addSphere(8, Mt((0.8, 0.8, 0.2), 0.4, 0.0))
    scene.scale(m, (1.6, 1.6, 1.6))
    scene.moveTo(m, (-0.6, 0.05, 4.6))
    ids["sphere"] = m
    return ids


GLASS_CENTRE, GLASS_HALF = np.array([0.6, 0.07, 1.6]), 0.8      # a box well inside the rotated glass cube
EMISSIVE_CENTRE, MIRROR_FRONT_Z = np.array([3.4, 0.9, 0.6]), -2.3
WHITE = (1.0, 0.95, 0.9)


def _pt(pos, **kw):
    return dict(type=LIGHT_POINT, position=pos, color=kw.pop("color", WHITE), **kw)


def _spot(pos, direction, **kw):
    return dict(type=LIGHT_SPOT, position=pos, direction=direction, color=kw.pop("color", WHITE), **kw)


LIGHT_SETS = {
    "A": [],
    "B": [dict(type=LIGHT_DIRECTIONAL, direction=(-0.3, -1.0, -0.2), color=WHITE, intensity=2.0)],
    "C": [_pt((0.5, 4.0, 0.0), intensity=40.0, range=20.0)],
    "D": [_pt((-1.0, 3.0, 0.5), intensity=30.0, range=50.0, radius=0.5)],
    "E": [_pt((-1.5, -0.2, 0.4), intensity=6.0, range=50.0, radius=1.5)],
    "F": [_spot((0.0, 5.0, 0.0), (0.1, -1.0, 0.05), intensity=60.0, inner=0.9, outer=0.7, range=60.0),
          _spot((-2.0, 4.0, 2.0), (0.0, -1.0, -0.2), intensity=60.0, inner=0.85, outer=0.85, range=60.0, color=(0.6, 0.8, 1.0)),
          _spot((2.0, 3.5, -1.0), (-0.2, -1.0, 0.1), intensity=50.0, inner=0.9, outer=0.75, range=60.0, radius=0.4, color=(1.0, 0.7, 0.5))],
    "G": [_pt((0.5, 4.0, 0.0), intensity=30.0, range=100.0),
          _pt((-3.0, 1.2, 1.0), intensity=8.0, range=2.0, color=(1.0, 0.4, 0.3)),
          dict(type=LIGHT_DIRECTIONAL, direction=(0.4, -1.0, 0.3), color=(0.5, 0.6, 0.9), intensity=1.0),
          _pt((2.0, 2.5, 3.0), intensity=25.0, range=100.0, radius=0.3),
          _spot((0.0, 5.0, -3.0), (0.0, -1.0, 0.1), intensity=60.0, inner=0.9, outer=0.7, range=100.0),
          _spot((-4.0, 3.0, -3.0), (0.5, -1.0, 0.2), intensity=40.0, inner=0.8, outer=0.8, range=2.0, radius=0.2),
          _pt((4.0, 1.0, 4.0), intensity=10.0, range=2.0, radius=0.6, color=(0.4, 1.0, 0.5))],
    "H": [_pt((0.0, 4.0, 0.0), intensity=4000.0, range=100.0, radius=0.003)],
}
UNDECIDED_BY_CONSTRUCTION = ("H",)
N_RAYS = 512


def _unit_rows(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ray_set(name, n=N_RAYS):
    """float32 (origins, unit directions) of a named set"""
    rs = np.random.RandomState(dict(free=1, glass=2, emissive=3, sky=4)[name])
    if name == "free":
        o = np.stack([rs.uniform(-6, 6, n), rs.uniform(1.5, 5.0, n), rs.uniform(-6, 6, n)], axis=1)
        target = np.stack([rs.uniform(-5, 5, n), rs.uniform(-1.0, 1.0, n), rs.uniform(-5, 5, n)], axis=1)
        d = target - o
    elif name == "glass":
        o = GLASS_CENTRE + rs.uniform(-GLASS_HALF, GLASS_HALF, (n, 3))
        d = rs.normal(size=(n, 3))
    elif name == "emissive":
        # half aimed at the emissive cube, half at the mirror so that its reflection meets the emissive cube
        o = np.stack([rs.uniform(0.0, 2.0, n), rs.uniform(0.5, 3.0, n), rs.uniform(-0.5, 3.0, n)], axis=1)
        d = EMISSIVE_CENTRE + rs.uniform(-0.3, 0.3, (n, 3)) - o
        half = n // 2
        p = np.stack([rs.uniform(2.3, 3.7, half), rs.uniform(-0.3, 0.7, half), np.full(half, MIRROR_FRONT_Z)], axis=1)
        r = _unit_rows(EMISSIVE_CENTRE + rs.uniform(-0.2, 0.2, (half, 3)) - p)
        d[half:half * 2] = r * np.array([1.0, 1.0, -1.0])
        o[half:half * 2] = p - d[half:half * 2] * rs.uniform(0.5, 1.0, (half, 1))
    else:
        o = np.stack([rs.uniform(-6, 6, n), rs.uniform(3.0, 6.0, n), rs.uniform(-6, 6, n)], axis=1)
        d = rs.normal(size=(n, 3))
        d[:, 1] = np.abs(d[:, 1]) + 0.05
    d32 = _unit_rows(d).astype(np.float32)
    d32 = (d32 / np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(o.astype(np.float32)), np.ascontiguousarray(d32)


RAY_SETS = ("free", "glass", "emissive", "sky")


def env_map():
    rs = np.random.RandomState(7)
    rgba = rs.uniform(0.0, 2.0, (8, 16, 4)).astype(np.float32)
    rgba[:, :, 3] = 1.0
    return rgba


SKIES = {"off": lambda: Sky(), "gradient": lambda: Sky(True, (0.2, 0.4, 0.9), (1.0, 0.9, 0.8)),
         "env": lambda: Sky(True, (0.2, 0.4, 0.9), (1.0, 0.9, 0.8), env_map())}


def cases():
    """(light set, ray set, sky) of every case: every light set with every ray set, sky off for the sets that hit things and
    gradient for half of them; the sky set with every sky on sets A and G."""
    out = []
    for k, ls in enumerate(LIGHT_SETS):
        for rset in RAY_SETS[:3]:
            out.append((ls, rset, "off" if k % 2 else "gradient"))
        out.append((ls, "sky", "gradient"))
    out += [("A", "sky", "off"), ("A", "sky", "env"), ("G", "sky", "env"), ("G", "free", "env")]
    return out


def ray_states(O, rset, n=N_RAYS):
    return O.xorwow_init(SEED, RAY_SETS.index(rset) * 4096, n)


# ------------------------------------------------------------------------------------------------------------ judging
def _mag(a):
    return np.sqrt((a * a).sum(axis=1)) if a.ndim == 2 else np.abs(a)


def _perturb(X, fn, keys, outputs):
    """|q| + sum_i |x_i dq/dx_i| of every output of fn(X) over every column of X[k], k in keys, by central differences with a
    relative step of one float32 ulp.  Vector outputs count by their norm."""
    q0 = fn(X)
    cond = {q: _mag(q0[q]) for q in outputs}
    for k in keys:
        a = X[k]
        for c in (range(a.shape[1]) if a.ndim == 2 else [None]):
            col = a[:, c] if c is not None else a
            if not np.any(col):
                continue
            res = []
            for sgn in (1.0, -1.0):
                w = a.copy()
                if c is None:
                    w *= 1.0 + sgn * T.FD_STEP
                else:
                    w[:, c] *= 1.0 + sgn * T.FD_STEP
                Y = dict(X)
                Y[k] = w
                res.append(fn(Y))
            with np.errstate(all="ignore"):
                for q in outputs:
                    cond[q] = cond[q] + np.nan_to_num(_mag(res[0][q] - res[1][q])) / (2.0 * T.FD_STEP)
    return cond


VERTEX_QUANTITIES = ("L", "pdf_sample", "light_dist", "contribution", "w", "throughput_absorbed", "p", "throughput_after",
                     "next_origin", "accumulated")
VERTEX_FLAGS = ("light_sampled", "light_index", "shadowed", "emission_added", "nee_added", "scatter_ok", "scatter_specular",
                "roulette", "survived", "draws")


def log_vertices(lg):
    """The logged vertices that hit something, flat, with what the vertex before left them: bounce, accumulated before,
    prev_was_specular, and what the next vertex's ray says about this one's scatter."""
    n, samples, depth = lg.shape
    vis = (lg["visited"] != 0) & (lg["hit"] != 0)
    ray, smp, bnc = np.nonzero(vis)
    v = lg[ray, smp, bnc]
    prev = lg[ray, smp, np.maximum(bnc - 1, 0)]
    first = bnc == 0
    acc0 = np.where(_col(first), 0.0, prev["accumulated"].astype(np.float64))
    prev_spec = np.where(first, True, prev["scatter_specular"] != 0)
    has_next = (bnc + 1 < depth)
    nxt = lg[ray, smp, np.minimum(bnc + 1, depth - 1)]
    has_next &= nxt["visited"] != 0
    return dict(v=v, ray=ray, sample=smp, bounce=bnc, acc_before=acc0, prev_spec=prev_spec, has_next=has_next, next=nxt)


def judge_log(world, O, lg, mis=None, tol=None, terms=True, floor=1.0):
    """Every logged vertex of oracle.trace_paths through `vertex` at the oracle's own inputs.  -> dict(units: {quantity: (m,)
    units, 0 where not judged}, bad: {flag: (m,) bool}, decided (m,), info)."""
    I = log_vertices(lg)
    v = I["v"]
    m = len(v)
    f64 = lambda name: v[name].astype(np.float64)
    uni = uniforms(O, v["state_before"], DRAWS_PER_VERTEX)
    S = dict(bounce=I["bounce"], spec=v["ray_specular"] != 0, mesh=v["mesh_index"].astype(np.int64), ff=v["front_face"] != 0,
             prev_spec=I["prev_spec"])
    hit = dict(t=f64("t"), point=f64("point"), normal=f64("normal"), mesh=S["mesh"], front_face=S["ff"])
    # 1. the statement's own sample at the oracle's inputs
    v0 = vertex(world, S["bounce"], f64("ray_dir"), S["spec"], hit, f64("throughput_before"), I["acc_before"], S["prev_spec"], uni, mis)
    sampled_both = v0["light_sampled"] & (v["light_sampled"] != 0)
    L_test = np.where(_col(sampled_both), f64("L"), v0.get("L", np.zeros((m, 3))))
    ok_both = v0["scatter_ok"] & (v["scatter_ok"] != 0)
    sdir_test = np.where(_col(ok_both), f64("scatter_dir"), v0["scatter_dir"])
    X = dict(d=f64("ray_dir"), t=hit["t"], point=hit["point"], normal=hit["normal"], thr=f64("throughput_before"),
             acc=I["acc_before"], uni=uni, em=v0["em"], L_eval=L_test, scatter_dir=sdir_test)
    for k, a in v0["M"].items():
        X["M." + k] = a
    if world.n_lights:
        for k in LIGHT_FIELDS:
            X["Lt." + k] = v0["Lt"][k]

    def fn(Y, sel=slice(None)):
        held = dict(M={k[2:]: a for k, a in Y.items() if k.startswith("M.")}, em=Y["em"], L_eval=Y["L_eval"], scatter_dir=Y["scatter_dir"])
        if world.n_lights:
            held.update(light_index=np.maximum(v0["light_index"][sel], 0), shadowed=v0["shadowed"][sel],
                        Lt=dict({k[3:]: a for k, a in Y.items() if k.startswith("Lt.")}, type=v0["Lt"]["type"][sel]))
        h = dict(t=Y["t"], point=Y["point"], normal=Y["normal"], mesh=S["mesh"][sel], front_face=S["ff"][sel])
        r = vertex(world, S["bounce"][sel], Y["d"], S["spec"][sel], h, Y["thr"], Y["acc"], S["prev_spec"][sel], Y["uni"], mis, held)
        for q in ("L", "pdf_sample", "light_dist"):
            r.setdefault(q, np.zeros((len(Y["t"]), 3) if q == "L" else len(Y["t"])))
        return r

    # 2. the values at the L and the scattered direction under test
    v1 = fn(X)
    decided = v0["decided"] & v1["decided"]
    got = dict(L=f64("L"), pdf_sample=f64("pdf_sample"), light_dist=f64("light_dist"), contribution=f64("contribution"), w=f64("w"),
               throughput_absorbed=f64("throughput_absorbed"), p=f64("p"), throughput_after=f64("throughput_after"),
               accumulated=f64("accumulated"), next_origin=I["next"]["ray_origin"].astype(np.float64))
    alive_both = v1["alive"] & I["has_next"]
    judged = dict(L=sampled_both, pdf_sample=sampled_both, light_dist=sampled_both, contribution=sampled_both,
                  w=sampled_both & v1["nee_added"] & (v["w"] != 0), throughput_absorbed=np.ones(m, bool), p=v1["roulette"] & (v["roulette"] != 0),
                  throughput_after=v1["alive"] & ok_both & (v["survived"] != 0) | (~v1["roulette"] & ok_both & (v["roulette"] == 0)),
                  accumulated=np.ones(m, bool), next_origin=alive_both)
    want = {q: v1[q] for q in VERTEX_QUANTITIES}
    if "L" in v0:
        want["L"], want["pdf_sample"], want["light_dist"] = v0["L"], v0["pdf_sample"], v0["light_dist"]
    # named terms (see TOLERANCES)
    zero = np.zeros(m)
    su = v0.get("solid_unit", zero) if terms else zero
    extra = {q: zero for q in VERTEX_QUANTITIES}
    if terms and "sample" in v0:
        extra["L"] = v0["sample"]["sin_unit"]
        extra["pdf_sample"] = su * np.abs(want["pdf_sample"])
        extra["contribution"] = su * _mag(want["contribution"])
        with np.errstate(all="ignore"):
            wterm = 2.0 * want["w"] * (1.0 - want["w"]) * (su + np.nan_to_num(v0["pdf_cancel"] / np.maximum(v1["pdf_brdf"], 1e-300)))
        extra["w"] = np.where(v1["nee_added"], wterm, 0.0)
        extra["accumulated"] = np.where(v1["nee_added"], _mag(v1["throughput_absorbed"] * want["contribution"]) * (su * want["w"] + extra["w"]), 0.0)
    dev = {q: np.where(judged[q] & decided, np.nan_to_num(_mag(got[q] - want[q]), nan=np.inf), 0.0) for q in VERTEX_QUANTITIES}
    with np.errstate(all="ignore"):
        units = {q: np.where(dev[q] == 0.0, 0.0, dev[q] / (EPS32 * _mag(want[q]) + extra[q])) for q in VERTEX_QUANTITIES}
    lim = floor if tol is None else None
    need = np.zeros(m, bool)
    for q in VERTEX_QUANTITIES:
        need |= np.nan_to_num(units[q], nan=np.inf) > (lim if lim is not None else tol[q])
    need &= decided
    if need.any():
        k = np.flatnonzero(need)
        Xk = {q: a[k] for q, a in X.items()}
        cond = _perturb(Xk, lambda Y: fn(Y, k), list(X), VERTEX_QUANTITIES)
        with np.errstate(all="ignore"):
            for q in VERTEX_QUANTITIES:
                units[q][k] = np.where(dev[q][k] == 0.0, 0.0, dev[q][k] / (EPS32 * cond[q] + extra[q][k]))
    units = {q: np.where(np.isnan(u), np.inf, u) for q, u in units.items()}
    # flags
    after = states_after(O, v["state_before"], v1["draws"])
    want_flag = dict(light_sampled=v0["light_sampled"], light_index=v0["light_index"], shadowed=v0.get("shadowed", np.zeros(m, bool)) & v0["light_sampled"],
                     emission_added=v1["emission_added"], nee_added=v1["nee_added"], scatter_ok=v1["scatter_ok"],
                     scatter_specular=v1["scatter_specular"] & v1["scatter_ok"], roulette=v1["roulette"], survived=v1["survived"] & v1["roulette"])
    got_flag = dict(light_sampled=v["light_sampled"] != 0, light_index=v["light_index"], shadowed=v["shadowed"] != 0,
                    emission_added=v["emission_added"] != 0, nee_added=v["w"] != 0, scatter_ok=v["scatter_ok"] != 0,
                    scatter_specular=v["scatter_specular"] != 0, roulette=v["roulette"] != 0, survived=v["survived"] != 0)
    bad = {q: decided & (np.asarray(got_flag[q]) != np.asarray(want_flag[q])) for q in want_flag}
    bad["draws"] = decided & (after != v["state_after"]).any(axis=1)
    bad["next_specular"] = decided & alive_both & ((I["next"]["ray_specular"] != 0) != v1["scatter_specular"])
    return dict(units=units, bad=bad, decided=decided, info=I, v0=v0, v1=v1)


def path_inputs(world, o, d, uni):
    X = dict(o=np.asarray(o, np.float64), d=np.asarray(d, np.float64), uni=uni)
    return X


def judge_paths(world, O, o, d, states, records, states_after_got, path, depth, tol=None, floor=1.0, terms=True):
    """Records (and the states left) of the code under test for the rays (o, d, states) at `depth` and one sample, against the
    statement's own path `path` (trace_path at DEPTH >= depth from the same rays and uniforms).  -> dict(radiance: units per ray
    (0 where undecided), first_bad, draws_bad: bool per ray, t, normal: errors by brute_force's measures, decided)."""
    n = len(o)
    k = depth - 1
    decided = path["decided"][k]
    want = path["radiance"][k]
    got = records["radiance"].astype(np.float64)
    dev = np.where(decided, np.nan_to_num(_mag(got - want), nan=np.inf), 0.0)
    with np.errstate(all="ignore"):
        units = np.where(dev == 0.0, 0.0, dev / (EPS32 * _mag(want)))
    need = decided & (np.nan_to_num(units, nan=np.inf) > (floor if tol is None else tol))
    if need.any():
        cond, term = path_conditioning(world, o, d, path, depth, np.flatnonzero(need), terms)
        units[need] = dev[need] / (EPS32 * cond + term)
    after = states_after(O, states, path["draws"][k])
    draws_bad = decided & (after != states_after_got).any(axis=1)
    fd = path["first_decided"]
    hit = path["object_id"] >= 0
    first_bad = fd & (records["object_id"] != path["object_id"])
    both = fd & hit & ~first_bad
    t_err = np.zeros(n)
    n_err = np.zeros(n)
    if both.any():
        t = path["depth"][both]
        t_err[both] = np.abs(records["depth"][both].astype(np.float64) - t) / (np.maximum(t, world.geom.radius) * path["first_invcos"][both])
        a, b = records["normal"][both].astype(np.float64), path["normal"][both]
        cr = np.cross(a, b)
        n_err[both] = np.arctan2(np.sqrt((cr * cr).sum(axis=1)), (a * b).sum(axis=1))
    miss = fd & ~hit
    first_bad |= miss & ((records["depth"] != np.float32(1e30)) | records["normal"].any(axis=1))
    return dict(radiance=np.where(np.isnan(units), np.inf, units), draws_bad=draws_bad, first_bad=first_bad, t=t_err, normal=n_err,
                decided=decided)


def path_conditioning(world, o, d, path, depth, sel, terms=True):
    """|R| + sum_i |x_i dR/dx_i| of the radiance of paths `sel` cut at `depth`: x_i over the ray (a float32 ulp up and down),
    the uniforms, and FIELD-WISE over the lights' and the materials' fields (one field of every light or every mesh scaled
    together: sum over objects of signed terms, a lower bound of the sum of their magnitudes, so the unit is not flattered).
    Branches held: the triangles hit, the light indices and the shadow rays' answers are those of `path`."""
    base = dict(vertices=[])
    for rec in path["vertices"][:depth]:
        # rows of rec are the rays that reached the bounce; keep those of sel
        keep = np.isin(rec["index"], sel)
        b = dict(index=None)
        if "hit" in rec:
            b["hit"] = {q: a[keep] for q, a in rec["hit"].items()}
            hk = np.isin(rec["hit_index"], sel)
            if "v" in rec:
                b["v"] = dict(light_index=rec["v"]["light_index"][hk], alive=rec["v"]["alive"][hk])
                if "shadowed" in rec["v"]:
                    b["v"]["shadowed"] = rec["v"]["shadowed"][hk]
        base["vertices"].append(b)
    o32, d32 = np.asarray(o, np.float32)[sel], np.asarray(d, np.float32)[sel]
    uni = path["uni"][sel]
    k = depth - 1

    def run(oo, dd, uu, w=world, nudge=None):
        return trace_path(w, oo, dd, uu, depth, base=base, nudge=nudge)["radiance"][k]

    q0 = run(o32.astype(np.float64), d32.astype(np.float64), uni)
    cond = _mag(q0)

    def add(hi, lo):
        nonlocal cond
        cond = cond + np.nan_to_num(_mag(hi - lo)) / (2.0 * T.FD_STEP)

    for which in (0, 1):
        for c in range(3):
            args = []
            for toward in (np.inf, -np.inf):
                a = [o32.copy(), d32.copy()]
                a[which][:, c] = np.nextafter(a[which][:, c], np.float32(toward))
                args.append(run(a[0].astype(np.float64), a[1].astype(np.float64), uni))
            add(*args)
    for c in range(uni.shape[1]):
        res = []
        for sgn in (1.0, -1.0):
            u = uni.copy()
            u[:, c] *= 1.0 + sgn * T.FD_STEP
            res.append(run(o32.astype(np.float64), d32.astype(np.float64), u))
        add(*res)
    import copy
    groups = [("lights", f) for f in LIGHT_FIELDS] if world.n_lights else []
    groups += [("lib", f) for f in world.lib] + [("emission", None)]
    for where, f in groups:
        arr = world.emission if where == "emission" else getattr(world, where)[f]
        for c in (range(arr.shape[1]) if arr.ndim == 2 else [None]):
            col = arr[:, c] if c is not None else arr
            if not np.any(col):
                continue
            res = []
            for sgn in (1.0, -1.0):
                w2 = copy.copy(world)
                a2 = arr.copy()
                if c is None:
                    a2 *= 1.0 + sgn * T.FD_STEP
                else:
                    a2[:, c] *= 1.0 + sgn * T.FD_STEP
                if where == "emission":
                    w2.emission = a2
                else:
                    setattr(w2, where, dict(getattr(world, where), **{f: a2}))
                res.append(run(o32.astype(np.float64), d32.astype(np.float64), uni, w2))
            add(*res)
    # the named terms (see TOLERANCES), at every vertex of the path: what they may do to a sampled direction, to the solid angle
    # and to material_pdf's weights, carried to the end of the path
    term = np.zeros(len(sel))
    if terms:
        o64, d64 = o32.astype(np.float64), d32.astype(np.float64)
        for b in range(depth):
            kinds = [("scatter", 0), ("scatter", 1)] + ([("L", 0), ("L", 1), ("solid", 0), ("cancel", 0)] if world.n_lights else [])
            for kind, axis in kinds:
                hi, lo = run(o64, d64, uni, nudge=(b, kind, 1.0, axis)), run(o64, d64, uni, nudge=(b, kind, -1.0, axis))
                term = term + 0.5 * np.nan_to_num(_mag(hi - lo))
    return cond, term


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """One (light set, ray set, sky): the world, the rays, the states, the uniforms, and the statement's own paths at DEPTH."""

    def __init__(self, P, O, world, ls, rset, sky, n=N_RAYS):
        self.name = f"{ls}-{rset}-{sky}"
        self.ls, self.rset, self.skyname = ls, rset, sky
        world.set_lights(P, LIGHT_SETS[ls])
        world.sky = SKIES[sky]()
        import copy
        self.world = copy.copy(world)
        self.o, self.d = ray_set(rset, n)
        self.states = ray_states(O, rset, n)
        self.uni = uniforms(O, self.states, DRAWS_PER_VERTEX * DEPTH * 3)
        self.path = trace_path(self.world, self.o, self.d, self.uni[:, :DRAWS_PER_VERTEX * DEPTH])
        self.path["uni"] = self.uni[:, :DRAWS_PER_VERTEX * DEPTH]

    def undecided(self):
        """(share of undecided vertices, share of undecided paths at DEPTH) from the statement alone"""
        nv = sum(len(r["index"]) for r in self.path["vertices"])
        und = 0
        for r in self.path["vertices"]:
            if "hit" not in r:
                continue
            bad = ~r["hit"]["decided"]
            if "v" in r:
                hitrow = r["hit"]["hit"]
                b2 = np.zeros(len(bad), bool)
                b2[hitrow] = ~r["v"]["decided"]
                bad = bad | b2
            und += int(bad.sum())
        return und / max(nv, 1), 1.0 - self.path["decided"][-1].mean()

    def oracle(self, P, O, depth=DEPTH, samples=1, log=False):
        st = self.states.copy()
        r = O.trace_paths(self.world.oracle_desc(P), self.o, self.d, st, samples, depth, log=log)
        return (r[0], r[1], st) if log else (r, st)


def open_lab(P):
    s = P.Scene(64, 64, device=P.HOST_ONLY)
    light_lab(P, s)
    return s, World(P, s)


def measure(P, O, which=None, verbose=False, terms=True):
    """Oracle against the statement over every case (or those named): -> {quantity: (case, largest deviation in units)}"""
    scene, world = open_lab(P)
    worst = {}
    for ls, rset, sky in cases():
        c = Case(P, O, world, ls, rset, sky)
        if which is not None and c.name not in which:
            continue
        rec, lg, st = c.oracle(P, O, log=True)
        j = judge_log(c.world, O, lg, terms=terms)
        row = {q: float(u.max()) if len(u) else 0.0 for q, u in j["units"].items()}
        for depth in (1, 2, 3, 5):
            r, st = c.oracle(P, O, depth)
            e = judge_paths(c.world, O, c.o, c.d, c.states, r, st, c.path, depth, terms=terms)
            row["radiance"] = max(row.get("radiance", 0.0), float(e["radiance"].max()))
            row["first_t"] = max(row.get("first_t", 0.0), float(e["t"].max()))
            row["first_normal"] = max(row.get("first_normal", 0.0), float(e["normal"].max()))
        flags = {q: int(b.sum()) for q, b in j["bad"].items() if b.any()}
        if verbose:
            print(f"{c.name:22s} " + " ".join(f"{q} {v:.3g}" for q, v in row.items()) + f"  bad flags {flags}  decided {j['decided'].mean() if len(j['decided']) else 1:.3f}", flush=True)
        for q, v in row.items():
            if ls in UNDECIDED_BY_CONSTRUCTION and q not in ("radiance", "first_t", "first_normal"):
                pass
            if v > worst.get(q, ("", -1.0))[1]:
                worst[q] = (c.name, v)
    scene.close()
    return worst


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "ptrt-game-engine_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests", "golden")]
    import oracle
    import ptrt_amd
    w = measure(ptrt_amd, oracle, verbose=True, terms="--without-terms" not in sys.argv)
    for q, (name, v) in w.items():
        print(f"    {q}=({name!r}, {v:.4g}),")
