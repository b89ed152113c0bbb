"""evaluateBSDF, material_pdf and material_scatter of the reference, stated once more in float64 numpy.

TEST INFRASTRUCTURE.  oracle/ptrt_oracle.cpp and csrc/pt_device.hip.h were written by ONE reading of the reference's
path_logic.cuh, pbr_utils.cuh, pdf.cuh and sampling.cuh and are held to each other at tolerance 0, so a shared misreading passes
every parity test.  This module is a second reading, made from the reference's text alone (file:line beside each function; the
paths are relative to the reference's src/pathtracer unless they start with common/), vectorised over items, in float64.  It
shares nothing with the oracle but two things that are pinned elsewhere: the material arrays of a flattened scene
(`load_materials`) and the uniforms of a generator state (`oracle_xorwow_draw`; XORWOW is held to rocRAND's known answers).
Literals are the float32 values the text spells (`1e-6f` is float32(1e-6)); everything else is float64.

material_scatter is stated as the reference computes it, in two halves: `scatter_sample` maps the three uniforms it draws to
(direction, ok, specular, lobe, is_refraction), and `scatter_value` maps a direction to (attenuation, out_pdf): everything the
reference computes after its sampling branch depends on the sampled direction only.  `material_scatter` is their composition.
The comparison uses the halves apart (see TOLERANCES): the direction against `scatter_sample`, the attenuation against
`scatter_value` AT THE DIRECTION UNDER TEST, so that a sampling error is not multiplied by the slope of a sharp lobe.

DECIDED.  float32 and float64 may legitimately take different branches next to a threshold.  Each answer carries `decided`,
computed here alone: every discontinuous decision on the item's path is away from its threshold by a margin:
    M_DOT  = 1e-6   sign of N.V, N.L, N.H (the flip of the refraction half vector), V.H of the sampled half vector
    M_K    = 1e-5 x max(1, eta^2)   k = 1 - eta^2 (1 - VdotH^2) against 0 (total internal reflection); none when eta = 1, where
                    1 - (1 - c^2) cannot round below 0 in any precision
    M_PROB = 1e-6   u against P_coat, P_coat + P_trans_reflect, P_coat + P_opaque_spec; sinThetaFilm^2 against 1
    M_DIFF = 5e-7   P_opaque_diff against 1e-6
    M_LEN  = 1e-5   |V x eta + L| against 0 before the refraction half vector is normalised (at ior 1 the refracted direction is
                    -V and the half vector is the normalised rounding error of the sum)
    M_P0   = 1e-20  P_trans_reflect > 0 and P_trans_refract > 0 where the reference gates a term by them
    0               trans > 0, metal < 0.1, metal > 0, clearcoat > 0, iridescence > 0, sheen > 0, roughness < 0.1 (the specular
                    flag), copysign(1, N.z): comparisons of a float32 INPUT (or its fmaxf / clamp01 with a literal) with a float32
                    literal, which both precisions evaluate on the same bits
Continuous clamps need none.  At most 2 % of any (material, item set) may be undecided (asserted in tests/test_shading_truth.py
from this module alone).  Two item sets are outside that bound and say so: `eval_nv0` (NdotV = 0 with a random normal: N.V is
rounding noise, the reference's early return is a coin toss -- asserted to be 100 % undecided, as section 5.1 asserts coplanar
faces to be) and `scatter_outside` (material_scatter with V in or below the surface, which tracePath never calls: the normal it
passes is turned against the ray; judged where decided, no bound).

ITEMS.  `add_library(P, scene)` adds the 21 materials of make_function_kats (ids kept) followed by SYNTHETIC.  `eval_items` / `scatter_items`
build the inputs of probe op 0 / op 1 in the probe's own layout (see pt_device.hip.h, shade_probe_kernel).  Scatter draws use
4,096 consecutive generator states per view (the GPU test holds the device to the statement on the first 256 of each and to
the oracle's bits on all); lobe boundaries and the `fminf(u2, 0.9999999f)` clamp are met by chance at this count (u2 = 1 has
probability 2^-24 per draw), not by construction.

TOLERANCES.  A deviation is counted in units of the statement's own conditioning,
    unit(q) = EPS32 x (|q| + sum_i |x_i dq/dx_i|),   EPS32 = 2^-23,
x_i running over the item's float32 inputs (N, V, L or the direction or the three uniforms, and every material field), by
central differences of this module with a relative step of 2^-23 (one float32 ulp: a finite step, so that (1 - cos)^5 next to cos = 1 is measured by what
an ulp does to it and not by a derivative that vanishes there).  Two cancelling expressions of the reference lose more than
any rounding of an input explains; each is NAMED here and adds a term of its own to the unit instead of widening the table
(`terms=False` in judge_eval / judge_scatter leaves them out, which is how the figures below are re-measured by the tests):
  * importance_sample_ggx, sampling.cuh:199-200: `1.0f + (a2 - 1.0f) * u2` adds a2 (1.6e-7 at roughness 0.02, 1e-12 at
    clearcoatRoughness 0.001) to -1 and so keeps it to 2^-24 absolute, twice; `1.0f - cosTheta * cosTheta` of a float32 cosTheta
    within an ulp of 1 is known to 2^-23 absolute (at a2 = 1e-12 sinTheta ~ 1e-6, float32 gives 0 or 3.45e-4).  With
    sin' = sqrt(1 - cos^2 at (a2 + 2^-23) + 2^-23):   unit(direction) = EPS32 x conditioning + 2 x (sin' - sinTheta).
    Without the term the direction is 5,134 units off on rough002 and 25,720 on CarPaintMidnight (clearcoatRoughness 0.03);
    the sampled direction is up to 3.2e-2 rad from the statement's (trans1_ior242, roughness 0.02 behind a refraction).
  * `1.0f - specular_prob` (pdf.cuh:216) and `1.0f - reflect_prob` (pdf.cuh:197/202) in material_pdf: at a grazing view the
    subtrahend is within 1e-2 of 1, so the weight of the diffuse / refraction lobe carries EPS32 ABSOLUTE:
    unit(pdf) += EPS32 x prob_base x (that lobe's pdf) (`cancel` of material_pdf).  Without the term the pdf is 36.0 units off
    on rough002 (NdotV = 1e-3) and 25.7 on Diamond (behind the surface).
The same differences stand in material_scatter (path_logic.cuh:541, :697, :762); its attenuation and out_pdf need no term:
their largest deviations in the table below are measured without one.
Measured on the CPU, oracle against this module, over all items of all materials (python tests/shading_truth.py prints it):

    51 materials; probe op 0: 2,520 items per opaque material, 5,040 per transmissive one (2,592 at ior 1), 161,352 in all;
    probe op 1: 8 views x 4,096 states = 32,768 items per material, 1,671,168 in all

    quantity                              largest deviation (units)   attained by            x 4 = TOL
    evaluateBSDF, any channel             1.242                       BrushedAluminum        4.97
    material_pdf                          1.240                       BrushedAluminum        4.96
    scattered direction (vector norm)     2.499                       trans1_ior15_tr0      10.0
    attenuation, any channel              1.755                       trans1_coat            7.02
    out_pdf                               2.198                       Silver                 8.79
    ok / specular flags, uniforms drawn   equal on every decided item
    undecided, most of any material       op 0: none (ior 1: 8 of 2,592 items);  op 1: sampling half 1 of 32,768, both halves
    (from the statement alone)            2 of 32,768 (ior 1: 24,164 = 73.7 %, every refracted sample -- V x eta + L = 0)
"""
import ctypes as C

import numpy as np


def F(x):
    return float(np.float32(x))


PI = F(3.14159265358979323846)       # math/mathutils.cuh:13
TWO_PI = F(6.28318530717958647692)   # math/mathutils.cuh:14
EPS32 = 2.0 ** -23
M_DOT, M_K, M_PROB, M_DIFF, M_P0, M_LEN = 1e-6, 1e-5, 1e-6, 5e-7, 1e-20, 1e-5
FD_STEP = EPS32
MAX_UNDECIDED = 0.02

# quantity -> (the material that attains the largest deviation, that deviation in units); tests/test_shading_truth.py re-measures
MEASURED = dict(f=("BrushedAluminum", 1.242), pdf=("BrushedAluminum", 1.240), direction=("trans1_ior15_tr0", 2.499),
                attenuation=("trans1_coat", 1.755), out_pdf=("Silver", 2.198))
# the same measurement with the named terms left out of the units (judge_*(terms=False)): (material, quantity) -> units; the
# last is the largest |direction - statement's| in radians with or without them.  tests/test_shading_truth.py re-measures these too
WITHOUT_TERMS = {("rough002", "pdf"): 36.02, ("Diamond", "pdf"): 25.68, ("rough002", "direction"): 5134.0,
                 ("CarPaintMidnight", "direction"): 25720.0, ("trans1_ior242", "direction_rad"): 0.03206}
# largest undecided fractions of a material, from the statement alone: op 0 (ior 1 apart: 0), op 0 at ior 1, op 1 sampling half,
# op 1 both halves (ior 1 apart), op 1 both halves at ior 1
UNDECIDED = dict(eval=0.0, eval_ior1=8 / 2592, scatter=1 / 32768, scatter_both=2 / 32768, scatter_both_ior1=24164 / 32768)
# 4 x the measured maxima, the convention of brute_force.py; the GPU test uses the same table
TOL = {q: 4 * v for q, (_, v) in MEASURED.items()}

MISREADINGS = ("fresnel_exp4", "k_over_2", "eta_back", "basis_sign", "specprob_vdoth")

FIELDS3 = ("albedo", "specular", "sheenTint")
FIELDS1 = ("metallic", "roughness", "transmission", "ior", "transmissionRoughness", "clearcoat", "clearcoatRoughness",
           "iridescence", "iridescenceThickness", "sheen")
_SNAKE = dict(sheenTint="sheen_tint", transmissionRoughness="transmission_roughness", clearcoatRoughness="clearcoat_roughness",
              iridescenceThickness="iridescence_thickness")


# ------------------------------------------------------------------------------------------------------------ materials
def load_materials(mats):
    """The material SoA of a flattened scene (ptrt_materials) as {field: float64 array}."""
    n = int(mats.count)
    out = {}
    for k in FIELDS3 + FIELDS1:
        w = 3 if k in FIELDS3 else 1
        p = C.cast(getattr(mats, _SNAKE.get(k, k)), C.POINTER(C.c_float))
        a = np.ctypeslib.as_array(p, shape=(n * w,)).astype(np.float64)
        out[k] = a.reshape(n, 3) if w == 3 else a
    return out


def gather(lib, ids):
    return {k: v[ids] for k, v in lib.items()}


def _syn(**kw):
    d = dict(albedo=(0.8, 0.5, 0.3), roughness=0.5, metallic=0.0)
    d.update(kw)
    return d


# name -> Material(albedo, roughness, metallic) arguments + field assignments
SYNTHETIC = [
    ("rough0", _syn(roughness=0.0)), ("rough002", _syn(roughness=0.02)), ("rough015", _syn(roughness=0.15)),
    ("rough016", _syn(roughness=0.16)), ("rough1", _syn(roughness=1.0)),
    ("metal005", _syn(metallic=0.05)), ("metal01", _syn(metallic=0.1)), ("metal1_r016", _syn(metallic=1.0, roughness=0.16)),
    ("metal1_r015", _syn(metallic=1.0, roughness=0.15)), ("metal1_r002", _syn(metallic=1.0, roughness=0.02)),
    ("metal1_r1", _syn(metallic=1.0, roughness=1.0)),
    ("trans05_ior15", _syn(transmission=0.5, ior=1.5, roughness=0.3)),
    ("trans1_ior1", _syn(transmission=1.0, ior=1.0, roughness=0.2)),
    ("trans1_ior133_tr03", _syn(transmission=1.0, ior=1.33, roughness=0.05, transmissionRoughness=0.3)),
    ("trans1_ior15_tr0", _syn(transmission=1.0, ior=1.5, roughness=0.16, transmissionRoughness=0.0)),
    ("trans1_ior242", _syn(transmission=1.0, ior=2.42, roughness=0.02)),
    ("trans1_metal005", _syn(transmission=1.0, ior=1.5, metallic=0.05, roughness=0.3)),
    ("trans1_metal01", _syn(transmission=1.0, ior=1.5, metallic=0.1, roughness=0.3)),
    ("trans1_coat", _syn(transmission=1.0, ior=1.5, roughness=0.2, clearcoat=1.0, clearcoatRoughness=0.3)),
    ("coat05_r0", _syn(clearcoat=0.5, clearcoatRoughness=0.0)), ("coat1_r01", _syn(clearcoat=1.0, clearcoatRoughness=0.1)),
    ("coat1_r03", _syn(clearcoat=1.0, clearcoatRoughness=0.3, roughness=0.16)),
    ("coat1_metal", _syn(clearcoat=1.0, clearcoatRoughness=0.3, metallic=1.0, roughness=0.3)),
    ("sheen_tint", _syn(sheen=1.0, sheenTint=(1.0, 0.2, 0.6))),
    ("irid100", _syn(iridescence=1.0, iridescenceThickness=100.0, roughness=0.3)),
    ("irid400", _syn(iridescence=1.0, iridescenceThickness=400.0, roughness=0.3)),
    ("irid800_metal", _syn(iridescence=1.0, iridescenceThickness=800.0, roughness=0.3, metallic=1.0)),
    ("albedo_zero_channel", _syn(albedo=(0.9, 0.0, 0.4))),
    ("albedo_zero_channel_metal", _syn(albedo=(0.9, 0.0, 0.4), metallic=1.0, roughness=0.3)),
    ("spec_white", _syn(specular=(1.0, 1.0, 1.0), roughness=0.3)),
]


def library_names():
    import make_function_kats as M
    return M.NAMES + ["GlowingNeon"] + [n for n, _ in SYNTHETIC]


def add_library(P, scene):
    """One cube per material: the 21 of make_function_kats in their order, then SYNTHETIC."""
    import make_function_kats as M
    for n in M.NAMES:
        scene.addCube(getattr(P.scenes.Materials, n)())
    scene.addCube(P.scenes.Materials.GlowingNeon((0.2, 1.0, 0.2)))
    for _, d in SYNTHETIC:
        d = dict(d)
        m = P.Material(d.pop("albedo"), d.pop("roughness"), d.pop("metallic"))
        for k, v in d.items():
            m.set(k, v)
        scene.addCube(m)
    return scene


def simple_variant_ok(lib):
    """Materials the kernels' simple shading variant is chosen for (ptrt_upload_materials in ptrt_capi.hip)."""
    return (lib["transmission"] <= 0) & (lib["clearcoat"] <= 0) & (lib["iridescence"] <= 0) & (lib["sheen"] <= 0)


# ------------------------------------------------------------------------------------------------------------ vec3
def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _col(s):
    return np.asarray(s)[:, None]


def _normalize(v):                                   # common/vec3.cuh:107-110
    ln = np.sqrt(_dot(v, v))
    return np.where(_col(ln > 0), v / _col(np.where(ln > 0, ln, 1.0)), 0.0)


def _cross(a, b):                                    # common/vec3.cuh:137
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _lerp(a, b, t):                                  # common/vec3.cuh:155-157
    return (1.0 - _col(t)) * a + _col(t) * b


def _clamp01(x):                                     # rendering/render_utils.cuh:33-35
    return np.minimum(np.maximum(x, 0.0), 1.0)


def _reflect(I, N):                                  # rendering/render_utils.cuh:41-44
    return I - 2.0 * _col(_dot(I, N)) * N


class Decisions:
    """Collects, per item, whether every decision met so far was away from its threshold."""

    def __init__(self, n):
        self.ok = np.ones(n, bool)

    def far(self, x, thr, margin, active=None):
        good = np.abs(x - thr) > margin
        if active is not None:
            good = good | ~active
        self.ok &= good


# ------------------------------------------------------------------------------------------------------------ pbr_utils.cuh
def fresnelSchlick(cosTheta, F0, mis=None):          # rendering/pbr_utils.cuh:16-22
    f = 1.0 - _clamp01(cosTheta)
    f5 = f * f * f * f if mis == "fresnel_exp4" else (f * f) * (f * f) * f
    return F0 + (1.0 - F0) * _col(f5)


def distributionGGX(N, H, roughness):                # rendering/pbr_utils.cuh:37-48
    a = roughness * roughness
    a2 = a * a
    NdotH = np.maximum(_dot(N, H), 0.0)
    denom = NdotH * NdotH * (a2 - 1.0) + 1.0
    denom = PI * denom * denom
    return a2 / np.maximum(denom, F(1e-6))


def geometrySchlickGGX(NdotV, roughness, mis=None):  # rendering/pbr_utils.cuh:56-62
    r = roughness + 1.0
    k = (r * r) * (0.5 if mis == "k_over_2" else 0.125)
    return NdotV / (NdotV * (1.0 - k) + k + F(1e-6))


def geometrySmith(N, V, L, roughness, mis=None):     # rendering/pbr_utils.cuh:64-72
    return geometrySchlickGGX(np.maximum(_dot(N, L), 0.0), roughness, mis) * \
        geometrySchlickGGX(np.maximum(_dot(N, V), 0.0), roughness, mis)


def geometrySmithTransmission(N, V, L, roughness, mis=None):   # rendering/path_logic.cuh:33-42
    return geometrySchlickGGX(np.abs(_dot(N, L)), roughness, mis) * \
        geometrySchlickGGX(np.maximum(_dot(N, V), 0.0), roughness, mis)


def calculateIridescence(thickness, cosTheta, filmIOR, baseIOR, dec=None, active=None):   # rendering/pbr_utils.cuh:85-125
    cosTheta = _clamp01(cosTheta)
    sinTheta = np.sqrt(1.0 - cosTheta * cosTheta)
    sinThetaFilm = sinTheta / filmIOR
    total = sinThetaFilm * sinThetaFilm > 1.0
    if dec is not None:
        dec.far(sinThetaFilm * sinThetaFilm, 1.0, M_PROB, active)
    cosThetaFilm = np.sqrt(np.maximum(1.0 - sinThetaFilm * sinThetaFilm, 0.0))
    OPD = 2.0 * filmIOR * thickness * cosThetaFilm
    R1 = ((1.0 - filmIOR) / (1.0 + filmIOR)) ** 2
    R2 = ((filmIOR - baseIOR) / (filmIOR + baseIOR)) ** 2
    sqrtR1R2 = np.sqrt(R1 * R2)
    R_max = (np.sqrt(R1) + np.sqrt(R2)) ** 2
    inv_R_max = 1.0 / (R_max + F(1e-6))
    out = []
    for wl in (650.0, 550.0, 450.0):
        delta = TWO_PI * OPD * F(1.0 / wl)
        out.append(_clamp01((R1 + R2 + 2.0 * sqrtR1R2 * np.cos(delta)) * inv_R_max))
    return np.where(_col(total), 1.0, np.stack(out, axis=1))


def schlick_dielectric(cosTheta, ior_i, ior_t):      # rendering/pbr_utils.cuh:127-138
    r0 = ((ior_i - ior_t) / (ior_i + ior_t)) ** 2
    f = 1.0 - _clamp01(cosTheta)
    return r0 + (1.0 - r0) * ((f * f) * (f * f) * f)


def F0_base(M, NdotV, dec=None):                     # path_logic.cuh:172-181 = 505-514 = math/pdf.cuh:144-153
    F0 = _lerp(M["specular"], M["albedo"], _clamp01(M["metallic"]))
    irid = _clamp01(M["iridescence"])
    on = irid > 0.0
    with np.errstate(all="ignore"):
        ic = calculateIridescence(M["iridescenceThickness"], NdotV, F(1.3), M["ior"], dec, on)
    return np.where(_col(on), _lerp(F0, ic, irid), F0)


# ------------------------------------------------------------------------------------------------------------ sampling.cuh
def createOrthoNormalBasis(N, mis=None):             # math/sampling.cuh:73-91
    len2 = _dot(N, N)
    small = len2 < F(1e-20)
    Nn = N / _col(np.sqrt(np.where(small, 1.0, len2)))
    s = np.ones(len(N)) if mis == "basis_sign" else np.copysign(1.0, Nn[:, 2])
    a = -1.0 / (s + Nn[:, 2])
    b = Nn[:, 0] * Nn[:, 1] * a
    T = np.stack([1.0 + s * Nn[:, 0] * Nn[:, 0] * a, s * b, -s * Nn[:, 0]], axis=1)
    B = _cross(Nn, T)
    T = np.where(_col(small), np.array([1.0, 0.0, 0.0]), T)
    B = np.where(_col(small), np.array([0.0, 1.0, 0.0]), B)
    return T, B


def hemisphere_to_world(sample, N, mis=None):        # math/sampling.cuh:159-164
    T, B = createOrthoNormalBasis(N, mis)
    return _col(sample[:, 0]) * T + _col(sample[:, 1]) * B + _col(sample[:, 2]) * N


def importance_sample_ggx(N, roughness, u1, u2, mis=None):   # math/sampling.cuh:187-208 (u1, u2 in the order they are drawn)
    a = roughness * roughness
    a2 = a * a
    u2 = np.minimum(u2, F(0.9999999))
    phi = TWO_PI * u1
    cosTheta = np.sqrt((1.0 - u2) / (1.0 + (a2 - 1.0) * u2))
    sinTheta = np.sqrt(np.maximum(0.0, 1.0 - cosTheta * cosTheta))
    H = np.stack([sinTheta * np.cos(phi), sinTheta * np.sin(phi), cosTheta], axis=1)
    # what float32 can lose in sinTheta (see TOLERANCES): `a2 - 1.0f` and `1.0f + (a2 - 1.0f) * u2` keep a2 to 2^-24 absolute
    # each, and `1.0f - cosTheta * cosTheta` is known to 2^-23 absolute
    cos2_alt = (1.0 - u2) / (1.0 + (a2 + EPS32 - 1.0) * u2)          # (a smaller cos: sinTheta grows with a2)
    sin_alt = np.sqrt(np.maximum(0.0, 1.0 - cos2_alt) + EPS32)
    return hemisphere_to_world(H, N, mis), sin_alt - sinTheta


def sample_cosine_hemisphere(u1, u2):                # math/sampling.cuh:141-147
    r = np.sqrt(u1)
    phi = TWO_PI * u2
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - u1))], axis=1)


# ------------------------------------------------------------------------------------------------------------ pdf.cuh
def pdf_ggx_reflect(N, V, L, roughness):             # math/pdf.cuh:80-94 (NdotV == 0 is decided by the caller)
    NdotV = np.maximum(_dot(N, V), 0.0)
    H = _normalize(V + L)
    NdotH = np.maximum(_dot(N, H), 0.0)
    VdotH = np.maximum(_dot(V, H), 0.0)
    D = distributionGGX(N, H, roughness)
    return np.where(NdotV == 0.0, 0.0, D * NdotH / (4.0 * VdotH + F(1e-6)))


def _refraction_half_vector(N, V, L, eta, dec, active):   # pdf.cuh:110-112 = path_logic.cuh:202-204 = 639-641
    S = -(V * _col(eta) + L)
    H = _normalize(S)
    nh = _dot(N, H)
    if dec is not None:
        dec.far(np.sqrt(_dot(S, S)), 0.0, M_LEN, active)
        dec.far(nh, 0.0, M_DOT, active)
    return np.where(_col(nh < 0.0), -H, H)


def pdf_ggx_refract(N, V, L, roughness, eta, dec=None, active=None):   # math/pdf.cuh:97-123
    NdotV = np.maximum(_dot(N, V), 0.0)
    NdotL = _dot(N, L)
    zero = (NdotV <= 0.0) | (NdotL >= 0.0)
    H = _refraction_half_vector(N, V, L, eta, dec, active)
    VdotH = np.maximum(_dot(V, H), 0.0)
    LdotH = np.abs(_dot(L, H))
    NdotH = np.maximum(_dot(N, H), 0.0)
    D = distributionGGX(N, H, roughness)
    dwh_dwo = (eta * eta * LdotH) / (eta * VdotH + LdotH) ** 2
    return np.where(zero, 0.0, D * NdotH * np.abs(dwh_dwo))


class _Pre:
    pass


def _prelude(M, N, V, ff, dec, mis=None):
    """What the three functions compute alike before they branch (path_logic.cuh:160-186, 495-544; pdf.cuh:131-181)."""
    p = _Pre()
    p.NdotV = np.maximum(_dot(N, V), 0.0)
    p.metal = _clamp01(M["metallic"])
    p.rough = np.maximum(M["roughness"], F(0.02))
    p.trans = _clamp01(M["transmission"])
    p.F0 = F0_base(M, p.NdotV, dec)
    p.transmissive = (p.trans > 0.0) & (p.metal < F(0.1))
    p.transRough = np.maximum(M["transmissionRoughness"], p.rough)
    front = ff != 0
    if mis == "eta_back":
        front = np.ones_like(front)
    p.eta = np.where(front, 1.0 / M["ior"], M["ior"])
    p.ior_i = np.where(ff != 0, 1.0, M["ior"])
    p.ior_t = np.where(ff != 0, M["ior"], 1.0)
    p.clearcoat = _clamp01(M["clearcoat"])
    p.coated = p.clearcoat > 0.0
    p.ccRough = np.where(p.coated, np.maximum(M["clearcoatRoughness"], F(0.001)), 0.0)
    n = len(p.NdotV)
    p.F0_coat = np.where(_col(p.coated), F(0.04), 0.0) * np.ones((n, 3))
    F_coat = fresnelSchlick(p.NdotV, np.full((n, 3), F(0.04)), mis)
    p.P_coat = np.where(p.coated, _clamp01(F_coat.sum(axis=1) * F(1.0 / 3.0) * p.clearcoat), 0.0)
    p.prob_base = 1.0 - p.P_coat
    p.F_base_NdotV = fresnelSchlick(p.NdotV, p.F0, mis)
    return p


def material_pdf(M, N, V, L, ff, mis=None):          # math/pdf.cuh:127-220
    """-> (pdf, decided, cancel): cancel is the named cancellation term of the pdf's unit (see TOLERANCES)."""
    n = len(N)
    dec = Decisions(n)
    with np.errstate(all="ignore"):
        p = _prelude(M, N, V, ff, dec, mis)
        dec.far(_dot(N, V), 0.0, M_DOT)                                          # pdf.cuh:135
        live = p.NdotV != 0.0
        ndl = _dot(N, L)
        NdotL = np.maximum(ndl, 0.0)
        up = NdotL > 0.0
        dec.far(ndl, 0.0, M_DOT, live)                                           # pdf.cuh:169, 183, 208
        total = np.where(p.coated & up, p.P_coat * pdf_ggx_reflect(N, V, L, p.ccRough), 0.0)   # pdf.cuh:160-174
        # transmissive: pdf.cuh:176-206.  schlick_dielectric_oneIOR(NdotV, ior_ratio) = schlick_dielectric(NdotV, 1, ior_ratio)
        reflect_prob = schlick_dielectric(p.NdotV, 1.0, p.eta)
        H = _normalize(V + L)
        VdotH = np.maximum(_dot(V, H), 0.0)
        k = 1.0 - p.eta * p.eta * (1.0 - VdotH * VdotH)
        dec.far(k, 0.0, M_K * np.maximum(1.0, p.eta ** 2), live & p.transmissive & up & (p.eta != 1.0))
        t_up = p.prob_base * reflect_prob * pdf_ggx_reflect(N, V, L, p.rough) + \
            np.where(k < 0.0, p.prob_base * (1.0 - reflect_prob) * pdf_ggx_reflect(N, V, L, p.transRough), 0.0)
        t_dn = p.prob_base * (1.0 - reflect_prob) * \
            pdf_ggx_refract(N, V, L, p.transRough, p.eta, dec, live & p.transmissive & ~up & (ndl < 0.0))
        # opaque: pdf.cuh:208-217
        Fb = p.F_base_NdotV
        if mis == "specprob_vdoth":
            Fb = fresnelSchlick(VdotH, p.F0)
        specular_prob = np.where(p.metal > 0.0, 1.0, Fb.max(axis=1))
        opaque = np.where(up, p.prob_base * (specular_prob * pdf_ggx_reflect(N, V, L, p.rough) +
                                             (1.0 - specular_prob) * NdotL * F(1.0 / PI)), 0.0)
        total = total + np.where(p.transmissive, np.where(up, t_up, t_dn), opaque)
        # `1.0f - specular_prob` (:216) and `1.0f - reflect_prob` (:197, :202) are differences of numbers near 1 at a grazing
        # view; a rounding of the subtrahend by one part in 2^23 moves the pdf by this much
        cancel = EPS32 * p.prob_base * np.where(p.transmissive, np.where(up, np.where(k < 0.0, pdf_ggx_reflect(N, V, L, p.transRough), 0.0),
                                                                         pdf_ggx_refract(N, V, L, p.transRough, p.eta)),
                                                np.where(p.metal > 0.0, 0.0, NdotL / PI))
        return np.where(live, total, 0.0), dec.ok, np.where(live, cancel, 0.0)


def evaluateBSDF(M, N, V, L, ff, mis=None):          # rendering/path_logic.cuh:157-250
    """-> (f (n,3), decided)"""
    n = len(N)
    dec = Decisions(n)
    with np.errstate(all="ignore"):
        p = _prelude(M, N, V, ff, dec, mis)
        dec.far(_dot(N, V), 0.0, M_DOT)                                          # :163
        live = p.NdotV > 0.0
        ndl = _dot(N, L)
        dec.far(ndl, 0.0, M_DOT, live)                                           # :189, :232
        up = ndl > 0.0
        NdotL = np.maximum(ndl, 0.0)
        H = _normalize(L + V)
        VdotH = np.maximum(_dot(V, H), 0.0)
        D = distributionGGX(N, H, p.rough)
        G = geometrySmith(N, V, L, p.rough, mis)
        Fr = fresnelSchlick(VdotH, p.F0, mis)
        DGF = _col(D * G) * Fr
        # transmissive, reflection side :189-199
        t_up = DGF / _col(4.0 * p.NdotV * ndl + F(1e-6)) * _col(ndl)
        # transmissive, refraction side :200-228
        act = live & p.transmissive & ~up
        eta = p.eta
        Hr = _refraction_half_vector(N, V, L, eta, dec, act)
        VdotHr = np.maximum(_dot(V, Hr), 0.0)
        LdotHr = np.abs(_dot(L, Hr))
        NdotL_abs = np.abs(ndl)
        k = 1.0 - eta * eta * (1.0 - VdotHr * VdotHr)
        dec.far(k, 0.0, M_K * np.maximum(1.0, eta ** 2), act & (eta != 1.0))
        Dr = distributionGGX(N, Hr, p.transRough)
        Gr = geometrySmithTransmission(N, V, L, p.transRough, mis)
        Ft = 1.0 - fresnelSchlick(VdotHr, p.F0, mis)
        numerator = eta * eta * (1.0 - p.metal) * Gr * Dr * VdotHr * LdotHr
        denominator = p.NdotV * NdotL_abs * (eta * VdotHr + LdotHr) ** 2
        btdf = M["albedo"] * Ft * _col(numerator) / _col(denominator + F(1e-6))
        t_dn = np.where(_col(k < 0.0), 0.0, btdf * _col(NdotL_abs))
        # opaque :231-249
        spec = DGF / _col(4.0 * p.NdotV * NdotL + F(0.001))
        kD = (1.0 - Fr) * _col(1.0 - p.metal)
        diffuse = kD * M["albedo"] / PI
        opaque = np.where(_col(NdotL <= 0.0), 0.0, (diffuse + spec) * _col(NdotL))
        f = np.where(_col(p.transmissive), np.where(_col(up), t_up, t_dn), opaque)
        return np.where(_col(live), f, 0.0), dec.ok


# ------------------------------------------------------------------------------------------------------------ material_scatter
def refraction_branch(V, H, eta):                    # rendering/path_logic.cuh:569-584
    """The refraction branch of material_scatter from a sampled half vector: -> (V.H as sampled, |V.H| after the flip, k, the
    reflected direction taken when k < 0, the refracted one taken otherwise)."""
    vh = _dot(V, H)
    H2 = np.where(_col(vh < 0.0), -H, H)
    VdotH = np.abs(_dot(V, H2))
    k = 1.0 - eta * eta * (1.0 - VdotH * VdotH)
    d_tir = _reflect(-V, H2)
    d_refr = _normalize(_col(eta) * (-V) + _col(eta * VdotH - np.sqrt(np.maximum(k, 0.0))) * H2)
    return vh, VdotH, k, d_tir, d_refr


LOBE_NONE, LOBE_COAT, LOBE_SPEC, LOBE_REFRACT, LOBE_TIR, LOBE_DIFFUSE = -1, 0, 1, 2, 3, 4


def scatter_sample(M, N, V, ff, u, u1, u2, mis=None):   # rendering/path_logic.cuh:490-586, 692-716
    """The sampling half: -> dict(direction, ok, specular, lobe, is_refraction, draws, sin_unit, decided).  u, u1, u2 are the
    uniforms in the order the reference draws them; `draws` is how many it consumed."""
    n = len(N)
    dec = Decisions(n)
    with np.errstate(all="ignore"):
        p = _prelude(M, N, V, ff, dec, mis)
        tr = p.transmissive
        # transmissive :533-586
        reflect_prob = schlick_dielectric(p.NdotV, p.ior_i, p.ior_t)
        P_tr = p.prob_base * reflect_prob
        # opaque :692-714
        specular_prob = np.where(p.metal > 0.0, 1.0, p.F_base_NdotV.max(axis=1))
        P_spec = p.prob_base * specular_prob
        P_diff = p.prob_base * (1.0 - specular_prob)
        second = p.P_coat + np.where(tr, P_tr, P_spec)
        dec.far(u, p.P_coat, M_PROB, p.coated)
        pick_coat = u < p.P_coat
        dec.far(u, second, M_PROB, ~pick_coat)
        pick_second = ~pick_coat & (u < second)
        third = ~pick_coat & ~pick_second
        dec.far(P_diff, F(1e-6), M_DIFF, ~tr & third)
        diffuse = ~tr & third & (P_diff > F(1e-6))
        ok = tr | pick_coat | pick_second | diffuse
        sr = np.where(pick_coat, p.ccRough, np.where(pick_second, p.rough, p.transRough))
        H, sin_loss = importance_sample_ggx(N, sr, u1, u2, mis)
        d_refl = _reflect(-V, H)
        # the refraction branch :563-586
        refr = tr & third
        eta = p.eta
        vh, VdotH, k, d_tir, d_refr = refraction_branch(V, H, eta)
        dec.far(vh, 0.0, M_DOT, refr)
        dec.far(k, 0.0, M_K * np.maximum(1.0, eta ** 2), refr & (eta != 1.0))
        tir = refr & (k < 0.0)
        d_diff = hemisphere_to_world(sample_cosine_hemisphere(u1, u2), N, mis)
        d = np.where(_col(refr), np.where(_col(tir), d_tir, d_refr), np.where(_col(diffuse), d_diff, d_refl))
        d = np.where(_col(tr), d, _normalize(d))                                 # :716 (the opaque path only)
        specular = np.where(diffuse, False, (sr < F(0.1)) | tir)
        lobe = np.where(pick_coat, LOBE_COAT, np.where(pick_second, LOBE_SPEC, np.where(
            refr, np.where(tir, LOBE_TIR, LOBE_REFRACT), np.where(diffuse, LOBE_DIFFUSE, LOBE_NONE))))
        sin_unit = np.where(diffuse | ~ok, 0.0, 2.0 * sin_loss)
        d = np.where(_col(ok), d, 0.0)
        return dict(direction=d, ok=ok, specular=specular & ok, lobe=lobe, is_refraction=refr, draws=np.where(ok, 3, 1),
                    sin_unit=sin_unit, decided=dec.ok)


def scatter_value(M, N, V, ff, d, is_refraction, mis=None):   # rendering/path_logic.cuh:588-690, 718-779
    """The evaluating half, at direction d: -> (attenuation (n,3), out_pdf, decided)."""
    n = len(N)
    dec = Decisions(n)
    with np.errstate(all="ignore"):
        p = _prelude(M, N, V, ff, dec, mis)
        tr = p.transmissive
        eta = p.eta
        reflect_prob = schlick_dielectric(p.NdotV, p.ior_i, p.ior_t)
        P_tr, P_rf = p.prob_base * reflect_prob, p.prob_base * (1.0 - reflect_prob)
        ndl = _dot(N, d)
        Hh = _normalize(V + d)
        NdotH = np.maximum(_dot(N, Hh), 0.0)
        VdotH = np.maximum(_dot(V, Hh), 0.0)

        def lobe(rough, Fr, NdotL):      # D, G, F of a reflection lobe with the 1e-6 denominator: :605-618 and its copies
            D = distributionGGX(N, Hh, rough)
            G = geometrySmith(N, V, d, rough, mis)
            pdf = D * NdotH / (4.0 * VdotH + F(1e-6))
            brdf = _col(D * G) * Fr / _col(4.0 * p.NdotV * NdotL + F(1e-6))
            return pdf, brdf

        # ---- transmissive :588-689
        dec.far(ndl, 0.0, M_DOT, tr)
        up, dn = ndl > 0.0, ndl < 0.0
        Hb = np.where(_col(is_refraction), _normalize(_col(eta) * V + d), Hh)             # :593-601
        F_coat_atten = fresnelSchlick(np.maximum(_dot(V, Hb), 0.0), p.F0_coat, mis)
        base_t = 1.0 - _col(p.clearcoat) * F_coat_atten
        f_t = np.zeros((n, 3))
        pdf_t = np.zeros(n)
        on = (p.P_coat > 0.0) & up                                                     # :604-619
        pdf, brdf = lobe(p.ccRough, fresnelSchlick(VdotH, p.F0_coat, mis), ndl)
        pdf_t += np.where(on, p.P_coat * pdf, 0.0)
        f_t += np.where(_col(on), _col(p.clearcoat) * brdf * _col(ndl), 0.0)
        dec.far(P_tr, 0.0, M_P0, tr & up)
        on = (P_tr > 0.0) & up                                                         # :621-636
        pdf, brdf = lobe(p.rough, fresnelSchlick(VdotH, p.F0, mis), ndl)
        pdf_t += np.where(on, P_tr * pdf, 0.0)
        f_t += np.where(_col(on), brdf * _col(ndl) * base_t, 0.0)
        dec.far(P_rf, 0.0, M_P0, tr & dn)
        on = (P_rf > 0.0) & dn                                                         # :638-669
        Hr = _refraction_half_vector(N, V, d, eta, dec, tr & on)
        VdotHr = np.maximum(_dot(V, Hr), 0.0)
        LdotHr = np.abs(_dot(d, Hr))
        NdotHr = np.maximum(_dot(N, Hr), 0.0)
        NdotL_abs = np.abs(ndl)
        k = 1.0 - eta * eta * (1.0 - VdotHr * VdotHr)
        dec.far(k, 0.0, M_K * np.maximum(1.0, eta ** 2), tr & on & (eta != 1.0))
        on = on & (k >= 0.0)
        Dr = distributionGGX(N, Hr, p.transRough)
        Gr = geometrySmithTransmission(N, V, d, p.transRough, mis)
        dwh_dwo = (eta * eta * LdotHr) / (eta * VdotHr + LdotHr) ** 2
        pdf_t += np.where(on, P_rf * Dr * NdotHr * np.abs(dwh_dwo), 0.0)
        Ft = 1.0 - fresnelSchlick(VdotHr, p.F0, mis)
        numerator = eta * eta * (1.0 - p.metal) * Gr * Dr * VdotHr * LdotHr
        denominator = p.NdotV * NdotL_abs * (eta * VdotHr + LdotHr) ** 2
        btdf = M["albedo"] * Ft * _col(numerator) / _col(denominator + F(1e-6))
        f_t += np.where(_col(on), btdf * _col(NdotL_abs) * base_t, 0.0)
        on = is_refraction & up                                                        # :671-685
        pdf, brdf = lobe(p.transRough, np.ones((n, 3)), ndl)
        pdf_t += np.where(on, P_rf * pdf, 0.0)
        f_t += np.where(_col(on), brdf * _col(ndl) * base_t, 0.0)
        out_pdf_t = np.maximum(pdf_t, F(1e-6))                                         # :687-688
        att_t = f_t / _col(out_pdf_t)

        # ---- opaque :718-779
        NdotL = np.maximum(ndl, 0.0)
        specular_prob = np.where(p.metal > 0.0, 1.0, p.F_base_NdotV.max(axis=1))
        P_spec = p.prob_base * specular_prob
        P_diff = p.prob_base * (1.0 - specular_prob)
        f_o = np.zeros((n, 3))
        pdf_o = np.zeros(n)
        on = p.P_coat > 0.0                                                            # :722-736
        pdf, brdf = lobe(p.ccRough, fresnelSchlick(VdotH, p.F0_coat, mis), NdotL)
        pdf_o += np.where(on, p.P_coat * pdf, 0.0)
        f_o += np.where(_col(on), _col(p.clearcoat) * brdf * _col(NdotL), 0.0)
        base_o = 1.0 - _col(p.clearcoat) * fresnelSchlick(VdotH, p.F0_coat, mis)           # :738-741
        pdf, brdf = lobe(p.rough, fresnelSchlick(VdotH, p.F0, mis), NdotL)             # :743-755
        pdf_o += P_spec * pdf
        f_o += brdf * _col(NdotL) * base_o
        dec.far(P_diff, F(1e-6), M_DIFF, ~tr)
        on = P_diff > F(1e-6)                                                          # :757-774
        pdf_o += np.where(on, P_diff * NdotL / PI, 0.0)
        sheen = _clamp01(M["sheen"])
        kD = (1.0 - p.F_base_NdotV) * _col(1.0 - p.metal)
        f_diff = (kD * M["albedo"] / PI) * _col(NdotL)
        FH = 1.0 - np.maximum(_dot(V, Hh), 0.0)
        Csheen = _lerp(np.ones((n, 3)), M["sheenTint"], np.full(n, 0.5))
        f_diff = np.where(_col(sheen > 0.0), f_diff + _col(sheen) * Csheen * _col(FH ** 5 * NdotL), f_diff)
        f_o += np.where(_col(on), f_diff * base_o, 0.0)
        att_o = f_o / _col(np.maximum(pdf_o, F(1e-6)))                                 # :776-777

        return np.where(_col(tr), att_t, att_o), np.where(tr, out_pdf_t, pdf_o), dec.ok


def material_scatter(M, N, V, ff, u, u1, u2, mis=None):
    """(uniforms) -> dict(direction, attenuation, out_pdf, ok, specular, lobe, draws, decided): the two halves composed."""
    s = scatter_sample(M, N, V, ff, u, u1, u2, mis)
    att, pdf, dv = scatter_value(M, N, V, ff, s["direction"], s["is_refraction"], mis)
    s.update(attenuation=np.where(_col(s["ok"]), att, 0.0), out_pdf=np.where(s["ok"], pdf, 0.0), decided=s["decided"] & (dv | ~s["ok"]))
    return s


# ------------------------------------------------------------------------------------------------------------ conditioning
def conditioning(fn, M, vecs, consts=(), fields=True):
    """|q| + sum_i |x_i dq/dx_i| of q = fn(M, *vecs, *consts) over every component of `vecs` ((n,3) arrays) and every field of
    M, by central differences with relative step FD_STEP.  q may be (n,) or (n,3)."""
    q0 = fn(M, *vecs, *consts)
    cond = np.abs(q0)

    def add(setter):
        nonlocal cond
        hi = setter(1.0 + FD_STEP)
        lo = setter(1.0 - FD_STEP)
        with np.errstate(all="ignore"):
            cond = cond + np.abs(hi - lo) / (2.0 * FD_STEP)

    for j, v in enumerate(vecs):
        for c in range(3):
            if not np.any(v[:, c]):
                continue

            def setter(s, j=j, c=c, v=v):
                w = v.copy()
                w[:, c] *= s
                return fn(M, *[w if i == j else x for i, x in enumerate(vecs)], *consts)
            add(setter)
    for key in (FIELDS3 + FIELDS1 if fields else ()):
        a = M[key]
        for c in (range(3) if a.ndim == 2 else [None]):
            col = a[:, c] if c is not None else a
            if not np.any(col):
                continue

            def setter(s, key=key, c=c, a=a):
                w = a.copy()
                if c is None:
                    w *= s
                else:
                    w[:, c] *= s
                M2 = dict(M)
                M2[key] = w
                return fn(M2, *vecs, *consts)
            add(setter)
    return cond


def _as(extra, like):
    return extra if extra.ndim == like.ndim else _col(extra)


def deviation_units(got, want_fn, M, vecs, consts=(), extra_unit=None, tol=None, norm=False):
    """|got - want| in units of EPS32 x conditioning (+ extra_unit); with `norm` the (n,3) quantity counts as a vector, by its
    norm.  The conditioning costs dozens of evaluations and is at least |want|: with `tol` given, items already within tol x
    EPS32 x |want| are reported by that (larger) figure, the others get the conditioning over the vector inputs (a lower bound
    still), and only what is left gets the material fields too.  -> units, (n,) with `norm`, else the shape of got"""
    def mag(a):
        return np.sqrt((a * a).sum(axis=1)) if norm else np.abs(a)

    want = want_fn(M, *vecs, *consts)
    dev = mag(got - want)

    def units_of(sel, size):
        ex = 0.0 if extra_unit is None else _as(extra_unit[sel], dev)
        with np.errstate(all="ignore"):
            return np.where(dev[sel] == 0.0, 0.0, dev[sel] / (EPS32 * size + ex))

    every = np.ones(len(got), bool)
    units = units_of(every, mag(want))
    todo = every if tol is None else np.nan_to_num(units > tol, nan=True).reshape(len(got), -1).any(axis=1)
    todo = todo & np.isfinite(dev).reshape(len(got), -1).all(axis=1)
    for fields in ((False, True) if tol is not None else (True,)):
        if todo.any():
            cond = conditioning(want_fn, {k: v[todo] for k, v in M.items()}, [v[todo] for v in vecs],
                                [c[todo] if isinstance(c, np.ndarray) else c for c in consts], fields)
            units[todo] = units_of(todo, mag(cond))
            if tol is not None:
                todo = todo & np.nan_to_num(units > tol, nan=True).reshape(len(got), -1).any(axis=1)
    return np.where(np.isnan(units), np.inf, units)


# ------------------------------------------------------------------------------------------------------------ items
def _unit(v):
    return v / np.linalg.norm(v)


def _frame(N):
    a = np.eye(3)[np.argmin(np.abs(N))]
    t = _unit(np.cross(N, a))
    return t, np.cross(N, t)


def normals():
    rs = np.random.RandomState(20261018)
    return {"rand0": _unit(rs.normal(size=3)), "rand1": _unit(rs.normal(size=3)), "+z": np.array([0.0, 0.0, 1.0]),
            "-z": np.array([0.0, 0.0, -1.0]), "z-0": np.array([0.6, 0.8, -0.0])}


def view(N, c, az=0.7):
    t, b = _frame(N)
    return c * N + np.sqrt(max(0.0, 1.0 - c * c)) * (np.cos(az) * t + np.sin(az) * b)


EVAL_NDOTV = (1.0, 0.7, 0.3, 0.05, 1e-3, -0.2)
OFFSETS = np.logspace(-4, 0, 25)


def _around(R, N, t):
    """R itself, then R turned by each of OFFSETS towards N and sideways."""
    w1 = N - np.dot(N, R) * R
    w1 = _unit(w1) if np.linalg.norm(w1) > 1e-6 else t
    w2 = np.cross(R, w1)
    return [R] + [np.cos(o) * R + np.sin(o) * w for o in OFFSETS for w in (w1, w2)]


def eval_directions(N, V, ior, ff):
    """L for one (N, V, face): the mirror direction and log-spaced offsets from it, the horizon +-1e-3, below the surface, the
    refracted direction (the critical one under total internal reflection) and log-spaced offsets from it."""
    t, _ = _frame(N)
    c = float(np.dot(N, V))
    R = 2.0 * c * N - V
    tang = V - c * N
    tang = _unit(tang) if np.linalg.norm(tang) > 1e-6 else t
    out = _around(R, N, t)
    for z in (1e-3, -1e-3, -0.5):
        out.append(z * N - np.sqrt(1.0 - z * z) * tang)
    if ior == 1.0:
        return out              # the refracted direction is -V: V + L = 0 and the refraction half vector does not exist
    eta = 1.0 / ior if ff else ior
    k = 1.0 - eta * eta * (1.0 - c * c)
    if k < 0.0:                 # total internal reflection for the mean normal: a grazing transmitted direction instead
        T = -0.02 * N - np.sqrt(1.0 - 0.02 ** 2) * tang
    else:
        T = _unit(eta * (-V) + (eta * c - np.sqrt(k)) * N)
    return out + _around(T, -N, t)


def eval_items(lib, ids=None, nv0=False):
    """Probe op 0 items (n, 11) float32: material, N, V, L, front_face.  `nv0`: the NdotV = 0 set."""
    nm = normals()
    rows = []
    for m in (range(len(lib["ior"])) if ids is None else ids):
        faces = (1, 0) if lib["transmission"][m] > 0 else (1,)
        for N in (nm["rand0"], nm["+z"], nm["-z"], nm["z-0"]):
            for c in ((0.0,) if nv0 else EVAL_NDOTV):
                V = view(N, c)
                for ff in faces:
                    for L in eval_directions(N, V, float(lib["ior"][m]), ff):
                        rows.append(np.concatenate([[m], N, V, L, [ff]]))
    return np.array(rows, np.float32)


# (NdotV, normal, front_face); the back-face views at 0.3 and 0.7 lie in the total-internal-reflection region of ior 1.5
SCATTER_VIEWS = ((1.0, "+z", 1), (0.7, "rand0", 1), (0.3, "-z", 0), (0.05, "rand1", 1), (1e-3, "z-0", 1), (0.7, "rand1", 0),
                 (0.3, "rand0", 1), (0.9, "z-0", 0))
OUTSIDE_VIEWS = ((0.0, "+z", 1), (-0.2, "rand0", 1))
STATES_PER_VIEW = 4096
SEED = 20261018


def scatter_states(O, views=SCATTER_VIEWS, per_view=STATES_PER_VIEW):
    """(len(views), per_view, 6) uint32: consecutive generator states, a run of its own per view."""
    return np.stack([O.xorwow_init(SEED, v * STATES_PER_VIEW, per_view) for v in range(len(views))])


def scatter_items(m, states, views=SCATTER_VIEWS):
    """Probe op 1 items (n, 14) float32 of material m: material, N, ray_dir = -V, front_face, state (6 words)."""
    nm = normals()
    nv, per = states.shape[:2]
    x = np.zeros((nv, per, 14), np.float32)
    for v, (c, nk, ff) in enumerate(views):
        N = nm[nk]
        x[v, :, 0] = m
        x[v, :, 1:4] = N
        x[v, :, 4:7] = -view(N, c)
        x[v, :, 7] = ff
        x[v, :, 8:14] = states[v].view(np.float32)
    return x.reshape(-1, 14)


def split_eval(x):
    x64 = x.astype(np.float64)
    return x[:, 0].astype(np.int64), x64[:, 1:4], x64[:, 4:7], x64[:, 7:10], x[:, 10] != 0


def split_scatter(x):
    x64 = x[:, :8].astype(np.float64)
    return x[:, 0].astype(np.int64), x64[:, 1:4], -x64[:, 4:7], x[:, 7] != 0


def advance(O, states):
    """-> (uniforms (n,3) float64, state after 1 draw, state after 3 draws) of each generator state."""
    st = states.reshape(-1, 6)
    uni = np.zeros((len(st), 3))
    a1, a3 = np.zeros_like(st), np.zeros_like(st)
    for i, s in enumerate(st):
        u, t = O.xorwow_draw(s, 1, uniform=True)
        uni[i, 0], a1[i] = u[0], t
        u, a3[i] = O.xorwow_draw(t, 2, uniform=True)
        uni[i, 1:] = u
    return uni, a1, a3


# ------------------------------------------------------------------------------------------------------------ judging
def _f_only(M, N, V, L, ff, mis=None):
    return evaluateBSDF(M, N, V, L, ff, mis)[0]


def _pdf_only(M, N, V, L, ff, mis=None):
    return material_pdf(M, N, V, L, ff, mis)[0]


def _dir_only(M, N, V, U, ff, mis=None):
    return scatter_sample(M, N, V, ff, U[:, 0], U[:, 1], U[:, 2], mis)["direction"]


def _value_only(M, N, V, d, ff, isr, mis=None):
    att, pdf = scatter_value(M, N, V, ff, d, isr, mis)[:2]
    return np.concatenate([att, _col(pdf)], axis=1)


def _units(got, fn, M, vecs, consts, sel, mis, tol, extra=None, norm=False, per_channel=False):
    """deviation_units on the selected items; 0 elsewhere; (n,) -- the largest channel, or the vector's norm."""
    out = np.zeros(got.shape if per_channel else len(got))
    if sel.any():
        u = deviation_units(got[sel].astype(np.float64), fn, {k: v[sel] for k, v in M.items()}, [v[sel] for v in vecs],
                            [c[sel] for c in consts] + [mis], extra_unit=None if extra is None else extra[sel], tol=tol, norm=norm)
        out[sel] = u if u.ndim == 1 or per_channel else u.max(axis=1)
    return out


def judge_eval(lib, x, out, mis=None, tol=None, terms=True):
    """Items x (n,11) and what the code under test made of them, out (n,4).  -> dict(f, pdf: units per item (0 where
    undecided), decided_f, decided_pdf).  `terms=False` leaves the named cancellation terms out of the units."""
    ids, N, V, L, ff = split_eval(x)
    M = gather(lib, ids)
    df = evaluateBSDF(M, N, V, L, ff, mis)[1]
    _, dp, cancel = material_pdf(M, N, V, L, ff, mis)
    if not terms:
        cancel = None
    t = tol or {}
    return dict(f=_units(out[:, :3], _f_only, M, [N, V, L], [ff], df, mis, t.get("f")),
                pdf=_units(out[:, 3], _pdf_only, M, [N, V, L], [ff], dp, mis, t.get("pdf"), extra=cancel), decided_f=df, decided_pdf=dp)


def judge_scatter(lib, x, adv, got, mis=None, tol=None, terms=True):
    """Items x (n,14), adv = advance() of their states, got = dict(direction (n,3), attenuation (n,3), out_pdf (n,) or None,
    flags (n,), state_after (n,6) uint32).  -> dict(direction, attenuation, out_pdf: units per item; flags_bad, draws_bad:
    bool per item; direction_rad: |direction - statement's| per item; decided (sampling half), decided_value (both halves, at
    the direction under test), sample).  `terms=False` leaves the named cancellation terms out of the units."""
    ids, N, V, ff = split_scatter(x)
    M = gather(lib, ids)
    uni, a1, a3 = adv
    u, u1, u2 = uni[:, 0], uni[:, 1], uni[:, 2]
    s = scatter_sample(M, N, V, ff, u, u1, u2, mis)
    dec = s["decided"]
    flags = got["flags"].astype(np.int64)
    want_flags = s["ok"].astype(np.int64) | (s["specular"].astype(np.int64) << 1)
    ok_got = (flags & 1) != 0
    flags_bad = dec & np.where(s["ok"], flags != want_flags, ok_got)       # `specular` is not set by a failed scatter
    after = np.where(_col(s["ok"]), a3, a1)
    draws_bad = dec & (got["state_after"] != after).any(axis=1)
    t = tol or {}
    sel = dec & s["ok"] & ok_got
    d = got["direction"].astype(np.float64)
    du = _units(got["direction"], _dir_only, M, [N, V, uni], [ff], sel, mis, t.get("direction"),
                extra=s["sin_unit"] if terms else None, norm=True)
    rad = np.where(sel, np.sqrt(((d - s["direction"]) ** 2).sum(axis=1)), 0.0)
    isr = s["is_refraction"]
    dv = scatter_value(M, N, V, ff, d, isr, mis)[2]
    selv = sel & dv
    # attenuation and out_pdf share one conditioning pass; where the code under test returns no out_pdf (the device probe) the
    # statement's own stands in and counts 0
    have_pdf = got.get("out_pdf") is not None
    g4 = np.concatenate([got["attenuation"].astype(np.float64),
                         _col(got["out_pdf"].astype(np.float64) if have_pdf else scatter_value(M, N, V, ff, d, isr, mis)[1])], axis=1)
    u4 = _units(g4, _value_only, M, [N, V, d], [ff, isr], selv, mis, None if not t else min(t["attenuation"], t.get("out_pdf", t["attenuation"])),
                per_channel=True)
    au, pu = u4[:, :3].max(axis=1), u4[:, 3]
    return dict(direction=du, direction_rad=rad, attenuation=au, out_pdf=pu, flags_bad=flags_bad, draws_bad=draws_bad, decided=dec,
                decided_value=selv | (dec & ~s["ok"]), sample=s)


def oracle_scatter_got(out14):
    return dict(direction=out14[:, 0:3], attenuation=out14[:, 3:6], out_pdf=out14[:, 6], flags=out14[:, 7],
                state_after=np.ascontiguousarray(out14[:, 8:14]).view(np.uint32))


def probe_scatter_got(out13):
    return dict(direction=out13[:, 0:3], attenuation=out13[:, 3:6], out_pdf=None, flags=out13[:, 6],
                state_after=np.ascontiguousarray(out13[:, 7:13]).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ the table
def open_library(P):
    """-> (host-only scene holding the library, its material arrays for the statement, ctypes reference for the oracle)."""
    s = add_library(P, P.Scene(64, 64, device=P.HOST_ONLY))
    desc = s.flatten()
    return s, load_materials(desc.contents.materials), C.byref(desc.contents.materials)


def measure(P, O, materials=None, floor=0.5, verbose=False, terms=True):
    """Oracle against the statement over every item set: -> {quantity: largest deviation in units}, {set: largest undecided
    fraction of a material}.  Deviations below `floor` units of EPS32 x |value| are not resolved further."""
    scene, lib, mats = open_library(P)
    names = library_names()
    ids = range(len(names)) if materials is None else [names.index(m) for m in materials]
    tol = dict(f=floor, pdf=floor, direction=floor, attenuation=floor)
    worst = dict(f=0.0, pdf=0.0, direction=0.0, attenuation=0.0, out_pdf=0.0, direction_rad=0.0)
    und = dict(eval_f=0.0, eval_pdf=0.0, scatter=0.0, scatter_value=0.0)
    states = scatter_states(O)
    adv = advance(O, states)
    for m in ids:
        x = eval_items(lib, [m])
        j = judge_eval(lib, x, O.eval_bsdf_n(mats, x), tol=tol, terms=terms)
        y = scatter_items(m, states)
        k = judge_scatter(lib, y, adv, oracle_scatter_got(O.scatter_n(mats, y)), tol=tol, terms=terms)
        row = dict(f=j["f"].max(), pdf=j["pdf"].max(), direction=k["direction"].max(), attenuation=k["attenuation"].max(),
                   out_pdf=k["out_pdf"].max(), direction_rad=k["direction_rad"].max())
        u = dict(eval_f=1 - j["decided_f"].mean(), eval_pdf=1 - j["decided_pdf"].mean(), scatter=1 - k["decided"].mean(),
                 scatter_value=1 - k["decided_value"].mean())
        if verbose:
            print(f"{names[m]:26s} " + " ".join(f"{q} {v:.4g}" for q, v in row.items()) + "  undecided " +
                  " ".join(f"{q} {100 * v:.4f}%" for q, v in u.items()) +
                  f"  flags {int(k['flags_bad'].sum())} draws {int(k['draws_bad'].sum())}", flush=True)
        for q in worst:
            worst[q] = max(worst[q], row[q])
        if lib["ior"][m] != 1.0:
            for q in und:
                und[q] = max(und[q], u[q])
    scene.close()
    return worst, und


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "ptrt-game-engine_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests", "golden")]
    import oracle
    import ptrt_amd
    w, u = measure(ptrt_amd, oracle, verbose=True, terms="--without-terms" not in sys.argv)
    print("largest deviation, units:", {k: round(v, 2) for k, v in w.items()})
    print("largest undecided fraction of a material:", {k: round(v, 4) for k, v in u.items()})
