"""The post chain of the reference -- motion vectors, firefly clamp, temporal accumulation, variance estimate, the a-trous
passes, bloom, bilinear up-scale, ACES/sRGB tonemap -- stated once more in float64 numpy.

TEST INFRASTRUCTURE.  oracle/denoiser_oracle.cpp, oracle/post_oracle.cpp and csrc/pt_denoise.hip.h, pt_post.hip.h were written by ONE
reading of the reference's denoiser.cuh, denoiser_kernels.cuh, scene_kernels.cuh and scene.cuh and are held to each other at
tolerance 0, so a shared misreading passes every parity test.  This module is a second reading, made from the reference's text alone
(file:line beside each function; paths relative to the reference's src/pathtracer unless they start with common/), vectorised over
the pixels of a frame, in float64.  It shares nothing with the oracle beyond the field names of the settings struct.  Literals are the
float32 values the text spells (`1e-6f` is float32(1e-6)); inputs are float32 arrays; everything else is float64.

SNAPSHOT SEMANTICS.  Denoiser::denoiseChannel launches temporal_accumulation_kernel with out_mean == current_color == d_ping
(rendering/denoiser.cuh:915-916): threads read the 3x3 neighbourhood of an image other threads are overwriting, a race.  The
statement (like the oracle and the kernels) gives every read the PRE-kernel image: the result of the race when every read
precedes every write.

IGNORED SETTINGS.  `firefly_threshold` reaches firefly_suppression_kernel and is never read (relaxation 1.25 and the cap 10 are
literals, denoiser.cuh:416-419); `sigma_normal` and `sigma_depth` reach atrous_filter_kernel and are never read (denoiser.cuh:650-749).
tests/test_post_truth.py asserts that changing them changes nothing here.

STAGE BY STAGE.  `denoise_frame` states ONE frame: it takes the float32 history (mean, m2, length, normal, depth, object id) the
implementation under test holds after the frame before, the float32 motion vectors of the frame (judged on their own), and runs
firefly -> temporal -> variance -> five a-trous passes in float64, returning the history after the temporal pass and the image after
k = 0..5 passes (what `atrous_iterations = k` gives).  Nothing drifts: frame f of the statement never sees frame f - 1 of the statement.

DECIDED.  float32 and float64 may take different branches next to a threshold.  Every answer carries `decided`, computed here alone.
With E = EPS32 = 2^-23 the margins are (|q - threshold| < margin means undecided; a margin of 0 never is):
    dot(n, n) < 0.1, dot(n0, n1) < threshold (edge rule, normal rejection)   2 E sum|a_i b_i|   (three products, two sums)
    |d0 - d1| / max_d > edge_depth_threshold                                 2 E q              (difference and quotient, E/2 each, x 2)
    prev_u, prev_v against 0.5, W - 0.5, H - 0.5; the cell of the taps; floor(prev_u) of `nearest`
                                           du = E (|mv W| + |prev_u|), and 0 where mv is exactly 0 (x + 0.5 - 0 is exact in float32)
    total_w < 1e-6 of the taps                                               2 du_x + 2 du_y + 4 E, and 0 where no tap is valid (0 exactly)
    total_w < 1e-6 of an a-trous pixel                                       the propagated unit of total_w (0 with no tap accepted)
    the two depth rejections                                                 unit(hist_d) + E (|d - hist_d| + threshold)
    (uint32_t)(s * 10000.0f) and its three kin of the lens hash              2 E x the factor (s, t <= 1; product and quotient)
    c <= 0.0031308 in the OETF                                               4 unit(c)
    (unsigned char)(c * 255.99f)                                             255.99 x 8 unit(c) + 256 E from the next integer
    0   depth > sky_depth_threshold, depth >= 1e29, max_d > 1e-6, lens_radius > 0, every comparison of object ids: a float32 or
        integer INPUT against a literal or another input, which both precisions evaluate on the same bits
The cell of the taps only counts when a tap is invalid: with all of them valid (the column or row across the near border included)
the blend is continuous across the border and the weights' uncertainty is in the unit.  A chain of tests that short-circuits is
decided as soon as one test decidedly ends it.  An invalid history is decided whatever its taps say (alpha = 1 multiplies them by 0).
Undecidedness PROPAGATES: a pixel of the variance image or of an a-trous pass is decided only if every pixel whose value reaches it
(the 3x3 window; the accepted taps) was.  At most MAX_UNDECIDED = 2 % of the pixels of any (item, frame, k) may be undecided -- a
condition on the ITEMS, asserted from this module alone.  Items marked `threshold` sit on a threshold on purpose: held to the oracle's
bits only and asserted to hold undecided pixels.

UNITS.  A deviation counts in units computed here alone by forward error analysis (class Q): every float32 operation adds
E |result|, inputs carry none, and an uncertainty u travels through the arithmetic to first order (a + b: u_a + u_b; a b: |a| u_b +
|b| u_a; a / b; sqrt(max(v, 0)): sqrt(v + u) - sqrt(v), finite at v = 0).  A weighted mean sum(w c) / sum(w) carries
(sum w u_c + sum |c - mean| u_w) / sum(w) + 3 E sum(w |c|) / sum(w).  Three cancelling expressions lose more than the rounding of their
own result explains; the analysis gives each its term and NAMED_TERMS switches it off to show what it is worth:
    "var"   m2 - mean^2 (neighbourhood variance, history variance, variance estimate x 2): u(m2) + 2 |mean| u(mean) + E mean^2
    "alpha" 1 - alpha: alpha near 1 is known to u(alpha) ABSOLUTE, and so is the weight of the history
    "exp"   exp(-ld^2 inv): the argument's uncertainty times the weight (and E |arg| for the exponential's own argument reduction)
Without "var" the history mean is 221.2 units off and m2 246.2 (plain_moved/131x77, frame 1: a history variance of nearly 0 under
tau = 0.11, where alpha hangs on sqrt(m2 - mean^2)); without "alpha" m2 is 72.8 units off and the mean 4.65 (same frame).  "exp" is
worth nothing at sigma_luminance >= 1.5, where the argument stays below 0.1: 0.575 instead of 0.573 after one pass (WITHOUT_TERMS).
Measured on the CPU, oracle against this module (python tests/post_truth.py prints it; tests/test_post_truth.py re-measures and
asserts each figure); TOL = 4 x the maximum, the convention of brute_force.py, and the GPU test uses the same table:

    quantity                      largest deviation (units)   attained by
    motion vector (u, v)          0.141                       plain/131x77, frame 1
    history mean                  0.315                       plain_moved/131x77, frame 1
    history m2                    0.497                       sky/96x64, frame 1
    history length                0.308                       plain/131x77, frame 2
    output after 0 passes         0.315                       plain_moved/131x77, frame 1   (the history mean)
    output after 1 pass           0.573                       plain/96x64, frame 2
    output after 2 passes         0.286                       sky/96x64, frame 1
    output after 3 passes         0.172                       plain_moved/131x77, frame 0
    output after 4 passes         0.153                       plain/131x77, frame 2
    output after 5 passes         0.133                       self_rejecting/7x5, frame 1
    bloom                         0.494                       spots, 640x360
    up-scale                      0.144                       64x64 -> 65x67
    tonemap before quantisation   0.272                       the bloomed spots image, 640x360
    RGB8                          equal on every decided byte, within 1 elsewhere
    undecided, most of any (item, frame, k) outside the threshold items: none

ITEMS.  G-buffers are built, not rendered: depths of a fronto-parallel plane seen through a narrow pinhole (tan(fov/2) = 0.02, so a
plane's depth varies by 0.06 % over the frame) at view depths 4 and 5; normals from {(0,0,1), (0,0.6,0.8), (0.5,0.5,0), 0}; object
ids in blocks; colours seeded uniforms with a few 40.0 spikes.  Motion comes from the camera: the previous
view-projection is the current one composed with a translation, which shifts a plane's image by a chosen amount (`view_proj`).  A
STATIC frame runs with the motion vectors off (exactly 0, `pvp = None`): vectors computed for an unmoved camera are rounding noise of
1e-8, which puts every reprojected position within an ulp of a cell border.  The moving frames shift by (+2.25, -1.75) px: a shift of
-1.5 rows puts floor(prev_v) of `nearest` on a row border for every pixel.  Both excluded cases run on the GPU against the oracle's
bits (tests/test_post_truth_gpu.py).  See ITEMS below for the list.
"""
import numpy as np


def F(x):
    return float(np.float32(x))


EPS32 = 2.0 ** -23
MAX_UNDECIDED = 0.02
NAMED_TERMS = {"var": True, "alpha": True, "exp": True}
MISREADINGS = ("atrous_kernel_1242", "luminance_rb", "boost_1", "taps_12", "alpha_1_over_len", "clamp_invalid", "clamp_never",
               "knee_1", "up_true_size", "gamma_22", "scale_255")
INT_MAX = 2 ** 31 - 1

# quantity -> (item that attains the largest deviation of the oracle from the statement, that deviation in units)
MEASURED = dict(motion=("plain/131x77 f1", 0.141), hmean=("plain_moved/131x77 f1", 0.315), hm2=("sky/96x64 f1", 0.497),
                hlen=("plain/131x77 f2", 0.308), out0=("plain_moved/131x77 f1", 0.315), out1=("plain/96x64 f2", 0.573),
                out2=("sky/96x64 f1", 0.286), out3=("plain_moved/131x77 f0", 0.172), out4=("plain/131x77 f2", 0.153),
                out5=("self_rejecting/7x5 f1", 0.133), bloom=("spots 640x360", 0.494), upscale=("64x64->65x67", 0.144),
                tonemap=("bloomed spots 640x360", 0.272))
TOL = {q: 4 * v for q, (_, v) in MEASURED.items()}
# the same measurement with one named term switched off: (term, item, quantity) -> units; tests/test_post_truth.py re-measures
WITHOUT_TERMS = {("var", "plain_moved/131x77", "hmean"): 221.2, ("var", "plain_moved/131x77", "hm2"): 246.2,
                 ("alpha", "plain_moved/131x77", "hm2"): 72.85, ("alpha", "plain_moved/131x77", "hmean"): 4.646,
                 ("exp", "plain/96x64", "out1"): 0.575}


# ---------------------------------------------------------------------------------------------------- forward error analysis
class Q:
    """A float64 value with the uncertainty a float32 evaluation of the same expression carries (first order, see UNITS)."""
    __slots__ = ("v", "u")

    def __init__(self, v, u=0.0):
        self.v = np.asarray(v, np.float64)
        self.u = np.array(np.broadcast_to(np.asarray(u, np.float64), self.v.shape))

    def __getitem__(self, i):
        return Q(self.v[i], self.u[i])

    def __add__(a, b):
        b = q_(b)
        v = a.v + b.v
        return Q(v, a.u + b.u + EPS32 * np.abs(v))

    def __sub__(a, b):
        b = q_(b)
        v = a.v - b.v
        return Q(v, a.u + b.u + EPS32 * np.abs(v))

    def __mul__(a, b):
        b = q_(b)
        v = a.v * b.v
        return Q(v, np.abs(a.v) * b.u + np.abs(b.v) * a.u + EPS32 * np.abs(v))

    def __truediv__(a, b):
        b = q_(b)
        v = a.v / b.v
        return Q(v, a.u / np.abs(b.v) + np.abs(v / b.v) * b.u + EPS32 * np.abs(v))

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(a, b):
        return q_(b) - a

    def __rtruediv__(a, b):
        return q_(b) / a

    def __neg__(a):
        return Q(-a.v, a.u)

    def abs(a):
        return Q(np.abs(a.v), a.u)

    def sqrt0(a):
        """sqrtf of a value that was clamped at 0 from below."""
        v = np.maximum(a.v, 0.0)
        r = np.sqrt(v)
        return Q(r, np.sqrt(v + a.u) - r + EPS32 * r)

    def exact(a):
        """The same value as an INPUT (no uncertainty): what NAMED_TERMS switches a term off with."""
        return Q(a.v, 0.0)


def q_(x):
    return x if isinstance(x, Q) else Q(x)


def qmax(a, b):
    """fmaxf: the larger operand's uncertainty where the order is certain, the larger uncertainty where it is not."""
    a, b = q_(a), q_(b)
    gap = a.v - b.v
    return Q(np.maximum(a.v, b.v), np.where(gap > a.u + b.u, a.u, np.where(-gap > a.u + b.u, b.u, np.maximum(a.u, b.u))))


def qmin(a, b):
    a, b = q_(a), q_(b)
    gap = a.v - b.v
    return Q(np.minimum(a.v, b.v), np.where(gap > a.u + b.u, b.u, np.where(-gap > a.u + b.u, a.u, np.maximum(a.u, b.u))))


def qwhere(c, a, b):
    a, b = q_(a), q_(b)
    return Q(np.where(c, a.v, b.v), np.where(c, a.u, b.u))


def qsum3(a):
    return a[..., 0] + a[..., 1] + a[..., 2]


def sub_named(a, b, name):
    """a - b of a cancelling expression: with the term switched off only the result's own rounding counts."""
    return a - b if NAMED_TERMS[name] else Q((a - b).v, EPS32 * np.abs(a.v - b.v))


# ---------------------------------------------------------------------------------------------------- settings
FIELDS = ("tau", "min_alpha", "max_history", "sigma_luminance", "sigma_normal", "sigma_depth", "atrous_iterations", "clamp_scale",
          "firefly_threshold", "depth_reject_absolute", "depth_reject_relative", "normal_reject_threshold", "sky_depth_threshold",
          "edge_depth_threshold", "edge_normal_threshold", "use_object_ids", "enable_firefly_suppression")
INT_FIELDS = ("atrous_iterations", "use_object_ids", "enable_firefly_suppression")


def settings(**kw):
    """DenoiserSettings, the diffuse_* channel the non-split path passes on (rendering/denoiser.cuh:40-71, :1041-1049)."""
    s = dict(tau=0.06, min_alpha=0.05, max_history=32.0, sigma_luminance=4.0, sigma_normal=64.0, sigma_depth=0.5,
             atrous_iterations=5, clamp_scale=1.2, firefly_threshold=3.0, depth_reject_absolute=0.1, depth_reject_relative=0.005,
             normal_reject_threshold=0.95, sky_depth_threshold=1e9, edge_depth_threshold=0.01, edge_normal_threshold=0.95,
             use_object_ids=1, enable_firefly_suppression=1)
    s.update(kw)
    return {k: (int(v) if k in INT_FIELDS else F(v)) for k, v in s.items()}


def atrous_passes(s):
    """`mini(atrous_iters, 5)` and a loop that a negative count never enters (denoiser.cuh:948-950)."""
    return max(0, min(int(s["atrous_iterations"]), 5))


# ---------------------------------------------------------------------------------------------------- pixel helpers
def shifted(a, dx, dy):
    """a[clamp(y + dy), clamp(x + dx)] over the frame (clamp_int, denoiser.cuh:136-138)."""
    H, W = a.shape[:2]
    return a[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def qshifted(a, dx, dy):
    return Q(shifted(a.v, dx, dy), shifted(a.u, dx, dy))


def inside(H, W, dx, dy):
    y, x = np.mgrid[0:H, 0:W]
    return (x + dx >= 0) & (x + dx < W) & (y + dy >= 0) & (y + dy < H)


def dot_margin(a, b):
    return 2 * EPS32 * np.abs(a * b).sum(-1)


def is_sky(depth, normal, s):
    """denoiser.cuh:119-122 -> (sky, decided)."""
    nn = (normal * normal).sum(-1)
    far = depth > s["sky_depth_threshold"]
    return far | (nn < F(0.1)), far | ~(np.abs(nn - F(0.1)) < dot_margin(normal, normal))


def edge_disc(d0, d1, n0, n1, o0, o1, s, use_obj):
    """is_edge_discontinuity, denoiser.cuh:195-216 -> (discontinuity, decided)."""
    ids = (o0 != o1) & (o0 >= 0) & (o1 >= 0) if use_obj else np.zeros(np.broadcast(d0, d1).shape, bool)
    max_d = np.maximum(d0, d1)
    guard = max_d > F(1e-6)
    qd = np.abs(d0 - d1) / np.where(guard, max_d, 1.0)
    dfar = guard & (qd > s["edge_depth_threshold"])
    dnear = guard & (np.abs(qd - s["edge_depth_threshold"]) < 2 * EPS32 * qd)
    nd = (n0 * n1).sum(-1)
    nrej = nd < s["edge_normal_threshold"]
    nnear = np.abs(nd - s["edge_normal_threshold"]) < dot_margin(n0, n1)
    return ids | dfar | nrej, ids | (dfar & ~dnear) | (nrej & ~nnear) | (~dnear & ~nnear)


def luminance(c, mis=()):
    """denoiser.cuh:108-110."""
    r, b = (2, 0) if "luminance_rb" in mis else (0, 2)
    return F(0.2126) * c[..., r] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., b]


# ---------------------------------------------------------------------------------------------------- motion vectors
def unit_disk_hash(x, y):
    """Camera::random_in_unit_disk_hash, scene/camera.cuh:55-72: exact uint32 arithmetic -> (r1, r2)."""
    m = np.uint64(0xFFFFFFFF)
    x, y = x.astype(np.uint64), y.astype(np.uint64)
    seed = ((x * np.uint64(1973)) & m) ^ ((y * np.uint64(9277)) & m) ^ np.uint64(0x9e3779b9)
    for sh, mul in ((17, 0xed5ad4bb), (11, 0xac4c1b51), (15, 0x31848bab)):
        seed ^= seed >> np.uint64(sh)
        seed = (seed * np.uint64(mul)) & m
    seed ^= seed >> np.uint64(14)
    r1 = ((seed & np.uint64(0xFFFF)).astype(np.float64) + 0.5) / 65536.0
    r2 = ((((seed * np.uint64(0x343fd) + np.uint64(0xc0f5)) & m) & np.uint64(0xFFFF)).astype(np.float64) + 0.5) / 65536.0
    return r1, r2


def motion_vectors(depth, cam, pvp):
    """motion_vector_kernel, rendering/denoiser_kernels.cuh:33-68, with Camera::get_ray(s, t) of the device
    (scene/camera.cuh:173-185, :201-205) -> (Q (H, W, 2), decided).  `cam`: dict of float32 origin, lower_left_corner, horizontal,
    vertical, u, v (3 each) and lens_radius; `pvp`: 16 floats, column-major (common/mat4.cuh:270-275)."""
    H, W = depth.shape
    d = depth.astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    u, v = Q(x + 0.5) / float(W), Q(y + 0.5) / float(H)
    s, t = u, 1.0 - v
    vec = {k: np.asarray(cam[k], np.float32).astype(np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical",
                                                                          "u", "v")}
    decided = np.ones((H, W), bool)
    org = [Q(np.full((H, W), vec["origin"][i])) for i in range(3)]
    rd = [Q(vec["lower_left_corner"][i]) + s * vec["horizontal"][i] + t * vec["vertical"][i] - vec["origin"][i] for i in range(3)]
    lens = F(cam["lens_radius"])
    if lens > 0:
        trunc = []
        for val, k in ((s, 10000.0), (t, 5000.0), (t, 10000.0), (s, 5000.0)):
            p = val.v * k
            trunc.append(np.floor(p))
            decided &= np.abs(p - np.round(p)) > 2 * EPS32 * k
        r1, r2 = unit_disk_hash(trunc[0] + trunc[1], trunc[2] + trunc[3])
        r = Q(r1).sqrt0()
        phi = Q(r2) * F(6.2831853)
        cs, sn = Q(np.cos(phi.v), phi.u + EPS32), Q(np.sin(phi.v), phi.u + EPS32)
        disk = (r * cs * lens, r * sn * lens)                           # lens_radius * random_in_unit_disk_hash
        off = [disk[0] * vec["u"][i] + disk[1] * vec["v"][i] for i in range(3)]
        rd = [rd[i] - off[i] for i in range(3)]
        org = [org[i] + off[i] for i in range(3)]
    ln = (rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]).sqrt0()        # vec3::normalized
    wp = [org[i] + rd[i] / ln * d for i in range(3)]
    m = np.asarray(pvp, np.float32).astype(np.float64)
    cx = wp[0] * m[0] + wp[1] * m[4] + wp[2] * m[8] + m[12]
    cy = wp[0] * m[1] + wp[1] * m[5] + wp[2] * m[9] + m[13]
    cw = wp[0] * m[3] + wp[1] * m[7] + wp[2] * m[11] + m[15]
    prev_u = (cx / cw + 1.0) * 0.5
    prev_v = (1.0 - cy / cw) * 0.5
    mx, my = u - prev_u, v - prev_v
    zero = d >= F(1e29)                                                 # DENOISER_SKY_DEPTH_THRESHOLD: an input against a literal
    out = Q(np.stack([np.where(zero, 0.0, mx.v), np.where(zero, 0.0, my.v)], -1),
            np.stack([np.where(zero, 0.0, mx.u), np.where(zero, 0.0, my.u)], -1))
    return out, decided | zero


# ---------------------------------------------------------------------------------------------------- denoiser stages
def firefly(color, depth, normal, s):
    """firefly_suppression_kernel, denoiser.cuh:376-424 (or the copy, :901-905) -> (Q image, decided)."""
    H, W = depth.shape
    c = Q(color)
    if not s["enable_firefly_suppression"]:
        return c, np.ones((H, W), bool)
    sky, sky_dec = is_sky(depth, normal, s)
    mx = np.zeros_like(color)
    any_n = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ins = inside(H, W, dx, dy)
            mx = np.where(ins[..., None], np.maximum(mx, shifted(color, dx, dy)), mx)
            any_n |= ins
    cl = qmin(qmin(c, Q(mx) * F(1.25)), F(10.0))                        # relaxation and MAX_RADIANCE are literals: the setting is ignored
    return qwhere((sky | ~any_n)[..., None], c, cl), sky_dec


def temporal(cur, depth, normal, obj, mv, hist, s, mis=()):
    """temporal_accumulation_kernel, denoiser.cuh:426-584, with edge_aware_bilinear_sample_* (:225-374) and nearest_sample_int
    (:218-223), snapshot semantics.  `hist` = dict(mean, m2, len (Q or arrays), normal, depth, obj) of the frame before.
    -> dict(mean, m2, len: Q; decided; valid; taps_valid (count of valid taps, -1 where none were read))."""
    H, W = depth.shape
    use_obj = bool(s["use_object_ids"]) and obj is not None and hist["obj"] is not None   # :440-441
    o = obj if use_obj else np.full((H, W), -1)
    sky, sky_dec = is_sky(depth, normal, s)
    # 3x3 neighbourhood statistics of the surface the pixel lies on (:461-506)
    nmean, nm2 = Q(np.zeros((H, W, 3))), Q(np.zeros((H, W, 3)))
    ncount = np.zeros((H, W))
    nb_dec = np.ones((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            disc, dec = edge_disc(depth, shifted(depth, dx, dy), normal, shifted(normal, dx, dy), o, shifted(o, dx, dy), s, use_obj)
            nc = qshifted(cur, dx, dy)
            same = (~disc)[..., None]
            nmean = qwhere(same, nmean + nc, nmean)
            nm2 = qwhere(same, nm2 + nc * nc, nm2)
            ncount += ~disc
            nb_dec &= dec
    none = (ncount == 0)[..., None]
    nmean, nm2 = qwhere(none, cur, nmean), qwhere(none, cur * cur, nm2)
    inv_n = (1.0 / Q(np.maximum(ncount, 1.0)))[..., None]
    nmean, nm2 = nmean * inv_n, nm2 * inv_n
    nstd = qmax(sub_named(nm2, nmean * nmean, "var"), 0.0).sqrt0()
    soft_min, soft_max = nmean - nstd * s["clamp_scale"], nmean + nstd * s["clamp_scale"]
    # reprojection (:508-516)
    y, x = np.mgrid[0:H, 0:W]
    mvx, mvy = mv[..., 0].astype(np.float64), mv[..., 1].astype(np.float64)
    pu, pv = x + 0.5 - mvx * W, y + 0.5 - mvy * H
    du = np.where(mvx == 0, 0.0, EPS32 * (np.abs(mvx * W) + np.abs(pu)))
    dv = np.where(mvy == 0, 0.0, EPS32 * (np.abs(mvy * H) + np.abs(pv)))
    on = ~((pu < 0.5) | (pv < 0.5) | (pu >= W - 0.5) | (pv >= H - 0.5))
    on_dec = ~((np.abs(pu - 0.5) < du) | (np.abs(pu - (W - 0.5)) < du) | (np.abs(pv - 0.5) < dv) | (np.abs(pv - (H - 0.5)) < dv))
    # the four taps (:232-281); validity of the 4 x 4 block around them, for the cell decision
    fx, fy = pu - 0.5, pv - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    sx = Q(fx - x0, np.where(mvx == 0, 0.0, du + EPS32 * np.abs(fx)))   # x + 0.5 - 0 - 0.5 - x0 is exact in float32
    sy = Q(fy - y0, np.where(mvy == 0, 0.0, dv + EPS32 * np.abs(fy)))
    hd, hn, ho = hist["depth"].astype(np.float64), hist["normal"].astype(np.float64), hist["obj"]

    def at(ix, iy):
        return (np.clip(iy, 0, H - 1).astype(int), np.clip(ix, 0, W - 1).astype(int))

    tap_ok, tap_dec = {}, {}
    for j in (-1, 0, 1, 2):
        for i in (-1, 0, 1, 2):
            k = at(x0 + i, y0 + j)
            disc, dec = edge_disc(depth, hd[k], normal, hn[k], o, ho[k] if use_obj else o, s, use_obj)
            tap_ok[i, j], tap_dec[i, j] = ~disc, dec
    near = {(-1, 0): sx.v < sx.u, (2, 0): 1.0 - sx.v < sx.u, (0, -1): sy.v < sy.u, (0, 2): 1.0 - sy.v < sy.u}
    cell_dec = np.ones((H, W), bool)
    for j in (-1, 0, 1, 2):
        for i in (-1, 0, 1, 2):
            need = np.ones((H, W), bool)                                # is tap (i, j) one the float32 evaluation may read?
            if i in (-1, 2):
                need &= near[i, 0]
            if j in (-1, 2):
                need &= near[0, j]
            cell_dec &= ~need | (tap_ok[i, j] & tap_dec[i, j])
    any_near = near[-1, 0] | near[2, 0] | near[0, -1] | near[0, 2]
    taps = [(0, 0), (1, 0), (0, 1), (1, 1)]
    if "taps_12" in mis:
        wts = [(1.0 - sx) * (1.0 - sy), (1.0 - sx) * sy, sx * (1.0 - sy), sx * sy]
    else:
        wts = [(1.0 - sx) * (1.0 - sy), sx * (1.0 - sy), (1.0 - sx) * sy, sx * sy]
    dwx = [-(1.0 - sy.v), (1.0 - sy.v), -sy.v, sy.v]                    # d w_k / d sx, d w_k / d sy
    dwy = [-(1.0 - sx.v), -sx.v, (1.0 - sx.v), sx.v]
    valid4 = [tap_ok[t] for t in taps]
    n_valid = sum(v.astype(int) for v in valid4)
    w = [qwhere(valid4[k], wts[k], 0.0) for k in range(4)]
    total = w[0] + w[1] + w[2] + w[3]
    tw_margin = np.where(n_valid > 0, 2 * sx.u + 2 * sy.u + 4 * EPS32, 0.0)
    small = total.v < F(1e-6)
    sample_dec = (tap_dec[0, 0] & tap_dec[1, 0] & tap_dec[0, 1] & tap_dec[1, 1] & (~any_near | cell_dec) &
                  ~(np.abs(total.v - F(1e-6)) < tw_margin))
    idx = [at(x0 + i, y0 + j) for i, j in taps]
    nearest = at(np.floor(pu), np.floor(pv))
    near_dec = ~((np.abs(pu - np.round(pu)) < du) | (np.abs(pv - np.round(pv)) < dv))
    pick = [np.where(valid4[0], idx[0][a], np.where(valid4[1], idx[1][a], np.where(valid4[2], idx[2][a],
            np.where(valid4[3], idx[3][a], nearest[a])))) for a in (0, 1)]
    pick = (pick[0], pick[1])
    safe_total = Q(np.where(small, 1.0, total.v), total.u)

    def sample(buf):
        """(c00 w00 + c10 w10 + c01 w01 + c11 w11) * (1 / total_w), or the first valid tap, or the nearest texel (:283-298)."""
        buf = q_(buf)
        vec = buf.v.ndim == 3
        ex = (lambda a: a[..., None]) if vec else (lambda a: a)
        cs = [buf[i] for i in idx]
        val = sum(cs[k].v * ex(w[k].v) for k in range(4)) / ex(safe_total.v)
        u_c = sum(cs[k].u * ex(w[k].v) for k in range(4)) / ex(safe_total.v)
        # the weights' share of the unit, correlated through the division: sum |dw_k| |c_k - s| / total_w
        u_w = sum(ex(valid4[k] * (np.abs(dwx[k]) * sx.u + np.abs(dwy[k]) * sy.u + EPS32 * w[k].v)) * np.abs(cs[k].v - val)
                  for k in range(4)) / ex(safe_total.v)
        mag = sum(np.abs(cs[k].v) * ex(w[k].v) for k in range(4)) / ex(safe_total.v)
        out = Q(val, u_c + u_w + 3 * EPS32 * mag)
        return qwhere(ex(small), buf[pick], out)

    h_mean, h_m2, h_len, h_d = sample(hist["mean"]), sample(hist["m2"]), sample(hist["len"]), sample(hd)
    # rejections (:542-560)
    id_fail = (ho[nearest] != o) if use_obj else np.zeros((H, W), bool)
    dad = (Q(depth) - h_d).abs()
    thr_rel = s["depth_reject_relative"] * np.maximum(F(1e-6), depth)
    d_fail = (dad.v > s["depth_reject_absolute"]) | (dad.v > thr_rel)
    d_near = ((np.abs(dad.v - s["depth_reject_absolute"]) < dad.u + EPS32 * s["depth_reject_absolute"]) |
              (np.abs(dad.v - thr_rel) < dad.u + EPS32 * thr_rel))
    ndot = (normal * hn[nearest]).sum(-1)
    n_fail = ndot < s["normal_reject_threshold"]
    n_near = np.abs(ndot - s["normal_reject_threshold"]) < dot_margin(normal, hn[nearest])
    valid = on & ~id_fail & ~d_fail & ~n_fail
    valid_dec = on_dec & (~on | (near_dec & id_fail) | (near_dec & ~n_near & n_fail) | (sample_dec & ~d_near & d_fail) |
                          (near_dec & ~n_near & sample_dec & ~d_near))
    exv = valid[..., None]
    zero3 = np.zeros((H, W, 3))
    h_mean, h_m2 = qwhere(on[..., None], h_mean, zero3), qwhere(on[..., None], h_m2, zero3)
    h_len = qwhere(on, h_len, 0.0)
    clamp_where = np.ones_like(exv) if "clamp_invalid" in mis else (np.zeros_like(exv) if "clamp_never" in mis else exv)
    h_mean = qwhere(clamp_where, qmin(qmax(h_mean, soft_min), soft_max), h_mean)
    # blend factor (:567-579)
    var = qmax(sub_named(h_m2, h_mean * h_mean, "var"), 0.0)
    sd = var.sqrt0()
    std_approx = qsum3(sd) * F(1.0 / 3.0)
    variance_alpha = std_approx / (std_approx + s["tau"])
    history_alpha = 1.0 / (qmax(h_len, 1e-30) if "alpha_1_over_len" in mis else h_len + 1.0)
    alpha = qwhere(valid, qmin(qmax(qmax(variance_alpha, history_alpha), s["min_alpha"]), 1.0), 1.0)
    new_len = qwhere(valid, qmin(h_len + 1.0, s["max_history"]), 1.0)
    one_m = sub_named(Q(1.0), alpha, "alpha")
    a3, o3 = Q(alpha.v[..., None], alpha.u[..., None]), Q(one_m.v[..., None], one_m.u[..., None])
    out_mean = h_mean * o3 + cur * a3                                   # (:581-583)
    out_m2 = h_m2 * o3 + (cur * cur) * a3
    # a sky pixel restarts its history (:454-459)
    out_mean, out_m2 = qwhere(sky[..., None], cur, out_mean), qwhere(sky[..., None], cur * cur, out_m2)
    new_len = qwhere(sky, 1.0, new_len)
    decided = sky_dec & (sky | (valid_dec & (nb_dec | ~valid)))
    return dict(mean=out_mean, m2=out_m2, len=new_len, decided=decided, valid=valid & ~sky,
                taps_valid=np.where(on & ~sky, n_valid, -1), on=on & ~sky, ncount=np.where(sky, -1, ncount))


def estimate_variance(c, m2, hlen, depth, normal, obj, s, mis=()):
    """estimate_variance_kernel, denoiser.cuh:586-648 -> Q (H, W).  Decisions: is_sky alone (the id test is exact)."""
    H, W = depth.shape
    use_obj = bool(s["use_object_ids"]) and obj is not None            # :592; settings.use_object_ids as passed at :936-939
    sky, _ = is_sky(depth, normal, s)
    var = qmax(sub_named(m2, c * c, "var"), 0.0)
    reliability = qmin(hlen * F(0.25), 1.0)
    boost = 1.0 + (1.0 - reliability) * (F(1.0) if "boost_1" in mis else F(3.0))
    smean, sm2 = Q(np.zeros((H, W, 3))), Q(np.zeros((H, W, 3)))
    count = np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            take = (shifted(obj, dx, dy) == obj) if use_obj else np.ones((H, W), bool)
            nc = qshifted(c, dx, dy)
            smean = qwhere(take[..., None], smean + nc, smean)
            sm2 = qwhere(take[..., None], sm2 + nc * nc, sm2)
            count += take
    inv = (1.0 / Q(count))[..., None]
    smean, sm2 = smean * inv, sm2 * inv
    svar = qmax(sub_named(sm2, smean * smean, "var"), 0.0)
    cv = qmax(var * Q(boost.v[..., None], boost.u[..., None]), svar)
    out = F(0.2126) * cv[..., 0] + F(0.7152) * cv[..., 1] + F(0.0722) * cv[..., 2]
    return qwhere(sky, 0.0, out)


def window_decided(dec, obj, use_obj):
    """A pixel of the variance image is decided if every pixel of its 3x3 window that it reads was."""
    out = dec.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            take = (shifted(obj, dx, dy) == obj) if use_obj else True
            out &= ~np.asarray(take) | shifted(dec, dx, dy)
    return out


ATROUS_ROW = (1.0, 4.0, 6.0, 4.0, 1.0)                                  # atrous_kernel, denoiser.cuh:140-147: outer product / 256


def atrous_pass(c, var, dec_in, depth, normal, obj, step, s, mis=()):
    """atrous_filter_kernel, denoiser.cuh:650-749, the luminance weight with the TRUE exponential -> (Q colour, Q variance, decided)."""
    H, W = depth.shape
    use_obj = bool(s["use_object_ids"]) and obj is not None            # :658
    row = (1.0, 2.0, 4.0, 2.0, 1.0) if "atrous_kernel_1242" in mis else ATROUS_ROW
    sky, sky_dec = is_sky(depth, normal, s)
    clum = luminance(c, mis)
    var_scale = qmax(var, F(1e-6)).sqrt0()
    asl = s["sigma_luminance"] * (1.0 + var_scale * 2.0)
    inv = 1.0 / (2.0 * asl * asl + F(1e-6))
    dec = sky_dec & dec_in
    taps = []
    tw = Q(np.zeros((H, W)))
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            ox, oy = dx * step, dy * step
            ins = inside(H, W, ox, oy)
            if not ins.any():
                continue
            nobj = shifted(obj, ox, oy) if use_obj else None
            idrej = ((obj != nobj) & (obj >= 0) & (nobj >= 0)) if use_obj else np.zeros((H, W), bool)   # :701-706
            nd, nn = shifted(depth, ox, oy), shifted(normal, ox, oy)
            max_d = np.maximum(depth, nd)
            guard = max_d > F(1e-6)
            qd = np.abs(depth - nd) / np.where(guard, max_d, 1.0)
            far = guard & (qd > s["edge_depth_threshold"])                                              # :710-714
            dnear = guard & (np.abs(qd - s["edge_depth_threshold"]) < 2 * EPS32 * qd)
            ndot = (normal * nn).sum(-1)
            nrej = ndot < s["edge_normal_threshold"]                                                    # :716-721
            nnear = np.abs(ndot - s["edge_normal_threshold"]) < dot_margin(normal, nn)
            nsky, nsky_dec = shifted(sky, ox, oy), shifted(sky_dec, ox, oy)                             # :723-724
            ok = ins & ~idrej & ~far & ~nrej & ~nsky & ~sky
            tap_dec = (~ins | idrej | (far & ~dnear) | (nrej & ~nnear) | (nsky & nsky_dec) | (~dnear & ~nnear & nsky_dec))
            dec &= sky | (tap_dec & (~ok | shifted(dec_in, ox, oy)))
            nc, nv = qshifted(c, ox, oy), qshifted(var, ox, oy)
            ld = (clum - qshifted(clum, ox, oy)).abs()
            arg = ld * ld * inv
            if not NAMED_TERMS["exp"]:
                arg = arg.exact()
            e = np.exp(-arg.v)
            wl = Q(e, e * (arg.u + EPS32 * (1.0 + (np.abs(arg.v) if NAMED_TERMS["exp"] else 0.0))))     # __expf, :731
            wt = wl * (row[dy + 2] * row[dx + 2] / 256.0)
            wt = qwhere(ok, wt, 0.0)
            taps.append((nc, nv, wt))
            tw = tw + wt
    any_ok = tw.v > 0
    small = tw.v < F(1e-6)                                                                              # :741-748
    dec &= sky | ~(any_ok & (np.abs(tw.v - F(1e-6)) < tw.u))
    T = np.where(small, 1.0, tw.v)

    def wmean(k, centre):
        vec = taps[0][k].v.ndim == 3
        ex = (lambda a: a[..., None]) if vec else (lambda a: a)
        val = sum(t[k].v * ex(t[2].v) for t in taps) / ex(T)
        u = (sum(t[k].u * ex(t[2].v) + np.abs(t[k].v - val) * ex(t[2].u) + 3 * EPS32 * np.abs(t[k].v) * ex(t[2].v) for t in taps) /
             ex(T) + EPS32 * np.abs(val))
        return qwhere(ex(small | sky), centre, Q(val, u))

    return wmean(0, c), wmean(1, var), dec


STEPS = (1, 2, 4, 8, 16)                                                # step_sizes, denoiser.cuh:947


def first_history(cur, normal, depth, obj):
    """The first frame's history: d_history_normal / _depth / _objectId are the frame's own (denoiser.cuh:990-1002), history_mean
    is the firefly-filtered frame and init_moments_kernel sets m2 = c * c, length = 1 (:907-913, :751-763)."""
    return dict(mean=cur, m2=cur * cur, len=Q(np.ones(depth.shape)), normal=normal, depth=depth, obj=obj)


def denoise_frame(s, hist, color, normal, depth, obj, mv, mis=()):
    """One Denoiser::denoise, non-split path (denoiser.cuh:973-1065 -> denoiseChannel :884-971) on (H, W[, 3]) arrays.
    `hist`: None on the first frame, else dict(mean, m2, len, normal, depth, obj) float32 of the implementation under test.
    -> dict(hmean, hm2, hlen: Q after the temporal pass, what becomes the next frame's history (:926-934, with this frame's normal,
    depth and ids, :1052-1062); t_decided; out: [Q image after k passes, k = 0..5]; decided: [per k]; temporal's masks)."""
    color, normal, depth = (np.asarray(a, np.float32).astype(np.float64) for a in (color, normal, depth))
    obj = np.asarray(obj).astype(np.int64)
    cur, ff_dec = firefly(color, depth, normal, s)
    if hist is None:
        hist = first_history(cur, normal, depth, obj)
    else:
        hist = dict(hist, obj=np.asarray(hist["obj"]).astype(np.int64))
    T = temporal(cur, depth, normal, obj, np.asarray(mv, np.float32), hist, s, mis)
    use_obj = bool(s["use_object_ids"])
    # a pixel's temporal answer is decided if its own decisions are and the firefly clamp of its window was
    t_dec = T["decided"] & window_decided(ff_dec, obj, False)
    var = estimate_variance(T["mean"], T["m2"], T["len"], depth, normal, obj, s, mis)
    sky, sky_dec = is_sky(depth, normal, s)
    v_dec = sky_dec & (sky | window_decided(t_dec, obj, use_obj))
    out, decided = [T["mean"]], [t_dec]
    c, dec = T["mean"], v_dec & t_dec
    for step in STEPS:
        c, var, dec = atrous_pass(c, var, dec, depth, normal, obj, step, s, mis)
        out.append(c)
        decided.append(dec)
    return dict(hmean=T["mean"], hm2=T["m2"], hlen=T["len"], t_decided=t_dec, out=out, decided=decided, valid=T["valid"],
                taps_valid=T["taps_valid"], on=T["on"], ncount=T["ncount"])


# ---------------------------------------------------------------------------------------------------- bloom
BLUR = (F(0.227027), F(0.316216), F(0.070270))                          # scene/scene_kernels.cuh:309, :337
BLOOM_MIP_LEVELS = 6                                                    # scene/scene.cuh:159


def _view(flat, h, w):
    """The first h*w pixels of a flat buffer as (h, w, 3): what a kernel that indexes y * w + x sees of it."""
    return Q(flat.v[:h * w].reshape(h, w, 3), flat.u[:h * w].reshape(h, w, 3))


def _store(flat, img):
    n = img.v.shape[0] * img.v.shape[1]
    flat.v[:n], flat.u[:n] = img.v.reshape(n, 3), img.u.reshape(n, 3)


def bright_pass(img, mis=()):
    """bloom_bright_pass_kernel, scene_kernels.cuh:283-299, threshold 1.5 and knee 0.5 (scene.cuh:1140-1141)."""
    threshold, knee = F(1.5), F(1.0) if "knee_1" in mis else F(0.5)
    b = qmax(img[..., 0], qmax(img[..., 1], img[..., 2]))
    soft_t = b - threshold + knee
    w = qmin(qmax(soft_t / (2.0 * knee) + 0.5, 0.0), 1.0)
    return img * Q(w.v[..., None], w.u[..., None])


def blur_h(img):
    """bloom_blur_h_kernel, scene_kernels.cuh:301-322."""
    out = img * BLUR[0]
    for i in (1, 2):
        out = out + qshifted(img, -i, 0) * BLUR[i]
        out = out + qshifted(img, i, 0) * BLUR[i]
    return out


def downsample_v(img):
    """bloom_downsample_v_kernel, scene_kernels.cuh:324-349: (in_H / 2, in_W / 2) from rows 2y - 2 .. 2y + 2 of column 2x."""
    H, W = img.v.shape[:2]
    oh, ow = H // 2, W // 2
    out = Q(np.zeros((oh, ow, 3)))
    for j in (-2, -1, 0, 1, 2):
        rows = np.clip(2 * np.arange(oh) + j, 0, H - 1)
        t = Q(img.v[rows][:, 0:2 * ow:2], img.u[rows][:, 0:2 * ow:2])
        out = out + t * BLUR[abs(j)]
    return out


def upsample_add(dst, low):
    """bloom_upsample_add_kernel, scene_kernels.cuh:351-386: dst (2 H_low, 2 W_low) += bilinear(low); lerp is (1 - t) a + t b
    (common/vec3.cuh:155-157).  The taps' fractions are .25 / .75 exactly; float32 knows them to 3 E W_low."""
    hl, wl = low.v.shape[:2]
    hh, wh = 2 * hl, 2 * wl
    ul = Q(np.arange(wh) + 0.5) / float(wh) * float(wl) - 0.5
    vl = Q(np.arange(hh) + 0.5) / float(hh) * float(hl) - 0.5
    x0, y0 = np.floor(ul.v), np.floor(vl.v)
    assert (np.abs(ul.v - np.round(ul.v)) > 0.2).all() and (np.abs(vl.v - np.round(vl.v)) > 0.2).all()   # no floor decision
    uf, vf = Q(ul.v - x0, ul.u)[None, :, None], Q(vl.v - y0, vl.u)[:, None, None]
    x1, y1 = np.minimum(x0 + 1, wl - 1).astype(int), np.minimum(y0 + 1, hl - 1).astype(int)
    x0, y0 = np.maximum(x0, 0).astype(int), np.maximum(y0, 0).astype(int)

    def g(yy, xx):
        return Q(low.v[yy][:, xx], low.u[yy][:, xx])

    def lerp(a, b, t):
        return (1.0 - t) * a + t * b
    bloom = lerp(lerp(g(y0, x0), g(y0, x1), uf), lerp(g(y1, x0), g(y1, x1), uf), vf)
    return dst + bloom


def bloom(image, w, h, mis=()):
    """Step 5 of Scene::render_to_device, scene/scene.cuh:1137-1183, on an (h*w, 3) image -> Q (h*w, 3).  mip_w / mip_h are halved
    on the way down and DOUBLED on the way up (:1172-1177), so where a size was odd the up passes address a mip with the doubled
    size, not the one it was written with; the buffers are flat, and so they are here."""
    img = q_(image)
    img = Q(img.v.reshape(-1, 3).copy(), img.u.reshape(-1, 3).copy())
    n = w * h
    bright = Q(np.zeros((n, 3)))
    _store(bright, bright_pass(_view(img, h, w), mis))
    chain, true_size = [], []
    mw, mh = w, h
    last = bright
    for i in range(BLOOM_MIP_LEVELS):
        nw, nh = mw // 2, mh // 2
        if nw == 0 or nh == 0:
            raise ValueError("a mip level of zero size (the reference reads a NULL mip)")
        level = Q(np.zeros((max(n // 4, nw * nh), 3)))
        _store(level, downsample_v(blur_h(_view(last, mh, mw))))
        chain.append(level)
        true_size.append((nw, nh))
        last, mw, mh = level, nw, nh
    wrong = "up_true_size" in mis

    def add_into(flat, hi_size, low_flat, lo_size, doubled):
        """One bloom_upsample_add_kernel launch.  The reference addresses both buffers with `doubled` (W_low, H_low) and twice
        that; the misreading addresses each with the size it was written with."""
        lw, lh = lo_size if wrong else doubled
        if wrong:
            hi, lo = _view(flat, hi_size[1], hi_size[0]), _view(low_flat, lo_size[1], lo_size[0])
            res = upsample_add(hi[:2 * lh, :2 * lw], lo)
            hi.v[:2 * lh, :2 * lw], hi.u[:2 * lh, :2 * lw] = res.v, res.u
            _store(flat, hi)
        else:
            _store(flat, upsample_add(_view(flat, 2 * lh, 2 * lw), _view(low_flat, lh, lw)))

    for i in range(BLOOM_MIP_LEVELS - 2, -1, -1):
        mw, mh = mw * 2, mh * 2
        add_into(chain[i], true_size[i], chain[i + 1], true_size[i + 1], (mw // 2, mh // 2))
    add_into(img, (w, h), chain[0], true_size[0], (w // 2, h // 2))   # the last add goes INTO the image (:1181-1182)
    return img


# ---------------------------------------------------------------------------------------------------- up-scale and tonemap
def upscale(image, out_w, out_h, in_w, in_h):
    """upscale_bilinear_kernel, scene_kernels.cuh:404-440, on an (in_h*in_w, 3) image -> Q (out_h*out_w, 3).  No decision: the
    blend is continuous across a cell border and the clamp of u, v is continuous."""
    src = q_(image)
    src = Q(src.v.reshape(in_h, in_w, 3), src.u.reshape(in_h, in_w, 3))

    def axis(n_out, n_in):
        c = Q(np.arange(n_out) + 0.5) * float(n_in) / float(n_out) - 0.5
        c = qmax(0.0, qmin(float(n_in - 1), c))
        i0 = np.floor(c.v).astype(int)
        return i0, np.minimum(i0 + 1, n_in - 1), Q(c.v - i0, c.u)
    x0, x1, fx = axis(out_w, in_w)
    y0, y1, fy = axis(out_h, in_h)
    fx, fy = fx[None, :, None], fy[:, None, None]

    def g(yy, xx):
        return Q(src.v[yy][:, xx], src.u[yy][:, xx])
    top = g(y0, x0) * (1.0 - fx) + g(y0, x1) * fx
    bot = g(y1, x0) * (1.0 - fx) + g(y1, x1) * fx
    out = top * (1.0 - fy) + bot * fy
    return Q(out.v.reshape(-1, 3), out.u.reshape(-1, 3))


ACES_IN = [[F(v) for v in r] for r in ((0.59719, 0.35458, 0.04823), (0.07600, 0.90834, 0.01566), (0.02840, 0.13383, 0.83777))]
ACES_OUT = [[F(v) for v in r] for r in ((1.60475, -0.53108, -0.07367), (-0.10208, 1.10813, -0.00605), (-0.00327, -0.07276, 1.07602))]


def _mat3(m, v):
    """mat3 * vec3, rows of the constructor's arguments (common/matrix.cuh:19-38)."""
    return [v[0] * m[i][0] + v[1] * m[i][1] + v[2] * m[i][2] for i in range(3)]


def tonemap(image, mis=()):
    """tonemap_kernel, scene/scene.cuh:2004-2047 with total_samples = 1, aces_tonemap (rendering/render_utils.cuh:77-95), the sRGB
    OETF with the true pow -> (Q value before `* 255.99f` (n, 3), bytes (n, 3), decided (n, 3)), in the image's own row order (the
    kernel writes row H - 1 - y)."""
    c = q_(image)
    c = Q(c.v.reshape(-1, 3), c.u.reshape(-1, 3))
    col = [c[:, i] / 1.0 for i in range(3)]
    a = _mat3(ACES_IN, col)
    num = [x * (x + F(0.0245786)) - F(0.000090537) for x in a]
    den = [x * (F(0.983729) * x + F(0.4329510)) + F(0.238081) for x in a]
    a = [qmin(qmax(n_ / d_, 0.0), 1.0) for n_, d_ in zip(num, den)]
    a = [qmin(qmax(x, 0.0), 1.0) for x in _mat3(ACES_OUT, a)]
    p = 1.0 / 2.2 if "gamma_22" in mis else F(1.0) / F(2.4)
    out, dec, sat = [], [], []
    for x in a:
        lin = x.v <= F(0.0031308)
        safe = np.maximum(x.v, 1e-30)
        pw = safe ** p
        hi = Q(pw, p * pw / safe * x.u + 2 * EPS32 * pw) * F(1.055) - F(0.055)
        pre = qwhere(lin, x * F(12.92), hi)
        sat.append((pre.v - 1.0 > pre.u) | (-pre.v > pre.u) | ((x.v == 0.0) & (x.u == 0.0)))   # clamp(color, 0, 1) decidedly at a bound: exact
        out.append(qmin(qmax(pre, 0.0), 1.0))
        dec.append(~(np.abs(x.v - F(0.0031308)) < 4 * x.u))
    val = Q(np.stack([o.v for o in out], -1), np.stack([o.u for o in out], -1))
    scale = 255.0 if "scale_255" in mis else F(255.99)
    scaled = val.v * scale
    byte = np.floor(scaled).astype(np.int64)
    near = np.minimum(scaled - np.floor(scaled), np.floor(scaled) + 1 - scaled) < scale * 8 * val.u + 256 * EPS32
    return val, byte, np.stack(dec, -1) & (~near | np.stack(sat, -1))


# ---------------------------------------------------------------------------------------------------- judging
def deviation(got, want, mask=None):
    """Largest |got - want| / unit over the (decided) entries -> (units, flat index); (0, -1) when nothing is judged."""
    want = q_(want)
    g = np.asarray(got, np.float64).reshape(want.v.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(np.abs(g - want.v) == 0, 0.0, np.abs(g - want.v) / want.u)
    if mask is not None:
        m = np.broadcast_to(mask[..., None] if mask.ndim < r.ndim else mask, r.shape)
        r = np.where(m, r, 0.0)
    if r.size == 0:
        return 0.0, -1
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i


# ---------------------------------------------------------------------------------------------------- items
TAN_HALF = 0.02


def camera(W, H, lens_radius=0.0, focus=1.0):
    """A pinhole (or thin lens) at the origin looking down -z, as `Camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist)`
    builds one (scene/camera.cuh:95-121) for tan(vfov / 2) = TAN_HALF."""
    vh, vw = 2 * TAN_HALF, 2 * TAN_HALF * W / H
    f32 = lambda *a: tuple(float(np.float32(v)) for v in a)
    return dict(origin=f32(0, 0, 0), horizontal=f32(focus * vw, 0, 0), vertical=f32(0, focus * vh, 0),
                lower_left_corner=f32(-focus * vw / 2, -focus * vh / 2, -focus), u=f32(1, 0, 0), v=f32(0, 1, 0), w=f32(0, 0, 1),
                lens_radius=float(np.float32(lens_radius)))


def view_proj(W, H, shift_px=(0.0, 0.0), z0=4.0):
    """proj * view of the camera above moved so that the image of the plane at view depth z0 was `shift_px` pixels further right /
    down in the previous frame: the temporal pass then reads its history at (x + 0.5 + sx, y + 0.5 + sy).  16 floats, column-major."""
    vh, vw = 2 * TAN_HALF, 2 * TAN_HALF * W / H
    tx, ty = shift_px[0] * vw * z0 / W, -shift_px[1] * vh * z0 / H
    m = np.zeros(16, np.float32)
    m[0], m[5], m[10], m[11] = 2 / vw, 2 / vh, -1.0, -1.0
    m[12], m[13], m[14] = 2 / vw * tx, 2 / vh * ty, -0.2
    return m


def plane_depth(W, H, z):
    """Distance along the pixel's ray to the plane at view depth z (array or scalar), float32."""
    y, x = np.mgrid[0:H, 0:W]
    vh, vw = 2 * TAN_HALF, 2 * TAN_HALF * W / H
    px, py = vw * ((x + 0.5) / W - 0.5), vh * (0.5 - (y + 0.5) / H)
    return (z * np.sqrt(px * px + py * py + 1.0)).astype(np.float32)


N_UP, N_TILT, N_HALF, N_ZERO = (0, 0, 1), (0, 0.6, 0.8), (0.5, 0.5, 0), (0, 0, 0)


def colours(W, H, seed, spikes=3):
    rs = np.random.RandomState(seed)
    c = rs.uniform(0.05, 1.0, (H, W, 3)).astype(np.float32)
    for _ in range(min(spikes, W * H // 8)):
        c[rs.randint(H), rs.randint(W)] = 40.0
    return c


def _frame(W, H, seed, z, normal, obj, pvp=None, lens=0.0, focus=1.0):
    """One frame of an item: colour, G-buffers, camera, and `pvp` (previous view-projection) or None for `mv0` (vectors off)."""
    z = np.broadcast_to(np.asarray(z, np.float64), (H, W))
    n = np.broadcast_to(np.asarray(normal, np.float32), (H, W, 3)).copy()
    depth = np.where(z >= 1e29, z, plane_depth(W, H, np.where(z >= 1e29, 1.0, z))).astype(np.float32)
    return dict(color=colours(W, H, seed), normal=n, depth=depth, obj=np.broadcast_to(np.asarray(obj, np.int32), (H, W)).copy(),
                cam=camera(W, H, lens, focus), pvp=pvp)


def blocks(W, H, size, values):
    y, x = np.mgrid[0:H, 0:W]
    return np.asarray(values)[(x // size + 3 * (y // size)) % len(values)]


SHIFT, PUSH = (2.25, -1.75), (-5.75, 3.25)


def plain(W, H, lens=0.0, **kw):
    """Static, a shift of (+2.25, -1.5) px, a shift that pushes the left and bottom strips off screen.  Ids in blocks
    of 16, two depth planes and a tilted normal in blocks of 24."""
    obj = blocks(W, H, 16, (0, 1, 2, 3, 4))
    z = np.where(blocks(W, H, 24, (0, 0, 1, 0)) == 1, 5.0, 4.0)
    nrm = np.where((blocks(W, H, 24, (0, 1, 0, 0, 0)) == 1)[..., None], np.float32(N_TILT), np.float32(N_UP))
    focus = 4.08 if lens > 0 else 1.0
    pv = [None, view_proj(W, H, SHIFT), view_proj(W, H, PUSH)]
    if lens > 0:                                                        # (a lens needs its vectors: the static frames keep the camera's)
        pv = [view_proj(W, H), view_proj(W, H, SHIFT), view_proj(W, H, PUSH)]
    return dict(W=W, H=H, settings=settings(**kw), frames=[_frame(W, H, 100 + f, z, nrm, obj, p, lens, focus) for f, p in enumerate(pv)])


def checkerboard(W, H, cell, ids):
    """Ids on a board of `cell`-pixel squares, one depth, one normal: in the 1-px board only the centre of a 3x3 window has the
    centre's id.  Static, shifted by (+2.25, -1.5), shifted by (0.25, 0.25)."""
    y, x = np.mgrid[0:H, 0:W]
    obj = np.asarray(ids, np.int64)[(x // cell) % 2 + 2 * ((y // cell) % 2)]   # four ids: no two squares that touch share one
    pv = [None, view_proj(W, H, SHIFT), view_proj(W, H, (0.25, 0.25))]
    return dict(W=W, H=H, settings=settings(), frames=[_frame(W, H, 200 + f, 4.0, N_UP, obj, p) for f, p in enumerate(pv)])


def island(W, H, ids):
    """3x3 islands of one id whose centre pixel has an id of its own, on a background id."""
    y, x = np.mgrid[0:H, 0:W]
    obj = np.full((H, W), ids[0], np.int64)
    isl = ((x % 6) < 3) & ((y % 5) < 3) & (x // 6 * 6 + 3 <= W) & (y // 5 * 5 + 3 <= H)
    obj[isl] = ids[1]
    obj[isl & (x % 6 == 1) & (y % 5 == 1)] = ids[2]
    pv = [None, view_proj(W, H, (0.25, 0.25)), view_proj(W, H, SHIFT)]
    return dict(W=W, H=H, settings=settings(), frames=[_frame(W, H, 300 + f, 4.0, N_UP, obj, p) for f, p in enumerate(pv)])


def steps_and_creases(W, H):
    """A depth step (4 | 5) along one diagonal and a normal crease along the other, one id: the taps of a moved frame straddle
    them.  Every frame moves, the first included, so its taps (into the frame's own G-buffer) straddle too."""
    y, x = np.mgrid[0:H, 0:W]
    z = np.where(x * H > y * W, 5.0, 4.0)
    nrm = np.where(((W - 1 - x) * H > y * W)[..., None], np.float32(N_TILT), np.float32(N_UP))
    pv = [view_proj(W, H, SHIFT), view_proj(W, H, (-1.375, 0.75)), view_proj(W, H, (0.875, 2.375))]
    return dict(W=W, H=H, settings=settings(), frames=[_frame(W, H, 400 + f, z, nrm, 0, p) for f, p in enumerate(pv)])


def sky_item(W, H):
    """Sky blocks (depth 1e30; a zero normal at a finite depth) beside surface, pixels that turn from sky to surface and back
    between frames, and depth exactly 1e29 (no motion vector) beside 0.99e29 (one)."""
    frames = []
    for f in range(3):
        b = blocks(W, H, 8, (0, 1, 0, 2, 0, 0, 3, 4))
        b = np.roll(b, 8 * f, axis=1)                                   # the blocks move: sky <-> surface
        z = np.where(b == 1, 1e30, np.where(b == 3, 1e29, np.where(b == 4, float(np.float32(0.99e29)), 4.0)))
        nrm = np.where((b == 2)[..., None], np.float32(N_ZERO), np.float32(N_UP))
        fr = _frame(W, H, 500 + f, 4.0, nrm, (b > 0).astype(np.int32), view_proj(W, H, (0.25, 0.25)) if f else None)
        fr["depth"] = np.where(z >= 0.9e29, z, fr["depth"]).astype(np.float32)
        frames.append(fr)
    return dict(W=W, H=H, settings=settings(), frames=frames)


def self_rejecting(W, H):
    """|n|^2 = 0.5: not sky (>= 0.1), yet dot(n, n) < edge_normal_threshold, so the pixel fails the edge rule against ITSELF: no
    neighbour and no tap is ever accepted, the centre included, and every pass hands the pixel through.  A block, and lone pixels."""
    y, x = np.mgrid[0:H, 0:W]
    half = ((x >= 3) & (x < 3 + min(9, W // 3)) & (y >= 1) & (y < 1 + min(6, H // 2))) | ((x % 11 == 7) & (y % 7 == 5))
    nrm = np.where(half[..., None], np.float32(N_HALF), np.float32(N_UP))
    pv = [None, view_proj(W, H, (0.25, 0.25)), view_proj(W, H, SHIFT)]
    it = dict(W=W, H=H, settings=settings(), frames=[_frame(W, H, 600 + f, 4.0, nrm, 0, p) for f, p in enumerate(pv)])
    it["half"] = half
    return it


def unsure_pairs(thr):
    """{ulps: (d0, d1)}: float32 pairs whose float32 quotient fl(fl(d1 - d0) / d1) is exactly `ulps` float32 steps from the
    float32 `thr`, for ulps in 0, +-1, +-2, +-4 (searched over d0 = 1 + j 2^-23: with d0 = 1.0 alone one step of d1 moves the
    quotient by 128 of its own ulps) and about 2^20 steps to either side; and under "d0=1" the four neighbours of the d1 nearest
    to the threshold for d0 = 1.0."""
    thr = np.float32(thr)
    j = np.arange(1 << 16)
    d0 = (np.float32(1.0).view(np.int32) + j.astype(np.int32)).view(np.float32)
    pairs, want = {}, (0, 1, -1, 2, -2, 4, -4)
    for k in (-1, 0, 1):
        near = np.float32(d0.astype(np.float64) / (1.0 - np.float64(thr)))
        d1 = (near.view(np.int32) + np.int32(k)).view(np.float32)
        q = ((d1 - d0).astype(np.float32) / d1).astype(np.float32)
        off = q.view(np.int32).astype(np.int64) - int(thr.view(np.int32))
        for w in want:
            hit = np.flatnonzero(off == w)
            if w not in pairs and hit.size:
                pairs[w] = (d0[hit[0]], d1[hit[0]])
    assert set(pairs) == set(want), sorted(pairs)
    for sign in (1, -1):
        q = (thr.view(np.int32) + np.int32(sign * 2 ** 20)).view(np.float32)
        pairs[sign * 2 ** 20] = (np.float32(1.0), np.float32(1.0 / (1.0 - np.float64(q))))
    n1 = np.float32(1.0 / (1.0 - np.float64(thr)))
    pairs["d0=1"] = [(np.float32(1.0), (n1.view(np.int32) + np.int32(k)).view(np.float32)) for k in (0, 1, -1, 2, -2, 4, -4)]
    return pairs


def unsure_band(W, H, big=False):
    """THRESHOLD ITEM.  Rows of a background depth d0 with lone pixels of d1, the pair's float32 quotient (d1 - d0) / d1 exactly at
    the float32 edge_depth_threshold and 1, 2, 4 and 2^20 float32 steps to either side (`unsure_pairs`), and the literal pairs
    (1.0, d1) around the d1 nearest to the threshold; columns 70 apart, so that some 64-lane rows of an a-trous workgroup hold such
    a pair and some do not.  Rows of (0, 0), (+0, -0) and (1e-7, 2e-7) for `max_d > 1e-6`.  `big`: the same pairs scaled by 2^121
    (2.7e36) and 2^125 (4.3e37) -- powers of two, so the quotients are the same bits -- with sky_depth_threshold = 3e38: the
    `!(max_d < 2^120)` leg of the kernel's depth test."""
    s = settings(sky_depth_threshold=3e38) if big else settings()
    pairs = unsure_pairs(s["edge_depth_threshold"])
    rows = [pairs[k] for k in (0, 1, -1, 2, -2, 4, -4, 2 ** 20, -2 ** 20)] + pairs["d0=1"]
    depth = np.ones((H, W), np.float32)
    for r in range(H):
        scale = np.float32(2.0 ** (121 if r < H // 2 else 125)) if big else np.float32(1.0)
        d0, d1 = rows[r % len(rows)]
        depth[r, :] = d0 * scale
        depth[r, 5 + (r % 3)::70] = d1 * scale
    if not big and H >= 12:
        depth[H - 3, :] = 0.0
        depth[H - 2, 0::2], depth[H - 2, 1::2] = 0.0, -0.0
        depth[H - 1, 0::2], depth[H - 1, 1::2] = 1e-7, 2e-7
    fr = []
    for f in range(2):
        fr.append(dict(color=colours(W, H, 700 + f, 0), normal=np.broadcast_to(np.float32(N_UP), (H, W, 3)).copy(), depth=depth.copy(),
                       obj=np.zeros((H, W), np.int32), cam=camera(W, H), pvp=None))
    return dict(W=W, H=H, settings=s, frames=fr, threshold=True)


def moved_settings():
    """Every setting but the switches and the three ignored ones off its default; max_history = 3 is reached by frame 3."""
    return dict(tau=0.11, min_alpha=0.2, max_history=3.0, sigma_luminance=1.5, clamp_scale=2.0, depth_reject_absolute=0.05,
                depth_reject_relative=0.01, normal_reject_threshold=0.7, edge_depth_threshold=0.03, edge_normal_threshold=0.9,
                sky_depth_threshold=1e12)


def ITEMS():
    """name -> item (dict: W, H, settings, frames[, threshold]).  Built on demand; every array is seeded."""
    it = {}
    for W, H in ((131, 77), (96, 64), (1, 1), (7, 5), (63, 3), (64, 4), (65, 17), (129, 33)):
        it[f"plain/{W}x{H}"] = plain(W, H)
    for uo in (0, 1):
        for ff in (0, 1):
            if not (uo and ff):
                it[f"plain_ids{uo}_firefly{ff}/96x64"] = plain(96, 64, use_object_ids=uo, enable_firefly_suppression=ff)
    it["plain_moved/65x17"] = plain(65, 17, **moved_settings())
    it["plain_moved/131x77"] = plain(131, 77, **moved_settings())
    it["checker1/65x17"] = checkerboard(65, 17, 1, (-1, 0, 5, INT_MAX))
    it["checker2/64x4"] = checkerboard(64, 4, 2, (5, INT_MAX, 0, -1))
    it["checker1/129x33"] = checkerboard(129, 33, 1, (0, 5, INT_MAX, 7))
    it["island/7x5"] = island(7, 5, (0, 5, INT_MAX))
    it["island/65x17"] = island(65, 17, (5, -1, 0))
    it["steps_creases/129x33"] = steps_and_creases(129, 33)
    it["steps_creases/63x3"] = steps_and_creases(63, 3)
    it["sky/65x17"] = sky_item(65, 17)
    it["sky/96x64"] = sky_item(96, 64)
    it["self_rejecting/65x17"] = self_rejecting(65, 17)
    it["self_rejecting/7x5"] = self_rejecting(7, 5)
    it["unsure/131x77"] = unsure_band(131, 77)
    it["unsure_big/129x33"] = unsure_band(129, 33, big=True)
    it["thin_lens/96x64"] = plain(96, 64, lens=0.2)
    return it


ATROUS_VARIANTS = (0, 1, 2, 3, 4, 5, 7, -1)                             # atrous_iterations of the plain sequence; 7 -> 5, -1 -> 0
BLOOM_SIZES = ((64, 64), (66, 65), (65, 64), (131, 77), (258, 130), (640, 360))
BLOOM_BEHIND_DENOISER = ((66, 65), (131, 77))
UPSCALES = (((64, 48), (128, 96)), ((70, 64), (200, 120)), ((98, 74), (131, 99)), ((64, 64), (64, 64)), ((64, 64), (65, 67)))


def bloom_images(W, H):
    """A dim floor with 40.0 spots at a corner, on an edge and in the interior; and a constant 2.5 image."""
    rs = np.random.RandomState(W * 1000 + H)
    img = rs.uniform(0.0, 0.45, (H, W, 3)).astype(np.float32)
    img[0:2, 0:2] = 40.0
    img[H // 2:H // 2 + 2, W - 1] = 40.0
    img[H // 3:H // 3 + 3, W // 3:W // 3 + 3] = 40.0
    img[2 * H // 3, 2 * W // 3] = (40.0, 1.0, 0.2)
    return {"spots": img.reshape(-1, 3), "constant": np.full((H * W, 3), 2.5, np.float32)}


def frame_arrays(fr):
    """The flat float32 / int32 arrays of a frame in the layout the oracle and ptrt_post_frame take."""
    return (np.ascontiguousarray(fr["color"].reshape(-1, 3), np.float32), np.ascontiguousarray(fr["normal"].reshape(-1, 3), np.float32),
            np.ascontiguousarray(fr["depth"].reshape(-1), np.float32), np.ascontiguousarray(fr["obj"].reshape(-1), np.int32))


class CameraView:
    """`cam` with the attribute names of ptrt_camera, for oracle.motion_vectors."""

    def __init__(self, cam):
        for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
            setattr(self, k, type("V", (), dict(zip("xyz", cam[k])))())
        self.lens_radius = cam["lens_radius"]


def history_of(dn, W, H):
    """The six history images an oracle.Denoiser holds, as the (H, W[, 3]) arrays `denoise_frame` takes (copies)."""
    return dict(mean=dn.hmean.reshape(H, W, 3).astype(np.float64), m2=dn.hm2.reshape(H, W, 3).astype(np.float64),
                len=dn.hlen.reshape(H, W).astype(np.float64), normal=dn.hnormal.reshape(H, W, 3).copy(),
                depth=dn.hdepth.reshape(H, W).copy(), obj=dn.hobj.reshape(H, W).copy())


# ---------------------------------------------------------------------------------------------------- oracle against the statement
def oracle_frames(O, item, ks=(0, 1, 2, 3, 4, 5), mis=()):
    """The item through oracle.Denoiser (one per k in `ks`, in step) and through the statement, frame by frame.  Yields
    dict(f, mv (oracle, float32), mv_truth (Q or None), mv_decided, T (denoise_frame's answer), outs {k: oracle image}, dn)."""
    W, H, S = item["W"], item["H"], item["settings"]
    dns = {k: O.Denoiser(W, H, O.DenoiserSettings(**dict(S, atrous_iterations=k))) for k in ks}
    for f, fr in enumerate(item["frames"]):
        color, normal, depth, obj = frame_arrays(fr)
        mv_truth = mv_dec = None
        if fr["pvp"] is None:
            mv = np.zeros((W * H, 2), np.float32)
        else:
            mv = O.motion_vectors(depth, W, H, CameraView(fr["cam"]), fr["pvp"])
            mv_truth, mv_dec = motion_vectors(fr["depth"], fr["cam"], fr["pvp"])
        hist = None if f == 0 else history_of(dns[ks[0]], W, H)
        T = denoise_frame(S, hist, fr["color"], fr["normal"], fr["depth"], fr["obj"], mv.reshape(H, W, 2), mis)
        outs = {k: dns[k].denoise(color, normal, depth, mv, obj) for k in ks}
        yield dict(f=f, mv=mv, mv_truth=mv_truth, mv_decided=mv_dec, T=T, outs=outs, dn=dns[ks[0]])


def judge_frame(r, W, H):
    """{quantity: (units, flat index)} of one `oracle_frames` record on decided pixels, and {k: undecided share}."""
    T, dn = r["T"], r["dn"]
    dev = {}
    if r["mv_truth"] is not None:
        dev["motion"] = deviation(r["mv"].reshape(H, W, 2), r["mv_truth"], r["mv_decided"])
    dev["hmean"] = deviation(dn.hmean.reshape(H, W, 3), T["hmean"], T["t_decided"])
    dev["hm2"] = deviation(dn.hm2.reshape(H, W, 3), T["hm2"], T["t_decided"])
    dev["hlen"] = deviation(dn.hlen.reshape(H, W), T["hlen"], T["t_decided"])
    for k, img in r["outs"].items():
        dev[f"out{k}"] = deviation(img.reshape(H, W, 3), T["out"][k], T["decided"][k])
    return dev, {k: 1.0 - float(T["decided"][k].mean()) for k in range(6)}


def measure(O, names=None, verbose=False):
    """The table: {quantity: (units, where)} over every item that is not a threshold item, and {item fN: {k: undecided share}}."""
    best, shares = {}, {}

    def note(qn, units, where):
        if units > best.get(qn, (-1.0, ""))[0]:
            best[qn] = (units, where)
    for name, item in ITEMS().items():
        if names is not None and name not in names:
            continue
        for r in oracle_frames(O, item):
            dev, und = judge_frame(r, item["W"], item["H"])
            shares[f"{name} f{r['f']}"] = und
            if verbose:
                print(f"{name} f{r['f']}: " + " ".join(f"{k}={v[0]:.3f}" for k, v in dev.items()) +
                      f" | undecided k0 {und[0]:.4f} k5 {und[5]:.4f}")
            if not item.get("threshold"):
                for qn, (units, _) in dev.items():
                    note(qn, units, f"{name} f{r['f']}")
    if names is None:
        for (W, H) in BLOOM_SIZES:
            for kind, img in bloom_images(W, H).items():
                want = bloom(img, W, H)
                note("bloom", deviation(O.bloom(img, W, H), want)[0], f"{kind} {W}x{H}")
                val, _, _ = tonemap(want.v.astype(np.float32))
                note("tonemap", deviation(O.tonemap_float(want.v.astype(np.float32)), val)[0], f"bloomed {kind} {W}x{H}")
        for (iw, ih), (ow, oh) in UPSCALES:
            img = bloom_images(iw, ih)["spots"]
            note("upscale", deviation(O.upscale(img, ow, oh, iw, ih), upscale(img, ow, oh, iw, ih))[0], f"{iw}x{ih}->{ow}x{oh}")
    return best, shares


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle
    table, shares = measure(oracle, verbose=True)
    print("\nquantity   largest deviation (units)   attained by")
    for qn in MEASURED:
        print(f"{qn:10s} {table[qn][0]:8.3f}   {table[qn][1]}")
    worst = max(((max(v.values()), k) for k, v in shares.items() if not ITEMS()[k.rsplit(" ", 1)[0]].get("threshold")))
    print(f"undecided, most of any (item, frame, k) outside the threshold items: {worst[0]:.4%} ({worst[1]})")
