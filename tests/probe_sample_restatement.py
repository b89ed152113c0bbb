"""CPU restatement of ptrt_probe_sample / ptrt_query_probe_light (csrc/pt_probe_sample.hip.h, probe_light) for the exact
comparisons of tests/test_probe_sample_gpu.py: numpy float32, operation by operation as include/ptrt.h states the record and
as the kernel's -ffp-contract=off build has it -- every product, sum, difference, quotient and root is one rounded float32
operation.  Vectorised over the points.

For a point P with normal N, the hit's face f and mesh m:
  1. a miss (hit == 0):  {0, 0, 0,  0,  -1, 0,  -1, -1}.
  2. P not finite:  {0, 0, 0,  0,  -1, 0,  f, m}.
  3. per axis  g = (P - origin) / spacing;  g = min(max(g, 0), counts - 1);  i0 = (int)floor(g);  i1 = min(i0 + 1, counts - 1);
     f = g - i0.  cell = i0x + nx * (i0y + ny * i0z).
  4. B_i = K_i * Y_i(N), Y_i with ptrt_query_probes' six-digit constants, K = 39.478418, 26.318945 (x3), 9.869604 (x5).
  5. corners 0..7 (bit 0: i1 on x, bit 1: on y, bit 2: on z), wt = (wx*wy)*wz; wt <= 0: skipped by selection.  TRILINEAR: w = wt.
     VISIBILITY: Q = origin + idx * spacing; Pb = P + bias * N; V = Q - Pb; r = sqrt((Vx*Vx + Vy*Vy) + Vz*Vz); D = r > 0 ? V / r : 0;
     c = (dot(D, N) + 1) * 0.5; wf = c*c + 0.2; var = |mean_sq - mean*mean|; wv = 1 if r <= mean else (ch*ch)*ch with
     ch = var / (var + d*d), d = r - mean; w = wf * wv; w < 0.2: w = w * ((w*w) / 0.04); w = w * wt.  w not > 0: skipped.
     A used corner: E_c = (((0 + B_0 sh[0][c]) + B_1 sh[1][c]) ..), num_c += w * E_c, den += w, bit set in `used`.
  6. den > 0: irradiance = num / den, a channel < 0 replaced by +0, weight = den; else zeros.

`evaluate` is that text once, over a number type: float32 with the six-digit constants is the restatement (`sample`), float64
with the exact constants of ptrt_amd.probes.sh9_basis and COSINE_LOBE the statement it is held against (`statement64`; the
definition's own parameters 0.2f, 0.04f and 0.5f are the same numbers in both).  `margins` bounds the difference."""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24
TRILINEAR, VISIBILITY = 0, 1
MODES = dict(trilinear=TRILINEAR, visibility=VISIBILITY)
LIGHT_DTYPE = np.dtype([("irradiance", "<f4", 3), ("weight", "<f4"), ("cell", "<i4"), ("used", "<i4"), ("face", "<i4"), ("mesh", "<i4")])
PROBE_DTYPE = np.dtype([("sh", "<f4", (9, 3)), ("mean_distance", "<f4"), ("mean_distance_sq", "<f4"), ("hit_fraction", "<f4"),
                        ("reserved", "<f4", 2)])
MISS = np.int32([0, 0, 0, 0, -1, 0, -1, -1])

# the basis constants: six digits in float32 (ptrt_query_probes), exact in float64 (probes.sh9_basis)
Y32 = [F(0.282095), F(0.488603), F(1.092548), F(0.315392), F(0.546274)]
Y64 = [0.5 * math.sqrt(1.0 / math.pi), math.sqrt(3.0 / (4.0 * math.pi)), 0.5 * math.sqrt(15.0 / math.pi), 0.25 * math.sqrt(5.0 / math.pi),
       0.25 * math.sqrt(15.0 / math.pi)]
# 4 pi times the cosine lobe's factors pi, 2 pi / 3, pi / 4 (probes.COSINE_LOBE)
K64 = [4.0 * math.pi * math.pi, 4.0 * math.pi * (2.0 * math.pi / 3.0), 4.0 * math.pi * (math.pi / 4.0)]
K32 = [F(39.478418), F(26.318945), F(9.869604)]
assert [F(k) for k in K64] == K32, "the six-digit K constants are the float64 values rounded once"
BAND = [0, 1, 1, 1, 2, 2, 2, 2, 2]          # coefficient -> band (K's index)
YC = [0, 1, 1, 1, 2, 2, 3, 2, 4]            # coefficient -> basis constant's index
WF_FLOOR, CRUSH, CRUSH_SQ, HALF = F(0.2), F(0.2), F(0.04), F(0.5)


def fields(rows):
    """the (n, 8) int32 rows as LIGHT_DTYPE records"""
    return np.ascontiguousarray(rows, np.int32).view(np.uint8).reshape(-1, 32).view(LIGHT_DTYPE).reshape(-1)


def probe_records(probes):
    """PROBE_DTYPE records from such records or from query_probes' (n, 32) float32 rows"""
    p = np.ascontiguousarray(probes)
    if p.dtype != PROBE_DTYPE:
        p = p.astype(F, copy=False).view(np.uint8).reshape(-1, 128).view(PROBE_DTYPE).reshape(-1)
    return p


def basis(N, T, Y):
    """(n, 9): Y_i(N) in ptrt_query_probes' operation order, in the type T with the constants Y"""
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    c = [T(v) for v in Y]
    return np.stack([np.full_like(x, c[0]), c[1] * y, c[1] * z, c[1] * x, c[2] * (x * y), c[2] * (y * z),
                     c[3] * (T(3.0) * (z * z) - T(1.0)), c[2] * (x * z), c[4] * (x * x - y * y)], axis=1)


def evaluate(points, normals, volume, probes, mode, bias, T=F):
    """The definition's steps 2 to 6 over the number type T for n points; a dict of what the record holds -- irradiance (n, 3),
    weight, cell, used, nocell -- and of what was decided and formed on the way, per corner (n, 8): wt, w, use, the four
    selections (`sel`), E (n, 8, 3), and in VISIBILITY mode the terms `margins` weighs."""
    mode = MODES.get(mode, mode)
    assert mode in (TRILINEAR, VISIBILITY)
    f32 = T is F
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    N = np.ascontiguousarray(normals, F).reshape(-1, 3).astype(T)
    n = len(P)
    rec = probe_records(probes)
    origin, spacing = np.asarray(volume.origin, F).astype(T), np.asarray(volume.spacing, F).astype(T)
    counts = [int(c) for c in volume.counts]
    assert len(rec) == counts[0] * counts[1] * counts[2]
    sh = rec["sh"].astype(T)
    mean_all, msq_all = rec["mean_distance"].astype(T), rec["mean_distance_sq"].astype(T)
    nocell = ~np.isfinite(P).all(axis=1)
    Pt = np.where(nocell[:, None], F(0), P).astype(T)  # (a placeholder where there is no cell: its record is fixed below)
    with np.errstate(all="ignore"):
        i0, i1, fr, g_all = [], [], [], []
        for a in range(3):
            g = (Pt[:, a] - origin[a]) / spacing[a]
            g = np.minimum(np.maximum(g, T(0.0)), T(counts[a] - 1))
            lo = np.floor(g).astype(np.int64)
            i0.append(lo)
            i1.append(np.minimum(lo + 1, counts[a] - 1))
            fr.append(g - lo.astype(T))
            g_all.append(g)
        cell = i0[0] + counts[0] * (i0[1] + counts[1] * i0[2])
        Yb = basis(N, T, Y32 if f32 else Y64)
        K = [T(k) for k in (K32 if f32 else K64)]
        B = np.stack([K[BAND[i]] * Yb[:, i] for i in range(9)], axis=1)
        Pb = Pt + T(bias) * N
        num, den = np.zeros((n, 3), T), np.zeros(n, T)
        used = np.zeros(n, np.int64)
        out = dict(wt=[], w=[], use=[], sel=[], E=[], row=[], r=[], mean=[], var=[], d=[], ch=[], wv=[], wf=[], cs=[], h0=[], idx=[], V=[])
        for c in range(8):
            idx = [(i1 if c >> a & 1 else i0)[a] for a in range(3)]
            wa = [fr[a] if c >> a & 1 else T(1.0) - fr[a] for a in range(3)]
            wt = (wa[0] * wa[1]) * wa[2]
            on = wt > 0
            row = idx[0] + counts[0] * (idx[1] + counts[1] * idx[2])
            sel = [on]
            w = wt
            if mode == VISIBILITY:
                mean, msq = mean_all[row], msq_all[row]
                Q = np.stack([origin[a] + idx[a].astype(T) * spacing[a] for a in range(3)], axis=1)
                V = Q - Pb
                r2 = (V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1]) + V[:, 2] * V[:, 2]
                r = np.sqrt(r2)
                D = np.where((r > 0)[:, None], V / r[:, None], T(0.0))
                cs = (((D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1]) + D[:, 2] * N[:, 2]) + T(1.0)) * T(HALF)
                wf = cs * cs + T(WF_FLOOR)
                var = np.abs(msq - mean * mean)
                near = r <= mean
                d = r - mean
                ch = var / (var + d * d)
                wv = np.where(near, T(1.0), (ch * ch) * ch)
                h0 = wf * wv
                low = h0 < T(CRUSH)
                h = np.where(low, h0 * ((h0 * h0) / T(CRUSH_SQ)), h0)
                w = h * wt
                sel += [near, low]
                for k, v in (("r", r), ("mean", mean), ("var", var), ("d", d), ("ch", ch), ("wv", wv), ("wf", wf), ("cs", cs), ("h0", h0),
                             ("V", V)):
                    out[k].append(v)
            use = on & (w > 0)
            sel.append(use)
            s = sh[row]  # (n, 9, 3)
            E = np.zeros((n, 3), T)
            for i in range(9):
                E = E + B[:, i, None] * s[:, i, :]
            num = np.where(use[:, None], num + w[:, None] * E, num)
            den = np.where(use, den + w, den)
            used |= np.where(use, 1 << c, 0)
            for k, v in (("wt", wt), ("w", w), ("use", use), ("sel", np.stack(sel, axis=1)), ("E", E), ("row", row), ("idx", np.stack(idx, 1))):
                out[k].append(v)
        lit = den > 0
        irr = num / den[:, None]
        irr = np.where(irr < 0, T(0.0), irr)
        irr = np.where(lit[:, None], irr, T(0.0))
        weight = np.where(lit, den, T(0.0))
    res = {k: np.stack(v, axis=1) for k, v in out.items() if v}
    dead = nocell
    res.update(irradiance=np.where(dead[:, None], T(0.0), irr), weight=np.where(dead, T(0.0), weight), cell=np.where(dead, -1, cell),
               used=np.where(dead, 0, used), nocell=nocell, B=B, N=N, g=np.stack(g_all, axis=1), mode=mode)
    return res


def rows_of(ev, face, mesh, hit):
    """(n, 8) int32 rows from evaluate's float32 answer: misses get the miss record"""
    n = len(ev["weight"])
    rows = np.zeros((n, 8), np.int32)
    rows[:, 0:3] = ev["irradiance"].astype(F).view(np.int32)
    rows[:, 3] = ev["weight"].astype(F).view(np.int32)
    rows[:, 4], rows[:, 5] = ev["cell"], ev["used"]
    rows[:, 6], rows[:, 7] = face, mesh
    rows[~np.asarray(hit, bool)] = MISS
    return rows


def sample(points, normals, face, mesh, hit, volume, probes, mode, bias):
    """The definition in numpy float32, operation by operation: (n, 8) int32 rows.  face, mesh: int32 (n,) or scalars (-1 for
    ptrt_probe_sample); hit: nonzero where there is a point at all."""
    n = len(np.asarray(points).reshape(-1, 3))
    hit = np.broadcast_to(np.asarray(hit), (n,)) != 0
    return rows_of(evaluate(points, normals, volume, probes, mode, bias, F), face, mesh, hit)


def sample_hits(hits, volume, probes, mode, bias):
    """`sample` over query_closest's records ((n, 16) int32 rows or HIT_DTYPE records): their point and normal columns"""
    h = np.ascontiguousarray(hits)
    if h.dtype.names is None:
        h = h.view(np.int32).reshape(-1, 16)
        hit, point, normal = h[:, 0], h[:, 2:5].view(F), h[:, 5:8].view(F)
        mesh, face = h[:, 8], h[:, 12]
    else:
        hit, point, normal, mesh, face = h["hit"], h["point"], h["normal"], h["mesh_index"], h["face_index"]
    return sample(point, normal, face, mesh, hit, volume, probes, mode, bias)


def statement64(points, normals, volume, probes, mode, bias):
    """The same text in float64 with the exact basis and lobe constants: evaluate's dict"""
    return evaluate(points, normals, volume, probes, mode, bias, np.float64)


def undecided(e32, e64):
    """(n,) bool: a sample whose cell or whose corner selections (wt > 0, r <= mean, w < 0.2, w > 0) differ between the two
    readings.  Only the selections that reach the result count: those of a corner both readings skip for its wt do not."""
    a, b = e32["sel"], e64["sel"]
    live = a[:, :, 0] | b[:, :, 0]
    diff = (a != b).any(axis=2) & live
    return diff.any(axis=1) | (e32["cell"] != e64["cell"]) | (e32["nocell"] != e64["nocell"])


def margins(e64, volume, probes, bias):
    """Per sample, the bound on |float32 - statement64| of a channel of the irradiance, (n, 3), for samples whose selections
    agree.  Every rounding counts U = 2^-24 relative, first order, and the whole is multiplied by 1.01 for the second-order
    terms, except the one place where first order is not enough -- the division by the weight -- which is bounded outright.
    All magnitudes are the float64 statement's.
      B_i        the constants: the six-digit Y constant's own relative error dY_i = |float32(six digits) - exact| / exact, K's
                 dK (under U / 2: K is the exact value rounded once).  The roundings: Y1..3 one product, Y4, 5, 7 two, B one more;
                 Y6 = c (3 (z z) - 1): 2 U on 3 z^2, one on the difference, absolute, then one product; Y8 = c (x x - y y): U (x^2 +
                 y^2) and one on the difference.  E_B_i = |B_i| (dY_i + dK + (roundings) U) + K c (the absolute inner terms).
      E          nine products and eight sums that round (the first adds to +0): E_E = sum_i E_B_i |sh_i| + 9 U sum_i |B_i sh_i|.
      wt         g = (P - origin) / spacing: 2 U g absolute; the clamp and f = g - floor(g) are exact; 1 - f one more: a factor is
                 off by e_a = 2 U g_a + U, and the product of three factors <= 1 by E_wt = e_x + e_y + e_z + 2 U.
      VISIBILITY Q = origin + idx spacing: U |idx spacing| + U |Q| per component; Pb = P + bias N: U |bias N| + U |Pb|; V = Q - Pb:
                 both and U |V| -- e_V.  r2: sum_a 2 |V_a| e_V_a + 3 U r2; r: e_r = e_r2 / (2 r) + U r.  D = V / r: e_D = e_V / r +
                 |V| e_r / r^2 + U |D|.  c = (dot(D, N) + 1) / 2: e_c = (sum_a e_D_a |N_a| + 3 U sum_a |D_a N_a| + U |dot + 1|) / 2.
                 wf = c c + 0.2: e_wf = 2 c e_c + U c^2 + U wf.  var = |mean_sq - mean mean|: e_var = U mean^2 + U var (the
                 cancellation is in the bound: relative to var it is U (mean^2 + var) / var).  d = r - mean: e_d = e_r + U |d|.
                 s = var + d d: e_s = e_var + 2 |d| e_d + U d^2 + U s.  ch = var / s: e_ch = e_var / s + var e_s / s^2 + U ch.
                 wv = ch^3: e_wv = 3 ch^2 e_ch + 2 U wv (0 where r <= mean: wv is the literal 1).  h0 = wf wv: e_h0 = wf e_wv +
                 wv e_wf + U h0.  Crushed (h0 < 0.2): h = h0^3 / 0.04: e_h = 3 h0^2 e_h0 / 0.04 + 3 U h.  w = h wt: e_w = h E_wt +
                 wt e_h + U w.  (TRILINEAR: h = 1, e_h = 0, no last product: e_w = E_wt.)
      the ratio  With weights w + dw, |dw| <= e_w, the quotient moves by exactly sum_c dw_c (E_c - avg) / den', den' = sum (w +
                 dw) >= den - sum e_w: bounded by sum_c e_w_c |E_c - avg| / (den - sum_c e_w_c), infinite where that is not
                 positive.  To it: the weighted mean of E_E, and the arithmetic of num, den and the quotient -- a product and up to
                 eight sums in num, eight in den, one division: 18 U sum_c w_c |E_c| / den.  The clamp at 0 moves nothing apart."""
    e = e64
    N = np.abs(e["N"])
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    dY = [abs(float(Y32[k]) - Y64[k]) / Y64[k] for k in range(5)]
    dK = [abs(float(K32[k]) - K64[k]) / K64[k] for k in range(3)]
    rounds = [0, 1, 1, 1, 2, 2, 1, 2, 1]  # products outside the inner absolute terms, before the product with K
    inner = [0 * x, 0 * x, 0 * x, 0 * x, 0 * x, 0 * x, 2 * U * 3 * z * z + U * np.abs(3 * z * z - 1), 0 * x,
             U * (x * x + y * y) + U * np.abs(x * x - y * y)]
    B = np.abs(e["B"])
    E_B = np.stack([B[:, i] * (dY[YC[i]] + dK[BAND[i]] + (rounds[i] + (1 if i else 0)) * U) + K64[BAND[i]] * Y64[YC[i]] * inner[i]
                    for i in range(9)], axis=1)
    E_B[:, 0] = B[:, 0] * (dY[0] + dK[0] + U)
    sh = np.abs(probe_records(probes)["sh"].astype(np.float64))
    use = e["use"]
    n = len(use)
    with np.errstate(all="ignore"):
        s = sh[e["row"]]                                       # (n, 8, 9, 3)
        s = np.where(use[:, :, None, None], s, 0.0)            # (what a skipped corner holds reaches nothing)
        E_E = np.einsum("ni,ncik->nck", E_B, s) + 9 * U * np.einsum("ni,ncik->nck", B, s)
        g = e["g"]
        e_a = 2 * U * g + U
        E_wt = e_a.sum(axis=1)[:, None] + 2 * U + 0 * e["wt"]
        wt = e["wt"]
        if e["mode"] == VISIBILITY:
            origin, spacing = np.asarray(volume.origin, F).astype(np.float64), np.asarray(volume.spacing, F).astype(np.float64)
            V = e["V"]                                          # (n, 8, 3)
            step = e["idx"] * spacing[None, None, :]
            Q = origin[None, None, :] + step
            Nn = np.stack([x, y, z], axis=1)[:, None, :]
            Pb = Q - V
            e_V = U * np.abs(step) + U * np.abs(Q) + U * abs(bias) * Nn + U * np.abs(Pb) + U * np.abs(V)
            r = e["r"]
            r2 = r * r
            e_r2 = (2 * np.abs(V) * e_V).sum(axis=2) + 3 * U * r2
            e_r = e_r2 / (2 * r) + U * r
            D = np.abs(V) / r[:, :, None]
            e_D = e_V / r[:, :, None] + np.abs(V) * e_r[:, :, None] / r2[:, :, None] + U * D
            cs = e["cs"]
            e_c = ((e_D * Nn).sum(axis=2) + 3 * U * (D * Nn).sum(axis=2) + U * np.abs(2 * cs)) / 2
            wf = e["wf"]
            e_wf = 2 * cs * e_c + U * cs * cs + U * wf
            mean, var, d, ch, wv, h0 = e["mean"], e["var"], e["d"], e["ch"], e["wv"], e["h0"]
            e_var = U * mean * mean + U * var
            e_d = e_r + U * np.abs(d)
            ssum = var + d * d
            e_s = e_var + 2 * np.abs(d) * e_d + U * d * d + U * ssum
            e_ch = e_var / ssum + var * e_s / (ssum * ssum) + U * ch
            near = e["sel"][:, :, 1]
            e_wv = np.where(near, 0.0, 3 * ch * ch * e_ch + 2 * U * wv)
            e_h0 = wf * e_wv + wv * e_wf + U * h0
            low = e["sel"][:, :, 2]
            h = np.where(low, h0 * h0 * h0 / float(CRUSH_SQ), h0)
            e_h = np.where(low, 3 * h0 * h0 * e_h0 / float(CRUSH_SQ) + 3 * U * h, e_h0)
            e_w = h * E_wt + wt * e_h + U * e["w"]
        else:
            e_w = E_wt
        w = np.where(use, e["w"], 0.0)
        e_w = np.where(use, e_w, 0.0)
        E = np.where(use[:, :, None], e["E"], 0.0)
        den = w.sum(axis=1)
        avg = (w[:, :, None] * E).sum(axis=1) / den[:, None]
        room = den - e_w.sum(axis=1)
        ratio = (e_w[:, :, None] * np.abs(E - avg[:, None, :])).sum(axis=1) / room[:, None]
        ratio = np.where((room > 0)[:, None], ratio, np.inf)
        mean_E = (w[:, :, None] * E_E).sum(axis=1) / den[:, None]
        arith = 18 * U * (w[:, :, None] * np.abs(E)).sum(axis=1) / den[:, None]
        m = 1.01 * (ratio + mean_E + arith)
    return np.where((den > 0)[:, None], m, 0.0)
