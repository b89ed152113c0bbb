"""CPU restatement of ptrt_atlas_sample / ptrt_query_lightmap (csrc/pt_lightmap.hip.h, lightmap_sample) for the exact comparisons
of tests/test_lightmap_sample_gpu.py: numpy float32, operation by operation as include/ptrt.h states the sample and as the
kernel's -ffp-contract=off build has it -- every product, sum, difference and quotient is one rounded float32 operation.
Vectorised over the hit records (HIT_DTYPE, or query_closest's (n, 16) int32 rows).

For one record H:
  1. H.hit == 0:  {0, 0, 0,  0,  0, 0,  -1, -1}.
  2. m = H.mesh_index, f = H.face_index; m outside the table (m < 0 or m >= len(chart_first)), first = chart_first[m] < 0, f < 0
     or first + f >= len(charts):  {0, 0, 0,  0,  0, 0,  f, m}.
  3. (x0, y0, x1, y1, x2, y2) = charts[first + f];  b0 = (1 - H.u) - H.v;  x = (b0*x0 + H.u*x1) + H.v*x2, y likewise;
     x or y not finite:  {0, 0, 0,  0,  x, y,  f, m}.
  4. a tap (i, j) is usable iff it lies in the atlas and image[j, i].valid != 0; unusable taps are skipped BY SELECTION.
       NEAREST   the tap (floor(x), floor(y)): usable, rgb = its three words copied, weight 1; else zeros.
       BILINEAR  tx = x - 0.5, ty = y - 0.5; fi = floor(tx), fj = floor(ty); fx = tx - fi, fy = ty - fj; gx = 1 - fx, gy = 1 - fy;
                 taps (i0, j0) gx*gy, (i0+1, j0) fx*gy, (i0, j0+1) gx*fy, (i0+1, j0+1) fx*fy in that order; a usable tap with
                 w > 0: num += w * rgb, den += w.  den > 0: rgb = num / den, weight = den; else zeros.
     fi or fj outside [-1, 2^28], compared as floats before any conversion: no tap is usable.
  5. {rgb, weight, x, y, f, m}."""
import numpy as np

F = np.float32
NEAREST, BILINEAR = 0, 1
MODES = dict(nearest=NEAREST, bilinear=BILINEAR)
LIMIT = F(2.0 ** 28)
HIT_DTYPE = np.dtype([("hit", "<i4"), ("t", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3), ("mesh_index", "<i4"),
                      ("front_face", "<i4"), ("u", "<f4"), ("v", "<f4"), ("face_index", "<i4"), ("local_point", "<f4", 3)])
SAMPLE_DTYPE = np.dtype([("rgb", "<f4", 3), ("weight", "<f4"), ("x", "<f4"), ("y", "<f4"), ("face", "<i4"), ("mesh", "<i4")])


def hit_records(hits):
    """HIT_DTYPE records from such records or from query_closest's (n, 16) int32 rows"""
    h = np.ascontiguousarray(hits)
    if h.dtype != HIT_DTYPE:
        h = h.view(np.uint8).reshape(-1, 64).view(HIT_DTYPE).reshape(-1)
    return h


def make_hits(mesh, face, u, v, hit=None):
    """HIT_DTYPE records with only the words a sample reads filled in"""
    mesh = np.atleast_1d(np.asarray(mesh, np.int32))
    h = np.zeros(len(mesh), HIT_DTYPE)
    h["mesh_index"], h["face_index"] = mesh, np.asarray(face, np.int32)
    h["u"], h["v"] = np.asarray(u, F), np.asarray(v, F)
    h["hit"] = 1 if hit is None else np.asarray(hit, np.int32)
    return h


def fields(rows):
    """the (n, 8) int32 rows as SAMPLE_DTYPE records"""
    return np.ascontiguousarray(rows, np.int32).view(np.uint8).reshape(-1, 32).view(SAMPLE_DTYPE).reshape(-1)


def sample(hits, charts, chart_first, image, mode):
    """(n, 8) int32 rows, one ptrt_lightmap_sample each: hits as for `hit_records`, charts (F, 6) float32, chart_first (M,)
    int32, image (h, w, 4) float32, mode NEAREST / BILINEAR or its name"""
    mode = MODES.get(mode, mode)
    assert mode in (NEAREST, BILINEAR)
    H = hit_records(hits)
    charts = np.ascontiguousarray(charts, F).reshape(-1, 6)
    chart_first = np.asarray(chart_first, np.int32).reshape(-1)
    image = np.ascontiguousarray(image, F)
    ah, aw, _ = image.shape
    texels = image.reshape(-1, 4)
    words = texels.view(np.int32)
    n = len(H)
    out = np.zeros((n, 8), np.int32)
    out[:, 6:8] = -1
    hit = H["hit"] != 0
    m, f = H["mesh_index"].astype(np.int64), H["face_index"].astype(np.int64)
    out[hit, 6], out[hit, 7] = f[hit], m[hit]
    in_table = hit & (m >= 0) & (m < len(chart_first))
    first = np.where(in_table, chart_first[np.where(in_table, m, 0)], -1).astype(np.int64)
    chart = in_table & (first >= 0) & (f >= 0) & (first + f < len(charts))
    c = charts[np.where(chart, first + f, 0)]
    u, v = H["u"], H["v"]
    with np.errstate(all="ignore"):
        b0 = (F(1.0) - u) - v
        x = (b0 * c[:, 0] + u * c[:, 2]) + v * c[:, 4]
        y = (b0 * c[:, 1] + u * c[:, 3]) + v * c[:, 5]
        assert x.dtype == F and y.dtype == F
        out[chart, 4], out[chart, 5] = x.view(np.int32)[chart], y.view(np.int32)[chart]
        fin = chart & np.isfinite(x) & np.isfinite(y)

        def tap(ok, i, j):
            """(usable, texel index) of the taps (i, j), int64 arrays"""
            inside = ok & (i >= 0) & (j >= 0) & (i < aw) & (j < ah)
            idx = np.where(inside, j * aw + i, 0)
            return inside & (texels[idx, 3] != 0), idx

        if mode == NEAREST:
            fi, fj = np.floor(x), np.floor(y)
            ok = fin & (fi >= F(-1.0)) & (fi <= LIMIT) & (fj >= F(-1.0)) & (fj <= LIMIT)
            i0, j0 = np.where(ok, fi, F(-1.0)).astype(np.int64), np.where(ok, fj, F(-1.0)).astype(np.int64)
            use, idx = tap(ok, i0, j0)
            out[use, 0:3] = words[idx[use], 0:3]
            out[use, 3] = F(1.0).view(np.int32)
            return out
        tx, ty = x - F(0.5), y - F(0.5)
        fi, fj = np.floor(tx), np.floor(ty)
        fx, fy = tx - fi, ty - fj
        gx, gy = F(1.0) - fx, F(1.0) - fy
        ok = fin & (fi >= F(-1.0)) & (fi <= LIMIT) & (fj >= F(-1.0)) & (fj <= LIMIT)
        i0, j0 = np.where(ok, fi, F(-1.0)).astype(np.int64), np.where(ok, fj, F(-1.0)).astype(np.int64)
        num, den = np.zeros((n, 3), F), np.zeros(n, F)
        for di, dj, w in ((0, 0, gx * gy), (1, 0, fx * gy), (0, 1, gx * fy), (1, 1, fx * fy)):
            use, idx = tap(ok, i0 + di, j0 + dj)
            take = use & (w > 0)  # selection: what a skipped tap holds, NaN included, enters nothing
            rgb = texels[idx, 0:3]
            num = np.where(take[:, None], num + w[:, None] * rgb, num)
            den = np.where(take, den + w, den)
        assert num.dtype == F and den.dtype == F
        done = den > 0
        res = np.zeros((n, 4), F)
        res[done, 0:3] = num[done] / den[done][:, None]
        res[done, 3] = den[done]
    out[:, 0:4] = res.view(np.int32)
    return out
