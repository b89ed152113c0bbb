"""Around Scene.query_irradiance: the sample set the texels share, per-texel phases, the texels of a planar quad and what to do
with the (n, 8) rows.  Plain numpy, no device code -- the arrays go to the device with torch.from_numpy(..).cuda() and the rows
come back with .cpu().numpy() (torch tensors on the host are accepted where rows are).

A texel's rays are cosine-distributed about its normal, so the mean of their radiance times pi is the irradiance; a texel whose
rays mostly end close by -- inside a wall, under a carpet -- is one a baker fills from its neighbours (`invalid_texels`).

Scene.query_direct adds what the gather cannot see, the analytic lights at the texel itself: `direct_irradiance`,
`penumbra_texels` and `total_irradiance` read its rows.  Scene.query_bounce adds the term both leave out, the lights' one bounce
off the surface a gather ray hits first: `bounce_irradiance` reads its rows and `full_irradiance` sums all three.

Scene.atlas_texels makes the texels of an uploaded mesh from its UV charts and Scene.atlas_dilate finishes a baked atlas:
`triangle_charts` (charts for a mesh that never had UVs), `uv_to_texels`, `covered`, `atlas_inputs` and `scatter` stand between
them and the queries; these take torch tensors as well as arrays and answer in kind.  Scene.atlas_filter stands between
`scatter` and the dilation -- the order of a bake is scatter, atlas_filter, atlas_dilate -- and `texel_pitch` and
`filter_sigmas` give it its two ranges.

Scene.atlas_sample and Scene.query_lightmap read the finished atlas back at ray hits: `chart_table` joins the meshes' charts into
the table they take, `sample_rgb` and `sample_weight` read their rows, `shade_samples` turns them into a Lambertian preview.  A
lightmapped view of a scene is Scene.camera_rays, then Scene.query_lightmap, then `shade_samples`."""
import math

import numpy as np


def _radical_inverse2(i):
    """van der Corput in base 2 of the uint32 array i: the bits mirrored about the binary point, exact in float64"""
    i = np.asarray(i, np.uint32).copy()
    i = (i << np.uint32(16)) | (i >> np.uint32(16))
    i = ((i & np.uint32(0x00ff00ff)) << np.uint32(8)) | ((i & np.uint32(0xff00ff00)) >> np.uint32(8))
    i = ((i & np.uint32(0x0f0f0f0f)) << np.uint32(4)) | ((i & np.uint32(0xf0f0f0f0)) >> np.uint32(4))
    i = ((i & np.uint32(0x33333333)) << np.uint32(2)) | ((i & np.uint32(0xcccccccc)) >> np.uint32(2))
    i = ((i & np.uint32(0x55555555)) << np.uint32(1)) | ((i & np.uint32(0xaaaaaaaa)) >> np.uint32(1))
    return i.astype(np.float64) * 2.0 ** -32


def hammersley2(n):
    """(n, 2) float32 points in [0,1)^2: the Hammersley set ((i + 0.5) / n, radical inverse of i in base 2).  The first
    coordinate picks the ring of the cosine map (u1), the second the azimuth (u2).  n up to 2^24: the radical inverse of such an
    i has at most 24 bits and is exact in float32, so no two points are equal."""
    n = int(n)
    if n < 1 or n > 1 << 24:
        raise ValueError(f"hammersley2: {n} points (1 .. 2^24)")
    i = np.arange(n, dtype=np.uint32)
    p = np.stack([(i.astype(np.float64) + 0.5) / n, _radical_inverse2(i)], axis=1).astype(np.float32)
    # (a first coordinate that rounds up to 1.0f: the largest float32 below it instead)
    return np.ascontiguousarray(np.minimum(p, np.nextafter(np.float32(1.0), np.float32(0.0))))


def texel_phases(n, seed=0):
    """(n,) float32 in [0,1): one rotation of the shared sample set per texel, from numpy's generator seeded with `seed`"""
    n = int(n)
    if n < 0:
        raise ValueError(f"texel_phases: {n} texels")
    p = np.random.default_rng(seed).random(n, dtype=np.float32)
    return np.ascontiguousarray(np.minimum(p, np.nextafter(np.float32(1.0), np.float32(0.0))))


def quad_texels(origin, eu, ev, nu, nv):
    """(positions (nu * nv, 3), normals (nu * nv, 3)), float32: the texel centres origin + (i + 0.5) / nu * eu +
    (j + 0.5) / nv * ev of the planar quad spanned by the edges eu and ev from `origin`, i running fastest, and the quad's unit
    normal eu x ev / |eu x ev| repeated for every texel.  Computed in float64, rounded once."""
    o, eu, ev = (np.asarray(a, np.float64).reshape(3) for a in (origin, eu, ev))
    nu, nv = int(nu), int(nv)
    if nu < 1 or nv < 1:
        raise ValueError(f"quad_texels: {nu} x {nv} texels")
    n = np.cross(eu, ev)
    length = math.sqrt(float(n @ n))
    if not length > 0.0:
        raise ValueError("quad_texels: the edges are parallel")
    n /= length
    a = (np.arange(nu) + 0.5) / nu
    b = (np.arange(nv) + 0.5) / nv
    pos = o[None, None, :] + b[:, None, None] * ev[None, None, :] + a[None, :, None] * eu[None, None, :]
    return (np.ascontiguousarray(pos.reshape(-1, 3).astype(np.float32)),
            np.ascontiguousarray(np.repeat(n[None, :], nu * nv, axis=0).astype(np.float32)))


def _rows(records):
    r = records.cpu().numpy() if hasattr(records, "cpu") else np.asarray(records)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"lightmap: rows of shape {r.shape}, expected (n, 8)")
    return r


def irradiance(records):
    """(n, 3) float32: pi times the mean radiance of query_irradiance's (n, 8) rows (one float32 product per value)"""
    return np.float32(math.pi) * _rows(records)[:, 0:3].astype(np.float32)


def invalid_texels(records, threshold):
    """(n,) bool: texels whose rays all hit something and on average within `threshold` -- hit_fraction == 1 and
    mean_distance < threshold: the texel lies inside or right under geometry, and a baker dilates its neighbours over it --
    leave such texels out of the indices given to `scatter` and Scene.atlas_dilate fills them with the empty ones."""
    r = _rows(records)
    return (r[:, 5] >= np.float32(1.0)) & (r[:, 3] < np.float32(threshold))


def direct_irradiance(rows):
    """(n, 3) float32: the irradiance columns of query_direct's (n, 8) rows -- already an irradiance (the lights' radiance times
    attenuation times the cosine, over the sample's density), no factor of pi"""
    return np.ascontiguousarray(_rows(rows)[:, 0:3].astype(np.float32))


def penumbra_texels(rows):
    """(n,) bool: texels of query_direct's rows that some shadow samples reached and some did not -- lit_fraction > 0 and
    shadowed_fraction > 0: a sphere light's penumbra, or a texel lit by some lights of the range and shadowed from others.
    These are the texels that gain from more shadow samples."""
    r = _rows(rows)
    return (r[:, 3] > np.float32(0.0)) & (r[:, 4] > np.float32(0.0))


def total_irradiance(direct_rows, gather_rows):
    """(n, 3) float32: direct_irradiance(direct_rows) + irradiance(gather_rows), the direct term of the analytic lights at the
    texel plus pi times the gather's mean radiance (one float32 product and one sum per value).

    What this sum still LACKS: a gather ray takes no light sample at its first hit (the quirk of a caller's ray, include/ptrt.h),
    so the analytic lights' one-bounce term -- light that reaches the texel after exactly one diffuse reflection off the surface
    a gather ray hits first -- is absent; emissive meshes, the sky and every later bounce are in the gather.  A lit first vertex
    for the gather is not built.  `full_irradiance` adds that term from Scene.query_bounce's rows.

    The order of a bake from here: `scatter` these values into the atlas, Scene.atlas_filter (the gather's Monte-Carlo noise,
    edge-aware, covered texels only), then Scene.atlas_dilate (the texels no chart covers)."""
    d, g = direct_irradiance(direct_rows), irradiance(gather_rows)
    if d.shape != g.shape:
        raise ValueError(f"total_irradiance: {d.shape[0]} direct rows, {g.shape[0]} gather rows")
    return d + g


def bounce_irradiance(rows):
    """(n, 3) float32: pi times the mean radiance of query_bounce's (n, 8) rows (one float32 product per value) -- the gather
    rays are cosine-distributed, as for `irradiance`"""
    return np.float32(math.pi) * _rows(rows)[:, 0:3].astype(np.float32)


def full_irradiance(direct_rows, gather_rows, bounce_rows):
    """(n, 3) float32: (direct_irradiance(direct_rows) + irradiance(gather_rows)) + bounce_irradiance(bounce_rows) -- what
    `total_irradiance` gives plus the analytic lights' one-bounce term from Scene.query_bounce, the term that sum lacks.  The
    three terms do not overlap: the lights at the texel; the lights after exactly one reflection; everything a path collects
    from its second vertex on, and emission, sky and environment at every vertex.  The order of a bake from here is
    `total_irradiance`'s."""
    t, b = total_irradiance(direct_rows, gather_rows), bounce_irradiance(bounce_rows)
    if t.shape != b.shape:
        raise ValueError(f"full_irradiance: {t.shape[0]} direct and gather rows, {b.shape[0]} bounce rows")
    return t + b


def triangle_charts(face_count, cell, gutter=1):
    """(uv (face_count, 6) float32 in texel units, atlas_w, atlas_h): a chart of its own for every face of a mesh without UVs,
    ready for Scene.atlas_texels.  The atlas is a grid of square cells of `cell` texels; a cell holds two right isosceles
    triangles with legs of cell - 2 * gutter - 0.5 texels, face 2k at the cell's low corner -- v0 at the right angle (X, Y),
    v1 along +x, v2 along +y -- and face 2k + 1 turned by half a turn at (X, Y) + cell - gutter.  The legs lie on integer
    lines and have a half-integer length, so every vertex is a multiple of 0.5 texel and no texel centre lies on a chart's edge
    (none comes closer than 0.35 texel); charts of different faces are at least `gutter` texels apart in the Chebyshev sense --
    no point of one is within `gutter` of a point of another in both axes at once --, and every chart holds at least one
    centre.  ValueError for face_count < 1, gutter < 0 or cell < 2 * gutter + 2 (integers all)."""
    if int(face_count) != face_count or int(cell) != cell or int(gutter) != gutter:
        raise ValueError(f"triangle_charts: face_count {face_count!r}, cell {cell!r}, gutter {gutter!r}: integers")
    face_count, cell, gutter = int(face_count), int(cell), int(gutter)
    if face_count < 1 or gutter < 0 or cell < 2 * gutter + 2:
        raise ValueError(f"triangle_charts: {face_count} faces, cells of {cell} texels, a gutter of {gutter} "
                         "(face_count >= 1, gutter >= 0, cell >= 2 * gutter + 2)")
    cells = (face_count + 1) // 2
    cols = int(math.ceil(math.sqrt(cells)))
    while cols * cols < cells:
        cols += 1
    rows = (cells + cols - 1) // cols
    if cols * cell * rows * cell > 1 << 28:
        raise ValueError(f"triangle_charts: {face_count} faces in cells of {cell} texels: more than 2^28 texels")
    leg, side = cell - 2 * gutter - 0.5, float(cell - gutter)
    f = np.arange(face_count)
    k = f // 2
    x, y = (k % cols).astype(np.float64) * cell, (k // cols).astype(np.float64) * cell
    low = (f % 2 == 0)
    ax, ay = np.where(low, x, x + side), np.where(low, y, y + side)  # the right angle
    d = np.where(low, leg, -leg)
    uv = np.stack([ax, ay, ax + d, ay, ax, ay + d], axis=1)
    return np.ascontiguousarray(uv.astype(np.float32)), cols * cell, rows * cell


def uv_to_texels(uv01, w, h):
    """(F, 6) float32: UVs in [0, 1]^2 -- (F, 6) or (F, 3, 2), u to the right, v up the rows -- scaled to the texel units of a
    w x h atlas (u * w, v * h; one float32 product each).  An array or a torch tensor, answered in kind."""
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"uv_to_texels: a {w} x {h} atlas")
    if hasattr(uv01, "cpu"):
        import torch
        uv = uv01.to(torch.float32).reshape(-1, 3, 2)
        return (uv * torch.tensor([w, h], dtype=torch.float32, device=uv.device)).reshape(-1, 6).contiguous()
    uv = np.asarray(uv01, np.float32).reshape(-1, 3, 2)
    return np.ascontiguousarray((uv * np.float32([w, h])).reshape(-1, 6))


def _atlas_rows(records):
    if records.ndim != 2 or records.shape[1] != 8 or "int32" not in str(records.dtype):
        raise ValueError(f"lightmap: atlas records of shape {tuple(records.shape)} and {records.dtype}, expected (n, 8) int32")
    return records


def covered(records):
    """The indices, ascending (row-major: texel (i, j) of a W-wide atlas is j * W + i), of the texels of Scene.atlas_texels'
    (n, 8) int32 rows that a face covers: mesh >= 0.  int64; a tensor for a tensor (on its device), an array for an array."""
    r = _atlas_rows(records)
    if hasattr(r, "cpu"):
        import torch
        return torch.nonzero(r[:, 7] >= 0).reshape(-1)
    return np.flatnonzero(np.asarray(r)[:, 7] >= 0)


def atlas_inputs(records):
    """(positions (n, 3), normals (n, 3)) float32, contiguous: the covered texels of Scene.atlas_texels' rows in the order of
    `covered`, as Scene.query_irradiance and Scene.query_direct take them (tensors for a tensor, arrays for an array)."""
    r = _atlas_rows(records)
    idx = covered(r)
    if hasattr(r, "cpu"):
        import torch
        rows = r[idx].view(torch.float32)
        return rows[:, 0:3].contiguous(), rows[:, 4:7].contiguous()
    rows = np.ascontiguousarray(np.asarray(r)[idx]).view(np.float32)
    return np.ascontiguousarray(rows[:, 0:3]), np.ascontiguousarray(rows[:, 4:7])


def scatter(values, indices, w, h):
    """(h * w, 4) float32 {r, g, b, valid}: values[k] (n, 3) at texel indices[k] with valid = 1, zeros elsewhere -- reshaped to
    (h, w, 4) the image Scene.atlas_dilate takes.  Tensors give a tensor on their device, arrays an array."""
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"scatter: a {w} x {h} atlas")
    if values.ndim != 2 or values.shape[1] != 3 or indices.ndim != 1 or indices.shape[0] != values.shape[0]:
        raise ValueError(f"scatter: values {tuple(values.shape)}, indices {tuple(indices.shape)}, expected (n, 3) and (n,)")
    if hasattr(values, "cpu"):
        import torch
        idx = torch.as_tensor(indices, dtype=torch.int64, device=values.device)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= w * h):
            raise ValueError(f"scatter: an index outside the {w} x {h} atlas")
        img = torch.zeros((h * w, 4), dtype=torch.float32, device=values.device)
        img[idx, 0:3] = values.to(torch.float32)
        img[idx, 3] = 1.0
        return img
    idx = np.asarray(indices.cpu() if hasattr(indices, "cpu") else indices, np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= w * h):
        raise ValueError(f"scatter: an index outside the {w} x {h} atlas")
    img = np.zeros((h * w, 4), np.float32)
    img[idx, 0:3] = np.asarray(values, np.float32)
    img[idx, 3] = 1.0
    return img


def texel_pitch(records, w, h):
    """The median world distance between horizontally adjacent covered texels of the same face and mesh of Scene.atlas_texels'
    (h * w, 8) int32 rows (a tensor or an array; computed where it is, in float32): how far apart in the world neighbouring
    texels of one chart are, the natural unit for Scene.atlas_filter's two sigmas.  A float -- of an even number of distances the
    lower of the two middle ones, for tensors and arrays alike --; 0.0 when the atlas has no such pair."""
    r = _atlas_rows(records)
    w, h = int(w), int(h)
    if w < 1 or h < 1 or r.shape[0] != w * h:
        raise ValueError(f"texel_pitch: {r.shape[0]} records for a {w} x {h} atlas")
    if hasattr(r, "cpu"):
        import torch
        g = r.reshape(h, w, 8)
        a, b = g[:, :-1], g[:, 1:]
        pair = (a[..., 7] >= 0) & (a[..., 7] == b[..., 7]) & (a[..., 3] == b[..., 3])
        if not bool(pair.any()):
            return 0.0
        d = b[..., 0:3].contiguous().view(torch.float32)[pair] - a[..., 0:3].contiguous().view(torch.float32)[pair]
        return float(torch.sqrt((d * d).sum(1)).median())
    g = np.asarray(r).reshape(h, w, 8)
    a, b = g[:, :-1], g[:, 1:]
    pair = (a[..., 7] >= 0) & (a[..., 7] == b[..., 7]) & (a[..., 3] == b[..., 3])
    if not pair.any():
        return 0.0
    d = np.ascontiguousarray(b[..., 0:3]).view(np.float32)[pair] - np.ascontiguousarray(a[..., 0:3]).view(np.float32)[pair]
    d = np.sort(np.sqrt((d * d).sum(1)))
    return float(d[(len(d) - 1) // 2])


def filter_sigmas(pitch):
    """(sigma_distance, sigma_plane) for Scene.atlas_filter from `texel_pitch`'s answer: 3 * pitch and pitch / 2.  These are
    CONVENTIONS, not measurements.  At three pitches the outermost ring of the 5 x 5 footprint -- two texels away along a row,
    2 * sqrt(2) along a diagonal, times the step -- still has weight (1 - (2 sqrt 2 / 3)^2 = 1/9 at the corners), so a flat
    chart is smoothed by the whole kernel; half a pitch off the centre's tangent plane is more than the texels of a flat chart
    ever are and less than the next texel round a right-angled crease.  A scene with fine curved detail wants a larger
    sigma_plane, a noisier gather a larger sigma_distance.  ValueError for a pitch that is not positive and finite (an atlas
    without a pair of neighbours has nothing to filter)."""
    pitch = float(pitch)
    if not (math.isfinite(pitch) and pitch > 0.0):
        raise ValueError(f"filter_sigmas: a texel pitch of {pitch} (positive and finite)")
    return 3.0 * pitch, 0.5 * pitch


def chart_table(charts_per_mesh):
    """(charts (sum F, 6) float32, chart_first (M,) int32) for Scene.atlas_sample and Scene.query_lightmap from a list with one
    entry per UPLOADED mesh, in upload order (the order ptrt_hit.mesh_index counts in): the (F_m, 6) charts Scene.atlas_texels
    took for that mesh -- an array or a tensor --, or None for a mesh without a lightmap, which gets chart_first -1.  Arrays,
    unless an entry is a tensor: then tensors on that tensor's device.  ValueError for an empty list, a list of Nones, an entry
    that is not (F, 6) with F >= 1, and more than 2^31 - 1 faces."""
    entries = list(charts_per_mesh)
    if not entries:
        raise ValueError("chart_table: no meshes")
    like = next((c for c in entries if hasattr(c, "cpu")), None)
    parts, first, total = [], [], 0
    for m, c in enumerate(entries):
        if c is None:
            first.append(-1)
            continue
        if hasattr(c, "cpu"):
            c = c.detach().cpu().numpy()
        c = np.asarray(c)
        if c.ndim != 2 or c.shape[1] != 6 or c.shape[0] < 1:
            raise ValueError(f"chart_table: mesh {m}: charts of shape {tuple(c.shape)}, expected (F, 6) with F >= 1")
        first.append(total)
        total += c.shape[0]
        parts.append(c.astype(np.float32))
    if not parts:
        raise ValueError("chart_table: no mesh has charts")
    if total >= 2 ** 31:
        raise ValueError(f"chart_table: {total} faces (at most 2^31 - 1)")
    charts, chart_first = np.ascontiguousarray(np.concatenate(parts)), np.asarray(first, np.int32)
    if like is not None:
        import torch
        return torch.from_numpy(charts).to(like.device), torch.from_numpy(chart_first).to(like.device)
    return charts, chart_first


def _sample_rows(rows):
    if rows.ndim != 2 or rows.shape[1] != 8 or "int32" not in str(rows.dtype):
        raise ValueError(f"lightmap: sample rows of shape {tuple(rows.shape)} and {rows.dtype}, expected (n, 8) int32")
    return rows


def sample_rgb(rows):
    """(n, 3) float32: the colour columns of Scene.atlas_sample's / query_lightmap's (n, 8) int32 rows -- the atlas at the hit,
    zeros where weight is 0 (a tensor for a tensor, an array for an array)"""
    r = _sample_rows(rows)
    if hasattr(r, "cpu"):
        import torch
        return r[:, 0:3].contiguous().view(torch.float32)
    return np.ascontiguousarray(np.asarray(r)[:, 0:3]).view(np.float32)


def sample_weight(rows):
    """(n,) float32: the weight column of those rows -- the sum of the weights of the taps used, 0 where there was nothing to
    sample: a miss, a mesh without a chart, a footprint with no valid texel"""
    r = _sample_rows(rows)
    if hasattr(r, "cpu"):
        import torch
        return r[:, 3].contiguous().view(torch.float32)
    return np.ascontiguousarray(np.asarray(r)[:, 3]).view(np.float32)


def shade_samples(rows, albedo, emission=None, background=(0.0, 0.0, 0.0)):
    """(n, 3) float32, the Lambertian preview of a bake: for a hit on mesh m  (albedo[m] * rgb) / pi + emission[m]  -- the baked
    irradiance times the surface's diffuse reflectance over pi, plus what the surface emits --, `background` on a miss (mesh
    < 0).  Each step is one float32 operation: the product, the quotient by float32(pi), the sum.  albedo and emission: (M, 3),
    one row per uploaded mesh (emission None: zeros).  Arrays or tensors, answered in the kind of `rows`.

    A lightmapped view of a scene is Scene.camera_rays, then Scene.query_lightmap, then this."""
    r = _sample_rows(rows)
    rgb = sample_rgb(r)
    if hasattr(r, "cpu"):
        import torch
        dev = r.device
        a = torch.as_tensor(albedo, dtype=torch.float32, device=dev)
        e = torch.zeros_like(a) if emission is None else torch.as_tensor(emission, dtype=torch.float32, device=dev)
        bg = torch.as_tensor(background, dtype=torch.float32, device=dev)
        mesh = r[:, 7].to(torch.int64)
    else:
        r = np.asarray(r)
        a = np.asarray(albedo.cpu() if hasattr(albedo, "cpu") else albedo, np.float32)
        e = np.zeros_like(a) if emission is None else np.asarray(emission.cpu() if hasattr(emission, "cpu") else emission, np.float32)
        bg = np.asarray(background, np.float32)
        mesh = r[:, 7].astype(np.int64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1 or tuple(e.shape) != tuple(a.shape) or tuple(bg.shape) != (3,):
        raise ValueError(f"shade_samples: albedo {tuple(a.shape)}, emission {tuple(e.shape)}, background {tuple(bg.shape)}: "
                         "expected (M, 3), (M, 3) and (3,)")
    if mesh.shape[0] and int(mesh.max()) >= a.shape[0]:
        raise ValueError(f"shade_samples: a hit on mesh {int(mesh.max())}, albedo has {a.shape[0]} rows")
    hit = mesh >= 0
    m = mesh * hit  # (a miss reads row 0 and is replaced below)
    if hasattr(rgb, "cpu"):
        import torch
        lit = (a[m] * rgb) / torch.tensor(math.pi, dtype=torch.float32, device=rgb.device) + e[m]
        return torch.where(hit[:, None], lit, bg[None, :].expand_as(lit)).contiguous()
    lit = (a[m] * rgb) / np.float32(math.pi) + e[m]
    return np.ascontiguousarray(np.where(hit[:, None], lit, bg[None, :]).astype(np.float32))
