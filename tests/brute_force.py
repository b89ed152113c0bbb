"""Closest hit and any hit of a ray with a scene, by geometry alone: every ray against every triangle of every mesh in float64.

TEST INFRASTRUCTURE.  No tree, no boxes, no culling, no early out, no stack: nothing the builder, a refit, a rebuild or a
traversal can get wrong exists here, so an answer of this module is the nearest triangle on the ray whatever anybody's walk
says.  It states the SPECIFICATION of the reference's queries (oracle/ptrt_oracle.cpp carries the line numbers), not their walk:

  * per mesh the ray is used as is, or, with `has_transform`, moved with the mesh's stored `inverse` (the 16 floats as they
    are, converted to float64; the direction renormalised; world t = local t / |inverse . d|);
  * a triangle is hit when |det| >= 1e-6, 0 <= u <= 1, v >= 0, u + v <= 1 and t > 1e-5 (Moeller-Trumbore on the float32
    inputs converted exactly);
  * CLOSEST: the smallest world t over all triangles of all meshes; OCCLUDED: any hit with local t < tmax x scale on a mesh
    whose transmission is <= 0.5.

The pair arithmetic is Moeller-Trumbore with its scalar triple products turned so that each is a matrix product over
(rays x triangles) -- with s = o - v0, N = e1 x e2, M = o x d:
    det = e1.(d x e2) = -d.N            u.det = s.(d x e2) = e2.M - d.(e2 x v0)
    t.det = e2.(s x e1) = o.N - v0.N    v.det = d.(s x e1) = -e1.M - d.(v0 x e1)
`literal_pairs` is the same test written term by term as the reference writes it; tests/test_brute_force.py holds the two
together.

DECIDED.  float32 and float64 may legitimately disagree for a ray that passes within rounding of an edge, of the t / det
thresholds, or of a second surface at nearly the same distance.  With every condition above LOOSENED by DELTA (u, v >= -DELTA,
u + v <= 1 + DELTA, t > 1e-5 - DELTA, any det):
  * a hit is decided when its own margins -- min(u, v, 1 - u - v), |det| - 1e-6, t - 1e-5 -- exceed DELTA and no OTHER triangle
    accepted under the loosened conditions is nearly as near (see UNCERTAINTY OF t);
  * a miss is decided when no triangle is accepted under the loosened conditions;
  * occluded = 1 is decided when a triangle of an opaque mesh is hit with those margins clearly before tmax, occluded = 0 when
    no triangle of an opaque mesh is accepted under the loosened conditions before or nearly at tmax.
A triangle with two equal corners takes no part (`_usable`).  Only finite, non-zero
directions are judged here.

THE INSTANCE INVERSE.  The reference's mat4::inverse is not a true inverse for a rotated instance with an x translation
(tests/test_host_scene.py::test_has_transform_flag_and_matrices).  For such an instance the local-space answer (stored inverse)
and the world-space TLAS box (world matrix) belong to different geometry and no geometric truth exists: `Mesh.proper` says
whether world @ inverse is the identity to 1e-5, and every answer carries `quirk`: an improper instance has a loosened hit on
that ray.

UNCERTAINTY OF t.  float32 computes t = (o - v0).N / d.N from coordinates of the scene's size, so its error grows with the
scene radius R and with 1 / cos(ray, normal): every distance here carries TOL_T x max(t, R) / cos as what float32 may make of
it.  A second surface is "nearly at the same distance" when its t less that uncertainty lies below t_hit x (1 + GAP) plus the
hit's own; tmax counts as reached or not reached only beyond GAP x tmax plus the uncertainty of the hit in question.

FRONT FACE.  For a mesh without a transform front_face is d . n < 0 of the geometric normal n = e1 x e2 and the normal
returned is n turned against the ray.  For an instance the reference takes the TURNED local normal to world space and
derives front_face from that one again (intersection.cuh:471-475), so a proper instance reports front_face = true from either
side; this module states that behaviour, it is the reference's.

NUMBERS.  Measured on the CPU, oracle against this module, on the host-built scenes of tests/test_brute_force.py.  The largest
u, v error of float32 is 4.6e-5, so a DELTA below that cannot be sound; DELTA = GAP = 1e-4 is the next power of ten.  (At
1e-5 no decided ray differed either in these samples; at 1e-3 the 0.999 t / 1.001 t occlusion cases are all undecided.)  The
tolerances are 4 x the largest error observed:

    scene (host-built, oracle against this module)   rays     undecided   t x cos / max(t, R)   u, v      normal (rad)
    cornell, leaf (1,0) (2,1) (4,0)      plain       8,192    0.04 %      2.04e-7               6.4e-6    2.4e-8
                                         targeted      188    0           1.6e-9                5.0e-8    2.4e-8
    cornell quads                        plain       8,192    0.09 %      2.04e-7               1.4e-6    2.4e-8
    showcase, segments 16                plain       8,192    0.04 %      1.48e-7               1.7e-5    7.2e-8
                                         targeted    9,604    0           1.4e-9                1.3e-7    7.2e-8
                                         box faces  28,808    1.9 %       1.3e-9                3.0e-7    7.2e-8
    fluid, cells 40                      plain       8,192    0.01 %      1.80e-7               1.3e-5    5.5e-8
                                         targeted    8,608    0           1.3e-9                1.4e-7    7.1e-8
                                         box faces  25,288    0.13 %      2.1e-9                3.2e-6    7.1e-8
    many, proper instances (72 meshes)   plain       8,192    0.06 %      1.91e-7               3.2e-5    7.0e-8
                                         targeted    3,516    0.11 %      4.6e-8                6.7e-6    1.2e-7
    instanced cornell, leaf (12,5) (2,0) plain       8,192    0.04 %      2.04e-7               6.4e-6    8.0e-8
                                         targeted      332    0           3.1e-8                3.5e-7    8.0e-8
    many as shipped (quirk case)         plain       8,192    (1.1 % left out)  1.80e-7         4.6e-5    5.0e-8
    largest                                                              2.04e-7               4.6e-5    1.16e-7
    x 4 = TOL_T, TOL_UV, TOL_NORMAL                                      8.2e-7                1.9e-4    4.7e-7
No decided ray differed in hit flag, mesh, face or front_face in any of them, at DELTA = 1e-5, 1e-4 or 1e-3.
"""
import ctypes as C

import numpy as np

DET_MIN, T_MIN = 1e-6, 1e-5          # the reference's EPSILON_F reject and its `t > 1e-5f`
DELTA = 1e-4
GAP = 1e-4
TOL_T = 8.2e-7                       # |t - t_bf| <= TOL_T x max(t_bf, scene radius) / cos(ray, normal)
TOL_UV = 1.9e-4                         # |u - u_bf|, |v - v_bf|
TOL_NORMAL = 4.7e-7                     # angle between the normals, radians
PROPER_TOL = 1e-5
TARGET_H = 0.004                     # targeted rays start this far (x scene radius) from the triangle they aim at
PAIRS_PER_CHUNK = 1 << 21            # rays x triangles held at once


class Mesh:
    def __init__(self, verts, faces, has_transform=False, world=None, inverse=None, transmission=0.0):
        self.verts = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3)
        self.has_transform = bool(has_transform)
        eye = np.eye(4)
        self.world = eye if world is None else np.asarray(world, np.float32).astype(np.float64).reshape(4, 4)
        self.inverse = eye if inverse is None else np.asarray(inverse, np.float32).astype(np.float64).reshape(4, 4)
        self.transmission = float(np.float32(transmission))
        self.opaque = not (np.float32(transmission) > np.float32(0.5))
        self.proper = (not self.has_transform) or bool(np.abs(self.world @ self.inverse - eye).max() <= PROPER_TOL)

    def triangles(self):
        """(F, 3, 3) local-space corners"""
        return self.verts[self.faces]

    def world_triangles(self):
        t = self.triangles()
        if not self.has_transform:
            return t
        return t @ self.world[:3, :3].T + self.world[:3, 3]


class Geometry:
    """The meshes of a scene and its radius (the largest absolute world-space coordinate)."""

    def __init__(self, meshes):
        self.meshes = list(meshes)
        self.radius = max([float(np.abs(m.world_triangles()).max()) for m in self.meshes if len(m.faces)] + [1.0])

    @classmethod
    def from_desc(cls, desc):
        """From `Scene.flatten()`: per mesh verts, faces, has_transform, world, inverse and materials.transmission -- copies,
        so the answer does not follow the scene when it changes afterwards."""
        d = desc.contents if hasattr(desc, "contents") else desc
        meshes = []
        for i in range(d.mesh_count):
            M = d.meshes[i]
            v = np.ctypeslib.as_array(C.cast(M.verts, C.POINTER(C.c_float)), (M.vert_count, 3)).copy()
            f = np.ctypeslib.as_array(C.cast(M.faces, C.POINTER(C.c_int32)), (M.face_count, 3)).copy()
            meshes.append(Mesh(v, f, M.has_transform, list(M.world), list(M.inverse), d.materials.transmission[i]))
        return cls(meshes)

    def face_count(self):
        return sum(len(m.faces) for m in self.meshes)


def _local_rays(mesh, o, d):
    """(origins, directions, scale): the ray in the mesh's space and |inverse . d|"""
    if not mesh.has_transform:
        return o, d, np.ones(len(o))
    A, b = mesh.inverse[:3, :3], mesh.inverse[:3, 3]
    lo = o @ A.T + b
    ld = d @ A.T
    scale = np.sqrt((ld * ld).sum(axis=1))
    return lo, ld / scale[:, None], scale


def _usable(tri):
    """triangles that can be hit at all.  e1 == 0 or e2 == 0: det == 0 exactly in every precision.  v1 == v2 (e1 == e2):
    det = e1 . (d x e1) is 0 here and rounding residue of about 1e-7 |e1|^2 in float32, below the 1e-6 reject for an edge
    shorter than 1."""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    twin = (e1 == e2).all(axis=1) & ((e1 * e1).sum(axis=1) < 1.0)
    return (e1 != 0).any(axis=1) & (e2 != 0).any(axis=1) & ~twin


def _pairs(tri, lo, ld, delta):
    """Every ray against every triangle.  Returns (t, u, v, det, strict, loose, robust, invcos), each (rays, triangles); t is
    local; invcos = |e1 x e2| |d| / |det|, one over the cosine between the ray and the triangle's normal."""
    v0 = tri[:, 0]
    e1, e2 = tri[:, 1] - v0, tri[:, 2] - v0
    N = np.cross(e1, e2)
    M = np.cross(lo, ld)
    det = -(ld @ N.T)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # a ray exactly parallel to the plane: no strict hit (|det| < 1e-6); for the loosened test its u, v, t are those of a
        # vanishing det, i.e. +-inf, or 0 where the numerator vanishes too (the ray lies in the plane: never decided)
        f = 1.0 / np.where(det == 0.0, 1e-300, det)
        u = f * (M @ e2.T - ld @ np.cross(e2, v0).T)
        v = f * (-(M @ e1.T) - ld @ np.cross(v0, e1).T)
        t = f * (lo @ N.T - (v0 * N).sum(axis=1)[None, :])
        w = 1.0 - u - v
        ok = _usable(tri)[None, :]
        absdet = np.abs(det)
        strict = ok & (absdet >= DET_MIN) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > T_MIN)
        loose = ok & (absdet >= DET_MIN - delta) & (u >= -delta) & (u <= 1.0 + delta) & (v >= -delta) & \
            (u + v <= 1.0 + delta) & (t > T_MIN - delta)
        robust = strict & (absdet > DET_MIN + delta) & (np.minimum(np.minimum(u, v), w) > delta) & (t > T_MIN + delta)
        invcos = (np.sqrt((N * N).sum(axis=1))[None, :] * np.sqrt((ld * ld).sum(axis=1))[:, None]) / np.maximum(absdet, 1e-300)
    return t, u, v, det, strict, loose, robust, invcos


def literal_pairs(tri, lo, ld):
    """The same test term by term as the reference writes it (intersection.cuh:219-255 through oracle/ptrt_oracle.cpp),
    float64: (t, u, v, det, strict) per (ray, triangle).  Slow; for checking `_pairs`."""
    v0, v1, v2 = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    o, d = lo[:, None, :], ld[:, None, :]
    e1, e2 = v1 - v0, v2 - v0
    h = np.cross(d, e2)
    a = (e1 * h).sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = 1.0 / a
        s = o - v0
        u = f * (s * h).sum(axis=2)
        q = np.cross(s, e1)
        v = f * (d * q).sum(axis=2)
        t = f * (e2 * q).sum(axis=2)
        strict = (np.abs(a) >= DET_MIN) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > T_MIN)
    return t, u, v, a, strict


def _as_rays(origins, directions):
    o = np.asarray(origins, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.asarray(directions, np.float32).astype(np.float64).reshape(-1, 3)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(axis=1).all(), "finite, non-zero rays only"
    return o, d


def _chunks(n, faces):
    step = max(1, PAIRS_PER_CHUNK // max(faces, 1))
    for a in range(0, n, step):
        yield slice(a, min(a + step, n))


def closest(geom, origins, directions, delta=None, gap=None):
    """dict of (n,) arrays: hit, t, mesh, face, u, v, normal (n, 3), front_face, decided, quirk, other_t (the smallest t of
    another triangle accepted under the loosened conditions, less its float32 uncertainty; inf if none), invcos."""
    delta = DELTA if delta is None else delta
    gap = GAP if gap is None else gap
    o, d = _as_rays(origins, directions)
    n = len(o)
    inf = np.inf
    best_t = np.full(n, inf)
    best_mesh, best_face = np.full(n, -1), np.full(n, -1)
    best_u, best_v, best_robust, best_invcos = np.zeros(n), np.zeros(n), np.zeros(n, bool), np.ones(n)
    normal, front = np.zeros((n, 3)), np.zeros(n, bool)
    quirk = np.zeros(n, bool)
    # per mesh: the two smallest loosened t and the face of the smallest
    loose1, loose2, loose1_face = [], [], []
    for mi, mesh in enumerate(geom.meshes):
        tri = mesh.triangles()
        l1, l2, l1f = np.full(n, inf), np.full(n, inf), np.full(n, -1)
        for sl in _chunks(n, len(tri)) if len(tri) else []:
            lo, ld, scale = _local_rays(mesh, o[sl], d[sl])
            t, u, v, det, strict, loose, robust, invcos = _pairs(tri, lo, ld, delta)
            tw = t / scale[:, None]
            rows = np.arange(tw.shape[0])
            ts = np.where(strict, tw, inf)
            k = ts.argmin(axis=1)
            tk = ts[rows, k]
            better = tk < best_t[sl]
            idx = np.flatnonzero(better) + sl.start
            kb = k[better]
            best_t[idx] = tk[better]
            best_mesh[idx], best_face[idx] = mi, kb
            best_u[idx], best_v[idx] = u[better, kb], v[better, kb]
            best_robust[idx] = robust[better, kb]
            best_invcos[idx] = invcos[better, kb]
            # the geometric normal, turned against the local direction; an instance's goes through inverse^T
            e1, e2 = tri[kb, 1] - tri[kb, 0], tri[kb, 2] - tri[kb, 0]
            g = np.cross(e1, e2)
            g /= np.sqrt((g * g).sum(axis=1))[:, None]
            ff = (ld[better] * g).sum(axis=1) < 0.0
            g = np.where(ff[:, None], g, -g)
            if mesh.has_transform:
                # the reference takes the ORIENTED local normal to world space (inverse^T) and derives front_face from that
                # one again (intersection.cuh:471-475): for a proper instance front_face is true from either side
                g = g @ mesh.inverse[:3, :3]
                g /= np.sqrt((g * g).sum(axis=1))[:, None]
                ff = (d[idx] * g).sum(axis=1) < 0.0
                g = np.where(ff[:, None], g, -g)
            normal[idx] = g
            front[idx] = ff
            with np.errstate(invalid="ignore", over="ignore"):
                tl = np.where(loose, tw - TOL_T * np.maximum(np.abs(tw), geom.radius) * invcos, inf)   # as near as float32 may see it
            k1 = tl.argmin(axis=1)
            l1[sl], l1f[sl] = tl[rows, k1], k1
            tl[rows, k1] = inf
            l2[sl] = tl.min(axis=1)
            if not mesh.proper:
                quirk[sl] |= loose.any(axis=1)
        loose1.append(l1), loose2.append(l2), loose1_face.append(l1f)
    hit = best_mesh >= 0
    other = np.full(n, inf)
    for mi in range(len(geom.meshes)):
        is_winner = hit & (best_mesh == mi) & (loose1_face[mi] == best_face)
        # the winner is accepted under the loosened conditions too; when it is not its mesh's smallest loosened t, that
        # smallest one is another triangle in front of it
        other = np.minimum(other, np.where(is_winner, loose2[mi], loose1[mi]))
    with np.errstate(invalid="ignore"):
        limit = best_t + gap * best_t + TOL_T * np.maximum(best_t, geom.radius) * best_invcos
        decided = np.where(hit, best_robust & ~(other < limit), other == inf)
    return dict(hit=hit, t=best_t, mesh=best_mesh, face=best_face, u=best_u, v=best_v, normal=normal, front_face=front,
                decided=decided, quirk=quirk, other_t=other, invcos=best_invcos)


def occluded(geom, origins, directions, tmax, delta=None, gap=None):
    """dict of (n,) arrays: occluded, decided, quirk"""
    delta = DELTA if delta is None else delta
    gap = GAP if gap is None else gap
    o, d = _as_rays(origins, directions)
    tm = np.asarray(tmax, np.float32).astype(np.float64).reshape(-1)
    assert len(tm) == len(o) and not np.isnan(tm).any()
    n = len(o)
    tf = np.minimum(np.abs(tm), 1e30)
    g, e = gap * tf, TOL_T * np.maximum(tf, geom.radius)
    flag, sure1, maybe1, quirk = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    for mesh in geom.meshes:
        tri = mesh.triangles()
        for sl in _chunks(n, len(tri)) if len(tri) else []:
            lo, ld, scale = _local_rays(mesh, o[sl], d[sl])
            t, u, v, det, strict, loose, robust, invcos = _pairs(tri, lo, ld, delta)
            if not mesh.proper:
                quirk[sl] |= loose.any(axis=1)
            if not mesh.opaque:
                continue
            with np.errstate(invalid="ignore"):
                flag[sl] |= (strict & (t < (tm[sl] * scale)[:, None])).any(axis=1)
                tw = t / scale[:, None]
                sure1[sl] |= (robust & (tw + e[sl][:, None] * invcos < (tm[sl] - g[sl])[:, None])).any(axis=1)
                maybe1[sl] |= (loose & ~(tw - e[sl][:, None] * invcos >= (tm[sl] + g[sl])[:, None])).any(axis=1)
    return dict(occluded=flag, decided=np.where(flag, sure1, ~maybe1), quirk=quirk)


def targeted_rays(geom, per_mesh=4096):
    """Two rays for every triangle (for a mesh of more than `per_mesh` triangles: every k-th, k the smallest stride that keeps
    it below): from centroid +- h x normal towards the centroid, h a quarter of sqrt(area) kept within 0.001 .. 0.02 of the
    scene radius.  Every leaf and every box on the way to it must let its own triangle through.  Returns float32 origins and
    directions, per ray the mesh and face aimed at, and how many triangles were left out for being too small to be hit with a
    margin (those with two equal corners, which nothing can hit, are left out and not counted)."""
    os_, ds_, ms_, fs_, small = [], [], [], [], 0
    for mi, mesh in enumerate(geom.meshes):
        tri = mesh.world_triangles()
        stride = max(1, -(-len(tri) // per_mesh))
        pick = np.arange(0, len(tri), stride)
        t = tri[pick]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        ln = np.sqrt((nrm * nrm).sum(axis=1))
        good = ln > 10.0 * (DET_MIN + DELTA)       # |det| <= |e1 x e2|: a smaller triangle cannot be hit with a margin
        small += int((~good & _usable(mesh.triangles()[pick])).sum())
        t, nrm, ln, pick = t[good], nrm[good], ln[good], pick[good]
        nrm = nrm / ln[:, None]
        c = t.mean(axis=1)
        h = np.full(len(t), TARGET_H * geom.radius)
        for sgn in (1.0, -1.0):
            o32 = (c + sgn * h[:, None] * nrm).astype(np.float32)
            dd = c - o32.astype(np.float64)
            d32 = (dd / np.sqrt((dd * dd).sum(axis=1))[:, None]).astype(np.float32)
            os_.append(o32), ds_.append(d32), ms_.append(np.full(len(pick), mi)), fs_.append(pick)
    return (np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds_)),
            np.concatenate(ms_), np.concatenate(fs_), small)


FACE_EPS = 1e-3


def box_face_rays(geom, per_mesh=4096):
    """Rays that lie IN the faces of a triangle's bounding box, where the centroid rays cannot tell a box that is a little too
    small: for every triangle, every axis k along which it has an extent and both of its extreme corners along k, a ray through
    p = corner + FACE_EPS x (centroid - corner) -- inside the triangle by a margin of FACE_EPS / 3 -- that runs along another
    axis j (the one the triangle faces most), i.e. within the plane x_k = p_k, FACE_EPS x extent from the box face.  A leaf or
    inner box shrunk by more than that along k is missed by this ray altogether, and the triangle with it."""
    os_, ds_ = [], []
    for mesh in geom.meshes:
        tri = mesh.world_triangles()
        pick = np.arange(0, len(tri), max(1, -(-len(tri) // per_mesh)))
        t = tri[pick]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        ln = np.sqrt((nrm * nrm).sum(axis=1))
        good = ln > 10.0 * (DET_MIN + DELTA)
        t, nrm = t[good], nrm[good] / ln[good][:, None]
        c = t.mean(axis=1)
        for k in range(3):
            others = [j for j in range(3) if j != k]
            j = np.where(np.abs(nrm[:, others[0]]) >= np.abs(nrm[:, others[1]]), others[0], others[1])
            facing = np.abs(nrm[np.arange(len(t)), j])
            for pick_corner in (np.argmax, np.argmin):
                corner = t[np.arange(len(t)), pick_corner(t[:, :, k], axis=1)]
                ok = (np.abs(corner[:, k] - c[:, k]) > 0.0) & (facing > 0.05)
                p = corner[ok] + FACE_EPS * (c[ok] - corner[ok])
                dirs = np.zeros((int(ok.sum()), 3))
                dirs[np.arange(len(dirs)), j[ok]] = 1.0
                os_.append((p - TARGET_H * geom.radius * dirs).astype(np.float32))
                ds_.append(dirs.astype(np.float32))
    return np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds_))


def targets_covered(geom, answer, mesh, face):
    """The share of the triangles aimed at for which at least one of their rays is decided and answered by that triangle."""
    ok = answer["decided"] & answer["hit"] & (answer["mesh"] == mesh) & (answer["face"] == face)
    key = mesh.astype(np.int64) * (1 << 32) + face
    keys, inv = np.unique(key, return_inverse=True)
    got = np.zeros(len(keys), bool)
    np.logical_or.at(got, inv, ok)
    return got.mean(), keys[~got]


def tmax_multiples(t, radius):
    """per ray, from its brute-force distance: 0.5 t, 0.999 t, 1.001 t, 2 t, +inf; for a miss: 1, the scene radius, +inf"""
    k = np.arange(len(t)) % 5
    mul = np.select([k == 0, k == 1, k == 2, k == 3], [0.5, 0.999, 1.001, 2.0], np.inf)
    with np.errstate(invalid="ignore"):
        out = np.where(np.isfinite(t), t * mul, np.select([k % 3 == 0, k % 3 == 1], [1.0, radius], np.inf))
    return out.astype(np.float32)


def compare_closest(answer, hits, radius, judged=None):
    """Worst disagreement of HIT_DTYPE records with the brute force on the judged (default: decided) rays:
    dict(n, wrong: indices whose hit flag, mesh, face or front_face differ, t, uv, normal: largest errors)."""
    j = answer["decided"] if judged is None else judged
    h = answer["hit"]
    wrong = j & ((hits["hit"] != 0) != h)
    both = j & h & (hits["hit"] != 0)
    wrong |= both & ((hits["mesh_index"] != answer["mesh"]) | (hits["face_index"] != answer["face"]) |
                     ((hits["front_face"] != 0) != answer["front_face"]))
    cmp = both & ~wrong
    out = dict(n=int(j.sum()), wrong=np.flatnonzero(wrong), t=0.0, uv=0.0, normal=0.0)
    if cmp.any():
        t = answer["t"][cmp]
        out["t"] = float((np.abs(hits["t"][cmp].astype(np.float64) - t) / (np.maximum(t, radius) * answer["invcos"][cmp])).max())
        out["uv"] = float(max(np.abs(hits["u"][cmp].astype(np.float64) - answer["u"][cmp]).max(),
                              np.abs(hits["v"][cmp].astype(np.float64) - answer["v"][cmp]).max()))
        a, b = hits["normal"][cmp].astype(np.float64), answer["normal"][cmp]
        cr = np.cross(a, b)
        out["normal"] = float(np.arctan2(np.sqrt((cr * cr).sum(axis=1)), (a * b).sum(axis=1)).max())
    return out
