"""What every box of a mesh's BVH must be, written from the definition alone, and triangle soups whose Morton keys are known
before any arithmetic of the builder is restated.  No GPU, no library call.

The statement (`boxes`):
  * a leaf's box is the min / max over the three vertices of every face prim[start : start + count];
  * an inner node's box is the union of its children's boxes; an absent child (index < 0) contributes nothing;
  * a node that nothing below node 0 references is not part of the tree and has no statement (`reached` is False there).
min and max of float32 values are exact -- the result is one of the inputs -- so the statement carries no tolerance, and
computing it in float64 would give the same values; it is computed in float32.  Compare by VALUE with `==`: fminf / fmaxf may
return either zero where both signs occur, and -0.0 == +0.0.  No NaN and no infinity belongs in any input here.

`cell_soup` builds a soup whose 30-bit keys follow from integers the caller chose: two anchor faces pin the bounds of the
centroids to [0, 1] exactly (lo = 0, ext = 1), every other face sits at the centre of a cell of the 1024^3 lattice, and the key
of a face is the bit-interleave of its three cell numbers, x highest.  The order a stable sort gives those integers is the
order the builder must produce."""
from collections import namedtuple

import numpy as np

BIG = np.float32(1e30)      # the empty box: what a leaf slot without faces holds on the device, inverted so it takes no part

Statement = namedtuple("Statement", "lo hi depth widths reached")


def topology(nodes):
    """(n, 4) int: left, right, start, count of a structured node array (or of an (n, 4) array already)"""
    if getattr(nodes, "dtype", None) is not None and nodes.dtype.names:
        return np.stack([nodes["left"], nodes["right"], nodes["start"], nodes["count"]], axis=1).astype(np.int64)
    return np.asarray(nodes, np.int64).reshape(-1, 4)


def boxes(nodes, prim, faces, verts):
    """Statement(lo (n, 3) float32, hi (n, 3) float32, depth (n,), widths, reached (n,) bool) of the tree below node 0.
    `nodes`: the node array (structured, or (n, 4) left / right / start / count; count > 0 marks a leaf); `prim`: leaf slot ->
    face; `faces` (F, 3) vertex indices; `verts` (V, 3).  depth: 1 for node 0, a child's is its parent's + 1, 0 where not
    reached.  widths[d - 1]: the number of INNER nodes at depth d (the levels a refit walks, deepest last)."""
    topo = topology(nodes)
    n = len(topo)
    prim = np.asarray(prim, np.int64)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert np.isfinite(v).all(), "the statement takes finite vertices only"
    corners = v[f]                                                  # (F, 3 corners, 3 axes)
    fmin, fmax = corners.min(axis=1), corners.max(axis=1)
    lo = np.full((n, 3), BIG, np.float32)
    hi = np.full((n, 3), -BIG, np.float32)
    depth = np.zeros(n, np.int64)
    reached = np.zeros(n, bool)
    order, stack = [], [(0, 1)]
    while stack:                                                    # node 0's tree, parents before children
        i, d = stack.pop()
        assert 0 <= i < n and not reached[i], f"node {i}: not a tree"
        reached[i], depth[i] = True, d
        order.append(i)
        left, right, _, count = topo[i]
        if count <= 0:
            stack.extend((int(c), d + 1) for c in (left, right) if c >= 0)
    for i in reversed(order):                                       # ... and children before parents
        left, right, start, count = topo[i]
        if count > 0:
            ids = prim[start:start + count]
            lo[i], hi[i] = fmin[ids].min(axis=0), fmax[ids].max(axis=0)
        else:
            for c in (left, right):
                if c >= 0:
                    lo[i], hi[i] = np.minimum(lo[i], lo[c]), np.maximum(hi[i], hi[c])
    inner = reached & (topo[:, 3] <= 0)
    widths = [int((inner & (depth == d)).sum()) for d in range(1, int(depth.max()) + 1)]
    while widths and widths[-1] == 0:                               # (the deepest depth holds leaves only)
        widths.pop()
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return Statement(lo, hi, depth, widths, reached)


def scene_widths(per_mesh):
    """The inner-level widths of a scene: a refit walks depth d of every mesh in one step, so the widths add up per depth."""
    out = [0] * max((len(w) for w in per_mesh), default=0)
    for w in per_mesh:
        for d, k in enumerate(w):
            out[d] += k
    return out


def differing(got, st):
    """indices of the reached nodes whose boxes in the structured array `got` differ in VALUE from the statement's"""
    bad = (got["bmin"] != st.lo).any(axis=1) | (got["bmax"] != st.hi).any(axis=1)
    return np.flatnonzero(bad & st.reached)


def assert_boxes(got, st, what=""):
    """every reached node of `got` (structured: bmin, bmax) has the statement's box, by value"""
    assert len(got) == len(st.lo), f"{what}: {len(got)} nodes, the statement has {len(st.lo)}"
    bad = differing(got, st)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {int(st.reached.sum())} boxes differ from the statement, first node {i} at depth "
                             f"{int(st.depth[i])}: has {got['bmin'][i]} .. {got['bmax'][i]}, must be {st.lo[i]} .. {st.hi[i]}")


# ---- soups with keys known a priori ------------------------------------------------------------------------------------
CELLS = 1024                # cells per axis: 10 bits


def interleave30(cells):
    """(n, 3) cell numbers 0 .. 1023 -> 30-bit keys: bit b of x, y, z lands at bit 3b + 2, 3b + 1, 3b"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    assert ((cells >= 0) & (cells < CELLS)).all()
    keys = np.zeros(len(cells), np.int64)
    for b in range(10):
        for axis, up in ((0, 2), (1, 1), (2, 0)):
            keys |= ((cells[:, axis] >> b) & 1) << (3 * b + up)
    return keys


def _offsets(n, rng):
    """(n, 3 corners, 3 axes) float64 offsets, exact multiples of 2^-16 within 2^-11 that sum to zero over the corners"""
    o = rng.randint(-16, 17, size=(n, 2, 3)).astype(np.int64)
    o = np.concatenate([o, -(o[:, 0:1] + o[:, 1:2])], axis=1)
    return o.astype(np.float64) / 65536.0


def cell_soup(cells, rng, anchors=True):
    """(tris (n, 9) float32, keys (n,) int64, order (n,) int32) for the faces of `cells` ((m, 3) lattice cells 0 .. 1023), with
    an anchor face in front (centroid (0, 0, 0) exactly: cell 0 0 0) and one behind (centroid (1, 1, 1) exactly: t = 1 is
    clamped into cell 1023 1023 1023), so n = m + 2.  A face's corners are its centre ((k + 1/2) / 1024 per axis; 0 and 1 for the
    anchors) plus offsets that are multiples of 2^-16 and sum to zero: corners and their sum 3 * centre are exact in float32,
    and (a + b + c) * fl(1/3) is the centre within two roundings (relative 2^-23) -- 2^-14 would still be an eighth of the
    distance to the cell's wall, 2^-11.  Both anchors come out exact: 0 * fl(1/3) = 0, and 3 * fl(1/3) = 1 + 2^-25 rounds
    to 1.  `order`: the stable sort of the keys.
    anchors=False: no anchors and every face in ONE cell -- all centroids are the same float, ext = 0, every key 0."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    centre = (cells.astype(np.float64) + 0.5) / CELLS
    if anchors:
        centre = np.concatenate([np.zeros((1, 3)), centre, np.ones((1, 3))])
        cells = np.concatenate([np.zeros((1, 3), np.int64), cells, np.full((1, 3), CELLS - 1, np.int64)])
        keys = interleave30(cells)
    else:
        assert (cells == cells[0]).all(), "without anchors the keys are known only where all centroids coincide"
        keys = np.zeros(len(cells), np.int64)
    tris64 = centre[:, None, :] + _offsets(len(centre), rng)
    tris = tris64.astype(np.float32)
    assert (tris.astype(np.float64) == tris64).all(), "a corner is not exact in float32"
    # the premise, checked in the builder's own float32 expression but against the cell walls, not against the builder
    c = ((tris[:, 0] + tris[:, 1]) + tris[:, 2]) * np.float32(1.0 / 3.0)
    assert c.dtype == np.float32 and (np.abs(c.astype(np.float64) - centre) <= 2.0 ** -14).all()
    if anchors:
        assert (c[0] == 0).all() and (c[-1] == 1).all()
    else:
        assert (c == c[0]).all()
    return tris.reshape(-1, 9), keys, np.argsort(keys, kind="stable").astype(np.int32)


def key_cells(m, rng):
    """name -> (m, 3) cells for the non-anchor faces of cell_soup: the keys at which a sort goes wrong"""
    r = rng.randint
    pick = np.array([0, 256, 512, 768])
    few = np.stack([r(0, CELLS, max(m // 8, 1)) for _ in range(3)], axis=1)
    alt = np.where((np.arange(m) % 2 == 0)[:, None], np.array([[512, 3, 3]]), np.array([[1, 2, 3]]))
    return {
        "one_cell": np.tile(np.array([[5, 700, 33]]), (m, 1)),                        # every key equal: the identity
        "two_cells": alt,                                                             # the higher key first, face by face
        "bits_24_29": np.stack([pick[r(0, 4, m)] for _ in range(3)], axis=1),         # bits 8, 9 of each axis
        "bits_0_7": np.stack([r(0, 4, m), r(0, 8, m), r(0, 8, m)], axis=1),           # z, y: bits 0-2; x: bits 0, 1
        "flat": np.stack([r(0, CELLS, m), np.full(m, 300), r(0, CELLS, m)], axis=1),  # one axis constant
        "line": np.stack([r(0, CELLS, m), np.full(m, 77), np.full(m, 900)], axis=1),  # two axes constant
        "repeats": few[r(0, len(few), m)],                                            # about m / 8 distinct keys
        "outlier": np.stack([r(0, 2, m) for _ in range(3)], axis=1),                  # the far anchor leaves eight cells to the rest
    }


def height_soup(n, rng, t=0.0, lift=0.0):
    """(n, 9) float32: small random triangles scattered about a water-like height field y(x, z; t) + lift over [-8, 8]^2"""
    c = np.zeros((n, 3))
    c[:, 0], c[:, 2] = rng.uniform(-8, 8, n), rng.uniform(-8, 8, n)
    c[:, 1] = 0.4 * np.sin(0.9 * c[:, 0] + t) * np.cos(0.7 * c[:, 2] - 0.5 * t) + lift
    return (c[:, None, :] + rng.uniform(-0.06, 0.06, (n, 3, 3))).astype(np.float32).reshape(n, 9)
