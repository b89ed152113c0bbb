"""Instance poses -> matrices (ptrt_set_instance_poses_device), the parts that need no GPU: the numpy restatement of the device's
arithmetic (tests/pose_restatement.py) against the C++ mirror's Transform3D, which was written separately from the same
reference text; the reference's quirks one by one; and the new entry points without a context.  No bound here comes from the
code under test: with rotation exactly +0 both arithmetics have sine 0 and cosine 1 and the matrices are compared for equality;
with rotations the two differ in their sines alone, and the bound is three times what 200,000 poses gave on the CPU."""
import ctypes as C

import numpy as np
import pytest

import pose_restatement as R

N = 512


def mirror(P, pos, rot, scl):
    """(world, inverse, normal rows (n, 3, 4) -- a normal row's fourth word zeroed, as the records keep it --, has_transform) of
    a HOST_ONLY scene of one-triangle meshes with these poses, from flatten()"""
    n = len(pos)
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    mat = P.Material((0.6, 0.6, 0.6), 0.5)
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    for k in range(n):
        m = s.addTriangles(tri, mat)
        s.setPosition(m, pos[k])
        s.setRotation(m, rot[k])
        s.setInstanceScale(m, scl[k])
    s.setCamera((0, 0, 20), (0, 0, 0), (0, 1, 0), 40.0)
    d = s.flatten().contents
    assert d.mesh_count == n
    out = [np.zeros((n, 3, 4), np.float32) for _ in range(3)]
    has = np.zeros(n, np.int32)
    for k in range(n):
        M = d.meshes[k]
        for a, src in zip(out, (M.world, M.inverse, M.normal)):
            a[k] = np.array(list(src), np.float32).reshape(4, 4)[:3]
        has[k] = M.has_transform
    out[2][:, :, 3] = 0.0
    s.close()
    return out[0], out[1], out[2], has


def random_poses(n, seed, rotated):
    rs = np.random.RandomState(seed)
    pos = rs.uniform(-10, 10, (n, 3)).astype(np.float32)
    rot = rs.uniform(-np.pi, np.pi, (n, 3)).astype(np.float32) if rotated else np.zeros((n, 3), np.float32)
    scl = rs.uniform(0.2, 3.0, (n, 3)).astype(np.float32)
    return pos, rot, scl


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- (a) zero rotation: the restatement is the mirror, bit for bit ---------------------------------------------------------------
def test_zero_rotation_equals_the_mirror_bit_for_bit(P, O):
    pos, rot, scl = random_poses(N, 11, rotated=False)
    pos[:8] = 0.0                                             # some at the origin, some unscaled in x: both has_transform values
    scl[:4, 0] = 1.0
    assert not np.signbit(rot).any()
    s0, c0 = R.detmath_sincos(O)(np.zeros(1, np.float32))
    assert bits(s0)[0] == 0 and c0[0] == 1.0
    got = R.compose(pos, rot, scl, R.detmath_sincos(O))
    want = mirror(P, pos, rot, scl)
    for name, g, w in zip(("world", "inverse", "normal"), got, want):
        bad = np.flatnonzero((bits(g) != bits(w)).any(axis=(1, 2)))
        assert bad.size == 0, f"{name}: {bad.size} of {N} poses differ, first {bad[0]}: {g[bad[0]]} vs the mirror's {w[bad[0]]}"
    assert np.array_equal(got[3], want[3])
    assert 0 < got[3].sum() < N


# ---- (b) random rotations: two different sines, nothing else ------------------------------------------------------------------------
def test_random_rotations_stay_within_the_two_sines_of_the_mirror(P, O):
    """Largest |world - mirror's world| over the 3x3 parts, in units of max(scale): 3.06e-7 over 200,000 poses on the CPU
    (position +-10, rotation +-pi, scale 0.2-3); the bound is 1e-6, three times that."""
    pos, rot, scl = random_poses(N, 12, rotated=True)
    got = R.compose(pos, rot, scl, R.detmath_sincos(O))
    want = mirror(P, pos, rot, scl)
    err = np.abs(got[0][:, :, :3].astype(np.float64) - want[0][:, :, :3]).max(axis=(1, 2)) / scl.max(axis=1)
    print(f"pose restatement (detmath sines) against the mirror (libm sines), {N} poses: largest world 3x3 difference "
          f"{err.max():.3e} x max(scale)")
    assert err.max() <= 1e-6
    assert np.array_equal(bits(got[0][:, :, 3]), bits(pos)) and np.array_equal(bits(want[0][:, :, 3]), bits(pos))
    assert np.array_equal(got[3], want[3]) and got[3].all()
    # ... and the restatement over numpy's sines stays as close: the difference is the sine, not the restatement
    lib = R.compose(pos, rot, scl, R.libm_sincos)
    err = np.abs(lib[0][:, :, :3].astype(np.float64) - want[0][:, :, :3]).max(axis=(1, 2)) / scl.max(axis=1)
    assert err.max() <= 1e-6


# ---- (c) the quirks ---------------------------------------------------------------------------------------------------------------
def one(O, pos=(0, 0, 0), rot=(0, 0, 0), scl=(1, 1, 1)):
    w, i, n, h = R.compose([pos], [rot], [scl], R.detmath_sincos(O))
    return w[0], i[0], n[0], int(h[0])


EYE = np.eye(4, dtype=np.float32)[:3]


def test_a_tiny_determinant_gives_the_identity_inverse(O):
    w, i, n, h = one(O, scl=(1e-4, 1e-4, 1e-4))              # det = 1e-12 < 1e-10
    assert np.array_equal(i, EYE) and np.array_equal(n, EYE)
    assert np.array_equal(np.diag(w[:, :3]), np.full(3, 1e-4, np.float32)) and h == 1
    w, i, n, h = one(O, scl=(1e-3, 1e-3, 1e-3))              # det = 1e-9: a true inverse
    assert np.allclose(np.diag(i[:, :3]), 1e3, rtol=1e-6) and np.allclose(np.diag(n[:, :3]), 1e3, rtol=1e-6)


def test_has_transform_thresholds(O):
    for axis in range(3):
        for v, want in ((0.0009, 0), (0.0011, 1)):
            p = [0.0, 0.0, 0.0]
            p[axis] = v
            assert one(O, pos=p)[3] == want, f"position length {v} along axis {axis}"
            assert one(O, rot=p)[3] == want, f"rotation length {v} along axis {axis}"
            p[axis] = -v
            assert one(O, pos=p)[3] == want and one(O, rot=p)[3] == want


def test_only_scale_x_makes_an_instance(O):
    w, i, n, h = one(O, scl=(1, 2, 1))
    assert h == 0                                            # scaled in y alone at the origin, unrotated: NOT an instance
    assert w[1, 1] == 2.0 and i[1, 1] == 0.5
    assert one(O, scl=(1, 1, 3))[3] == 0
    assert one(O, scl=(1.002, 1, 1))[3] == 1
    assert one(O, scl=(0.998, 1, 1))[3] == 1
    assert one(O, scl=(1.0005, 1, 1))[3] == 0


def test_the_translation_sits_in_the_fourth_column_and_a_nan_stays_in_its_row(O):
    w, i, n, h = one(O, pos=(3, -4, 5), scl=(2, 2, 2))
    assert np.array_equal(w[:, 3], np.array([3, -4, 5], np.float32)) and np.array_equal(n[:, 3], np.zeros(3, np.float32))
    w, i, n, h = one(O, pos=(1, 2, 3), scl=(2, np.nan, 2))
    assert np.isnan(w[1, :3]).all() and not np.isnan(w[[0, 2]]).any() and w[1, 3] == 2.0 and h == 1


# ---- (d) the entry points without a context ------------------------------------------------------------------------------------------
def test_entry_points_refuse_a_null_context(P):
    pose = (P.InstancePose * 1)()
    xf = (P.InstanceXform * 1)()
    assert C.sizeof(P.InstancePose) == 36 and P.InstancePose.rotation.offset == 12 and P.InstancePose.scale.offset == 24
    assert P.lib.ptrt_set_instance_poses_device(None, 0, 1, C.cast(pose, C.c_void_p)) == -1      # PTRT_E_INVALID
    assert P.lib.ptrt_read_instance_transforms(None, 0, 1, C.cast(xf, C.c_void_p)) == -1
    assert P.lib.ptrt_abi_version() == 6
    for n in ("set_instance_poses_device", "read_instance_transforms"):
        assert callable(getattr(P.Scene, n, None)), n
    s = P.Scene(16, 16, device=P.HOST_ONLY)                   # no back end: the binding checks the tensor first
    with pytest.raises(ValueError):
        s.set_instance_poses_device(0, np.zeros((1, 9), np.float32))
    s.close()
