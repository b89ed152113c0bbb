"""The wireframe view (Scene::render_to_device_wireframe, ptrt_render_wireframe) without a GPU: the entry point refuses
what is not a live context and touches nothing, a host-only scene cannot render it, and the CPU restatement's rules
(tests/wireframe_restatement.py) hold on hand-computed values."""
import ctypes
import math

import numpy as np
import pytest

import wireframe_restatement as R


def test_refused_without_a_live_context(P):
    buf = ctypes.create_string_buffer(4096)  # stands in for a freed ptrt_ctx: never in the live set
    stale = ctypes.cast(buf, ctypes.c_void_p)
    before = bytes(buf.raw)
    out = np.full((8, 8, 3), 7, dtype=np.uint8)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    for handle in (None, stale):
        for kind in (0, 1, 2):
            assert P.lib.ptrt_render_wireframe(handle, 0.02, ptr, kind) == -1
    assert bytes(buf.raw) == before, "ptrt_render_wireframe wrote into a handle that is not a live context"
    assert b"ptrt_render_wireframe" in P.lib.ptrt_last_error(stale)
    # a host-only scene has no back end: its handle is NULL, the call is refused the same way
    s = P.Scene(8, 8, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    assert not s.ctx
    assert P.lib.ptrt_render_wireframe(s.ctx, 0.02, ptr, 0) == -1
    assert (out == 7).all(), "a refused call wrote into the target"
    s.close()


def test_host_only_scene_cannot_render_the_wireframe(P):
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    with pytest.raises(P.PtrtError, match="host-only"):
        s.render_wireframe_to_host(0.02)
    with pytest.raises(P.PtrtError, match="host-only"):
        s.render_to_device_wireframe(0, 0.02)
    s.close()


def test_gamma_of_zero_is_zero(O):
    """det_pow is only defined for x > 0; powf(0, 1 / 2.2) is 0, and so is a negative colour after the clamp."""
    c = np.array([0.0, -0.0, -0.5, 1e-30, 0.25], dtype=np.float32)
    g = R.gamma(c, O)
    assert g[0] == 0 and g[1] == 0 and g[2] == 0
    assert 0 < g[3] < 1e-10 and abs(g[4] - 0.25 ** (1 / 2.2)) < 1e-6
    # black sky, white edge, an emission: Reinhard, gamma, * 255.99, truncated (hand-computed: 255.99 * (c / (c + 1)) ** (1 / 2.2))
    rgb = R.reinhard_gamma_rgb8(np.array([[0, 0, 0], [1, 1, 1], [5, 0, 0.5]], dtype=np.float32), O)
    assert rgb.tolist() == [[0, 0, 0], [186, 186, 186], [235, 0, 155]]


def test_only_emission_x_selects_the_emission():
    e = np.array([[0, 5, 0], [2, 0, 0], [0, 0, 0], [-1, 3, 3], [0.5, 0.25, 4]], dtype=np.float32)
    assert R.edge_colour(e).tolist() == [[1, 1, 1], [2, 0, 0], [1, 1, 1], [1, 1, 1], [0.5, 0.25, 4]]


@pytest.mark.parametrize("x,y,seed", [(0, 0, 0xfd42f46a), (1, 0, 0x8a824ec0), (12345, 6789, 0x171a95ef),
                                      (15000, 15000, 0x8cc887a5)])
def test_lens_hash_disk(O, x, y, seed):
    """random_in_unit_disk_hash (camera.cuh:55-70): seeds computed by hand from the integer hash, then the point of the
    disk from them in double precision."""
    lo = seed & 0xFFFF
    hi = ((seed * 0x343FD + 0xC0F5) & 0xFFFFFFFF) & 0xFFFF
    r, phi = math.sqrt((lo + 0.5) / 65536.0), 6.2831853 * (hi + 0.5) / 65536.0
    px, py = R.disk_hash(np.array([x]), np.array([y]), O)
    assert abs(px[0] - r * math.cos(phi)) < 2e-7 and abs(py[0] - r * math.sin(phi)) < 2e-7
    assert px[0] * px[0] + py[0] * py[0] < 1


def test_fma32_rounds_once():
    """dot() is fused; the restatement's fma must not round twice.  (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 midpoint:
    alone it rounds to even, with 2^-60 added it must round up -- rounding the float64 sum to float32 would round down."""
    a = np.float32(1 + 2 ** -12)
    assert R.fma32(a, a, np.float32(0)) == np.float32(1 + 2 ** -11)
    assert R.fma32(a, a, np.float32(2 ** -60)) == np.float32(1 + 2 ** -11 + 2 ** -23)
    assert R.fma32(a, a, np.float32(-(2 ** -60))) == np.float32(1 + 2 ** -11)
    rs = np.random.RandomState(1)
    x, y, z = (rs.uniform(-4, 4, 4096).astype(np.float32) for _ in range(3))
    got = R.fma32(x, y, z)
    want = (x.astype(np.float64) * y + z).astype(np.float32)  # (a double-rounding case among these is vanishingly rare)
    assert (got == want).mean() > 0.999


def test_primary_rays_of_a_pinhole_camera_are_unit_and_centred(P, O):
    s = P.Scene(32, 24, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    desc = ctypes.cast(s.flatten(), ctypes.POINTER(P.SceneDesc)).contents
    o, d = R.primary_rays(desc.camera, 32, 24, 0, 24, O)
    assert o.shape == d.shape == (32 * 24, 3)
    assert np.allclose((d.astype(np.float64) ** 2).sum(1), 1, atol=1e-6)
    assert (o == o[0]).all()
    # the four pixels around the image centre look symmetrically around the view direction
    c = d.reshape(24, 32, 3)[11:13, 15:17].reshape(4, 3).mean(0)
    fwd = -np.array([desc.camera.w.x, desc.camera.w.y, desc.camera.w.z])
    assert np.dot(c / np.linalg.norm(c), fwd / np.linalg.norm(fwd)) > 0.9999
    s.close()
