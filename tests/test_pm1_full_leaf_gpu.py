"""ptrt_set_option "pm1_full_leaf": when every leaf staged for PMODE 1 has exactly pair_max_leaf triangles, the triangle
loops of closest_hit_pairs / any_hit_pairs leave out the partial-leaf handling (pt_render.hip.h).  The same
tests run in the same order, so every buffer, generator state and ray count must equal the oracle's AND the other setting's,
bit for bit.  Also here: rcp_ieee_above (tri_test's reciprocal) against the compiler's division over all 2^32 inputs."""
import ctypes as C

import numpy as np
import pytest

from common import assert_frames_equal, bits, render_both

pytestmark = pytest.mark.gpu


def _cornell(P, s):
    P.scenes.cornell(s)


def _cornell_quads(P, s):
    P.scenes.cornell(s, quads=True)


def _cornell_instance(P, s):
    """The Cornell box plus a cube that keeps an instance transform (not baked): any_transform, so pair_split is off and every
    batch runs at one lane per pair; all leaves still hold 12 triangles."""
    P.scenes.cornell(s)
    m = s.addCube(P.Material((0.8, 0.6, 0.3), 0.4, 0.0))
    s.setPosition(m, (1.2, -1.0, -3.5))
    s.setRotation(m, (0.3, 0.7, -0.2))
    s.setInstanceScale(m, (0.8, 1.3, 0.6))


def _gpu_frames(P, s, spp, depth, frames):
    """The GPU half of common.render_both: same calls, same order."""
    s.setPerfSamplesPerPixel(spp)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(P.DEFAULT_SEED)
    s.set_option("count_rays", 1)
    out = []
    for f in range(frames):
        rgb = s.render_to_host()
        out.append(dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                        object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats()))
    return out


_oracle = {}  # (scene, size, spp, depth, frames) -> the oracle's frames: computed once, shared by the option sets, never changed


def _both_ways(P, O, blue_noise, make, size, spp, depth, frames, opts, settings=(0, -1), eff=None):
    """`eff`: what pm1_full_leaf_eff must read per setting (default: on unless the option is 0)"""
    key = (make.__name__, size, spp, depth, frames)
    got = {}
    for fl in settings:
        s = P.Scene(size[0], size[1])
        make(P, s)
        for k, v in opts.items():
            s.set_option(k, v)
        s.set_option("pm1_full_leaf", fl)
        if key not in _oracle:
            got[fl], _oracle[key] = render_both(P, O, s, blue_noise, spp, depth, frames)
        else:
            got[fl] = _gpu_frames(P, s, spp, depth, frames)
        assert s.get_option("pmode") == 1, "the scene does not run PMODE 1"
        want = (0 if fl == 0 else 1) if eff is None else eff
        assert s.get_option("pm1_full_leaf_eff") == want, (fl, s.get_option("pm1_full_leaf_eff"))
        if "refill" in opts:  # (the two-tiles-per-workgroup kernel has no lane-refill variant: forced on, it still reads 0)
            assert s.get_option("refilled") == (1 if opts["refill"] and opts.get("pm1_wg", 1) != 2 else 0)
        s.close()
    for fl in settings:
        assert_frames_equal(got[fl], _oracle[key])
    a0 = got[settings[0]]
    for fl in settings[1:]:
        for f, (a, b) in enumerate(zip(a0, got[fl])):
            assert a["stats"] == b["stats"], f"frame {f}: ray counts {a['stats']} vs {b['stats']}"
            assert "shadow_rays_walked" in a["stats"]
            for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
                assert np.array_equal(bits(a[k]), bits(b[k])), f"frame {f}: {k} differs between pm1_full_leaf {settings[0]} and {fl}"


CASES = {"64x48": ((64, 48), 4, 4), "ragged37x21": ((37, 21), 4, 4), "8x8": ((8, 8), 1, 1)}


@pytest.mark.parametrize("wg", [1, 2])
@pytest.mark.parametrize("refill", [0, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_cornell_full_leaf(P, O, blue_noise, case, refill, wg):
    """64x48 at 4 spp, 4 bounces: full batches and partial ones at 1, 2 and 4 lanes per pair; 37x21: ragged tiles; 8x8 at
    1 spp, 1 bounce: one tile, thin waves."""
    size, spp, depth = CASES[case]
    _both_ways(P, O, blue_noise, _cornell, size, spp, depth, 2, dict(refill=refill, pm1_wg=wg))


@pytest.mark.parametrize("refill", [0, 2])
def test_mixed_leaves_keep_the_guarded_loop(P, O, blue_noise, refill):
    """Leaves of 2 and of 12 triangles: the fast path is off whatever the option says."""
    _both_ways(P, O, blue_noise, _cornell_quads, (40, 24), 2, 4, 2, dict(refill=refill), settings=(0, -1, 1), eff=0)


@pytest.mark.parametrize("refill", [0, 2])
def test_instanced_box_one_lane_per_pair(P, O, blue_noise, refill):
    _both_ways(P, O, blue_noise, _cornell_instance, (40, 24), 2, 4, 2, dict(refill=refill))


def test_queries_take_the_same_path(P):
    """ray_query_kernel's PMODE 1 shares the two functions: closest hit and occlusion over 4,096 random rays in the box,
    option 0 against -1."""
    import torch
    rs = np.random.RandomState(5)
    n = 4096
    o = rs.uniform(-4.5, 4.5, (n, 3)).astype(np.float32)
    o[:, 2] = rs.uniform(-9.5, 4.0, n).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    tmax = rs.uniform(0.0, 12.0, n).astype(np.float32)
    s = P.Scene(32, 32)
    P.scenes.cornell(s)
    s.uploadToGPU()
    to, td, tt = (torch.from_numpy(a).cuda() for a in (o, d, tmax))
    got = {}
    for fl in (0, -1):
        s.set_option("pm1_full_leaf", fl)
        h = s.query_closest(to, td).cpu().numpy()
        assert s.get_option("query_pmode") == 1
        f = s.query_occluded(to, td, tt).cpu().numpy()
        got[fl] = (h, f)
    s.close()
    assert np.array_equal(got[0][0], got[-1][0]), "closest-hit records differ between pm1_full_leaf 0 and -1"
    assert np.array_equal(got[0][1], got[-1][1]), "occlusion flags differ between pm1_full_leaf 0 and -1"
    hit = np.ascontiguousarray(got[0][0]).view(P.HIT_DTYPE).reshape(n)["hit"]
    assert hit.mean() > 0.5 and 0 < got[0][1].mean() < 1


def test_rcp_ieee_above_is_exact_where_its_contract_holds(P):
    """rcp_ieee_above (v_rcp_f32 + one Newton step, guarded by |y| < 2^60 alone) == 1.0f / y for every input with
    |y| >= 2^-60, NaN and the infinities included: all 2^32 bit patterns are swept, the mismatches counted."""
    s = P.Scene(8, 8)
    out = (C.c_uint * 9)()
    P.lib.ptrt_debug_rcp_above_check.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    assert P.lib.ptrt_debug_rcp_above_check(s.ctx, out) == 0
    s.close()
    assert out[0] == 0, f"{out[0]} mismatches, first inputs {[hex(v) for v in list(out)[1:9]]}"
