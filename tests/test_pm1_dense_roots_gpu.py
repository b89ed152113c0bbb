"""ptrt_set_option "pm1_dense_roots": PMODE 1 deals the root-box tests of a trace whose live rays fill at most half the
wave over all 64 lanes (build_pairs_dense, pt_render.hip.h).  It builds the pair list the lock-step loop builds, so every
buffer, generator state and ray count must equal the oracle's AND the other setting's, bit for bit."""
import numpy as np
import pytest

from common import assert_frames_equal, bits, render_both

pytestmark = pytest.mark.gpu


def _cornell(P, s):
    P.scenes.cornell(s)


def _cubes(n):
    """n single-leaf meshes in one TLAS leaf (odd counts against 2 and 4 meshes per round): every third an instance with its
    own transform (head flag bit 0), every fourth transmissive (bit 1: skipped by shadow rays), under a point light."""
    def make(P, s):
        rs = np.random.RandomState(100 + n)
        for k in range(n):
            mat = P.Material(tuple(rs.uniform(0.2, 0.9, 3)), float(rs.uniform(0.05, 0.8)), float(k % 5 == 2),
                             transmission=1.0 if k % 4 == 1 else 0.0, ior=1.4)
            m = s.addCube(mat)
            pos = (float(rs.uniform(-2.5, 2.5)), float(rs.uniform(-1.5, 1.5)), float(rs.uniform(-8, -4)))
            if k % 3 == 0:
                s.setPosition(m, pos)
                s.setRotation(m, tuple(rs.uniform(-1, 1, 3)))
                s.setInstanceScale(m, tuple(rs.uniform(0.4, 1.2, 3)))
            else:
                s.scale(m, tuple(rs.uniform(0.4, 1.2, 3)))
                s.moveTo(m, pos)
        s.addPointLight((0.5, 4.0, -3.0), (1.0, 0.95, 0.9), 40.0)
    return make


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


def _both_ways(P, O, blue_noise, make, size, spp, depth, frames, opts):
    got = {}
    cpu = None
    for dense in (0, 1):
        s = P.Scene(size[0], size[1])
        make(P, s)
        for k, v in opts.items():
            s.set_option(k, v)
        s.set_option("pm1_dense_roots", dense)
        if cpu is None:
            got[dense], cpu = render_both(P, O, s, blue_noise, spp, depth, frames)
        else:
            got[dense] = _gpu_frames(P, s, spp, depth, frames)
        assert s.get_option("pmode") == 1, "the scene does not run PMODE 1"
        assert s.get_option("pm1_dense_roots_eff") == dense
        if "refill" in opts:
            assert s.get_option("refilled") == (1 if opts["refill"] else 0)
        s.close()
    for dense in (0, 1):
        assert_frames_equal(got[dense], cpu)
    for f, (a, b) in enumerate(zip(got[0], got[1])):
        assert a["stats"] == b["stats"], f"frame {f}: ray counts {a['stats']} vs {b['stats']}"
        assert "shadow_rays_walked" in a["stats"]
        for k in ("accum", "normal", "depth", "object_id", "rgb8", "rng"):
            assert np.array_equal(bits(a[k]), bits(b[k])), f"frame {f}: {k} differs between pm1_dense_roots 0 and 1"


@pytest.mark.parametrize("refill", [0, 2])
@pytest.mark.parametrize("size", [(64, 64), (8, 8), (1, 1), (13, 9)])
def test_cornell_dense_roots(P, O, blue_noise, size, refill):
    """4 spp, 4 bounces with the samples in step: the shadow traces and the deep bounces carry half a wave and less; the
    8x8 and 1x1 frames have few rays from the first call, 13x9 has ragged tiles."""
    _both_ways(P, O, blue_noise, _cornell, size, 4, 4, 2, dict(refill=refill))


@pytest.mark.parametrize("refill", [0, 2])
@pytest.mark.parametrize("sync", [0, 1])
def test_rays_thin_out_and_come_back(P, O, blue_noise, sync, refill):
    """1 spp, 6 bounces: Russian roulette takes the live rays of a tile's wave through 32 and 16; with refill 2 (and with
    sample_sync 0) finished lanes take new pixels, so the count climbs back over both thresholds inside one tile."""
    _both_ways(P, O, blue_noise, _cornell, (40, 24), 1, 6, 3, dict(refill=refill, sample_sync=sync))


@pytest.mark.parametrize("refill", [0, 2])
@pytest.mark.parametrize("n", [1, 9, 17])
def test_mesh_counts_instances_and_glass(P, O, blue_noise, n, refill):
    _both_ways(P, O, blue_noise, _cubes(n), (40, 24), 2, 4, 2, dict(refill=refill))


@pytest.mark.parametrize("opts", [dict(force_full=1, refill=0), dict(force_full=1, refill=2), dict(pm1_wg=2)],
                         ids=["full", "full-refill", "wg2"])
def test_other_pmode1_kernels(P, O, blue_noise, opts):
    """The all-materials kernel (both STREAM variants) and two tiles per workgroup share the builder."""
    _both_ways(P, O, blue_noise, _cornell, (40, 24), 2, 4, 2, opts)
