"""configs[4]'s path reached from the reference's call sites only.

oracle/_ref/transfer_probe is the reference's own src/common/PTRTtransfer.cuh compiled in place over the C++ mirror
(tools/refapp/transfer_probe.cpp).  On the GPU it builds a scene with buildPTScene, renders, and twice lets the
"application" move a `Triangles` mesh's vertices, a dynamic cube and the camera and call the UNCHANGED sequence
    updatePTScene(scene, unified)   ->  ... mesh->bvhDirty = mesh->vertsDirty = true ... scene.commitObjectChanges()
    updatePTCamera(scene, unified)
then renders again -- under each dynamic-geometry policy (Scene::setDynamicGeometryPolicy: the one line an application
adds).  What it reported is held in tests/golden/transfer_probe_gpu.json (tests/golden/make_transfer_probe_golden.py); where
the probe is built, it is run as well and must still report exactly that.  Checked here: under GpuRefit / GpuRebuild the
commits reach ptrt_update_vertices + ptrt_refit / ptrt_build_bvh (the geometry is uploaded ONCE), and under every policy each
frame -- RGB8 and the HDR image -- equals the oracle's rendering of the scene the probe reports, which in turn equals, byte
for byte, the scene the Python recipe builds the same way."""
import json
import os
import subprocess

import numpy as np
import pytest

from common import bits
from make_transfer_probe_golden import EXE, digest, summarize  # (tests/golden is on the path: conftest.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "transfer_probe_gpu.json")))


@pytest.mark.parametrize("policy", ["HostRebuild", "GpuRefit", "GpuRebuild"])
def test_update_pt_scene_then_commit_reaches_the_gpu_path(P, O, blue_noise, tmp_path, policy):
    w, h, spp, depth = GOLD["width"], GOLD["height"], GOLD["spp"], GOLD["depth"]
    frames = GOLD["policies"][policy]
    if os.path.exists(EXE):  # built from the reference's sources (tools/refapp): the probe itself still reports the golden
        dump = str(tmp_path / f"transfer_{P.Scene.POLICIES[policy]}.bin")
        # the probe links libptrt_amd.so by name and its run path is the directory it was built in: point the loader at this tree's
        pkg = os.path.dirname(os.path.abspath(P.__file__))
        env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(p for p in (pkg, os.environ.get("LD_LIBRARY_PATH")) if p))
        r = subprocess.run([EXE, "gpu", str(P.Scene.POLICIES[policy]), dump], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert summarize(dump) == dict(width=w, height=h, spp=spp, depth=depth, frames=frames)
    assert (w, h) == P.scenes.TRANSFER_SIZE and len(frames) == 3

    # the reference's caller reached the refit: two commits on the GPU path, the geometry uploaded once
    if policy == "HostRebuild":
        assert [(f["gpu_commits"], f["uploads"]) for f in frames] == [(0, 1), (0, 2), (0, 3)]
    else:
        assert [(f["gpu_commits"], f["uploads"]) for f in frames] == [(0, 1), (1, 1), (2, 1)]

    # the same sequence through the Python recipe, same policy: same scene bytes at every step, same frames, == oracle
    s = P.Scene(w, h, device=0)
    water, cube = P.scenes.transfer_demo(s)
    s.setDynamicGeometryPolicy(policy)
    s.setPerfSamplesPerPixel(spp)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, w * h)
    for k, f in enumerate(frames):
        if k > 0:
            P.scenes.transfer_step(s, water, cube, k)
        fc = s.getFrameCount()  # (a commit restarts the accumulation: the frame index, and with it the jitter, begins again)
        assert fc == 0
        rgb = s.render_to_host()
        accum = s.read(P.BUF_ACCUM)
        scene = s.serialize()
        assert len(scene) == f["scene_bytes"] and digest(scene) == f["scene_sha256"], f"step {k}: the probe's scene and the recipe's differ"
        assert digest(rgb.reshape(-1, 3).tobytes()) == f["rgb8_sha256"] and digest(bits(accum).tobytes()) == f["accum_sha256"], f"step {k}"
        c = O.render(s.flatten(), w, h, spp, depth, fc, blue_noise, rng, threads=8)
        assert np.array_equal(bits(c["accum"]), bits(accum))
        assert digest(bits(c["accum"]).tobytes()) == f["accum_sha256"], f"step {k}: the probe's frame differs from the oracle's"
        assert digest(np.ascontiguousarray(O.tonemap(c["accum"], w, h, threads=4).reshape(-1, 3)).tobytes()) == f["rgb8_sha256"]
        assert np.array_equal(s.read(P.BUF_RNG), rng)
    assert s.commitCounts() == ((0, 3) if policy == "HostRebuild" else (2, 1))
    assert accum.any() and frames[1]["accum_sha256"] != frames[2]["accum_sha256"]
    s.close()


@pytest.mark.parametrize("cube_moves", [True, False])
@pytest.mark.parametrize("policy", ["GpuRefit", "GpuRebuild"])
def test_fewer_triangles_right_after_a_gpu_commit(P, O, blue_noise, policy, cube_moves):
    """A commit on the GPU path, then at once -- no flatten(), read or frame in between -- a commit that rewrites the same
    mesh with fewer triangles: the host tree the first commit left stale cannot describe the new arrays, so it is neither read
    back nor refitted but rebuilt and uploaded, and the frame equals the oracle's.  `cube_moves`: the first step is
    transfer_step, whose moved instance makes that commit sync the host trees itself; without it the mark is still pending
    when the smaller mesh arrives (tests/test_host_commit_traces.py has the call sequence)."""
    w, h = 96, 64
    s = P.Scene(w, h, device=0)
    water, cube = P.scenes.transfer_demo(s)
    s.setDynamicGeometryPolicy(policy)
    s.setPerfSamplesPerPixel(1)
    s.setMaxBounceDepth(3)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, w * h)

    def frame():
        fc = s.getFrameCount()
        rgb = s.render_to_host()
        c = O.render(s.flatten(), w, h, 1, 3, fc, blue_noise, rng, threads=4)
        assert np.array_equal(bits(s.read(P.BUF_ACCUM)), bits(c["accum"]))
        assert np.array_equal(O.tonemap(c["accum"], w, h).reshape(-1), rgb.reshape(-1))

    frame()
    if cube_moves:
        P.scenes.transfer_step(s, water, cube, 1)
    else:
        s.setTriangleSoup(water, P.scenes.transfer_sheet(1))
        s.commitObjectChanges()
    assert s.commitCounts() == (1, 1)
    s.setTriangleSoup(water, P.scenes.transfer_sheet(2)[:200])
    s.commitObjectChanges()
    assert s.commitCounts() == (1, 2)
    frame()
    assert s.commitCounts() == (1, 2)
    s.close()


def test_policy_falls_back_when_the_topology_changes(P, O, blue_noise):
    """A commit whose mesh has a different face count (or a new mesh) takes the reference's route whatever the policy, and the
    policy resumes on the next commit with the new topology."""
    w, h = 96, 64
    s = P.Scene(w, h, device=0)
    water, cube = P.scenes.transfer_demo(s)
    s.setPerfSamplesPerPixel(1)
    s.setMaxBounceDepth(3)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.setDynamicGeometryPolicy("GpuRefit")  # chosen AFTER the upload: the untouched meshes' face lists are what the device holds
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, w * h)

    def frame(k):
        fc = s.getFrameCount()
        rgb = s.render_to_host()
        c = O.render(s.flatten(), w, h, 1, 3, fc, blue_noise, rng, threads=4)
        assert np.array_equal(bits(s.read(P.BUF_ACCUM)), bits(c["accum"])), k
        assert np.array_equal(O.tonemap(c["accum"], w, h).reshape(-1), rgb.reshape(-1))

    frame(0)
    P.scenes.transfer_step(s, water, cube, 1)
    assert s.commitCounts() == (1, 1)
    frame(1)
    s.setTriangleSoup(water, P.scenes.transfer_sheet(2)[:200])  # fewer triangles: host rebuild + upload
    s.commitObjectChanges()
    assert s.commitCounts() == (1, 2)
    frame(2)
    s.setTriangleSoup(water, P.scenes.transfer_sheet(1)[:200])  # same count again: back on the GPU path
    s.commitObjectChanges()
    assert s.commitCounts() == (2, 2)
    frame(3)
    s.scale(s.addCube(P.Material((0.5, 0.5, 0.5))), (0.3, 0.3, 0.3))  # a new mesh: upload
    s.setTriangleSoup(water, P.scenes.transfer_sheet(2)[:200])
    s.commitObjectChanges()
    assert s.commitCounts() == (2, 3)
    frame(4)
    s.close()
