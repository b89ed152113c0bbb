"""bench.py keeps its contract: ONE JSON line on rank 0 with the agreed keys, for one process and -- rehearsed on this
one-GPU box over gloo (PTRT_BENCH_REHEARSE=1: every rank renders on cuda:0, host-staged gather; not a measurement) -- for
the N > 1 path with both ways of cutting the frame.  A plain run measures the headline only (the rest is behind --full), and
--dump-outputs writes what its last timed frame computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline"}
SMALL = ["--width", "320", "--height", "200", "--steps", "3", "--warmup", "1"]


def _line(out):
    lines = [l for l in out.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.decode()[-2000:]
    return json.loads(lines[0])


def _oracle_frame(P, O, frames):
    """The oracle's HDR image and RGB8 frame of SMALL's workload after `frames` frames from the upload's generator states."""
    s = P.Scene(320, 200, device=P.HOST_ONLY)
    P.scenes.cornell(s)
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, 320 * 200)
    for f in range(frames):
        c = O.render(s.flatten(), 320, 200, 4, 4, f, P.blue_noise_table(), rng, threads=8)
    s.close()
    return c["accum"], O.tonemap(c["accum"], 320, 200).reshape(-1, 3)


def test_single_process_line():
    d = _line(subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, "--full"], cwd=ROOT,
                                      stderr=subprocess.DEVNULL))
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert d["metric"] == "Mrays/s" and d["dtype"] == "f32" and d["vs_baseline"] is None and d["scaling"] == "strong"
    assert d["config"]["workload"].startswith("cornell 320x200 4spp 4-bounce") and d["config"]["parallelism"] == "single"
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5
    assert r["valu_issue_frac"] is None  # (profile-derived fields only for the exact workload the profile was taken on)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["single_thread"]["cores"] == 1
    assert "configs3" not in d  # only the default (headline) run carries the 4K split


def test_plain_run_is_lean_and_dumps_its_last_step(P, O, tmp_path):
    """No CPU baseline, no extra frames after the timed ones; the dumped frame is the oracle's frame 2 + steps - 1 from the
    generator states of the upload (two untimed frames and the timed ones start there, whatever the ramp took), and a second run
    dumps the same bits."""
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        d = _line(subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, "--dump-outputs", str(out)],
                                          cwd=ROOT, stderr=subprocess.DEVNULL, timeout=300))
        assert KEYS <= set(d) and d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
        assert "cpu_baseline" not in d and "configs3" not in d and "kernel_alone_ms" not in d["roofline"]
        assert sorted(os.listdir(out)) == ["accum.npy", "rgb8.npy"]
        runs.append({k: np.load(out / f"{k}.npy") for k in ("rgb8", "accum")})
    for k in ("rgb8", "accum"):
        assert runs[0][k].dtype == np.float32 and runs[0][k].shape == (200, 320, 3)
        assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), k
    accum, rgb8 = _oracle_frame(P, O, 2 + 3)
    assert np.array_equal(runs[0]["accum"].reshape(-1, 3).view(np.uint32), accum.view(np.uint32))
    assert np.array_equal(runs[0]["rgb8"].reshape(-1, 3), rgb8.astype(np.float32))
    assert runs[0]["accum"].any()


@pytest.mark.parametrize("layout", ["strips", "bands"])
def test_two_rank_rehearsal(P, O, tmp_path, layout):
    env = dict(os.environ, PTRT_BENCH_REHEARSE="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541" if layout == "strips" else "29542", os.path.join(ROOT, "bench.py"), "--gpus", "2", *SMALL,
           "--layout", layout, "--dump-outputs", str(tmp_path)]
    d = _line(subprocess.check_output(cmd, cwd=ROOT, env=env, stderr=subprocess.DEVNULL, timeout=300))
    assert KEYS <= set(d) and d["n_gpus"] == 2 and "rehearsal" in d and d["config"]["parallelism"] == f"tile2-{layout}"
    assert d["rays_per_frame"] > 320 * 200 * 4  # both ranks' rays
    # rank 0's assembled frame is the one-GPU frame (per-pixel generator streams keyed by the global pixel index)
    assert os.listdir(tmp_path) == ["rgb8.npy"]
    assert np.array_equal(np.load(tmp_path / "rgb8.npy").reshape(-1, 3), _oracle_frame(P, O, 2 + 3)[1].astype(np.float32))


def test_plain_invocation_starts_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` with no launcher and no WORLD_SIZE (how the driver starts it): the process -- before it
    imports anything that touches a device -- starts the two ranks itself (python -m torch.distributed.run as a child, a free
    rendezvous port on 127.0.0.1), passes rank 0's line through and exits with the child's code."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PTRT_BENCH_REHEARSE="1", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", *SMALL], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
    assert r.returncode == 0
    d = _line(r.stdout)
    assert KEYS <= set(d) and d["n_gpus"] == 2 and "rehearsal" in d and d["config"]["parallelism"] == "tile2-strips"
    assert d["config"]["ramp_frames"] >= 10
