#!/usr/bin/env python3
"""What moving instances behind a real TLAS costs per frame: the `many` recipe at bench.py's size (136 meshes), k instances
moved every frame for a run of frames, committed
  (a) by commitObjectChanges() under the default policy: TLAS rebuilt on the host, ptrt_update_instances (synchronises);
  (b) by refitInstanceChanges(): ptrt_set_instance_transforms + ptrt_refit_tlas on the stream, TLAS topology kept.
Per frame: host microseconds inside the commit call (perf_counter around it) and the frame time -- HIP events on the context's
stream around the whole run of commit + render_to_device, divided by the frames, so a stall of the host shows as a gap.  The two
paths alternate, window by window, in one process; medians over the windows are reported with their range.

And while the instances random-walk away from where the TLAS was built (--walk-frames of cumulative steps), every
--reorder-every-th frame is committed
  (c) by reorderTLAS(): ptrt_reorder_tlas re-deals the meshes over the kept TLAS shape on the stream, then refits;
beside refitInstanceChanges() on every frame and reseatTLAS() (host rebuild, synchronises) on those frames.  Reported: the
frame time of the frames AFTER such a frame (events around the refit-only frames up to the next one), i.e. what the fresher
tree is worth, and the host microseconds of the call itself.

Also: the PMODE 3 frame time after a vertex refit of one mesh, with the instances' first-pass boxes left invalid (ptrt_refit
alone: inst_pre_ok 0) and recomputed on the device (ptrt_refit + ptrt_refit_tlas: inst_pre_ok 1), same frames otherwise.

    python3 tools/tlas_refit_time.py --out profiles/tlas_refit_time.json

--poses-device measures this instead, and nothing else: the same k moving instances per frame committed
  (b) by refitInstanceChanges(), as above: matrices made by the host mirror, staged, scattered;
  (d) by a pose tensor written on the device (torch, on the context's stream) + set_instance_poses_device +
      ptrt_refit_tlas: nine floats per mesh of the moved span, matrices derived by the device, no host copy of anything.
Host microseconds per commit and event-timed frame time, the same windows and medians.

    python3 tools/tlas_refit_time.py --poses-device --out profiles/instance_pose_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402

N_EXTRA, BASE = 128, 8  # bench.py's `many`: the Cornell box's 8 meshes + 128


def build(width, height, spp, depth):
    s = P.Scene(width, height)
    P.scenes.many(s, N_EXTRA, sphere_segments=32)
    s.setPerfSamplesPerPixel(spp)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    return s


def run_frames(s, stream, out, frames, k, commit, frame0):
    """`frames` frames of: move k instances (every third extra mesh is one), commit, render.  Returns (host us per commit,
    ms per frame by events on the stream)."""
    inst = [BASE + j for j in range(0, N_EXTRA, 3)][:k]
    host = 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for f in range(frames):
        a = 0.05 * (frame0 + f)
        for j, m in enumerate(inst):
            s.setPosition(m, (3.0 * np.sin(a + j), -1.0 + 2.0 * np.cos(0.7 * a + j), -5.0 + 2.0 * np.sin(0.3 * a + 2 * j)))
        t0 = time.perf_counter()
        commit()
        host += time.perf_counter() - t0
        s.render_to_device(out.data_ptr())
    e1.record(stream)
    e1.synchronize()
    return 1e6 * host / frames, e0.elapsed_time(e1) / frames


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def measure_moves(a):
    rows = []
    for k in (int(x) for x in a.moved.split(",")):
        scenes = {"commit": build(a.width, a.height, a.spp, a.depth), "refit": build(a.width, a.height, a.spp, a.depth)}
        stream = torch.cuda.Stream()
        out = torch.empty(a.width * a.height * 3, dtype=torch.uint8, device="cuda")
        res = {name: {"host_us": [], "frame_ms": []} for name in scenes}
        for s in scenes.values():
            s.set_stream(stream.cuda_stream)
        commits = {"commit": scenes["commit"].commitObjectChanges, "refit": scenes["refit"].refitInstanceChanges}
        with torch.cuda.stream(stream):
            for w in range(a.windows + 1):  # (window 0 warms both paths up)
                for name, s in scenes.items():
                    h, ms = run_frames(s, stream, out, a.frames, k, commits[name], w * a.frames)
                    if w:
                        res[name]["host_us"].append(h)
                        res[name]["frame_ms"].append(ms)
        counts = {name: s.get_option("tlas_refits") for name, s in scenes.items()}
        row = {"case": "moved_instances", "meshes": BASE + N_EXTRA, "moved_per_frame": k, "frames_per_window": a.frames,
               "size": [a.width, a.height], "spp": a.spp, "depth": a.depth, "pmode": scenes["refit"].get_option("pmode"),
               "tlas_refits": counts, "library": P.library_info()["sha16"]}
        for name in scenes:
            row[f"{name}_host_us"] = summary(res[name]["host_us"])
            row[f"{name}_frame_ms"] = summary(res[name]["frame_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        for s in scenes.values():
            s.sync()
            s.close()
    return rows


def home_poses():
    """(N_EXTRA, 9) float32: the pose of every extra mesh of scenes.many, by replaying its draws; a mesh with baked vertices has
    the identity pose, which is what its record holds"""
    rs = np.random.RandomState(3)
    out = np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1, 1], np.float32), (N_EXTRA, 1))
    for k in range(N_EXTRA):
        rs.uniform(0.2, 0.9, 3), rs.uniform(0.05, 0.8)
        pos = (rs.uniform(-4, 4), rs.uniform(-4.5, 3.5), rs.uniform(-9, -2))
        if k % 3 == 0:
            out[k] = np.concatenate([pos, rs.uniform(-1, 1, 3), rs.uniform(0.2, 0.5, 3)])
        else:
            rs.uniform(0.2, 0.5, 3)
    return out


def measure_poses(a):
    """k moving instances per frame: (b) refitInstanceChanges() against (d) poses written on the device +
    set_instance_poses_device + ptrt_refit_tlas, alternating window by window in one process"""
    rows = []
    for k in (int(x) for x in a.moved.split(",")):
        k = min(k, (N_EXTRA + 2) // 3)
        scenes = {"refit": build(a.width, a.height, a.spp, a.depth), "poses": build(a.width, a.height, a.spp, a.depth)}
        stream = torch.cuda.Stream()
        out = torch.empty(a.width * a.height * 3, dtype=torch.uint8, device="cuda")
        for s in scenes.values():
            s.set_stream(stream.cuda_stream)
        span = 3 * (k - 1) + 1                                # meshes BASE .. BASE + span - 1 hold the k instances
        poses = torch.from_numpy(home_poses()[:span]).cuda()
        moving = poses[::3, 0:3]                              # the instances' positions: a view into the pose tensor
        j = torch.arange(k, dtype=torch.float32, device="cuda")
        sp = scenes["poses"]
        frame = {"f": 0}

        def commit_poses():
            t = 0.05 * frame["f"]
            moving[:, 0] = 3.0 * torch.sin(t + j)
            moving[:, 1] = -1.0 + 2.0 * torch.cos(0.7 * t + j)
            moving[:, 2] = -5.0 + 2.0 * torch.sin(0.3 * t + 2.0 * j)
            sp.set_instance_poses_device(BASE, poses)
            sp._cchk(P.lib.ptrt_refit_tlas(sp.ctx))
            frame["f"] += 1

        commits = {"refit": scenes["refit"].refitInstanceChanges, "poses": commit_poses}
        res = {name: {"host_us": [], "frame_ms": []} for name in scenes}
        with torch.cuda.stream(stream):
            for w in range(a.windows + 1):  # (window 0 warms both paths up)
                for name, s in scenes.items():
                    frame["f"] = w * a.frames
                    h, ms = run_frames(s, stream, out, a.frames, k if name == "refit" else 0, commits[name], w * a.frames)
                    if w:
                        res[name]["host_us"].append(h)
                        res[name]["frame_ms"].append(ms)
        row = {"case": "poses_on_the_device", "meshes": BASE + N_EXTRA, "moved_per_frame": k, "posed_span": span,
               "frames_per_window": a.frames, "size": [a.width, a.height], "spp": a.spp, "depth": a.depth,
               "pmode": sp.get_option("pmode"), "tlas_refits": {name: s.get_option("tlas_refits") for name, s in scenes.items()},
               "library": P.library_info()["sha16"]}
        for name in scenes:
            row[f"{name}_host_us"] = summary(res[name]["host_us"])
            row[f"{name}_frame_ms"] = summary(res[name]["frame_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        for s in scenes.values():
            s.sync()
            s.close()
    return rows


def measure_walk(a):
    """instances random-walk; every `reorder_every`-th frame goes through refit / reorderTLAS / reseatTLAS, the others through
    refitInstanceChanges; timed: the frames between those frames"""
    inst = [BASE + j for j in range(0, N_EXTRA, 3)]
    names = ("refit", "reorder", "reseat")
    scenes = {name: build(a.width, a.height, a.spp, a.depth) for name in names}
    special = {"refit": scenes["refit"].refitInstanceChanges, "reorder": scenes["reorder"].reorderTLAS, "reseat": scenes["reseat"].reseatTLAS}
    stream = torch.cuda.Stream()
    out = torch.empty(a.width * a.height * 3, dtype=torch.uint8, device="cuda")
    for s in scenes.values():
        s.set_stream(stream.cuda_stream)
    d0 = scenes["refit"].flatten().contents
    pos = {name: np.array([[d0.meshes[m].world[3], d0.meshes[m].world[7], d0.meshes[m].world[11]] for m in inst]) for name in names}
    rs = {name: np.random.RandomState(1) for name in names}  # the same walk in every scene
    res = {name: {"host_us": [], "frame_ms": []} for name in names}

    def step(name):
        pos[name] += rs[name].uniform(-a.walk_step, a.walk_step, pos[name].shape)
        for m, p in zip(inst, pos[name]):
            scenes[name].setPosition(m, tuple(float(x) for x in p))

    with torch.cuda.stream(stream):
        for seg in range(a.walk_frames // a.reorder_every):
            for name, s in scenes.items():
                step(name)
                t0 = time.perf_counter()
                special[name]()
                host = 1e6 * (time.perf_counter() - t0)
                s.render_to_device(out.data_ptr())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reorder_every - 1):
                    step(name)
                    s.refitInstanceChanges()
                    s.render_to_device(out.data_ptr())
                e1.record(stream)
                e1.synchronize()
                if seg:  # (segment 0 warms every path up)
                    res[name]["host_us"].append(host)
                    res[name]["frame_ms"].append(e0.elapsed_time(e1) / (a.reorder_every - 1))
    row = {"case": "random_walk", "meshes": BASE + N_EXTRA, "walking": len(inst), "step": a.walk_step, "frames": a.walk_frames,
           "every": a.reorder_every, "size": [a.width, a.height], "spp": a.spp, "depth": a.depth,
           "tlas_reorders": scenes["reorder"].get_option("tlas_reorders"), "library": P.library_info()["sha16"]}
    for name in names:
        row[f"{name}_call_host_us"] = summary(res[name]["host_us"])
        row[f"{name}_frames_after_ms"] = summary(res[name]["frame_ms"])
    print(json.dumps(row), flush=True)
    for s in scenes.values():
        s.sync()
        s.close()
    return [row]


def measure_pretest(a):
    """frames after a vertex refit of one mesh, first-pass boxes invalid vs recomputed on the device"""
    s = build(a.width, a.height, a.spp, a.depth)
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    out = torch.empty(a.width * a.height * 3, dtype=torch.uint8, device="cuda")
    mesh = BASE + 1  # a sphere with baked vertices
    md = s.flatten().contents.meshes[mesh]
    import ctypes as C
    base = np.ctypeslib.as_array(C.cast(md.verts, C.POINTER(C.c_float)), (md.vert_count, 3)).copy()
    dev = torch.from_numpy(base).cuda()
    res = {0: [], 1: []}
    with torch.cuda.stream(stream):
        for w in range(a.windows + 1):
            for ok in (0, 1):
                s._cchk(P.lib.ptrt_update_vertices(s.ctx, mesh, C.cast(dev.data_ptr(), C.POINTER(C.c_float)), len(base), 1))
                s._cchk(P.lib.ptrt_refit(s.ctx))
                if ok:
                    s._cchk(P.lib.ptrt_refit_tlas(s.ctx))
                assert s.get_option("inst_pre_ok") == ok
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.render_to_device(out.data_ptr())  # (gathers the heads with this state)
                e0.record(stream)
                for _ in range(a.frames):
                    s.render_to_device(out.data_ptr())
                e1.record(stream)
                e1.synchronize()
                if w:
                    res[ok].append(e0.elapsed_time(e1) / a.frames)
    row = {"case": "first_pass_boxes_after_vertex_refit", "meshes": BASE + N_EXTRA, "size": [a.width, a.height], "spp": a.spp,
           "depth": a.depth, "pmode": s.get_option("pmode"), "frame_ms_inst_pre_ok_0": summary(res[0]),
           "frame_ms_inst_pre_ok_1": summary(res[1]), "library": P.library_info()["sha16"]}
    print(json.dumps(row), flush=True)
    s.sync()
    s.close()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moved", default="1,8,44", help="instances moved per frame (the recipe has 43 instances; more are clipped)")
    ap.add_argument("--frames", type=int, default=100, help="frames per window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per path (they alternate)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--walk-frames", type=int, default=600, help="frames of the random walk (0: skip it)")
    ap.add_argument("--walk-step", type=float, default=0.05, help="largest step per axis and frame")
    ap.add_argument("--reorder-every", type=int, default=20, help="every k-th frame of the walk takes the path under test")
    ap.add_argument("--poses-device", action="store_true", help="only: refitInstanceChanges() against poses written on the device")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.poses_device:
        rows = measure_poses(a)
    else:
        rows = measure_moves(a) + (measure_walk(a) if a.walk_frames >= 2 * a.reorder_every else []) + measure_pretest(a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": f"python3 tools/tlas_refit_time.py {'--poses-device ' if a.poses_device else ''}"
                                  f"--moved {a.moved} --frames {a.frames} --windows {a.windows} "
                                  f"--width {a.width} --height {a.height} --spp {a.spp} --depth {a.depth}",
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
