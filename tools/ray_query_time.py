#!/usr/bin/env python3
"""Throughput of the batched ray queries (ptrt_query_rays) on the four bench scenes, in Grays/s.

Per scene, per batch size (2^20 and 2^24 rays, the camera's primary rays of a square frame) and per ray set:
  coherent    the camera's primary rays (pinhole, pixel centres);
  incoherent  cosine-hemisphere directions from the primary hits (fixed seed; a primary ray that misses is replaced by a
              uniformly random direction from the camera);
CLOSEST is timed with the pair traversal (the default options: query_pmode 1..3 where the path tracer pairs), the per-lane walk
(option pair_trace 0) and, for comparison, the same batch through the host-staged ptrt_trace_rays (host arrays in, host records
out, wall clock: what device residency is worth); OCCLUDED with tmax = 0.5x and 1x the closest-hit distance (1e30 for a miss)
and tmax = 1e30, pair traversal and per-lane walk.  Device columns: HIP events on the context's stream around back-to-back
launches, windows of at least --window seconds after a warm-up.

    python3 tools/ray_query_time.py --out profiles/ray_query_time.json
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402

SCENES = {
    "cornell": lambda s: P.scenes.cornell(s),
    "showcase": lambda s: P.scenes.showcase(s),
    "fluid": lambda s: P.scenes.fluid(s, cells=256, t=0.0),
    "many": lambda s: P.scenes.many(s, 128, sphere_segments=32),  # bench.py's `many`
}


def window(stream, launch, seconds):
    """Launches back to back until the events span `seconds`; returns (launches, ms)."""
    n = 2
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            launch()
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * seconds:
            return n, ms
        n = max(n * 2, int(n * 1.2e3 * seconds / max(ms, 1e-3)))


def wall_window(launch, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        launch()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n, 1e3 * dt


def primary_rays(scene, side):
    """pinhole rays through the pixel centres of a side x side frame, from the flattened camera"""
    cam = C.cast(scene.flatten(), C.POINTER(P.SceneDesc)).contents.camera
    v = lambda p: torch.tensor([p.x, p.y, p.z], dtype=torch.float32, device="cuda")  # noqa: E731
    llc, hor, ver, org = v(cam.lower_left_corner), v(cam.horizontal), v(cam.vertical), v(cam.origin)
    idx = torch.arange(side, device="cuda", dtype=torch.float32) + 0.5
    ys, xs = torch.meshgrid(idx, idx, indexing="ij")
    s = (xs.reshape(-1) / side)[:, None]
    t = (1.0 - ys.reshape(-1) / side)[:, None]
    d = llc + s * hor + t * ver - org
    d = d / d.norm(dim=1, keepdim=True)
    return org.expand_as(d).contiguous(), d.contiguous()


def scatter_rays(o, d, hits, seed):
    """cosine-hemisphere directions about the primary hits' normals, from just off the hit points"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    f = P.hit_fields(hits)
    hit = f["hit"].bool()
    n, p = f["normal"], f["point"]
    u1, u2 = torch.rand(len(o), device="cuda", generator=g), torch.rand(len(o), device="cuda", generator=g)
    r, phi = u1.sqrt(), 2 * math.pi * u2
    local = torch.stack([r * phi.cos(), r * phi.sin(), (1 - u1).clamp_min(0).sqrt()], dim=1)
    a = torch.where(n[:, 0:1].abs() > 0.9, torch.tensor([0.0, 1.0, 0.0], device="cuda"), torch.tensor([1.0, 0.0, 0.0], device="cuda"))
    t = torch.linalg.cross(a, n)
    t = t / t.norm(dim=1, keepdim=True).clamp_min(1e-20)
    b = torch.linalg.cross(n, t)
    dn = local[:, 0:1] * t + local[:, 1:2] * b + local[:, 2:3] * n
    rnd = torch.randn(len(o), 3, device="cuda", generator=g)
    rnd = rnd / rnd.norm(dim=1, keepdim=True)
    o2 = torch.where(hit[:, None], p + 1e-3 * n, o)
    d2 = torch.where(hit[:, None], dn / dn.norm(dim=1, keepdim=True).clamp_min(1e-20), rnd)
    return o2.contiguous(), d2.contiguous()


def measure(name, side, seconds):
    s = P.Scene(64, 64)
    SCENES[name](s)
    s.uploadToGPU()
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    ctx = s.ctx
    n = side * side
    rows = []
    with torch.cuda.stream(stream):
        o, d = primary_rays(s, side)
        hits = torch.empty((n, 16), dtype=torch.int32, device="cuda")
        flags = torch.empty(n, dtype=torch.int32, device="cuda")
        s.query_closest(o, d)  # (commits the scene)
        for set_name in ("coherent", "incoherent"):
            if set_name == "incoherent":
                o, d = scatter_rays(o, d, s.query_closest(o, d), seed=1234)
            tfar = P.hit_fields(s.query_closest(o, d))["t"]
            tmaxes = {"0.5t": (tfar * 0.5).contiguous(), "1t": tfar.contiguous(), "1e30": torch.full((n,), 1e30, device="cuda")}
            po, pd = C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())
            row = {"scene": name, "rays": n, "set": set_name, "hit_fraction": round(float((tfar < 1e30).float().mean()), 4)}

            def q(kind, out, tm=None):
                def go():
                    if P.lib.ptrt_query_rays(ctx, kind, po, pd, tm, n, C.c_void_p(out.data_ptr())) != 0:
                        raise P.PtrtError(P.lib.ptrt_last_error(ctx).decode())
                return go

            for variant, pt in (("pair", 1), ("lane", 0)):
                s.set_option("pair_trace", pt)
                cases = [("closest", q(P.QUERY_CLOSEST, hits))] + [
                    (f"occluded_{k}", q(P.QUERY_OCCLUDED, flags, C.c_void_p(v.data_ptr()))) for k, v in tmaxes.items()]
                for case, fn in cases:
                    fn()
                    row[f"{case}_{variant}_pmode"] = s.get_option("query_pmode")
                    window(stream, fn, 0.1)  # warm-up
                    k, ms = window(stream, fn, seconds)
                    row[f"{case}_{variant}_grays"] = round(n * k / (ms * 1e-3) / 1e9, 4)
            s.set_option("pair_trace", 1)
            ho, hd = o.cpu().numpy(), d.cpu().numpy()
            out = np.empty(n, dtype=P.HIT_DTYPE)

            def host():
                if P.lib.ptrt_trace_rays(ctx, P._fptr(ho), P._fptr(hd), n, out.ctypes.data_as(C.c_void_p)) != 0:
                    raise P.PtrtError(P.lib.ptrt_last_error(ctx).decode())
            host()
            k, ms = wall_window(host, seconds)
            row["closest_host_staged_grays"] = round(n * k / (ms * 1e-3) / 1e9, 4)
            row["library"] = P.library_info()["sha16"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    s.sync()
    s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--sides", default="1024,4096", help="square frames of primary rays: 1024 -> 2^20 rays, 4096 -> 2^24")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for name in a.scenes.split(","):
        for side in (int(x) for x in a.sides.split(",")):
            rows += measure(name, side, a.window)
    if a.out:
        with open(a.out, "w") as f:
            # (the settings that shape the measurement; where the table was written is not one of them)
            json.dump({"command": f"python3 tools/ray_query_time.py --scenes {a.scenes} --sides {a.sides} --window {a.window}",
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
