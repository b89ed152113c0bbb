#!/usr/bin/env python3
"""Time of the radiance query (ptrt_query_radiance) beside the frame that does the same work, on the four bench scenes.

Per scene at 1920 x 1080: the frame's own primary rays (ptrt_camera_rays of frame 0) and one generator state per pixel go
through ptrt_query_radiance at 1 sample / 4 bounces; beside it ptrt_render at 1 spp / 4 bounces into a device buffer -- the same
paths in the tuned kernel (lane refill, staged shading inputs, frames that overlap).  The states advance in place from call to
call, as a frame's do, so every launch traces fresh paths.  Both are timed with HIP events on the context's stream around
back-to-back launches, in windows of at least --window seconds after a warm-up, the two alternating --repeats times; the table
gives the medians and the spread (min .. max) of the per-launch times, Mpaths/s of the query and the ratio query / frame.

    python3 tools/radiance_query_time.py --out profiles/radiance_query_time.json
"""
import argparse
import json
import os
import statistics
import sys

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
    """Launches back to back until the events span `seconds`; returns ms per launch."""
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
            return ms / n
        n = max(n * 2, int(n * 1.2e3 * seconds / max(ms, 1e-3)))


def measure(name, width, height, samples, depth, seconds, repeats):
    s = P.Scene(width, height)
    SCENES[name](s)
    s.setPerfSamplesPerPixel(samples)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(P.DEFAULT_SEED)
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    n = width * height
    with torch.cuda.stream(stream):
        o, d = s.camera_rays(0, 0)
        st = s.init_rng_states(P.DEFAULT_SEED, 0, n)
        out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        bufs = [torch.empty(n * 3, dtype=torch.uint8, device="cuda") for _ in range(2)]
        k = [0]

        def query():
            s.query_radiance(o, d, st, samples=samples, max_depth=depth, out=out)

        def frame():
            s.render_to_device(bufs[k[0] & 1].data_ptr())
            k[0] += 1

        query()
        pmode = s.get_option("query_pmode")
        window(stream, query, 0.2)  # warm-up: code objects, clocks
        window(stream, frame, 0.2)  # (and the frame's loop-shape choice where it has one)
        q_ms, f_ms = [], []
        for _ in range(repeats):
            q_ms.append(window(stream, query, seconds))
            f_ms.append(window(stream, frame, seconds))
    s.sync()
    row = {"scene": name, "rays": n, "samples": samples, "max_depth": depth, "query_pmode": pmode,
           "frame_pmode": s.get_option("pmode"), "frame_refilled": s.get_option("refilled"),
           "frame_pipelined": s.get_option("pipelined"),
           "query_ms": round(statistics.median(q_ms), 4), "query_ms_min_max": [round(min(q_ms), 4), round(max(q_ms), 4)],
           "query_mpaths": round(n * samples / statistics.median(q_ms) / 1e3, 1),
           "frame_ms": round(statistics.median(f_ms), 4), "frame_ms_min_max": [round(min(f_ms), 4), round(max(f_ms), 4)],
           "ratio": round(statistics.median(q_ms) / statistics.median(f_ms), 3), "library": P.library_info()["sha16"]}
    print(json.dumps(row), flush=True)
    s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3, help="alternating (query, frame) windows per scene")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radiance_query_time: no GPU; a time is measured on one or not at all")
    w, h = (int(x) for x in a.size.split("x"))
    rows = [measure(name, w, h, a.samples, a.depth, a.window, a.repeats) for name in a.scenes.split(",")]
    print(f"{'scene':10} {'query ms':>9} {'Mpaths/s':>9} {'frame ms':>9} {'query / frame':>13}")
    for r in rows:
        print(f"{r['scene']:10} {r['query_ms']:9.3f} {r['query_mpaths']:9.1f} {r['frame_ms']:9.3f} {r['ratio']:13.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": f"python3 tools/radiance_query_time.py --scenes {a.scenes} --size {a.size} --samples {a.samples} "
                                  f"--depth {a.depth} --window {a.window} --repeats {a.repeats}",
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
