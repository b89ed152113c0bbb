#!/usr/bin/env python3
"""Time of a wireframe frame (ptrt_render_wireframe) next to a 1 spp / 1 bounce path frame (ptrt_render) of the same
scene, in one process: HIP events on the context's stream around windows of back-to-back launches into one device
target, each window at least --window seconds after a warm-up, the two kinds alternating.  Prints one JSON line per
scene (median and min microseconds per frame over the windows, Grays/s of the wireframe: one primary ray per pixel)
and writes them to --out.

    python3 tools/wireframe_time.py --out profiles/wireframe_time.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402

SCENES = {
    "cornell_1080p": (1920, 1080, P.scenes.cornell),
    "showcase_1080p": (1920, 1080, P.scenes.showcase),
    "showcase_2160p": (3840, 2160, P.scenes.showcase),
    "many_1080p": (1920, 1080, P.scenes.many),
}


def window(stream, launch, seconds):
    """Launches back to back until the events span `seconds`; returns (frames, ms)."""
    n = 8
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


def measure(name, thickness, windows, seconds):
    W, H, build = SCENES[name]
    s = P.Scene(W, H)
    build(s)
    s.setPerfSamplesPerPixel(1)
    s.setMaxBounceDepth(1)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    tgt = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    ptr = C.c_void_p(tgt.data_ptr())
    s.render_to_device(tgt.data_ptr())  # (camera, sky and the rest reach the context)
    s.render_to_device_wireframe(tgt.data_ptr(), thickness)
    ctx, frame = s.ctx, [0]

    def wire():
        if P.lib.ptrt_render_wireframe(ctx, thickness, ptr, 1) != 0:
            raise P.PtrtError(P.lib.ptrt_last_error(ctx).decode())

    def path():
        frame[0] += 1
        if P.lib.ptrt_render(ctx, frame[0], 1, 1, ptr, 1) != 0:  # (same target every frame: frames do not overlap)
            raise P.PtrtError(P.lib.ptrt_last_error(ctx).decode())

    res = {"wire": [], "path": []}
    for kind, fn in (("wire", wire), ("path", path)):  # warm-up
        window(stream, fn, 0.3)
    for _ in range(windows):
        for kind, fn in (("wire", wire), ("path", path)):
            n, ms = window(stream, fn, seconds)
            res[kind].append(1e3 * ms / n)
    s.sync()
    pmode = s.get_option("pmode")
    s.close()
    out = {"scene": name, "width": W, "height": H, "thickness": thickness, "windows": windows, "window_s": seconds}
    for kind in ("wire", "path"):
        v = sorted(res[kind])
        out[f"{kind}_us_median"] = round(v[len(v) // 2], 2)
        out[f"{kind}_us_min"] = round(v[0], 2)
    out["wire_grays_per_s"] = round(W * H / (out["wire_us_median"] * 1e-6) / 1e9, 3)
    out["wire_over_path"] = round(out["wire_us_median"] / out["path_us_median"], 3)
    out["path_pmode"] = pmode  # loop shape of the path frame (ptrt_get_option "pmode"; 0: closest_hit<GEOM>, as the wireframe)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--thickness", type=float, default=0.02)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per window (at least)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for name in a.scenes.split(","):
        r = measure(name, a.thickness, a.windows, a.window)
        r["library"] = P.library_info()["sha16"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": "python3 tools/wireframe_time.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
