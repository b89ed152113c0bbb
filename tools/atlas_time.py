#!/usr/bin/env python3
"""Time of the lightmap atlas kernels: the rasteriser (ptrt_atlas_texels) and a dilation pass (ptrt_atlas_dilate).

Meshes: the showcase's largest mesh and the Cornell scene's tall box (12 faces).  Atlases of 256^2, 1024^2 and 4096^2 texels,
the mesh's faces on `lightmap.triangle_charts` with the largest cell that fits the atlas.  The rasteriser under every
`atlas_lanes` (1, 4, 16, 64) and under -1, with what the host's rule chose: one call is three launches -- prime, the atomic
minimum, the winners' records -- timed together (the entry point has no seam between them).  HIP events on the context's
stream around back-to-back calls, windows of at least --window seconds after a warm-up, --repeats of them; medians.

Beside each time the compulsory-traffic floor at --hbm GB/s: the rasteriser writes 32 B per texel (the prime pass) and reads
the mesh's packets (48 B per leaf slot) and charts (24 B per face); a dilation pass reads 16 B and writes 16 B per texel.  A time
within a few launch latencies (--launch-us each) of nothing is launch-bound; otherwise the floor's share says how far from HBM.

    python3 tools/atlas_time.py --out profiles/atlas_time.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402


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


def median_ms(stream, launch, seconds, repeats):
    launch()
    window(stream, launch, seconds / 4)  # warm-up
    t = [window(stream, launch, seconds) for _ in range(repeats)]
    return statistics.median(t), min(t), max(t)


def largest_mesh(s):
    n = 0
    while True:
        try:
            s.meshCounts(n)
        except P.PtrtError:
            break
        n += 1
    return max(range(n), key=lambda m: s.meshCounts(m)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--hbm", type=float, default=8000.0, help="GB/s the floors are stated at")
    ap.add_argument("--launch-us", type=float, default=3.0, help="what one launch costs when it has nothing to do")
    a = ap.parse_args()
    results = []
    for name, recipe, pick in (("showcase", P.scenes.showcase, largest_mesh), ("cornell", P.scenes.cornell, lambda s: 6)):
        s = P.Scene(64, 64)
        recipe(s)
        s.uploadToGPU()
        mesh = pick(s)
        faces = s.meshCounts(mesh)[1]
        stream = torch.cuda.ExternalStream(s.get_option("stream"))
        with torch.cuda.stream(stream):
            for side in a.sides:
                cells = (faces + 1) // 2
                cell = side // math.ceil(math.sqrt(cells))
                if cell < 4:
                    continue
                uv, w, h = P.lightmap.triangle_charts(faces, cell)
                uv = torch.from_numpy(uv).cuda()
                out = torch.empty((side * side, 8), dtype=torch.int32, device="cuda")
                floor_us = (side * side * 32 + faces * (48 + 24)) / (a.hbm * 1e3)
                for lanes in (1, 4, 16, 64, -1):
                    s.set_option("atlas_lanes", lanes)
                    med, lo, hi = median_ms(stream, lambda: s.atlas_texels(mesh, uv, side, side, out=out), a.window, a.repeats)
                    us = med * 1e3
                    bound = "launch latency" if us < 4 * 3 * a.launch_us else ("HBM" if floor_us / us > 0.5 else "the texel loop (VALU, atomics)")
                    results.append(dict(kernel="atlas_texels", scene=name, mesh=mesh, faces=faces, atlas=side, cell=cell,
                                        texels_per_face=side * side // faces, atlas_lanes=lanes,
                                        atlas_lanes_eff=s.get_option("atlas_lanes_eff"), us=round(us, 2),
                                        us_range=[round(lo * 1e3, 2), round(hi * 1e3, 2)], floor_us=round(floor_us, 2),
                                        floor_share=round(floor_us / us, 4), sits_on=bound))
                    print(json.dumps(results[-1]), flush=True)
                s.set_option("atlas_lanes", -1)
                if name == "cornell":
                    img = (torch.rand((side, side, 4), device="cuda") < 0.3).float()
                    other = torch.empty_like(img)
                    vp = P.C.c_void_p
                    med, lo, hi = median_ms(stream, lambda: P.lib.ptrt_atlas_dilate(s.ctx, vp(img.data_ptr()), vp(other.data_ptr()), side, side, 1),
                                            a.window, a.repeats)
                    us, floor_us = med * 1e3, side * side * 32 / (a.hbm * 1e3)
                    bound = "launch latency" if us < 4 * a.launch_us else ("HBM" if floor_us / us > 0.5 else "the neighbour loads (L2)")
                    results.append(dict(kernel="atlas_dilate, one pass", atlas=side, us=round(us, 2),
                                        us_range=[round(lo * 1e3, 2), round(hi * 1e3, 2)], floor_us=round(floor_us, 2),
                                        floor_share=round(floor_us / us, 4), sits_on=bound))
                    print(json.dumps(results[-1]), flush=True)
                del out, uv
        s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_gbs=a.hbm, window_s=a.window, repeats=a.repeats,
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
