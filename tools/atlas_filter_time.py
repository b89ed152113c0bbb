#!/usr/bin/env python3
"""Time of a pass of the lightmap filter (ptrt_atlas_filter, atlas_filter_kernel) per step, under both shapes of the kernel.

Atlases of 256^2, 1024^2 and 4096^2 texels.  Two images each: a real one -- the showcase's largest mesh on
`lightmap.triangle_charts` with the largest cell that fits the atlas, its covered texels valid (skipped where the mesh's faces
do not fit the atlas) -- and a synthetic one, fully covered: a plane on a grid of one pitch, every texel valid.  Sigmas from
`lightmap.filter_sigmas(lightmap.texel_pitch(..))`, normal_power 2.  `atlas_filter_tile` 0 (global loads at every step) and 1
(the LDS tile where it fits: steps 1, 2 and 4).

The entry point has no seam for a single step -- pass s has step 1 << s, and rr follows it -- so the CUMULATIVE pass counts
1 .. 6 are timed (steps 1 .. 32) and a step's time is the difference of two neighbouring medians; the cumulative times are kept
beside it.  HIP events on the context's stream around back-to-back calls, windows of at least --window seconds after a
warm-up, --repeats of them; medians.

Beside each time the compulsory-traffic floor of a pass at --hbm GB/s: 16 B read and 16 B written per texel and 32 B of guide.

    python3 tools/atlas_filter_time.py --out profiles/atlas_filter_time.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402
from atlas_time import largest_mesh, median_ms  # noqa: E402


def plane_records(side, pitch=0.01):
    """(side^2, 8) int32 rows on the device: the plane z = 0 on a grid of `pitch`, normal +z, mesh 0, face 0"""
    i = torch.arange(side, device="cuda", dtype=torch.float32) * pitch
    rec = torch.zeros((side, side, 8), dtype=torch.float32, device="cuda")
    rec[:, :, 0] = i[None, :]
    rec[:, :, 1] = i[:, None]
    rec[:, :, 6] = 1.0
    return rec.view(torch.int32).reshape(side * side, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--max-passes", type=int, default=6, help="steps 1 .. 2^(max-passes - 1)")
    ap.add_argument("--hbm", type=float, default=8000.0, help="GB/s the floors are stated at")
    a = ap.parse_args()
    L = P.lightmap
    s = P.Scene(64, 64)
    P.scenes.showcase(s)
    s.uploadToGPU()
    mesh = largest_mesh(s)
    faces = s.meshCounts(mesh)[1]
    stream = torch.cuda.ExternalStream(s.get_option("stream"))
    vp = P.C.c_void_p
    results = []
    with torch.cuda.stream(stream):
        for side in a.sides:
            images = []
            cell = side // math.ceil(math.sqrt((faces + 1) // 2))
            if cell >= 4:
                uv, w, h = L.triangle_charts(faces, cell)
                rec = torch.full((side * side, 8), -1, dtype=torch.int32, device="cuda")
                s.atlas_texels(mesh, torch.from_numpy(uv).cuda(), side, side, out=rec)
                images.append((f"showcase mesh {mesh}, {faces} faces, cells of {cell}", rec))
            images.append(("plane, fully covered", plane_records(side)))
            for name, rec in images:
                covered = int((rec[:, 7] >= 0).sum())
                sd, sp = L.filter_sigmas(L.texel_pitch(rec, side, side))
                img = torch.rand((side * side, 4), device="cuda")
                img[:, 3] = (rec[:, 7] >= 0).float()
                other = torch.empty_like(img)
                floor_us = side * side * 64 / (a.hbm * 1e3)
                for tile in (0, 1):
                    s.set_option("atlas_filter_tile", tile)
                    prev = 0.0
                    for passes in range(1, a.max_passes + 1):
                        def call():
                            rc = P.lib.ptrt_atlas_filter(s.ctx, vp(rec.data_ptr()), vp(img.data_ptr()), vp(other.data_ptr()), side, side,
                                                         passes, sd, sp, 2)
                            assert rc == P.PTRT_OK, rc
                        med, lo, hi = median_ms(stream, call, a.window, a.repeats)
                        us = (med - prev) * 1e3
                        prev = med
                        results.append(dict(kernel="atlas_filter, one pass", image=name, atlas=side, covered=covered,
                                            atlas_filter_tile=tile, step=1 << (passes - 1),
                                            tiled=bool(s.get_option("atlas_filter_tile_eff") >= passes),
                                            us=round(us, 2), cumulative_us=round(med * 1e3, 2),
                                            cumulative_range=[round(lo * 1e3, 2), round(hi * 1e3, 2)], floor_us=round(floor_us, 2),
                                            floor_share=round(floor_us / us, 4) if us > 0 else None))
                        print(json.dumps(results[-1]), flush=True)
                s.set_option("atlas_filter_tile", -1)
                del img, other
            del images, rec
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_gbs=a.hbm, window_s=a.window, repeats=a.repeats,
                           method="cumulative pass counts differenced", results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
