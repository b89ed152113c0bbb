#!/usr/bin/env python3
"""Time of reading a baked lightmap at ray hits: the fused query (ptrt_query_lightmap, lightmap_query_kernel) beside the two
launches it replaces.

Rays: the 1920 x 1080 primary rays (`camera_rays(0)`) of the four bench scenes -- cornell, showcase, fluid, million.  Atlas: a
synthetic one that covers every mesh -- all the scene's faces on `lightmap.triangle_charts`, in cells large enough for an atlas
of at least --side texels a side, every texel valid, random colours; the chart table has every mesh.  Timed, per scene and mode
('nearest', 'bilinear'):
  (a) query_closest alone                      ptrt_query_rays(PTRT_QUERY_CLOSEST): 64 B written per ray
  (b) query_closest followed by atlas_sample   ... and ptrt_atlas_sample: 64 B read, 32 B written per ray, a second launch
  (c) query_lightmap                           ptrt_query_lightmap: 32 B written per ray, one launch
through the C ABI on the context's stream, every buffer allocated beforehand.  HIP events around back-to-back calls, windows of
at least --window seconds after a warm-up, --repeats of them, the windows of (b) and (c) taken in turn; medians, with the range
of the windows beside them.  What the traversal was is recorded (query_pmode), and (c) against (a) and (b).

    python3 tools/lightmap_sample_time.py --out profiles/lightmap_sample_time.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402
from atlas_time import median_ms, window  # noqa: E402

RECIPES = dict(cornell=lambda s: P.scenes.cornell(s), showcase=lambda s: P.scenes.showcase(s),
               fluid=lambda s: P.scenes.fluid(s, cells=256, t=0.0), million=lambda s: P.scenes.million(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", nargs="+", default=list(RECIPES))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--side", type=int, default=1024, help="the atlas is at least this many texels a side")
    a = ap.parse_args()
    L = P.lightmap
    vp = P.C.c_void_p
    results = []
    for name in a.scenes:
        s = P.Scene(a.width, a.height)
        RECIPES[name](s)
        s.uploadToGPU()
        meshes = s.flatten().contents.mesh_count
        faces = [s.meshCounts(m)[1] for m in range(meshes)]
        total = sum(faces)
        cols = math.ceil(math.sqrt((total + 1) // 2))
        uv, w, h = L.triangle_charts(total, max(4, -(-a.side // cols)))
        starts = [sum(faces[:m]) for m in range(meshes)]
        charts, first = L.chart_table([uv[b:b + f] for b, f in zip(starts, faces)])
        stream = torch.cuda.ExternalStream(s.get_option("stream"))
        with torch.cuda.stream(stream):
            o, d = s.camera_rays(0)
            n = int(o.shape[0])
            dc, df = torch.from_numpy(charts).cuda(), torch.from_numpy(first).cuda()
            img = torch.rand((h, w, 4), device="cuda")
            img[:, :, 3] = 1.0
            hits = torch.empty((n, 16), dtype=torch.int32, device="cuda")
            out_b, out_c = (torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))
            args = (vp(dc.data_ptr()), len(charts), vp(df.data_ptr()), vp(img.data_ptr()), w, h)

            def closest():
                rc = P.lib.ptrt_query_rays(s.ctx, P.QUERY_CLOSEST, vp(o.data_ptr()), vp(d.data_ptr()), None, n, vp(hits.data_ptr()))
                assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

            a_ms, a_lo, a_hi = median_ms(stream, closest, a.window, a.repeats)
            for mode_name, mode in P.LIGHTMAP_MODES.items():
                def sample():
                    rc = P.lib.ptrt_atlas_sample(s.ctx, vp(hits.data_ptr()), n, *args, mode, vp(out_b.data_ptr()))
                    assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

                def two():
                    closest()
                    sample()

                def fused():
                    rc = P.lib.ptrt_query_lightmap(s.ctx, vp(o.data_ptr()), vp(d.data_ptr()), n, *args, mode, vp(out_c.data_ptr()))
                    assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

                s_ms, _, _ = median_ms(stream, sample, a.window, a.repeats)
                for f in (two, fused):  # warm-up, then the windows of (b) and (c) in turn: a drift of the clocks meets both alike
                    window(stream, f, a.window / 4)
                tb, tc = [], []
                for _ in range(a.repeats):
                    tb.append(window(stream, two, a.window))
                    tc.append(window(stream, fused, a.window))
                b_ms, b_lo, b_hi = statistics.median(tb), min(tb), max(tb)
                c_ms, c_lo, c_hi = statistics.median(tc), min(tc), max(tc)
                stream.synchronize()
                same = bool(torch.equal(out_b, out_c))
                sampled = float((out_c[:, 3] != 0).float().mean())
                results.append(dict(scene=name, rays=n, meshes=meshes, faces=total, atlas=[w, h], mode=mode_name,
                                    query_pmode=int(s.get_option("query_pmode")),
                                    a_closest_us=round(a_ms * 1e3, 1), a_range=[round(a_lo * 1e3, 1), round(a_hi * 1e3, 1)],
                                    sample_alone_us=round(s_ms * 1e3, 1),
                                    b_closest_then_sample_us=round(b_ms * 1e3, 1), b_range=[round(b_lo * 1e3, 1), round(b_hi * 1e3, 1)],
                                    c_fused_us=round(c_ms * 1e3, 1), c_range=[round(c_lo * 1e3, 1), round(c_hi * 1e3, 1)],
                                    c_over_a=round(c_ms / a_ms, 3), c_over_b=round(c_ms / b_ms, 3),
                                    mrays_per_s_fused=round(n / c_ms / 1e3, 1), rays_sampled=round(sampled, 4), same_bytes=same))
                print(json.dumps(results[-1]), flush=True)
            del img, hits, out_b, out_c, dc, df, o, d
        s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), window_s=a.window, repeats=a.repeats,
                           method="HIP events round back-to-back calls on the context's stream; median of the windows after a warm-up",
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
