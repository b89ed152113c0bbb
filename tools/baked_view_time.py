#!/usr/bin/env python3
"""Time of the baked-light view (ptrt_render_baked, baked_view_kernel) beside what it replaces and beside the other views.

Frame: 1920 x 1080 of the four bench scenes -- cornell, showcase, fluid, million.  Lightmap: lightmap_sample_time.py's synthetic
atlas that covers every mesh (all faces on `lightmap.triangle_charts`, at least --side texels a side, every texel valid, random
colours).  Volume: 16 x 16 x 16 synthetic VISIBILITY probes over the box of the frame's own hit points.  Timed per scene:
  view_lightmap, view_probes, view_both   ptrt_render_baked into a device RGB8 target, with that half or both
  chain_lightmap, chain_probes            the two launches the view replaces: ptrt_camera_rays + ptrt_query_lightmap (or
                                          + ptrt_query_probe_light) -- without the shading, tonemap and RGB8 that still follow them
  wireframe                               ptrt_render_wireframe into the same target
  path_1spp_1bounce                       ptrt_render(frame, 1, 1) into the same target
through the C ABI on the context's stream, every buffer allocated beforehand.  HIP events around back-to-back calls, windows of
at least --window seconds after a warm-up, --repeats of them, the windows of a view and of its chain taken in turn; medians,
with the range of the windows beside them.

    python3 tools/baked_view_time.py --out profiles/baked_view_time.json
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


def us(t):
    return dict(us=round(t[0] * 1e3, 1), range=[round(t[1] * 1e3, 1), round(t[2] * 1e3, 1)])


def in_turn(stream, f, g, seconds, repeats):
    """the windows of f and g taken in turn after a warm-up of each: a drift of the clocks meets both alike"""
    for h in (f, g):
        h()
        window(stream, h, seconds / 4)
    tf, tg = [], []
    for _ in range(repeats):
        tf.append(window(stream, f, seconds))
        tg.append(window(stream, g, seconds))
    return (statistics.median(tf), min(tf), max(tf)), (statistics.median(tg), min(tg), max(tg))


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
        s.setPerfSamplesPerPixel(1)
        s.setMaxBounceDepth(1)
        s.setDenoiserEnabled(False)
        s.setBloomEnabled(False)
        s.initBlueNoise()
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
            hits = P.hit_fields(s.query_closest(o, d))
            hit = hits["hit"] != 0
            pts = hits["point"][hit] if bool(hit.any()) else torch.zeros((1, 3), device="cuda")
            lo, hi = pts.min(0).values.cpu().numpy(), pts.max(0).values.cpu().numpy()
            vol = P.probes.ProbeVolume.from_corners(lo, hi, (16, 16, 16))
            rec = torch.rand((vol.rows, 32), device="cuda")
            rec[:, 27] = rec[:, 27] * float(vol.spacing.mean()) * 2.0                  # mean_distance
            rec[:, 28] = rec[:, 27] * rec[:, 27] + 0.1 * rec[:, 28]                  # mean_distance_sq
            dc, df = torch.from_numpy(charts).cuda(), torch.from_numpy(first).cuda()
            img = torch.rand((h, w, 4), device="cuda")
            img[:, :, 3] = 1.0
            rgb = torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda")
            rows = torch.empty((n, 8), dtype=torch.int32, device="cuda")
            lm = dict(charts=dc, chart_first=df, image=img, lightmap_mode="bilinear")
            pv = dict(volume=vol, probes=rec, probe_mode="visibility", normal_bias=0.05)
            views = {k: P.baked.baked_view(s, **kw) for k, kw in (("lightmap", lm), ("probes", pv), ("both", dict(lm, **pv)))}
            desc = views["probes"][0].volume

            def ok(rc):
                assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

            def view(k):
                return lambda: ok(P.lib.ptrt_render_baked(s.ctx, 0, P.C.byref(views[k][0]), vp(rgb.data_ptr()), 1))

            def rays():
                ok(P.lib.ptrt_camera_rays(s.ctx, 0, 0, vp(o.data_ptr()), vp(d.data_ptr())))

            def chain_lightmap():
                rays()
                ok(P.lib.ptrt_query_lightmap(s.ctx, vp(o.data_ptr()), vp(d.data_ptr()), n, vp(dc.data_ptr()), len(charts), vp(df.data_ptr()),
                                             vp(img.data_ptr()), w, h, P.LIGHTMAP_BILINEAR, vp(rows.data_ptr())))

            def chain_probes():
                rays()
                ok(P.lib.ptrt_query_probe_light(s.ctx, vp(o.data_ptr()), vp(d.data_ptr()), n, P.C.byref(desc), vp(rec.data_ptr()),
                                                P.PROBES_VISIBILITY, 0.05, vp(rows.data_ptr())))

            def wireframe():
                ok(P.lib.ptrt_render_wireframe(s.ctx, 0.02, vp(rgb.data_ptr()), 1))

            def path():
                ok(P.lib.ptrt_render(s.ctx, 0, 1, 1, vp(rgb.data_ptr()), 1))

            v_lm, c_lm = in_turn(stream, view("lightmap"), chain_lightmap, a.window, a.repeats)
            v_pv, c_pv = in_turn(stream, view("probes"), chain_probes, a.window, a.repeats)
            v_both = median_ms(stream, view("both"), a.window, a.repeats)
            wire = median_ms(stream, wireframe, a.window, a.repeats)
            pt = median_ms(stream, path, a.window, a.repeats)
            stream.synchronize()
            results.append(dict(scene=name, pixels=n, meshes=meshes, faces=total, atlas=[w, h], probes=list(vol.counts),
                                query_pmode=int(s.get_option("query_pmode")), pixels_hit=round(float(hit.float().mean()), 4),
                                view_lightmap=us(v_lm), chain_lightmap=us(c_lm), view_over_chain_lightmap=round(v_lm[0] / c_lm[0], 3),
                                view_probes=us(v_pv), chain_probes=us(c_pv), view_over_chain_probes=round(v_pv[0] / c_pv[0], 3),
                                view_both=us(v_both), wireframe=us(wire), path_1spp_1bounce=us(pt),
                                view_both_over_path=round(v_both[0] / pt[0], 3)))
            print(json.dumps(results[-1]), flush=True)
            del views, img, rec, rgb, rows, dc, df, o, d
        s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), window_s=a.window, repeats=a.repeats,
                           command="python3 tools/baked_view_time.py --out profiles/baked_view_time.json",
                           method="HIP events round back-to-back calls on the context's stream; median of the windows after a warm-up; "
                                  "a view and the chain it replaces in turn",
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
