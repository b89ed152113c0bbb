#!/usr/bin/env python3
"""Time of reading a probe volume at ray hits: the fused query (ptrt_query_probe_light, probe_light_query_kernel) beside the
chain it replaces.

Rays: the 1920 x 1080 primary rays (`camera_rays(0)`) of the four bench scenes -- cornell, showcase, fluid, million.  Volume:
--grid^3 probes (8 x 8 x 8) over the scene's box (the root of its top-level tree), synthetic records -- coefficients in
[-1, 2], mean distances of 0.2 to 2 spacings with some variance.  Timed, per scene and mode ('trilinear', 'visibility', the
latter with a normal bias of a twentieth of the mean spacing):
  (a) query_closest alone                        ptrt_query_rays(PTRT_QUERY_CLOSEST): 64 B written per ray
  (b) query_closest, the point and normal columns copied out of the records (two strided copies), then probe_sample
                                                 ptrt_probe_sample: 24 B read, 32 B written per ray; four launches in all
  (c) query_probe_light                          ptrt_query_probe_light: 32 B written per ray, one launch
through the C ABI on the context's stream, every buffer allocated beforehand.  HIP events around back-to-back calls, windows of
at least --window seconds after a warm-up, --repeats of them, the windows of (b) and (c) taken in turn; medians, with the range
of the windows beside them.  What the traversal was is recorded (query_pmode), and (c) against (a) and (b).

    python3 tools/probe_sample_time.py --out profiles/probe_sample_time.json
"""
import argparse
import json
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


def scene_box(s):
    d = s.flatten().contents
    assert d.tlas_node_count > 0
    root = d.tlas_nodes[0]
    return (root.bmin.x, root.bmin.y, root.bmin.z), (root.bmax.x, root.bmax.y, root.bmax.z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", nargs="+", default=list(RECIPES))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, default=8, help="probes per axis")
    a = ap.parse_args()
    vp = P.C.c_void_p
    results = []
    for name in a.scenes:
        s = P.Scene(a.width, a.height)
        RECIPES[name](s)
        s.uploadToGPU()
        lo, hi = scene_box(s)
        vol = P.probes.ProbeVolume.from_corners(lo, hi, (a.grid,) * 3)
        desc = P.ProbeVolumeDesc((P.C.c_float * 3)(*vol.origin), (P.C.c_float * 3)(*vol.spacing), (P.C.c_int32 * 3)(*vol.counts))
        spacing = float(vol.spacing.mean())
        stream = torch.cuda.ExternalStream(s.get_option("stream"))
        with torch.cuda.stream(stream):
            o, d = s.camera_rays(0)
            n = int(o.shape[0])
            g = torch.Generator(device="cuda").manual_seed(5)
            probes = torch.zeros((vol.rows, 32), device="cuda")
            probes[:, :27] = torch.rand((vol.rows, 27), device="cuda", generator=g) * 3 - 1
            probes[:, 27] = (torch.rand(vol.rows, device="cuda", generator=g) * 1.8 + 0.2) * spacing
            probes[:, 28] = probes[:, 27] ** 2 + torch.rand(vol.rows, device="cuda", generator=g) * (0.1 * spacing * spacing)
            hits = torch.empty((n, 16), dtype=torch.int32, device="cuda")
            cols = hits.view(torch.float32)
            pos, nrm = (torch.empty((n, 3), device="cuda") for _ in range(2))
            out_b, out_c = (torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))

            def closest():
                rc = P.lib.ptrt_query_rays(s.ctx, P.QUERY_CLOSEST, vp(o.data_ptr()), vp(d.data_ptr()), None, n, vp(hits.data_ptr()))
                assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

            a_ms, a_lo, a_hi = median_ms(stream, closest, a.window, a.repeats)
            for mode_name, mode in P.PROBES_MODES.items():
                bias = 0.05 * spacing if mode == P.PROBES_VISIBILITY else 0.0

                def sample():
                    rc = P.lib.ptrt_probe_sample(s.ctx, vp(pos.data_ptr()), vp(nrm.data_ptr()), n, P.C.byref(desc), vp(probes.data_ptr()),
                                                 mode, bias, vp(out_b.data_ptr()))
                    assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

                def chain():
                    closest()
                    pos.copy_(cols[:, 2:5])  # (torch's current stream is the context's)
                    nrm.copy_(cols[:, 5:8])
                    sample()

                def fused():
                    rc = P.lib.ptrt_query_probe_light(s.ctx, vp(o.data_ptr()), vp(d.data_ptr()), n, P.C.byref(desc), vp(probes.data_ptr()),
                                                      mode, bias, vp(out_c.data_ptr()))
                    assert rc == P.PTRT_OK, P.lib.ptrt_last_error(s.ctx)

                chain()
                s_ms, _, _ = median_ms(stream, sample, a.window, a.repeats)
                for f in (chain, fused):  # warm-up, then the windows of (b) and (c) in turn: a drift of the clocks meets both alike
                    window(stream, f, a.window / 4)
                tb, tc = [], []
                for _ in range(a.repeats):
                    tb.append(window(stream, chain, a.window))
                    tc.append(window(stream, fused, a.window))
                b_ms, b_lo, b_hi = statistics.median(tb), min(tb), max(tb)
                c_ms, c_lo, c_hi = statistics.median(tc), min(tc), max(tc)
                stream.synchronize()
                # the chain's rows carry no face and mesh and no miss record of their own: the first six words are the comparison
                hit = hits[:, 0] != 0
                same = bool(torch.equal(out_b[hit][:, :6], out_c[hit][:, :6])) and bool((out_c[~hit][:, 4] == -1).all())
                lit = float((out_c[:, 3] != 0).float().mean())
                results.append(dict(scene=name, rays=n, box=[list(lo), list(hi)], probes=list(vol.counts), mode=mode_name,
                                    normal_bias=round(bias, 6), query_pmode=int(s.get_option("query_pmode")),
                                    a_closest_us=round(a_ms * 1e3, 1), a_range=[round(a_lo * 1e3, 1), round(a_hi * 1e3, 1)],
                                    sample_alone_us=round(s_ms * 1e3, 1),
                                    b_chain_us=round(b_ms * 1e3, 1), b_range=[round(b_lo * 1e3, 1), round(b_hi * 1e3, 1)],
                                    c_fused_us=round(c_ms * 1e3, 1), c_range=[round(c_lo * 1e3, 1), round(c_hi * 1e3, 1)],
                                    c_over_a=round(c_ms / a_ms, 3), c_over_b=round(c_ms / b_ms, 3),
                                    mrays_per_s_fused=round(n / c_ms / 1e3, 1), rays_hit=round(float(hit.float().mean()), 4),
                                    rays_lit=round(lit, 4), same_bytes=same))
                print(json.dumps(results[-1]), flush=True)
            del probes, hits, cols, pos, nrm, out_b, out_c, o, d
        s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), library=os.environ.get("PTRT_AMD_LIB", "default"), window_s=a.window,
                           repeats=a.repeats,
                           method="HIP events round back-to-back calls on the context's stream; median of the windows after a warm-up",
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
