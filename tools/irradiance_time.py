#!/usr/bin/env python3
"""Time of the lightmap bake (ptrt_query_irradiance) beside the unfused route it replaces, on the four bench scenes.

Per scene and direction count (16 and 64): a 256 x 256 lightmap -- 65,536 texels on quads of the scene, a Hammersley set shared
by all texels, one phase per texel --, 1 sample / 4 bounces: 1,048,576 and 4,194,304 paths per call.  Fused:
Scene.query_irradiance, one (65536, 8) tensor out.  Unfused, on the same commit: Scene.irradiance_rays into 24 bytes per ray,
Scene.query_radiance on them into 32-byte records, then the segmented mean in torch -- the clamped distance, its square and the
hit flag, a mean over each texel's directions (torch's own sum order, not the contract's fold: it is timed, not compared).  The
three parts of the unfused route are timed and reported separately.  The states advance in place from call to call, so every
launch traces fresh paths.  HIP events on the context's stream around back-to-back launches, windows of at least --window
seconds after a warm-up, the four alternating --repeats times; medians with their range, and the ratio fused / unfused.

    python3 tools/irradiance_time.py --out profiles/irradiance_query_time.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ptrt-game-engine_amd"))
import torch  # noqa: E402  (one HIP runtime per process: torch first)
import ptrt_amd as P  # noqa: E402

# scene -> (recipe, quads (origin, eu, ev) the lightmap is dealt over in equal strips: the Cornell box's floor, left and back
# walls; the showcase's floor under its objects; a plane over the water looking down and one beside the ship)
SCENES = {
    "cornell": (lambda s: P.scenes.cornell(s), [((-4.95, -4.95, -9.95), (0, 0, 9.9), (9.9, 0, 0)),
                                                ((-4.95, -4.95, -9.95), (0, 9.9, 0), (0, 0, 9.9)),
                                                ((-4.95, -4.95, -9.95), (9.9, 0, 0), (0, 9.9, 0))]),
    "showcase": (lambda s: P.scenes.showcase(s), [((-10.0, -3.0, -15.0), (0, 0, 12.0), (20.0, 0, 0))]),
    "fluid": (lambda s: P.scenes.fluid(s, cells=256, t=0.0), [((-8.0, 4.0, -8.0), (16.0, 0, 0), (0, 0, 16.0)),
                                                              ((-9.0, 0.5, -8.0), (0, 5.0, 0), (0, 0, 16.0))]),
    "many": (lambda s: P.scenes.many(s, 128, sphere_segments=32), [((-4.95, -4.95, -9.95), (0, 0, 9.9), (9.9, 0, 0)),
                                                                    ((-4.95, -4.95, -9.95), (0, 9.9, 0), (0, 0, 9.9)),
                                                                    ((-4.95, -4.95, -9.95), (9.9, 0, 0), (0, 9.9, 0))]),
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


def lightmap_texels(quads, side):
    """side x side texels dealt over the quads in strips of rows"""
    rows = [side // len(quads) + (1 if i < side % len(quads) else 0) for i in range(len(quads))]
    parts = [P.lightmap.quad_texels(o, eu, ev, side, r) for (o, eu, ev), r in zip(quads, rows)]
    return np.concatenate([p for p, _ in parts]), np.concatenate([n for _, n in parts])


def segmented_mean(records, n, k, max_distance):
    """the unfused route's last part: (n * k, 8) records -> (n, 8) rows, in torch"""
    r = records.view(n, k, 8)
    dist = r[:, :, 3].clamp(max=max_distance)
    hit = (r[:, :, 7].view(torch.int32) >= 0).to(torch.float32)
    z = torch.zeros((n, 2), dtype=torch.float32, device=records.device)
    return torch.cat([r[:, :, 0:3].mean(dim=1), dist.mean(dim=1, keepdim=True), (dist * dist).mean(dim=1, keepdim=True),
                      hit.mean(dim=1, keepdim=True), z], dim=1)


def med(x):
    return round(statistics.median(x), 4), [round(min(x), 4), round(max(x), 4)]


def measure(name, side, k, samples, depth, seconds, repeats):
    recipe, quads = SCENES[name]
    s = P.Scene(64, 64)
    recipe(s)
    s.uploadToGPU()
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    n = side * side
    max_distance, offset = 1e30, 1e-3
    with torch.cuda.stream(stream):
        pos_np, nrm_np = lightmap_texels(quads, side)
        pos, nrm = torch.from_numpy(pos_np).cuda(), torch.from_numpy(nrm_np).cuda()
        s2 = torch.from_numpy(P.lightmap.hammersley2(k)).cuda()
        ph = torch.from_numpy(P.lightmap.texel_phases(n, 1)).cuda()
        st = s.init_rng_states(P.DEFAULT_SEED, 0, n * k)
        rows = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        rec = torch.empty((n * k, 8), dtype=torch.float32, device="cuda")
        rays = list(s.irradiance_rays(pos, nrm, s2, offset=offset, phases=ph))

        def fused():
            s.query_irradiance(pos, nrm, s2, st, samples=samples, max_depth=depth, max_distance=max_distance, offset=offset, phases=ph,
                               out=rows)

        def make_rays():
            rays[0], rays[1] = s.irradiance_rays(pos, nrm, s2, offset=offset, phases=ph)

        def radiance():
            s.query_radiance(rays[0], rays[1], st, samples=samples, max_depth=depth, out=rec)

        def reduction():
            segmented_mean(rec, n, k, max_distance)

        fused()
        pmode = s.get_option("query_pmode")
        parts = (fused, make_rays, radiance, reduction)
        for f in parts:
            window(stream, f, 0.2)  # warm-up: code objects, clocks, torch's allocator
        ms = [[] for _ in parts]
        for _ in range(repeats):
            for i, f in enumerate(parts):
                ms[i].append(window(stream, f, seconds))
        hit_fraction = float(rows[:, 5].mean())
    s.sync()
    (fm, fr), (ym, yr), (rm, rr), (pm, pr) = (med(x) for x in ms)
    unfused = ym + rm + pm
    row = {"scene": name, "texels": n, "directions": k, "samples": samples, "max_depth": depth, "query_pmode": pmode,
           "mean_hit_fraction": round(hit_fraction, 4),
           "fused_ms": fm, "fused_ms_min_max": fr, "fused_mpaths": round(n * k * samples / fm / 1e3, 1),
           "rays_ms": ym, "rays_ms_min_max": yr, "radiance_ms": rm, "radiance_ms_min_max": rr,
           "reduction_ms": pm, "reduction_ms_min_max": pr,
           "unfused_ms": round(unfused, 4), "ratio_fused_to_unfused": round(fm / unfused, 3),
           "ratio_fused_to_radiance": round(fm / rm, 3), "library": P.library_info()["sha16"]}
    print(json.dumps(row), flush=True)
    s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--side", type=int, default=256, help="texels per side of the lightmap (256: 65,536 texels)")
    ap.add_argument("--directions", default="16,64")
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3, help="alternating (fused, rays, radiance, reduction) windows per case")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("irradiance_time: no GPU; a time is measured on one or not at all")
    rows = [measure(name, a.side, int(k), a.samples, a.depth, a.window, a.repeats)
            for name in a.scenes.split(",") for k in a.directions.split(",")]
    print(f"{'scene':10} {'dirs':>5} {'fused ms':>9} {'Mpaths/s':>9} {'rays ms':>8} {'radiance ms':>12} {'reduction ms':>13} {'fused / unfused':>16}")
    for r in rows:
        print(f"{r['scene']:10} {r['directions']:5d} {r['fused_ms']:9.3f} {r['fused_mpaths']:9.1f} {r['rays_ms']:8.3f} "
              f"{r['radiance_ms']:12.3f} {r['reduction_ms']:13.3f} {r['ratio_fused_to_unfused']:16.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": f"python3 tools/irradiance_time.py --scenes {a.scenes} --side {a.side} --directions {a.directions} "
                                  f"--samples {a.samples} --depth {a.depth} --window {a.window} --repeats {a.repeats}",
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
