#!/usr/bin/env python3
"""Time of the probe query (ptrt_query_probes) beside the unfused route it replaces, on the four bench scenes.

Per scene: 4096 probes on a 16 x 16 x 16 grid inside the scene x 256 Fibonacci directions, 1 sample / 4 bounces -- 1,048,576
paths per call.  Fused: Scene.query_probes, one (4096, 32) tensor out.  Unfused, on the same commit: Scene.query_radiance on
PREBUILT origins and directions (their construction is not timed) into 32-byte records, then the projection and reduction in
torch -- the basis at the directions, nine products per channel, the clamped distance, its square and the hit flag, a mean over
the directions (torch's own sum order, not the contract's fold: it is timed, not compared).  The two parts of the unfused route
are timed and reported separately.  The states advance in place from call to call, so every launch traces fresh paths.  HIP
events on the context's stream around back-to-back launches, windows of at least --window seconds after a warm-up, the three
alternating --repeats times; medians with their range, and the ratio fused / (radiance + projection).

    python3 tools/probe_time.py --out profiles/probe_time.json
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

# scene -> (recipe, the box the probe grid fills: inside the Cornell box; around the showcase's rows of objects above its floor;
# over the water)
SCENES = {
    "cornell": (lambda s: P.scenes.cornell(s), (-4.5, -4.5, -9.5), (4.5, 4.5, -0.5)),
    "showcase": (lambda s: P.scenes.showcase(s), (-9.0, -2.5, -14.0), (9.0, 5.0, -4.0)),
    "fluid": (lambda s: P.scenes.fluid(s, cells=256, t=0.0), (-8.0, 1.0, -8.0), (8.0, 6.0, 8.0)),
    "many": (lambda s: P.scenes.many(s, 128, sphere_segments=32), (-4.5, -4.5, -9.5), (4.5, 4.5, -0.5)),  # bench.py's `many`
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


def project(records, basis, n, k, max_distance):
    """the unfused route's second half: (n * k, 8) records -> (n, 32) rows, in torch"""
    r = records.view(n, k, 8)
    sh = (basis[None, :, :, None] * r[:, :, None, 0:3]).mean(dim=1).reshape(n, 27)
    dist = r[:, :, 3].clamp(max=max_distance)
    hit = (r[:, :, 7].view(torch.int32) >= 0).to(torch.float32)
    z = torch.zeros((n, 2), dtype=torch.float32, device=records.device)
    return torch.cat([sh, dist.mean(dim=1, keepdim=True), (dist * dist).mean(dim=1, keepdim=True), hit.mean(dim=1, keepdim=True), z], dim=1)


def med(x):
    return round(statistics.median(x), 4), [round(min(x), 4), round(max(x), 4)]


def measure(name, side, k, samples, depth, seconds, repeats):
    recipe, lo, hi = SCENES[name]
    s = P.Scene(64, 64)
    recipe(s)
    s.uploadToGPU()
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    n = side ** 3
    max_distance = 1e30
    with torch.cuda.stream(stream):
        pos = torch.from_numpy(P.probes.probe_grid(lo, hi, (side, side, side))).cuda()
        dirs_np = P.probes.fibonacci_sphere(k)
        dirs = torch.from_numpy(dirs_np).cuda()
        basis = torch.from_numpy(P.probes.sh9_basis(dirs_np).astype("float32")).cuda()
        st = s.init_rng_states(P.DEFAULT_SEED, 0, n * k)
        rows = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        # the unfused route's inputs, built once
        o = pos.repeat_interleave(k, dim=0).contiguous()
        d = dirs.repeat(n, 1).contiguous()
        rec = torch.empty((n * k, 8), dtype=torch.float32, device="cuda")

        def fused():
            s.query_probes(pos, dirs, st, samples=samples, max_depth=depth, max_distance=max_distance, out=rows)

        def radiance():
            s.query_radiance(o, d, st, samples=samples, max_depth=depth, out=rec)

        def projection():
            project(rec, basis, n, k, max_distance)

        fused()
        pmode = s.get_option("query_pmode")
        for f in (fused, radiance, projection):
            window(stream, f, 0.2)  # warm-up: code objects, clocks, torch's allocator
        f_ms, r_ms, p_ms = [], [], []
        for _ in range(repeats):
            f_ms.append(window(stream, fused, seconds))
            r_ms.append(window(stream, radiance, seconds))
            p_ms.append(window(stream, projection, seconds))
        hit_fraction = float(rows[:, 29].mean())
    s.sync()
    (fm, fr), (rm, rr), (pm, pr) = med(f_ms), med(r_ms), med(p_ms)
    row = {"scene": name, "probes": n, "directions": k, "samples": samples, "max_depth": depth, "query_pmode": pmode,
           "mean_hit_fraction": round(hit_fraction, 4),
           "fused_ms": fm, "fused_ms_min_max": fr, "fused_mpaths": round(n * k * samples / fm / 1e3, 1),
           "radiance_ms": rm, "radiance_ms_min_max": rr, "projection_ms": pm, "projection_ms_min_max": pr,
           "unfused_ms": round(rm + pm, 4), "ratio_fused_to_unfused": round(fm / (rm + pm), 3),
           "ratio_fused_to_radiance": round(fm / rm, 3), "library": P.library_info()["sha16"]}
    print(json.dumps(row), flush=True)
    s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--side", type=int, default=16, help="probes per axis of the grid (16: 4096 probes)")
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3, help="alternating (fused, radiance, projection) windows per scene")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_time: no GPU; a time is measured on one or not at all")
    rows = [measure(name, a.side, a.directions, a.samples, a.depth, a.window, a.repeats) for name in a.scenes.split(",")]
    print(f"{'scene':10} {'fused ms':>9} {'Mpaths/s':>9} {'radiance ms':>12} {'projection ms':>14} {'fused / unfused':>16}")
    for r in rows:
        print(f"{r['scene']:10} {r['fused_ms']:9.3f} {r['fused_mpaths']:9.1f} {r['radiance_ms']:12.3f} {r['projection_ms']:14.3f} "
              f"{r['ratio_fused_to_unfused']:16.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": f"python3 tools/probe_time.py --scenes {a.scenes} --side {a.side} --directions {a.directions} "
                                  f"--samples {a.samples} --depth {a.depth} --window {a.window} --repeats {a.repeats}",
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
