#!/usr/bin/env python3
"""Time of the one-bounce bake (ptrt_query_bounce) beside the unfused chain it replaces, on the four bench scenes.

Per scene: a 128 x 128 lightmap -- 16,384 texels on quads of the scene --, 64 gather directions per texel (a Hammersley set
shared by all texels, one phase per texel), all of the scene's lights, one shadow sample per light.  Fused: Scene.query_bounce,
one (16384, 8) tensor out.  Unfused, on the same commit: Scene.irradiance_rays (24 bytes per ray), Scene.query_closest (64 bytes
per ray), Scene.bounce_terms (40 bytes per term), Scene.query_occluded on ALL the terms (leaving out those that are not walked
is a compaction of its own), then the segmented sums in torch -- the value where the term is walked and not blocked, the two
counts, the hits, a sum over each texel's terms (torch's own sum order, not the contract's: it is timed, not compared).  The
five parts of the chain are timed and reported separately.  HIP events on the context's stream around back-to-back launches,
windows of at least --window seconds after a warm-up, the six interleaved --repeats times; medians with their range, and the
ratio fused / unfused.  What the fused call saves is the rays', the hits' and the terms' trip through memory; what it costs is
Q any-hit walks per closest-hit walk inside one wave, where a lane whose gather ray missed idles.

    python3 tools/bounce_time.py --out profiles/bounce_time.json
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
# walls; the showcase's floor under its objects; a plane under the water looking up and one beside the ship)
SCENES = {
    "cornell": (lambda s: P.scenes.cornell(s), [((-4.95, -4.95, -9.95), (0, 0, 9.9), (9.9, 0, 0)),
                                                ((-4.95, -4.95, -9.95), (0, 9.9, 0), (0, 0, 9.9)),
                                                ((-4.95, -4.95, -9.95), (9.9, 0, 0), (0, 9.9, 0))]),
    "showcase": (lambda s: P.scenes.showcase(s), [((-10.0, -3.0, -15.0), (0, 0, 12.0), (20.0, 0, 0))]),
    "fluid": (lambda s: P.scenes.fluid(s, cells=256, t=0.0), [((-8.0, -1.5, 8.0), (16.0, 0, 0), (0, 0, -16.0)),
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


def segmented_sum(values, flags, hits, n, k, Q):
    """the chain's last part: (n * k * Q, 3) values, (n * k * Q,) flags, (n * k, 16) hit records -> (n, 8) rows, in torch"""
    v = values.view(n, k * Q, 3)
    walked = (v > 0).any(dim=2)
    dark = walked & (flags.view(n, k * Q) != 0)
    lit = walked & ~dark
    z = torch.zeros((n, 2), dtype=torch.float32, device=values.device)
    hit = (hits[:, 0] != 0).view(n, k).sum(dim=1, keepdim=True) / k
    return torch.cat([(v * lit[:, :, None]).sum(dim=1) / k, lit.sum(dim=1, keepdim=True) / (k * Q),
                      dark.sum(dim=1, keepdim=True) / (k * Q), hit, z], dim=1)


def med(x):
    return round(statistics.median(x), 4), [round(min(x), 4), round(max(x), 4)]


def measure(name, side, k, m, seconds, repeats):
    recipe, quads = SCENES[name]
    s = P.Scene(64, 64)
    recipe(s)
    s.uploadToGPU()
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    n = side * side
    lights = s.lightCount()
    Q = lights * m
    with torch.cuda.stream(stream):
        pos_np, nrm_np = lightmap_texels(quads, side)
        pos, nrm = torch.from_numpy(pos_np).cuda(), torch.from_numpy(nrm_np).cuda()
        s2 = torch.from_numpy(P.lightmap.hammersley2(k)).cuda()
        sh2 = torch.from_numpy(P.lightmap.hammersley2(m)).cuda()
        ph = torch.from_numpy(P.lightmap.texel_phases(n, 1)).cuda()
        rows = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        rays = list(s.irradiance_rays(pos, nrm, s2, phases=ph))
        hits = [s.query_closest(rays[0], rays[1])]
        terms = list(s.bounce_terms(hits[0], rays[1], k, sh2, phases=ph))
        flags = [s.query_occluded(terms[0], terms[1], terms[2])]

        def fused():
            s.query_bounce(pos, nrm, s2, sh2, phases=ph, out=rows)

        def make_rays():
            rays[:] = s.irradiance_rays(pos, nrm, s2, phases=ph)

        def closest():
            hits[0] = s.query_closest(rays[0], rays[1])

        def make_terms():
            terms[:] = s.bounce_terms(hits[0], rays[1], k, sh2, phases=ph)

        def occluded():
            flags[0] = s.query_occluded(terms[0], terms[1], terms[2])

        def reduction():
            segmented_sum(terms[3], flags[0], hits[0], n, k, Q)

        fused()
        pmode = s.get_option("query_pmode")
        parts = (fused, make_rays, closest, make_terms, occluded, reduction)
        for f in parts:
            window(stream, f, 0.2)  # warm-up: code objects, clocks, torch's allocator
        ms = [[] for _ in parts]
        for _ in range(repeats):
            for i, f in enumerate(parts):
                ms[i].append(window(stream, f, seconds))
        lit, dark, hit = float(rows[:, 3].mean()), float(rows[:, 4].mean()), float(rows[:, 5].mean())
        agree = float((segmented_sum(terms[3], flags[0], hits[0], n, k, Q)[:, 3:6] - rows[:, 3:6]).abs().max())
    s.sync()
    (fm, fr), (ym, yr), (cm, cr), (tm, tr), (om, orr), (pm, pr) = (med(x) for x in ms)
    unfused = ym + cm + tm + om + pm
    row = {"scene": name, "texels": n, "directions": k, "lights": lights, "shadow_samples": m, "query_pmode": pmode,
           "mean_lit_fraction": round(lit, 4), "mean_shadowed_fraction": round(dark, 4), "mean_hit_fraction": round(hit, 4),
           "fractions_max_difference": agree,
           "fused_ms": fm, "fused_ms_min_max": fr, "fused_mterms": round(n * k * Q / fm / 1e3, 1),
           "rays_ms": ym, "rays_ms_min_max": yr, "closest_ms": cm, "closest_ms_min_max": cr, "terms_ms": tm, "terms_ms_min_max": tr,
           "occluded_ms": om, "occluded_ms_min_max": orr, "reduction_ms": pm, "reduction_ms_min_max": pr,
           "unfused_ms": round(unfused, 4), "ratio_fused_to_unfused": round(fm / unfused, 3),
           "ratio_fused_to_walks": round(fm / (cm + om), 3), "library": P.library_info()["sha16"]}
    print(json.dumps(row), flush=True)
    s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--side", type=int, default=128, help="texels per side of the lightmap (128: 16,384 texels)")
    ap.add_argument("--dirs", type=int, default=64, help="gather directions per texel")
    ap.add_argument("--shadow", type=int, default=1, help="shadow samples per light")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=5, help="interleaved (fused, rays, closest, terms, occluded, reduction) windows per scene")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bounce_time: no GPU; a time is measured on one or not at all")
    rows = [measure(name, a.side, a.dirs, a.shadow, a.window, a.repeats) for name in a.scenes.split(",")]
    print(f"{'scene':10} {'lights':>6} {'fused ms':>9} {'Mterms/s':>9} {'rays':>7} {'closest':>8} {'terms':>7} {'occluded':>9} {'reduction':>10} {'fused / unfused':>16}")
    for r in rows:
        print(f"{r['scene']:10} {r['lights']:6d} {r['fused_ms']:9.3f} {r['fused_mterms']:9.1f} {r['rays_ms']:7.3f} {r['closest_ms']:8.3f} "
              f"{r['terms_ms']:7.3f} {r['occluded_ms']:9.3f} {r['reduction_ms']:10.3f} {r['ratio_fused_to_unfused']:16.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": f"python3 tools/bounce_time.py --scenes {a.scenes} --side {a.side} --dirs {a.dirs} --shadow {a.shadow} "
                                  f"--window {a.window} --repeats {a.repeats}",
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
