"""Times the one-bounce ray tracer (ptrt_amd.rt.Scene.render_to_device -> rt_render_kernel) on one GPU.

Scenes: the five procedural DemoScenes (ptrt_amd.rt.scenes.DEMO_SCENES) and a dense mesh (a grid of 2 x 2
256-segment spheres, 524288 triangles, two lights), each at 1920x1080.  Each render is bracketed by HIP events on the
current stream (torch.cuda.Event): descriptors, launch and the synchronisation the reference's render_to_device
does.  Rays per frame are counted on the CPU by tests/rt_restatement.py's rules (one primary ray per pixel, one
shadow ray per light at every shaded hit, a reflection and a refraction ray per glass pixel) from the scene's
snapshot; Grays/s = rays per frame / median frame time.  Prints and writes profiles/rt_time.json.
usage: python tools/rt_time.py [--frames 20] [--warmup 5] [--out profiles/rt_time.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ptrt-game-engine_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402  (first: one HIP runtime, see tests/conftest.py)

import ptrt_amd.rt as rt  # noqa: E402
import oracle as O  # noqa: E402
import rt_restatement as R  # noqa: E402


def dense(s):
    for k in range(4):
        i = s.addSphere(256, rt.Material((0.9, 0.9, 0.9), 0.3, 0.0))
        s.mesh(i).scale((1.8, 1.8, 1.8)).moveTo((-1.0 + 2.0 * (k % 2), -0.2 + 1.9 * (k // 2), -5.0))
    s.addPlaneXZ(-1.5, 20.0, rt.Material((0.6, 0.6, 0.6), 0.8, 0.0))
    s.addPointLight((3, 4, 0), (1, 1, 1), 2.0)
    s.addDirectionalLight((0.2, -1, -0.3), (0.6, 0.7, 1.0), 0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_time.json"))
    a = ap.parse_args()
    W, H = 1920, 1080
    res = {"command": "python tools/rt_time.py --frames %d --warmup %d" % (a.frames, a.warmup),
           "device": torch.cuda.get_device_name(0), "width": W, "height": H, "scenes": {}}
    for name, recipe in list(rt.scenes.DEMO_SCENES.items()) + [("dense_sphere256_grid", dense)]:
        s = rt.Scene(W, H, device=0)
        recipe(s)
        out = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda:0")
        ms = []
        for k in range(a.warmup + a.frames):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.render_to_device(out)
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        counts = {}
        R.render(s.snapshot(), W, H, O, counts)
        rays = sum(counts.values())
        med = ms[len(ms) // 2]
        res["scenes"][name] = {"us_per_frame_median": round(med * 1000, 1), "us_per_frame_min": round(ms[0] * 1000, 1),
                               "meshes": s.getMeshCount(), "rays_per_frame": rays, "rays": counts,
                               "grays_per_s": round(rays / (med * 1e-3) / 1e9, 3)}
        print(name, res["scenes"][name], flush=True)
        s.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
