#!/usr/bin/env python3
"""Writes tests/golden/transfer_probe_gpu.json from oracle/_ref/transfer_probe run on the GPU under every dynamic-geometry
policy (`transfer_probe gpu <policy id> <dump>`; the probe is the reference's src/common/PTRTtransfer.cuh compiled in place
over the C++ mirror by tools/refapp, where the reference's sources are).  Per policy and frame it keeps what
tests/test_transfer_gpu.py checks the Python recipe against: the commit counters, and SHA-256 digests of the flattened
scene's byte stream, the RGB8 image and the HDR image.
   python tests/golden/make_transfer_probe_golden.py                    (runs the probe; needs a GPU)
   python tests/golden/make_transfer_probe_golden.py D0 D1 D2           (from the probe's dumps of policies 0, 1, 2)"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "transfer_probe_gpu.json")
EXE = os.path.join(ROOT, "oracle", "_ref", "transfer_probe")
POLICIES = ("HostRebuild", "GpuRefit", "GpuRebuild")  # = ptrt_amd.Scene.POLICIES ids 0, 1, 2


def read_probe(path):
    """The probe's dump: (width, height, spp, depth, [per frame: commit counters, scene bytes, RGB8, HDR])."""
    raw = open(path, "rb").read()
    magic, w, h, frames, spp, depth = struct.unpack_from("<6I", raw, 0)
    assert magic == 0x54525046
    off, out = 24, []

    def blob():
        nonlocal off
        (n,) = struct.unpack_from("<Q", raw, off)
        off += 8
        b = raw[off:off + n]
        off += n
        return b

    for _ in range(frames):
        gpu_commits, uploads = struct.unpack_from("<2Q", raw, off)
        off += 16
        scene, rgb, accum = blob(), blob(), blob()
        out.append(dict(gpu_commits=gpu_commits, uploads=uploads, scene=scene,
                        rgb8=np.frombuffer(rgb, np.uint8).reshape(-1, 3), accum=np.frombuffer(accum, np.float32).reshape(-1, 3)))
    assert off == len(raw)
    return w, h, spp, depth, out


def digest(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def summarize(path):
    w, h, spp, depth, frames = read_probe(path)
    return dict(width=w, height=h, spp=spp, depth=depth,
                frames=[dict(gpu_commits=f["gpu_commits"], uploads=f["uploads"], scene_bytes=len(f["scene"]),
                             scene_sha256=digest(f["scene"]), rgb8_sha256=digest(f["rgb8"].tobytes()),
                             accum_sha256=digest(f["accum"].tobytes())) for f in frames])


def main():
    dumps = sys.argv[1:]
    tmp = None
    if not dumps:
        tmp = tempfile.mkdtemp()
        for pid in range(len(POLICIES)):
            dumps.append(os.path.join(tmp, f"transfer_{pid}.bin"))
            subprocess.check_call([EXE, "gpu", str(pid), dumps[-1]])
    assert len(dumps) == len(POLICIES)
    per = {p: summarize(d) for p, d in zip(POLICIES, dumps)}
    first = per[POLICIES[0]]
    assert all((v["width"], v["height"], v["spp"], v["depth"]) == (first["width"], first["height"], first["spp"], first["depth"])
               for v in per.values())
    doc = {"what": "oracle/_ref/transfer_probe gpu <policy>: the reference's buildPTScene, then twice updatePTScene -> "
                   "commitObjectChanges() + updatePTCamera, a frame rendered after each; per frame the commit counters "
                   "(commits on the GPU refit / rebuild path, geometry uploads) and SHA-256 of the scene's byte stream "
                   "(host/ptrt/serialize.hpp), the RGB8 image and the HDR image (float32 bits)",
           "width": first["width"], "height": first["height"], "spp": first["spp"], "depth": first["depth"],
           "policies": {p: v["frames"] for p, v in per.items()}}
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", os.path.basename(GOLDEN), file=sys.stderr)
    if tmp:
        for d in dumps:
            os.remove(d)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
