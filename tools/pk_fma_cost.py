#!/usr/bin/env python3
"""What a packed fp32 instruction costs in a plain VALU stream on the GPU (tools/pk_fma_cost.hip):
   python tools/pk_fma_cost.py --build     -> compiles tools/build/pk_fma_cost for gfx950 (needs no GPU)
   python tools/pk_fma_cost.py             -> runs it once (a few seconds) and prints, per waves per SIMD, the ticks of one
                                              v_pk_fma_f32 against one v_fma_f32 and their ratio; the raw JSON line last"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "pk_fma_cost.hip")
EXE = os.path.join(ROOT, "tools", "build", "pk_fma_cost")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

if "--build" in sys.argv or not os.path.exists(EXE):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", SRC, "-o", EXE])
    if "--build" in sys.argv:
        sys.exit(0)

line = subprocess.run([EXE], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1]
res = json.loads(line)
by = {(r["waves_per_simd"], r["kind"]): r for r in res["runs"]}
print(f"{res['device']}, {res['cus']} CUs, {res['trips']} trips of {res['plain_per_trip']} v_fma_f32 / {res['packed_per_trip']} v_pk_fma_f32")
print("waves/SIMD | ticks per v_fma_f32 on the SIMD | per v_pk_fma_f32 | packed / plain | wall ms plain | wall ms packed")
for w in sorted({k[0] for k in by}):
    p, q = by[(w, "v_fma_f32")], by[(w, "v_pk_fma_f32")]
    print(f"{w:10d} | {p['ticks_per_instr_simd']:31.3f} | {q['ticks_per_instr_simd']:16.3f} | "
          f"{q['ticks_per_instr_simd'] / p['ticks_per_instr_simd']:14.3f} | {p['wall_ms_median']:13.4f} | {q['wall_ms_median']:14.4f}")
print(line)
