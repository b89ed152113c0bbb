"""The device's evaluateBSDF, material_pdf and material_scatter (ptrt_debug_shade) against tests/shading_truth.py, the float64
statement made from the reference's text alone: the same items, the same decided rule and the same table of
tolerances as tests/test_shading_truth.py holds the oracle to -- none of its own.  Probe op 0 is judged on every item; probe
op 1 on the first 256 of the 4,096 generator states of each view, because the statement is evaluated on the host for every
item -- and on ALL 4,096 (and on every op 0 item) the device must give the bits of the oracle, which the CPU test holds to the
statement on all of them.  The probe returns no
out_pdf for op 1: it is checked as material_pdf at the scattered direction through op 0 wherever the statement says the two are
the same number (test_4c of the CPU file says where they are not)."""
import ctypes as C

import numpy as np
import pytest

import shading_truth as T

GPU_STATES_PER_VIEW = 256


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Probe:
    def __init__(self, P):
        self.P = P
        self.scene = T.add_library(P, P.Scene(64, 64))
        self.scene.uploadToGPU()
        self.desc = self.scene.flatten()
        self.lib = T.load_materials(self.desc.contents.materials)
        self.mats = C.byref(self.desc.contents.materials)
        P.lib.ptrt_debug_shade.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]

    def run(self, op, full, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros((len(x), 4 if op == 0 else 13), np.float32)
        rc = self.P.lib.ptrt_debug_shade(self.scene.ctx, op, full, fp(x), len(x), fp(out))
        assert rc == 0, self.P.lib.ptrt_last_error(self.scene.ctx)
        return out


@pytest.fixture(scope="module")
def probe(P):
    p = Probe(P)
    yield p
    p.scene.close()


def bits_differ(a, b):
    """Per row: any word differs.  Two NaNs count as the same: an invalid operation returns the platform's default NaN, whose
    sign IEEE 754 leaves open (0xFFC00000 from x86, 0x7FC00000 from the GPU)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any(axis=1)


@pytest.mark.gpu
def test_device_eval_and_pdf_match_the_statement(probe):
    lib = probe.lib
    x = T.eval_items(lib)
    out = probe.run(0, 1, x)
    j = T.judge_eval(lib, x, out, tol=T.TOL)
    assert j["decided_f"].mean() > 0.98 and j["decided_pdf"].mean() > 0.98
    for q in ("f", "pdf"):
        i = int(np.argmax(j[q]))
        print(f"{q}: no deviation above {j[q][i]:.3f} units (allowed {T.TOL[q]:.2f}) at item {i}, material {int(x[i, 0])}")
        assert j[q][i] <= T.TOL[q], f"{q} of item {i} (material {int(x[i, 0])}) is {j[q][i]:.3g} units off"
    # the simple-material variant on the materials it is chosen for: the same bits get the same verdict, any others their own
    simple = T.simple_variant_ok(lib)[x[:, 0].astype(int)]
    assert simple.sum() > 10000
    out0 = probe.run(0, 0, x)
    own = simple & bits_differ(out0, out)
    print(f"simple variant: {int(simple.sum())} items, {int(own.sum())} with bits of their own")
    if own.any():
        k = T.judge_eval(lib, x[own], out0[own], tol=T.TOL)
        assert k["f"].max() <= T.TOL["f"] and k["pdf"].max() <= T.TOL["pdf"]


@pytest.mark.gpu
def test_device_scatter_matches_the_statement(probe, O):
    lib = probe.lib
    states = T.scatter_states(O, per_view=GPU_STATES_PER_VIEW)
    uni, a1, a3 = T.advance(O, states)
    nmat = len(lib["ior"])
    y = np.concatenate([T.scatter_items(m, states) for m in range(nmat)])
    adv = (np.tile(uni, (nmat, 1)), np.tile(a1, (nmat, 1)), np.tile(a3, (nmat, 1)))
    out = probe.run(1, 1, y)
    got = T.probe_scatter_got(out)
    # out_pdf: material_pdf of the device at the device's direction, where the statement says they are the same number
    ids, N, V, ff = T.split_scatter(y)
    M = T.gather(lib, ids)
    d = got["direction"].astype(np.float64)
    smp = T.scatter_sample(M, N, V, ff, adv[0][:, 0], adv[0][:, 1], adv[0][:, 2])
    want_pdf = T.scatter_value(M, N, V, ff, d, smp["is_refraction"])[1]
    mp, dp, _ = T.material_pdf(M, N, V, d, ff)
    with np.errstate(all="ignore"):
        same = smp["ok"] & dp & (np.abs(want_pdf - mp) <= 1e-6 * np.maximum(want_pdf, mp))
    z = np.concatenate([y[:, 0:4], -y[:, 4:7], got["direction"], y[:, 7:8]], axis=1)
    dev_pdf = probe.run(0, 1, z)[:, 3]
    got["out_pdf"] = np.where(same, dev_pdf, want_pdf.astype(np.float32))
    assert same.mean() > 0.5
    j = T.judge_scatter(lib, y, adv, got, tol=T.TOL)
    assert j["decided"].mean() > 0.98
    assert not j["flags_bad"].any(), f"ok / specular flags differ at items {np.flatnonzero(j['flags_bad'])[:8]}"
    assert not j["draws_bad"].any(), f"number of uniforms drawn differs at items {np.flatnonzero(j['draws_bad'])[:8]}"
    for q in ("direction", "attenuation", "out_pdf"):
        i = int(np.argmax(j[q]))
        print(f"{q}: no deviation above {j[q][i]:.3f} units (allowed {T.TOL[q]:.2f}) at item {i}, material {int(y[i, 0])}")
        assert j[q][i] <= T.TOL[q], f"{q} of item {i} (material {int(y[i, 0])}) is {j[q][i]:.3g} units off"
    # the simple-material variant
    simple = T.simple_variant_ok(lib)[ids]
    assert simple.sum() > 10 * 8 * GPU_STATES_PER_VIEW
    out0 = probe.run(1, 0, y)
    own = simple & bits_differ(out0, out)
    print(f"simple variant: {int(simple.sum())} items, {int(own.sum())} with bits of their own")
    if own.any():
        k = T.judge_scatter(lib, y[own], tuple(a[own] for a in adv), T.probe_scatter_got(out0[own]), tol=T.TOL)
        assert not k["flags_bad"].any() and not k["draws_bad"].any()
        assert k["direction"].max() <= T.TOL["direction"] and k["attenuation"].max() <= T.TOL["attenuation"]


@pytest.mark.gpu
def test_device_gives_the_oracles_bits_on_every_item(probe, O):
    """All op 0 items and all 4,096 states of every view of every material: the bits of the oracle, which
    tests/test_shading_truth.py holds to the statement on every one of them.  NaN is the documented answer of material_pdf at
    ior 1 for L = -V (8 items here, the horizon direction at NdotV = 1e-3): device and oracle both give it, with the default
    NaN of their platforms."""
    x = T.eval_items(probe.lib)
    dev, cpu = probe.run(0, 1, x), O.eval_bsdf_n(probe.mats, x)
    bad = np.flatnonzero(bits_differ(dev, cpu))
    assert bad.size == 0, f"op 0 items {bad[:8]}: device {dev[bad[:8]]} oracle {cpu[bad[:8]]}"
    nan = np.isnan(cpu).any(axis=1)
    assert nan.sum() == 8 and (probe.lib["ior"][x[nan, 0].astype(int)] == 1.0).all() and np.isnan(dev[nan, 3]).all()
    states = T.scatter_states(O)
    for m in range(len(probe.lib["ior"])):
        y = T.scatter_items(m, states)
        dev, cpu = probe.run(1, 1, y), O.scatter_n(probe.mats, y)
        ok = (cpu[:, 7].astype(np.int64) & 1) != 0
        assert np.array_equal(dev[:, 6], cpu[:, 7]), f"material {m}: flags"
        assert not bits_differ(dev[:, 7:13], cpu[:, 8:14]).any(), f"material {m}: generator states"
        assert not bits_differ(dev[ok, :6], cpu[ok, :6]).any(), f"material {m}: direction or attenuation"
