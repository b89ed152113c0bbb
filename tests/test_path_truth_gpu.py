"""Scene.query_radiance on the light lab of tests/path_truth.py: the device's radiance for rays that are no camera's, held to the
float64 statement of next-event estimation and the integrator within the table tests/test_path_truth.py measures on the CPU
(DESIGN.md 5.3), and to oracle.trace_paths bit for bit -- records and generator states, undecided paths included -- under every
light set, ray set and sky, at depths 1 to 8, with one and three samples, and under the six loop shapes of the geometric queries
on two light sets; and one case through query_probes.  The statement is evaluated once per case and kept for the module."""
import ctypes as C

import numpy as np
import pytest

import brute_force as bf
import path_truth as PT
import probe_restatement as R
from test_radiance_query_gpu import dev_states, host_states, records
from test_ray_query_gpu import VARIANTS

pytestmark = pytest.mark.gpu

CASES = PT.cases()
IDS = ["-".join(c) for c in CASES]


class GpuLab:
    def __init__(self, P, O):
        import torch
        self.P, self.O, self.torch = P, O, torch
        self.scene = P.Scene(64, 64)
        PT.light_lab(P, self.scene)
        self.scene.uploadToGPU()
        # one query flushes whatever the host scene still holds back (lights, sky), so that what is set below stays
        z = torch.zeros((1, 3), device="cuda")
        self.scene.query_radiance(z, z + 1.0, dev_states(O.xorwow_init(1, 0, 1)), max_depth=1)
        self.scene.sync()
        self.world = PT.World(P, self.scene)
        self.cases, self.env_set = {}, False

    def case(self, key):
        """the case's statement (cached) with its lights and sky set on the device"""
        if key not in self.cases:
            self.cases[key] = PT.Case(self.P, self.O, self.world, *key)
        c = self.cases[key]
        s = self.scene
        w = c.world
        rc = self.P.lib.ptrt_upload_lights(s.ctx, w.light_array, w.n_lights)
        assert rc == self.P.PTRT_OK, self.P.lib.ptrt_last_error(s.ctx)
        if self.env_set and w.sky.env is None:
            s.freeHDRI()
            self.env_set = False
        if w.sky.use:
            s.setSkyGradient(tuple(w.sky.top), tuple(w.sky.bottom))
            if w.sky.env is not None:
                s.setEnvironmentMap(w.sky.env)
                self.env_set = True
        else:
            s.disableSky()
        return c

    def query(self, c, depth, samples=1, n=None):
        t = self.torch
        n = len(c.o) if n is None else n
        st = dev_states(c.states[:n])
        r = self.scene.query_radiance(t.from_numpy(c.o[:n]).cuda(), t.from_numpy(c.d[:n]).cuda(), st, samples=samples, max_depth=depth)
        return records(self.P, r), host_states(st)


@pytest.fixture(scope="module")
def lab(P, O):
    lab = GpuLab(P, O)
    yield lab
    lab.scene.close()


def bits_differ(a, b):
    """Per record: any word differs; two NaNs count as the same (the platforms' default NaNs differ in sign)."""
    a = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), 8)
    b = np.ascontiguousarray(b).view(np.uint32).reshape(len(b), 8)
    fa, fb = a[:, :7].view(np.float32), b[:, :7].view(np.float32)
    same_nan = np.concatenate([np.isnan(fa) & np.isnan(fb), np.zeros((len(a), 1), bool)], axis=1)
    return ((a != b) & ~same_nan).any(axis=1)


def against_the_statement(lab, key, depth, full):
    c = lab.case(key)
    s = lab.scene
    s.set_option("force_full", full)
    try:
        rec, st = lab.query(c, depth)
    finally:
        s.set_option("force_full", 0)
    e = PT.judge_paths(c.world, lab.O, c.o, c.d, c.states, rec, st, c.path, depth, tol=PT.TOL["radiance"])
    i = int(np.argmax(e["radiance"]))
    print(f"{c.name} depth {depth} full {full}: radiance {e['radiance'][i]:.3g} units (ray {i}), t {e['t'].max():.3g}, normal {e['normal'].max():.3g}, "
          f"decided {e['decided'].mean():.3f}")
    assert e["radiance"][i] <= PT.TOL["radiance"], f"{c.name}, depth {depth}: radiance of ray {i} is {e['radiance'][i]:.3g} units off"
    assert not e["first_bad"].any(), f"{c.name}: first-hit object of rays {np.flatnonzero(e['first_bad'])[:8]}"
    assert not e["draws_bad"].any(), f"{c.name}, depth {depth}: uniforms consumed differ at rays {np.flatnonzero(e['draws_bad'])[:8]}"
    assert e["t"].max() <= bf.TOL_T and e["normal"].max() <= bf.TOL_NORMAL
    if key[0] not in PT.UNDECIDED_BY_CONSTRUCTION:
        assert e["decided"].mean() >= 1.0 - PT.MAX_UNDECIDED_PATHS


@pytest.mark.parametrize("full", [0, 1], ids=["force_full=0", "force_full=1"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_device_radiance_is_the_statements(lab, key, depth, full):
    against_the_statement(lab, key, depth, full)


@pytest.mark.parametrize("key", [k for k in CASES if k[0] in "BDG"], ids=[i for k, i in zip(CASES, IDS) if k[0] in "BDG"])
def test_device_radiance_is_the_statements_at_depth_5(lab, key):
    against_the_statement(lab, key, 5, 1)


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_device_gives_the_oracles_bits(lab, P, O, key):
    """Records and states equal oracle.trace_paths byte for byte on every path, undecided ones included."""
    c = lab.case(key)
    s = lab.scene
    variants = VARIANTS if key[0] in "DG" else [(-1, 1)]
    lit = False
    for depth in (1, 2, 3, 5, 8):
        for samples in (1, 3):
            st = c.states.copy()
            want = O.trace_paths(c.world.oracle_desc(P), c.o, c.d, st, samples, depth)
            for fg, pt in (variants if (depth, samples) in ((3, 1), (5, 3)) else variants[:1]):
                s.set_option("force_geom", fg)
                s.set_option("pair_trace", pt)
                try:
                    got, after = lab.query(c, depth, samples)
                finally:
                    s.set_option("force_geom", -1)
                    s.set_option("pair_trace", 1)
                bad = np.flatnonzero(bits_differ(got, want))
                what = f"{c.name}, depth {depth}, {samples} samples, force_geom {fg}, pair_trace {pt}"
                assert bad.size == 0, f"{what}: {bad.size} records differ, first {bad[:8]}: {got[bad[0]]} vs {want[bad[0]]}"
                assert np.array_equal(after, st), f"{what}: states differ"
            lit |= bool(np.nan_to_num(want["radiance"]).any())
    assert lit or key[2] == "off"


def test_probes_reduce_the_radiance_just_pinned(lab, P, O):
    """Light set G through query_probes: 8 positions (one inside the glass) x 64 directions; the probe record is
    probe_restatement over oracle.trace_paths' records of the same rays and states, bit for bit."""
    import torch
    c = lab.case(("G", "free", "gradient"))
    s = lab.scene
    pos = np.array([[-2.0, 2.0, 0.0], [2.0, 1.5, -1.0], [0.0, 3.0, 3.0], [-4.0, 0.5, -4.0], [4.0, 2.5, 2.0], [1.0, 4.0, -4.0],
                    [-1.5, 1.0, 3.0], PT.GLASS_CENTRE], np.float32)
    dirs = P.probes.fibonacci_sphere(64) if hasattr(P.probes, "fibonacci_sphere") else None
    if dirs is None:
        rs = np.random.RandomState(5)
        dirs = rs.normal(size=(64, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs = np.ascontiguousarray(np.asarray(dirs.cpu() if hasattr(dirs, "cpu") else dirs, np.float32))
    n, k = len(pos), len(dirs)
    states = O.xorwow_init(PT.SEED, 50000, n * k)
    for samples, depth in ((1, 3), (2, 5)):
        st = dev_states(states)
        rows = s.query_probes(torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda(), st, samples=samples, max_depth=depth,
                              max_distance=20.0).cpu().numpy()
        so = states.copy()
        r = O.trace_paths(c.world.oracle_desc(P), np.repeat(pos, k, axis=0), np.tile(dirs, (n, 1)), so, samples, depth)
        want = R.restate(r["radiance"], r["depth"], r["object_id"], dirs, k, 20.0)
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), f"{samples} samples, depth {depth}"
        assert np.array_equal(host_states(st), so)
        assert (r["object_id"].reshape(n, k)[-1] == 4).all() and rows[:, :3].any()
