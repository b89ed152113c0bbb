"""The contract of ptrt_set_option / ptrt_get_option, name by name: defaults of a fresh context, which values are
rejected, and what an accepted value is normalised to.

EXPECTED below was recorded from the library as it stood BEFORE the two entry points were put on one table, so it pins the
earlier behaviour and is no restatement of the table.  How: that commit's ptrt_capi.hip was compiled, unchanged, together
with one extra function that makes a ptrt_ctx with `new` and enters it in the live set (ptrt_create itself needs a HIP
device; the two option entry points touch nothing but the context's fields), and observe() of this file was run against
that build with the function in ptrt_create's place.  The harness is not part of the repository.  One entry differs from
that recording on purpose: `pm1_wg` = 3.  The earlier library accepted 0..20 although its own message and include/ptrt.h
say 0..2 (3..20 behaved as 0); it now rejects above 2, and the recorded [0, 3] at that probe reads [-1, 2] here.

The first and the fourth test below read only this file's literals: they keep EXPECTED, the probes and the documented
ranges consistent with each other, and call no library code."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

OK, E_INVALID = 0, -1

# how each settable option is probed: the values handed to ptrt_set_option, in order, on one fresh context per option.
# Rejecting options: lo - 1, lo, hi, hi + 1 of the range include/ptrt.h documents.
REJECT = {"force_geom": (-1, 2), "steal": (0, 64), "csteal": (0, 64), "csteal_leaf_min": (1, 64), "csteal_min": (0, 1024),
          "lds_pad": (0, 32768), "tile_run": (0, 64), "split": (1, 4), "pm1_wg": (0, 2), "shade_min": (1, 64),
          "leaf_min": (1, 64), "fetch_min": (0, 64)}
BOOLEAN = ["count_rays", "force_full", "pair_trace", "atrous_exp", "csteal_follow", "leaf_pairs", "time_kernels",
           "time_launches", "pipeline", "tlas_rounds", "pair_split", "async_lanes", "wavefront", "denoiser_active",
           "motion_vectors", "use_graphs"]
NORMALISED = {  # clamp, mask, tri-state, snap
    "lds_nodes": [-1, 0, 1, 2, 3, 100], "ticket_tiles": [0, 1, 7, 16, 17, -3], "refill": [-1, 0, 1, 2, 3], "persist": [-1, 0, 5, 1000],
    "tm_prio": [-1, 0, 2, 3, 4, 7], "stage": [-1, 0, 5, 7, 8, 13],
    "merged": [-5, -1, 0, 1, 7], "sample_sync": [-5, -1, 0, 1, 7],
    "wf_sort": [-1, 0, 1, 2, 3, 4, 5, 9],
}
READ_ONLY = ["sample_sync_eff", "refilled", "split_eff", "pipelined", "render_mode", "pmode", "merged_eff", "merged_decided",
             "launches", "query_pmode", "inst_pre_ok", "tlas_refits", "stream"]


def probes():
    p = {n: [lo - 1, lo, hi, hi + 1] for n, (lo, hi) in REJECT.items()}
    p.update({n: [1, 0, 2, -1] for n in BOOLEAN})
    p.update(NORMALISED)
    return p


class Ctx:
    def __init__(self, P):
        self.lib, self.h = P.lib, C.c_void_p()
        assert P.lib.ptrt_create(16, 16, 0, 16, 0, C.byref(self.h)) == OK

    def set(self, name, value):
        return self.lib.ptrt_set_option(self.h, name.encode(), value)

    def get(self, name):
        v = C.c_longlong(-12345)
        rc = self.lib.ptrt_get_option(self.h, name.encode(), C.byref(v))
        return rc, v.value

    def close(self):
        self.lib.ptrt_destroy(self.h)


def observe(P):
    """{"defaults": {name: value on a fresh context}, "set": {name: [[result code of set, value get returns afterwards], ...]}},
    the second in the order of probes()[name]."""
    c = Ctx(P)
    defaults = {}
    for n in sorted(probes()) + READ_ONLY:
        rc, v = c.get(n)
        assert rc == OK, n
        defaults[n] = v
    c.close()
    defaults.pop("stream")  # a handle: differs run by run (test_stream_is_the_context_s_stream)
    seen = {}
    for n, values in probes().items():
        c = Ctx(P)
        seen[n] = []
        for v in values:
            rc = c.set(n, v)
            grc, got = c.get(n)
            assert grc == OK, n
            seen[n].append([rc, got])
        c.close()
    return {"defaults": defaults, "set": seen}


EXPECTED = {
    "defaults": {
        "async_lanes": 0, "atrous_exp": 0, "count_rays": 0, "csteal": 2, "csteal_follow": 1, "csteal_leaf_min": 32,
        "csteal_min": 0, "denoiser_active": 1, "fetch_min": 16, "force_full": 0, "force_geom": -1, "inst_pre_ok": 0,
        "launches": 0, "lds_nodes": 0, "lds_pad": 0, "leaf_min": 8, "leaf_pairs": 1, "merged": -1,
        "merged_decided": 1, "merged_eff": 0, "motion_vectors": 1, "pair_split": 1, "pair_trace": 1, "persist": 0,
        "pipeline": 1, "pipelined": 0, "pm1_wg": 1, "pmode": 0, "query_pmode": -1, "refill": 1, "refilled": 0,
        "render_mode": 0, "sample_sync": -1, "sample_sync_eff": 0, "shade_min": 32, "split": 2, "split_eff": 1,
        "stage": 7, "steal": 1, "ticket_tiles": 1, "tile_run": 8, "time_kernels": 1, "time_launches": 0,
        "tlas_refits": 0, "tlas_rounds": 0, "tm_prio": 0, "use_graphs": 0, "wavefront": 0, "wf_sort": 0,
    },
    "set": {
        "async_lanes": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "atrous_exp": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "count_rays": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "csteal": [[-1, 2], [0, 0], [0, 64], [-1, 64]],
        "csteal_follow": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "csteal_leaf_min": [[-1, 32], [0, 1], [0, 64], [-1, 64]],
        "csteal_min": [[-1, 0], [0, 0], [0, 1024], [-1, 1024]],
        "denoiser_active": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "fetch_min": [[-1, 16], [0, 0], [0, 64], [-1, 64]],
        "force_full": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "force_geom": [[-1, -1], [0, -1], [0, 2], [-1, 2]],
        "lds_nodes": [[0, 0], [0, 0], [0, 1], [0, 2], [0, 2], [0, 2]],
        "lds_pad": [[-1, 0], [0, 0], [0, 32768], [-1, 32768]],
        "leaf_min": [[-1, 8], [0, 1], [0, 64], [-1, 64]],
        "leaf_pairs": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "merged": [[0, -1], [0, -1], [0, 0], [0, 1], [0, 1]],
        "motion_vectors": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "pair_split": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "pair_trace": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "persist": [[0, 0], [0, 0], [0, 5], [0, 1000]],
        "pipeline": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "pm1_wg": [[-1, 1], [0, 0], [0, 2], [-1, 2]],  # recorded [0, 3] at the last probe: the earlier library took 0..20
        "refill": [[0, 0], [0, 0], [0, 1], [0, 2], [0, 2]],
        "sample_sync": [[0, -1], [0, -1], [0, 0], [0, 1], [0, 1]],
        "shade_min": [[-1, 32], [0, 1], [0, 64], [-1, 64]],
        "split": [[-1, 2], [0, 1], [0, 4], [-1, 4]],
        "stage": [[0, 7], [0, 0], [0, 5], [0, 7], [0, 0], [0, 5]],
        "steal": [[-1, 1], [0, 0], [0, 64], [-1, 64]],
        "ticket_tiles": [[0, 1], [0, 1], [0, 7], [0, 16], [0, 16], [0, 1]],
        "tile_run": [[-1, 8], [0, 0], [0, 64], [-1, 64]],
        "time_kernels": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "time_launches": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "tlas_rounds": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "tm_prio": [[0, 3], [0, 0], [0, 2], [0, 3], [0, 0], [0, 3]],
        "use_graphs": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "wavefront": [[0, 1], [0, 0], [0, 1], [0, 1]],
        "wf_sort": [[0, 0], [0, 0], [0, 1], [0, 2], [0, 2], [0, 4], [0, 4], [0, 4]],
    },
}


def test_there_are_37_settable_options_and_13_read_only_facts():
    assert len(probes()) == 37 and len(READ_ONLY) == 13 and not set(probes()) & set(READ_ONLY)
    assert set(EXPECTED["defaults"]) == (set(probes()) | set(READ_ONLY)) - {"stream"}
    assert set(EXPECTED["set"]) == set(probes())
    for n, rows in EXPECTED["set"].items():
        assert len(rows) == len(probes()[n]), n


@pytest.fixture(scope="module")
def observed(P):
    return observe(P)


def test_defaults_of_a_fresh_context(observed):
    got = observed["defaults"]
    for n, v in EXPECTED["defaults"].items():
        assert got[n] == v, (n, got[n], v)


@pytest.mark.parametrize("name", sorted(probes()))
def test_set_result_and_normalised_value(observed, name):
    got = observed["set"][name]
    assert got == EXPECTED["set"][name], (name, probes()[name], got, EXPECTED["set"][name])


def test_rejecting_options_reject_exactly_outside_their_range():
    """The recorded table again, read as the rule it should follow: lo - 1 and hi + 1 refused and the value kept, lo and hi taken."""
    for n, (lo, hi) in REJECT.items():
        below, at_lo, at_hi, above = EXPECTED["set"][n]
        assert below == [E_INVALID, EXPECTED["defaults"][n]] and at_lo == [OK, lo] and at_hi == [OK, hi] and above == [E_INVALID, hi], n


def test_read_only_names_are_refused_by_set(P):
    c = Ctx(P)
    for n in READ_ONLY:
        before = c.get(n)
        assert c.set(n, 1) == E_INVALID, n
        assert b"unknown option" in P.lib.ptrt_last_error(c.h), n
        assert c.get(n) == before, n
    c.close()


def test_unknown_name_is_refused_by_both(P):
    c = Ctx(P)
    for n in ("no_such_option", "", "pm1_wg ", "PM1_WG"):
        assert c.set(n, 1) == E_INVALID, n
        assert c.get(n) == (E_INVALID, -12345), n  # and the caller's value is left alone
    assert c.lib.ptrt_set_option(c.h, None, 1) == E_INVALID
    assert c.lib.ptrt_get_option(c.h, b"split", None) == E_INVALID
    c.close()


def test_stream_is_the_context_s_stream(P):
    c = Ctx(P)
    rc, v = c.get("stream")
    assert rc == OK and v != 0
    c.close()


def test_leaf_min_round_trips(P):
    c = Ctx(P)
    for v in (1, 17, 64, 8):
        assert c.set("leaf_min", v) == OK
        assert c.get("leaf_min") == (OK, v)
    assert c.set("leaf_min", 0) == E_INVALID and c.get("leaf_min") == (OK, 8)
    c.close()
