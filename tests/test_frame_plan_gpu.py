"""What ptrt_render decides about a frame -- which loop shape renders it, whether it is dealt to several launches, whether
it overlaps its predecessor, whether lanes are refilled -- case by case, as the read-only options report it afterwards.

Every case builds one Scene, renders FRAMES frames into two alternating device targets (or to the host, where the case
says so) and notes after every frame

    (render_mode, pmode, merged_eff, split_eff, pipelined, refilled, sample_sync_eff, pm1_dense_roots_eff, pm1_full_leaf_eff)

EXPECTED below was recorded from the library as it stood BEFORE these decisions were gathered into one FramePlan
(csrc/ptrt_render.hip.h: plan_frame, plan_overlap, launch_frame), at the commit "PMODE 1: full-leaf triangle loop; tri_test
with one bound, one guard": observe() of this file was run on an MI355X against that commit's build, and every tuple was
then read against the rules in plan_overlap, pair_mode and the lane-refill comment of ptrt_render before it was taken
as truth.  So the table pins the earlier behaviour and is no restatement of plan_frame.  It asserts facts only: the frames'
bits at these shapes are compared with the oracle by test_parity_gpu, test_misc_gpu, test_pm1_*_gpu, test_wavefront_gpu and
test_async_gpu.

The frames are 64 x 48 at 2 spp and 4 bounces unless a case says otherwise: six rows of tiles, so a split of 2 is possible.
No case sets option "merged" = -1, and what its sampling of kernel times chooses is not this table's to pin.  It is the
default, though, and some cases run scenes that have both loop shapes with it: cornell-force_geom1, showcase-lds_nodes1 / 2,
showcase-wavefront and the many6 cases.  Their FRAMES = TUNE_WARM = 4 frames are the sampling's warm-up frames, which measure
nothing: the separate-phase loop (merged_eff 0, PMODE 2), ordered behind the stream, whatever the clock says -- which is
why cornell-force_geom1 and many6 never overlap.

One recording contradicted what its cases were written to exercise, not the library's rules: scenes.many(n=6) has 13
meshes, which one TLAS leaf holds, so it renders in PMODE 2 (not 3) and the wavefront stages and the asynchronous lanes
take it (render_mode 1 and 2).  Those cases stay as recorded; the many30 cases beside them have the TLAS with inner nodes
(tests/test_tlas_refit.py relies on it): PMODE 3, and both other loop shapes fall back to render_mode 0.

`shape` in CASES is the FramePlan::shape each case is expected to run (TILES, PM1_WG2, LDS_NODES, WAVEFRONT, ASYNC); the
library does not report it, the last test below only keeps the list of cases covering all five."""
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 4
FACTS = ("render_mode", "pmode", "merged_eff", "split_eff", "pipelined", "refilled", "sample_sync_eff",
         "pm1_dense_roots_eff", "pm1_full_leaf_eff")

# (name, scene, options, extras, shape).  extras: size, depth, denoiser, host (render to host memory), escape (the frame
# before which ptrt_device_buffer is called once)
CASES = [
    ("cornell", "cornell", {}, {}, "TILES"),
    ("cornell-refill2", "cornell", {"refill": 2}, {}, "TILES"),
    ("cornell-pm1_wg2", "cornell", {"pm1_wg": 2}, {}, "PM1_WG2"),
    ("cornell-pm1_wg2-refill2", "cornell", {"pm1_wg": 2, "refill": 2}, {}, "PM1_WG2"),
    ("cornell-pair_trace0", "cornell", {"pair_trace": 0}, {}, "TILES"),
    ("cornell-force_geom1", "cornell", {"force_geom": 1}, {}, "TILES"),
    ("cornell-force_geom2", "cornell", {"force_geom": 2}, {}, "TILES"),
    ("cornell-pipeline0", "cornell", {"pipeline": 0}, {}, "TILES"),
    ("cornell-split1", "cornell", {"split": 1}, {}, "TILES"),
    ("cornell-split4", "cornell", {"split": 4}, {}, "TILES"),
    ("cornell-64x24", "cornell", {}, {"size": (64, 24)}, "TILES"),
    ("cornell-depth8", "cornell", {}, {"depth": 8}, "TILES"),
    ("cornell-lds_pad32768", "cornell", {"lds_pad": 32768}, {}, "TILES"),
    ("cornell-wavefront", "cornell", {"wavefront": 1}, {}, "WAVEFRONT"),
    ("cornell-async_lanes", "cornell", {"async_lanes": 1}, {}, "ASYNC"),
    ("cornell-denoiser", "cornell", {}, {"denoiser": True}, "TILES"),
    ("cornell-to-host", "cornell", {}, {"host": True}, "TILES"),
    ("cornell-escaped", "cornell", {}, {"escape": 2}, "TILES"),
    ("showcase-merged0", "showcase", {"merged": 0}, {}, "TILES"),
    ("showcase-merged1", "showcase", {"merged": 1}, {}, "TILES"),
    ("showcase-lds_nodes1", "showcase", {"lds_nodes": 1}, {}, "LDS_NODES"),
    ("showcase-lds_nodes2", "showcase", {"lds_nodes": 2}, {}, "LDS_NODES"),
    ("showcase-wavefront", "showcase", {"wavefront": 1}, {}, "WAVEFRONT"),
    ("many6", "many6", {}, {}, "TILES"),
    ("many6-wavefront", "many6", {"wavefront": 1}, {}, "WAVEFRONT"),
    ("many6-async_lanes", "many6", {"async_lanes": 1}, {}, "ASYNC"),
    ("many30", "many30", {}, {}, "TILES"),
    ("many30-wavefront", "many30", {"wavefront": 1}, {}, "TILES"),
    ("many30-async_lanes", "many30", {"async_lanes": 1}, {}, "TILES"),
]

EXPECTED = {
    "cornell": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] + [(0, 1, 0, 2, 1, 0, 1, 1, 1)] * 3,
    "cornell-refill2": [(0, 1, 0, 1, 0, 1, 1, 1, 1)] + [(0, 1, 0, 2, 1, 1, 1, 1, 1)] * 3,
    "cornell-pm1_wg2": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-pm1_wg2-refill2": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-pair_trace0": [(0, 0, 0, 1, 0, 0, 1, 0, 0)] + [(0, 0, 0, 2, 1, 0, 1, 0, 0)] * 3,
    "cornell-force_geom1": [(0, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "cornell-force_geom2": [(0, 3, 0, 1, 0, 0, 1, 0, 0)] + [(0, 3, 0, 2, 1, 0, 1, 0, 0)] * 3,
    "cornell-pipeline0": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-split1": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-split4": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-64x24": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-depth8": [(0, 1, 0, 1, 0, 0, 0, 1, 1)] + [(0, 1, 0, 2, 1, 0, 0, 1, 1)] * 3,
    "cornell-lds_pad32768": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] + [(0, 1, 0, 2, 1, 0, 1, 1, 1)] * 3,
    "cornell-wavefront": [(1, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-async_lanes": [(2, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-denoiser": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] + [(0, 1, 0, 2, 1, 0, 1, 1, 1)] * 3,
    "cornell-to-host": [(0, 1, 0, 1, 0, 0, 1, 1, 1)] * 4,
    "cornell-escaped": [(0, 1, 0, 1, 0, 0, 1, 1, 1), (0, 1, 0, 2, 1, 0, 1, 1, 1), (0, 1, 0, 1, 0, 0, 1, 1, 1), (0, 1, 0, 1, 0, 0, 1, 1, 1)],
    "showcase-merged0": [(0, 2, 0, 1, 0, 0, 1, 0, 0)] + [(0, 2, 0, 2, 1, 0, 1, 0, 0)] * 3,
    "showcase-merged1": [(0, 4, 1, 1, 0, 0, 1, 0, 0)] + [(0, 4, 1, 2, 1, 0, 1, 0, 0)] * 3,
    "showcase-lds_nodes1": [(0, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "showcase-lds_nodes2": [(0, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "showcase-wavefront": [(1, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "many6": [(0, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "many6-wavefront": [(1, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "many6-async_lanes": [(2, 2, 0, 1, 0, 0, 1, 0, 0)] * 4,
    "many30": [(0, 3, 0, 1, 0, 0, 1, 0, 0)] + [(0, 3, 0, 2, 1, 0, 1, 0, 0)] * 3,
    "many30-wavefront": [(0, 3, 0, 1, 0, 0, 1, 0, 0)] + [(0, 3, 0, 2, 1, 0, 1, 0, 0)] * 3,
    "many30-async_lanes": [(0, 3, 0, 1, 0, 0, 1, 0, 0)] + [(0, 3, 0, 2, 1, 0, 1, 0, 0)] * 3,
}


def observe(P, case):
    """The FACTS after each of the case's FRAMES frames."""
    import torch
    _, scene, options, extras, _ = case
    W, H = extras.get("size", (64, 48))
    s = P.Scene(W, H)
    if scene == "cornell":
        P.scenes.cornell(s)
    elif scene == "showcase":
        P.scenes.showcase(s, segments=8)
    else:
        P.scenes.many(s, n=int(scene[4:]))
    s.setPerfSamplesPerPixel(2)
    s.setMaxBounceDepth(extras.get("depth", 4))
    s.setDenoiserEnabled(extras.get("denoiser", False))
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    for name, value in options.items():
        s.set_option(name, value)
    tgt = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    seen = []
    for f in range(FRAMES):
        if extras.get("escape") == f:
            assert P.lib.ptrt_device_buffer(s.ctx, P.BUF_ACCUM)
        if extras.get("host"):
            s.render_to_host()
        else:
            s.render_to_device(tgt[f & 1].data_ptr())
        seen.append(tuple(s.get_option(n) for n in FACTS))
    s.sync()
    s.close()
    return seen


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_frame_facts(P, case):
    got = observe(P, case)
    print(case[0], got)
    assert got == EXPECTED[case[0]], (case[0], FACTS, got, EXPECTED[case[0]])


def test_cases_are_unique_and_cover_every_shape():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names) and set(names) == set(EXPECTED)
    assert {c[4] for c in CASES} == {"TILES", "PM1_WG2", "LDS_NODES", "WAVEFRONT", "ASYNC"}
    for rows in EXPECTED.values():
        assert len(rows) == FRAMES and all(len(r) == len(FACTS) for r in rows)
