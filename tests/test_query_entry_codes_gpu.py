"""Return code AND ptrt_last_error text of the device-query entry points (csrc/ptrt_query.hip.h): ptrt_trace_rays,
ptrt_query_rays, ptrt_query_radiance, ptrt_query_probes, ptrt_camera_rays, ptrt_init_rng_states -- for every call they refuse,
and, where two reasons apply at once, which one wins.  The table was written from the source of the commit before these entry
points got a file of their own (the order of the checks in each function) and confirmed against a build of it.  The span
messages carry their byte counts: "<fn>: <name> is not <bytes> bytes of device memory on device <d>" for every pointer in turn
pointing at pageable and at pinned host memory.  Sizes: a 16x16 context, 8 rays, 2 probes x 3 directions.  Nothing here
reaches a kernel with a bad argument: every refused call returns before it enqueues anything."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, NOT_READY = 0, -1, -4
VP = C.c_void_p
N, PROBES, DIRS, W, H = 8, 2, 3, 16, 16
INT_MAX = 2 ** 31 - 1


def ptr(p):
    """printf's %p"""
    v = p.value if isinstance(p, VP) else p
    return "(nil)" if not v else hex(v)


@pytest.fixture(scope="module")
def desc(P):
    """(host-only Scene that owns the arrays, its ptrt_scene_desc): two meshes of two triangles each"""
    s = P.Scene(W, H, device=P.HOST_ONLY)
    mat = P.Material((0.7, 0.7, 0.7), 0.5)
    for z in (-3.0, -4.0):
        a, b, c, d = (-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)
        s.addTriangles([a + b + c, a + c + d], mat)
    s.setCamera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0)
    d = C.cast(s.flatten(), C.POINTER(P.SceneDesc)).contents
    assert d.mesh_count == 2 and d.materials.count == 2 and d.camera.lens_radius == 0.0
    yield s, d
    s.close()


@pytest.fixture(scope="module")
def mem():
    """name -> pointer: the good device arrays of every entry point, one pageable and one pinned host block"""
    import torch
    dev = torch.device("cuda", 0)
    o = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    d = torch.tensor([[0.0, 0.0, -1.0]] * N, dtype=torch.float32, device=dev)
    keep = {
        "o": o, "d": d, "tmax": torch.full((N,), 10.0, dtype=torch.float32, device=dev),
        "hits": torch.zeros((N, 16), dtype=torch.int32, device=dev), "occ": torch.zeros((N,), dtype=torch.int32, device=dev),
        "st": torch.zeros((N, 6), dtype=torch.int32, device=dev), "rad": torch.zeros((N, 8), dtype=torch.float32, device=dev),
        "pos": torch.zeros((PROBES, 3), dtype=torch.float32, device=dev), "dirs": d[:DIRS].clone(),
        "pst": torch.zeros((PROBES * DIRS, 6), dtype=torch.int32, device=dev),
        "pout": torch.zeros((PROBES, 32), dtype=torch.float32, device=dev),
        "cam_o": torch.zeros((W * H, 3), dtype=torch.float32, device=dev), "cam_d": torch.zeros((W * H, 3), dtype=torch.float32, device=dev),
        "pinned": torch.zeros(4096, dtype=torch.uint8).pin_memory(),
    }
    pageable = np.zeros(4096, np.uint8)
    m = {k: VP(t.data_ptr()) for k, t in keep.items()}
    m["pageable"] = VP(pageable.ctypes.data)
    torch.cuda.synchronize()
    yield m
    torch.cuda.synchronize()
    del keep, pageable


@pytest.fixture(scope="module")
def ctxs(P, desc):
    """state -> context.  null / stale / destroyed: no context; empty: created, nothing uploaded; geom: geometry only; few: one
    material for the two meshes; full: the scene; lens: the scene under a thin-lens camera"""
    lib = P.lib
    _, d = desc

    def create():
        ctx = VP()
        assert lib.ptrt_create(W, H, 0, 0, 0, C.byref(ctx)) == OK
        return ctx

    def geometry(ctx):
        assert lib.ptrt_upload_geometry(ctx, d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == OK

    buf = C.create_string_buffer(8192)  # stands in for a freed ptrt_ctx: never in the live set
    c = {"null": None, "stale": C.cast(buf, VP), "destroyed": create(), "empty": create(), "geom": create(), "few": create(),
         "full": create(), "lens": create()}
    lib.ptrt_destroy(c["destroyed"])
    geometry(c["geom"])
    geometry(c["few"])
    one = P.Materials()
    C.memmove(C.byref(one), C.byref(d.materials), C.sizeof(P.Materials))
    one.count = 1
    assert lib.ptrt_upload_materials(c["few"], C.byref(one)) == OK
    for k in ("full", "lens"):
        assert lib.ptrt_upload_scene(c[k], C.byref(d)) == OK
    cam = P.Camera()
    C.memmove(C.byref(cam), C.byref(d.camera), C.sizeof(P.Camera))
    cam.lens_radius = 0.25
    assert lib.ptrt_set_camera(c["lens"], C.byref(cam)) == OK
    before = bytes(buf.raw)
    yield c
    assert bytes(buf.raw) == before, "an entry point wrote into a handle that is not a live context"
    for k in ("empty", "geom", "few", "full", "lens"):
        assert lib.ptrt_sync(c[k]) == OK
        lib.ptrt_destroy(c[k])


# ---- the entry points: default (good) arguments by name, and the call ------------------------------------------------
HOST_O = np.zeros((N, 3), np.float32)
HOST_D = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (N, 1))
HOST_HITS = np.zeros(N * 16, np.int32)
FP = C.POINTER(C.c_float)


def good_args(m):
    return {
        "trace": dict(o=VP(HOST_O.ctypes.data), d=VP(HOST_D.ctypes.data), n=N, out=VP(HOST_HITS.ctypes.data)),
        "closest": dict(kind=0, o=m["o"], d=m["d"], tmax=None, n=N, out=m["hits"]),
        "occluded": dict(kind=1, o=m["o"], d=m["d"], tmax=m["tmax"], n=N, out=m["occ"]),
        "radiance": dict(o=m["o"], d=m["d"], st=m["st"], n=N, samples=1, max_depth=2, out=m["rad"]),
        "probes": dict(pos=m["pos"], n=PROBES, dirs=m["dirs"], n_dirs=DIRS, st=m["pst"], samples=1, max_depth=2, max_distance=5.0, out=m["pout"]),
        "camera": dict(frame=0, sample=0, o=m["cam_o"], d=m["cam_d"]),
        "init": dict(seed=7, first=0, n=N, st=m["st"]),
    }


def call(lib, entry, ctx, a):
    if entry == "trace":
        return lib.ptrt_trace_rays(ctx, C.cast(a["o"], FP), C.cast(a["d"], FP), a["n"], a["out"])
    if entry in ("closest", "occluded"):
        return lib.ptrt_query_rays(ctx, a["kind"], a["o"], a["d"], a["tmax"], a["n"], a["out"])
    if entry == "radiance":
        return lib.ptrt_query_radiance(ctx, a["o"], a["d"], a["st"], a["n"], a["samples"], a["max_depth"], a["out"])
    if entry == "probes":
        return lib.ptrt_query_probes(ctx, a["pos"], a["n"], a["dirs"], a["n_dirs"], a["st"], a["samples"], a["max_depth"],
                                     a["max_distance"], a["out"])
    if entry == "camera":
        return lib.ptrt_camera_rays(ctx, a["frame"], a["sample"], a["o"], a["d"])
    return lib.ptrt_init_rng_states(ctx, a["seed"], a["first"], a["n"], a["st"])


FN = {"trace": "ptrt_trace_rays", "closest": "ptrt_query_rays", "occluded": "ptrt_query_rays", "radiance": "ptrt_query_radiance",
      "probes": "ptrt_query_probes", "camera": "ptrt_camera_rays", "init": "ptrt_init_rng_states"}
# the pointer arguments that must be device memory, in the order they are checked: (argument, its name in the message, bytes)
SPANS = {
    "closest": [("o", "origins", N * 12), ("d", "directions", N * 12), ("out", "out", N * 64)],
    "occluded": [("o", "origins", N * 12), ("d", "directions", N * 12), ("tmax", "tmax", N * 4), ("out", "out", N * 4)],
    "radiance": [("o", "origins", N * 12), ("d", "directions", N * 12), ("st", "rng_states", N * 24), ("out", "out", N * 32)],
    "probes": [("pos", "positions", PROBES * 12), ("dirs", "directions", DIRS * 12), ("st", "rng_states", PROBES * DIRS * 24),
               ("out", "out", PROBES * 128)],
    "camera": [("o", "d_origins", W * H * 12), ("d", "d_directions", W * H * 12)],
    "init": [("st", "d_states", N * 24)],
}
# what each entry point says of a NULL pointer; {..} are the call's own arguments as printf prints them
BAD_RAYS = "ptrt_query_rays: bad argument (n {n}, origins {o}, directions {d}, out {out})"
BAD_RADIANCE = "ptrt_query_radiance: bad argument (n {n}, origins {o}, directions {d}, rng_states {st}, out {out})"
BAD_PROBES = "ptrt_query_probes: bad argument (n_probes {n}, n_dirs {n_dirs}, positions {pos}, directions {dirs}, rng_states {st}, out {out})"
BAD_INIT = "ptrt_init_rng_states: bad argument (n {n}, d_states {st})"
NULL_TEXT = {"trace": "ptrt_trace_rays: bad argument", "closest": BAD_RAYS, "occluded": BAD_RAYS, "radiance": BAD_RADIANCE,
             "probes": BAD_PROBES, "camera": "ptrt_camera_rays: a target is NULL", "init": BAD_INIT}
BAD_CONTEXT = {e: f"{FN[e]}: bad context" for e in FN}
BAD_CONTEXT["trace"] = "ptrt_trace_rays: bad argument"
LENS = "ptrt_camera_rays: a thin lens (lens_radius 0.25): the lens sample of a primary ray is drawn from the pixel's generator stream"

# (entry point, context state, arguments that differ from the good ones, return code, message).  `HOST`: the pageable block.
HOST = "pageable"
TABLE = [
    # ---- ptrt_trace_rays: host arrays, one message for every bad argument
    ("trace", "empty", {}, NOT_READY, "ptrt_trace_rays: geometry not uploaded"),
    ("trace", "empty", {"n": 0}, NOT_READY, "ptrt_trace_rays: geometry not uploaded"),
    ("trace", "empty", {"n": -1}, INVALID, "ptrt_trace_rays: bad argument"),            # the argument wins over the missing geometry
    ("trace", "full", {"n": -1}, INVALID, "ptrt_trace_rays: bad argument"),
    ("trace", "full", {"n": 0}, OK, None),
    ("trace", "geom", {}, OK, None),                                                     # (needs no materials)
    # ---- ptrt_query_rays
    ("closest", "full", {"kind": 2}, INVALID, "ptrt_query_rays: kind 2 (PTRT_QUERY_CLOSEST or PTRT_QUERY_OCCLUDED)"),
    ("closest", "full", {"kind": -1, "n": -1, "o": None}, INVALID, "ptrt_query_rays: kind -1 (PTRT_QUERY_CLOSEST or PTRT_QUERY_OCCLUDED)"),
    ("closest", "full", {"n": -1}, INVALID, BAD_RAYS),
    ("occluded", "empty", {"n": -1, "tmax": None}, INVALID, BAD_RAYS),                   # n before tmax before the geometry
    ("occluded", "empty", {"tmax": None}, INVALID, "ptrt_query_rays: PTRT_QUERY_OCCLUDED needs tmax"),
    ("occluded", "full", {"tmax": None, "n": 0}, INVALID, "ptrt_query_rays: PTRT_QUERY_OCCLUDED needs tmax"),
    ("closest", "empty", {"tmax": HOST}, INVALID, "ptrt_query_rays: PTRT_QUERY_CLOSEST takes no tmax (pass NULL)"),
    ("closest", "empty", {}, NOT_READY, "ptrt_query_rays: geometry not uploaded"),
    ("occluded", "empty", {"n": 0}, NOT_READY, "ptrt_query_rays: geometry not uploaded"),  # n == 0 is OK only of a scene
    ("closest", "full", {"n": 0, "o": HOST, "d": HOST, "out": HOST}, OK, None),          # ... and before any pointer is inspected
    ("occluded", "geom", {"n": 0, "o": HOST, "d": HOST, "tmax": HOST, "out": HOST}, OK, None),
    ("closest", "geom", {}, OK, None),
    ("occluded", "geom", {}, OK, None),
    # ---- ptrt_query_radiance
    ("radiance", "empty", {"n": -1, "samples": 0}, INVALID, BAD_RADIANCE),
    ("radiance", "empty", {"samples": 0}, INVALID, "ptrt_query_radiance: samples=0 max_depth=2 (1..32767)"),  # before the scene
    ("radiance", "full", {"samples": 32768}, INVALID, "ptrt_query_radiance: samples=32768 max_depth=2 (1..32767)"),
    ("radiance", "full", {"max_depth": 0, "n": 0}, INVALID, "ptrt_query_radiance: samples=1 max_depth=0 (1..32767)"),
    ("radiance", "full", {"max_depth": 32768}, INVALID, "ptrt_query_radiance: samples=1 max_depth=32768 (1..32767)"),
    ("radiance", "empty", {}, NOT_READY, "ptrt_query_radiance: geometry not uploaded"),
    ("radiance", "empty", {"n": 0}, NOT_READY, "ptrt_query_radiance: geometry not uploaded"),
    ("radiance", "geom", {}, NOT_READY, "ptrt_query_radiance: materials not uploaded"),
    ("radiance", "few", {}, NOT_READY, "ptrt_query_radiance: 1 materials for 2 meshes"),
    ("radiance", "few", {"n": 0}, NOT_READY, "ptrt_query_radiance: 1 materials for 2 meshes"),
    ("radiance", "full", {"n": 0, "o": HOST, "d": HOST, "st": HOST, "out": HOST}, OK, None),
    ("radiance", "full", {"samples": 32767, "max_depth": 1}, OK, None),                  # (the range's upper end; one bounce)
    # ---- ptrt_query_probes
    ("probes", "full", {"n": -1}, INVALID, BAD_PROBES),
    ("probes", "full", {"n_dirs": 0}, INVALID, BAD_PROBES),
    ("probes", "empty", {"n_dirs": 0, "samples": 0, "max_distance": 0.0}, INVALID, BAD_PROBES),
    ("probes", "empty", {"samples": 0, "max_distance": 0.0}, INVALID, "ptrt_query_probes: samples=0 max_depth=2 (1..32767)"),
    ("probes", "full", {"samples": 32768}, INVALID, "ptrt_query_probes: samples=32768 max_depth=2 (1..32767)"),
    ("probes", "full", {"max_depth": 0}, INVALID, "ptrt_query_probes: samples=1 max_depth=0 (1..32767)"),
    ("probes", "full", {"max_depth": 32768}, INVALID, "ptrt_query_probes: samples=1 max_depth=32768 (1..32767)"),
    ("probes", "empty", {"max_distance": 0.0}, INVALID, "ptrt_query_probes: max_distance=0 (positive and finite)"),  # before the scene
    ("probes", "full", {"max_distance": -1.0}, INVALID, "ptrt_query_probes: max_distance=-1 (positive and finite)"),
    ("probes", "full", {"max_distance": float("inf"), "n": 0}, INVALID, "ptrt_query_probes: max_distance=inf (positive and finite)"),
    ("probes", "full", {"max_distance": float("nan")}, INVALID, "ptrt_query_probes: max_distance=nan (positive and finite)"),
    ("probes", "empty", {}, NOT_READY, "ptrt_query_probes: geometry not uploaded"),
    ("probes", "geom", {"n": 0}, NOT_READY, "ptrt_query_probes: materials not uploaded"),
    ("probes", "few", {}, NOT_READY, "ptrt_query_probes: 1 materials for 2 meshes"),
    ("probes", "full", {"n": 0, "pos": HOST, "dirs": HOST, "st": HOST, "out": HOST}, OK, None),
    ("probes", "full", {}, OK, None),
    # ---- ptrt_camera_rays
    ("camera", "full", {"frame": -1, "o": None}, INVALID, "ptrt_camera_rays: frame_index=-1 sample=0"),
    ("camera", "full", {"sample": -1}, INVALID, "ptrt_camera_rays: frame_index=0 sample=-1"),
    ("camera", "full", {"frame": INT_MAX, "sample": 1}, INVALID, f"ptrt_camera_rays: frame_index={INT_MAX} sample=1"),
    ("camera", "lens", {"d": None}, INVALID, "ptrt_camera_rays: a target is NULL"),      # the NULL before the lens
    ("camera", "lens", {}, INVALID, LENS),
    ("camera", "lens", {"o": HOST, "d": HOST}, INVALID, LENS),                           # the lens before the spans
    ("camera", "full", {"frame": INT_MAX - 1, "sample": 1}, OK, None),
    ("camera", "empty", {}, OK, None),                                                   # (the camera's rays need no scene)
    # ---- ptrt_init_rng_states
    ("init", "empty", {"n": -1, "st": None}, INVALID, BAD_INIT),
    ("init", "empty", {"n": 0, "st": HOST, "first": 2 ** 64 - 1}, OK, None),
    ("init", "empty", {"first": 2 ** 64 - 2, "n": 3, "st": HOST}, INVALID, "ptrt_init_rng_states: subsequence numbers beyond 2^64"),
    ("init", "empty", {"first": 2 ** 64 - 1, "n": 2}, INVALID, "ptrt_init_rng_states: subsequence numbers beyond 2^64"),
    ("init", "empty", {"first": 2 ** 64 - 1, "n": 1, "st": HOST}, INVALID,              # (no overflow: the span, before the jump matrices)
     "ptrt_init_rng_states: d_states is not 24 bytes of device memory on device 0"),
    ("init", "empty", {"first": 2 ** 40}, INVALID,
     "ptrt_init_rng_states: subsequence numbers of 41 bits (at most 40: 2^40 pixels or states)"),
    ("init", "empty", {"first": 2 ** 40 - N}, OK, None),
]


def resolve(m, over):
    return {k: (m[v] if isinstance(v, str) else v) for k, v in over.items()}


def check(lib, ctxs, mem, entry, state, over, rc, text):
    a = dict(good_args(mem)[entry], **resolve(mem, over))
    got = call(lib, entry, ctxs[state], a)
    said = lib.ptrt_last_error(ctxs[state]).decode()
    print(f"{FN[entry]} [{state}] {over}: {got} {said if got else ''}")
    assert got == rc, (entry, state, over, said)
    if text is not None:
        want = text.format(**{k: (ptr(v) if v is None or isinstance(v, VP) else v) for k, v in a.items()})
        assert said == want, (entry, state, over)


def test_no_context(P, ctxs, mem):
    """NULL, a handle that never was a context and one that no longer is: PTRT_E_INVALID whatever else is wrong"""
    for state in ("null", "stale", "destroyed"):
        for entry in FN:
            check(P.lib, ctxs, mem, entry, state, {}, INVALID, BAD_CONTEXT[entry])
        check(P.lib, ctxs, mem, "closest", state, {"kind": 2, "n": -1}, INVALID, BAD_CONTEXT["closest"])
        check(P.lib, ctxs, mem, "probes", state, {"n_dirs": 0, "samples": 0}, INVALID, BAD_CONTEXT["probes"])
        check(P.lib, ctxs, mem, "init", state, {"n": 0}, INVALID, BAD_CONTEXT["init"])


def test_table(P, ctxs, mem):
    for entry, state, over, rc, text in TABLE:
        check(P.lib, ctxs, mem, entry, state, over, rc, text)


def test_each_pointer_null(P, ctxs, mem):
    """a NULL pointer is PTRT_E_INVALID before the scene is looked at, and with n == 0 as well"""
    args = good_args(mem)
    for entry in FN:
        names = [k for k, v in args[entry].items() if isinstance(v, VP)]
        assert len(names) == {"trace": 3, "closest": 3, "occluded": 4, "radiance": 4, "probes": 4, "camera": 2, "init": 1}[entry]
        for k in names:
            if (entry, k) == ("occluded", "tmax"):
                continue  # (its own message: the table)
            for state in ("empty", "full"):
                check(P.lib, ctxs, mem, entry, state, {k: None}, INVALID, NULL_TEXT[entry])
                if "n" in args[entry]:
                    check(P.lib, ctxs, mem, entry, state, {k: None, "n": 0}, INVALID, NULL_TEXT[entry])


def test_each_pointer_in_host_memory(P, ctxs, mem):
    """pageable and pinned host memory where device memory is needed: PTRT_E_INVALID, the argument's name and ITS byte count;
    of several, the first in the argument order; behind every other refusal"""
    lib = P.lib
    for entry, spans in SPANS.items():
        state = "empty" if entry == "init" else "full"
        for host in ("pageable", "pinned"):
            for k, name, nbytes in spans:
                check(lib, ctxs, mem, entry, state, {k: host}, INVALID,
                      f"{FN[entry]}: {name} is not {nbytes} bytes of device memory on device 0")
            for first in range(len(spans)):
                _, name, nbytes = spans[first]
                check(lib, ctxs, mem, entry, state, {k: host for k, _, _ in spans[first:]}, INVALID,
                      f"{FN[entry]}: {name} is not {nbytes} bytes of device memory on device 0")
    # the byte counts follow the counts of the call: 3 rays, 1 probe of 2 directions
    check(lib, ctxs, mem, "closest", "full", {"n": 3, "out": HOST}, INVALID, "ptrt_query_rays: out is not 192 bytes of device memory on device 0")
    check(lib, ctxs, mem, "occluded", "full", {"n": 3, "out": HOST}, INVALID, "ptrt_query_rays: out is not 12 bytes of device memory on device 0")
    check(lib, ctxs, mem, "probes", "full", {"n": 1, "n_dirs": 2, "st": HOST}, INVALID,
          "ptrt_query_probes: rng_states is not 48 bytes of device memory on device 0")
    # every other refusal comes first
    check(lib, ctxs, mem, "closest", "empty", {"o": HOST}, NOT_READY, "ptrt_query_rays: geometry not uploaded")
    check(lib, ctxs, mem, "radiance", "few", {"o": HOST}, NOT_READY, "ptrt_query_radiance: 1 materials for 2 meshes")
    check(lib, ctxs, mem, "radiance", "full", {"o": HOST, "samples": 0}, INVALID, "ptrt_query_radiance: samples=0 max_depth=2 (1..32767)")
    check(lib, ctxs, mem, "probes", "full", {"pos": HOST, "max_distance": 0.0}, INVALID, "ptrt_query_probes: max_distance=0 (positive and finite)")


def test_the_good_calls_still_answer(P, ctxs, mem):
    """after all the refusals the contexts are in order: the good arguments of every entry point are accepted, and the queries
    see the quad at z = -3"""
    import torch
    lib = P.lib
    for entry in FN:
        check(lib, ctxs, mem, entry, "empty" if entry in ("init", "camera") else "full", {}, OK, None)
    assert lib.ptrt_sync(ctxs["full"]) == OK and lib.ptrt_sync(ctxs["empty"]) == OK
    hits = HOST_HITS.view(P.HIT_DTYPE)
    assert (hits["hit"] == 1).all() and (hits["t"] == 3.0).all() and (hits["mesh_index"] == 0).all()
    torch.cuda.synchronize()
