"""Return codes of the acceleration-structure entry points (csrc/ptrt_accel.hip.h) for the calls their shared preamble
answers: a destroyed handle, a live context before any geometry upload, a mesh index of -1 and of the mesh count, a NULL
array -- and, where two of these apply at once, which one wins.  The table was written from the source of the commit
before the entry points moved into that file (order of the checks in each function) and confirmed against a build of it.
Two state facts ride along: a ptrt_build_bvh refused for its mesh index still marks the instances' first-pass boxes stale,
and a failed ptrt_upload_geometry on a fresh context leaves it answering PTRT_E_NOT_READY to ptrt_render.  Nothing here
reaches a kernel with a bad argument: every refused call returns before it enqueues anything."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, NOT_READY = 0, -1, -4
VP = C.c_void_p


def two_quads(P, s):
    """two meshes of two triangles each: a one-leaf TLAS"""
    mat = P.Material((0.7, 0.7, 0.7), 0.5)
    for z in (-3.0, -4.0):
        a, b, c, d = (-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)
        s.addTriangles([a + b + c, a + c + d], mat)


def eighteen(P, s):
    """the Cornell box's eight meshes and ten more: the smallest scene whose TLAS has inner nodes"""
    P.scenes.many(s, 10)


@pytest.fixture(scope="module", params=[two_quads, eighteen], ids=["two_quads", "eighteen"])
def desc(P, request):
    """(host-only Scene that owns the arrays, its ptrt_scene_desc)"""
    lib = P.lib
    lib.ptrt_update_instances.restype = C.c_int
    lib.ptrt_update_instances.argtypes = [VP, C.POINTER(P.MeshDesc), C.c_int, C.POINTER(P.BvhNode), C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.ptrt_debug_upload_counts.restype = C.c_int
    lib.ptrt_debug_upload_counts.argtypes = [VP, C.POINTER(C.c_int)]
    s = P.Scene(16, 16, device=P.HOST_ONLY)
    request.param(P, s)
    d = C.cast(s.flatten(), C.POINTER(P.SceneDesc)).contents
    assert d.mesh_count == (2 if request.param is two_quads else 18)
    assert (d.tlas_node_count == 1) == (request.param is two_quads)
    yield s, d
    s.close()


def create(P):
    ctx = VP()
    assert P.lib.ptrt_create(16, 16, 0, 0, 0, C.byref(ctx)) == OK
    return ctx


def calls(P, d, dev_xf, mesh=0, null=False):
    """name -> thunk(ctx) for every moved entry point, with well-formed arguments for scene `d` -- or, with `null`, its array
    argument NULL (entry points without one are left out); `mesh`: the mesh index of those that take one"""
    lib = P.lib
    n = d.mesh_count
    M = d.meshes[mesh] if 0 <= mesh < n else d.meshes[0]
    xf = (P.InstanceXform * 1)()
    for k in (0, 5, 10, 15):
        xf[0].world[k] = xf[0].inverse[k] = xf[0].normal[k] = 1.0
    verts = np.ctypeslib.as_array(C.cast(M.verts, C.POINTER(C.c_float)), (M.vert_count * 3,)).copy()  # (as uploaded: nothing moves)
    order = (C.c_int * max(M.face_count, 1))()
    nodes = (P.BvhNode * d.tlas_node_count)()
    bnodes = (P.BvhNode * max(M.node_count, 1))()
    ids = (C.c_int32 * d.tlas_index_count)()
    counts = (C.c_int * 2)()
    fp = C.POINTER(C.c_float)
    t = {
        "ptrt_upload_geometry": None if not null else lambda c: lib.ptrt_upload_geometry(c, None, n, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count),
        "ptrt_upload_geometry:tlas_nodes": None if not null else lambda c: lib.ptrt_upload_geometry(c, d.meshes, n, None, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count),
        "ptrt_upload_geometry:tlas_mesh_indices": None if not null else lambda c: lib.ptrt_upload_geometry(c, d.meshes, n, d.tlas_nodes, d.tlas_node_count, None, d.tlas_index_count),
        "ptrt_update_instances": lambda c: lib.ptrt_update_instances(c, None if null else d.meshes, n, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count),
        "ptrt_set_instance_transforms": lambda c: lib.ptrt_set_instance_transforms(c, mesh, 1, None if null else xf),
        "ptrt_set_instance_transforms_device": lambda c: lib.ptrt_set_instance_transforms_device(c, mesh, 1, None if null else dev_xf),
        "ptrt_refit_tlas": None if null else lambda c: lib.ptrt_refit_tlas(c),
        "ptrt_reorder_tlas": None if null else lambda c: lib.ptrt_reorder_tlas(c),
        "ptrt_read_tlas_order": lambda c: lib.ptrt_read_tlas_order(c, None if null else ids, d.tlas_index_count),
        "ptrt_read_tlas": lambda c: lib.ptrt_read_tlas(c, None if null else nodes, d.tlas_node_count),
        "ptrt_debug_upload_counts": lambda c: lib.ptrt_debug_upload_counts(c, None if null else counts),
        "ptrt_update_vertices": lambda c: lib.ptrt_update_vertices(c, mesh, None if null else verts.ctypes.data_as(fp), M.vert_count, 0),
        "ptrt_refit": None if null else lambda c: lib.ptrt_refit(c),
        "ptrt_build_bvh": None if null else lambda c: lib.ptrt_build_bvh(c, mesh),
        "ptrt_update_triangles": lambda c: lib.ptrt_update_triangles(c, mesh, None if null else verts.ctypes.data, 1, 0),
        "ptrt_read_prim_order": lambda c: lib.ptrt_read_prim_order(c, mesh, None if null else order, M.face_count),
        "ptrt_read_bvh": lambda c: lib.ptrt_read_bvh(c, mesh, None if null else bnodes, M.node_count),
    }
    t = {k: v for k, v in t.items() if v is not None}
    t["_keep"] = lambda c, keep=(xf, verts, order, nodes, bnodes, ids, counts): OK  # (the thunks borrow these)
    return t


def run(table, ctx, only=None):
    got = {k: f(ctx) for k, f in table.items() if k != "_keep" and (only is None or k in only)}
    for k, v in got.items():
        print(f"{k}: {v}")
    return got


MOVED = ["ptrt_update_instances", "ptrt_set_instance_transforms", "ptrt_set_instance_transforms_device", "ptrt_refit_tlas",
         "ptrt_reorder_tlas", "ptrt_read_tlas_order", "ptrt_read_tlas", "ptrt_debug_upload_counts", "ptrt_update_vertices",
         "ptrt_refit", "ptrt_build_bvh", "ptrt_update_triangles", "ptrt_read_prim_order", "ptrt_read_bvh"]
WITH_ARRAY = ["ptrt_upload_geometry", "ptrt_upload_geometry:tlas_nodes", "ptrt_upload_geometry:tlas_mesh_indices",
              "ptrt_update_instances", "ptrt_set_instance_transforms", "ptrt_set_instance_transforms_device", "ptrt_read_tlas_order",
              "ptrt_read_tlas", "ptrt_debug_upload_counts", "ptrt_update_vertices", "ptrt_update_triangles", "ptrt_read_prim_order",
              "ptrt_read_bvh"]
WITH_MESH = ["ptrt_set_instance_transforms", "ptrt_set_instance_transforms_device", "ptrt_update_vertices", "ptrt_build_bvh",
             "ptrt_update_triangles", "ptrt_read_prim_order", "ptrt_read_bvh"]


@pytest.fixture(scope="module")
def dev_xf():
    import torch
    one = np.zeros(49, np.float32)      # ptrt_instance_xform: world, inverse, normal = identity; has_transform = 0
    one[[0, 5, 10, 15, 16, 21, 26, 31, 32, 37, 42, 47]] = 1.0
    t = torch.from_numpy(np.tile(one, 4)).cuda()
    yield VP(t.data_ptr())
    del t


def test_a_destroyed_handle_is_invalid_everywhere_and_left_alone(P, desc, dev_xf):
    _, d = desc
    buf = C.create_string_buffer(8192)  # stands in for a freed ptrt_ctx: never in the live set
    stale = C.cast(buf, VP)
    before = bytes(buf.raw)
    good = run(calls(P, d, dev_xf), stale)
    null = run(calls(P, d, dev_xf, null=True), stale)
    assert good == {k: INVALID for k in MOVED}
    assert null == {k: INVALID for k in WITH_ARRAY}
    assert P.lib.ptrt_upload_geometry(stale, d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices,
                                      d.tlas_index_count) == INVALID
    assert bytes(buf.raw) == before, "an entry point wrote into a handle that is not a live context"
    ctx = create(P)     # ... and a handle that WAS one
    P.lib.ptrt_destroy(ctx)
    assert run(calls(P, d, dev_xf), ctx) == {k: INVALID for k in MOVED}


def test_before_any_upload(P, desc, dev_xf):
    """PTRT_E_NOT_READY, except where a NULL array is looked at first -- and where it is not"""
    _, d = desc
    ctx = create(P)
    try:
        good = run(calls(P, d, dev_xf), ctx)
        assert good == {k: (OK if k == "ptrt_debug_upload_counts" else NOT_READY) for k in MOVED}
        null = run(calls(P, d, dev_xf, null=True), ctx)
        # the two transform calls look for geometry before they look at their array; everything else refuses the NULL first
        assert null == {k: (NOT_READY if k.startswith("ptrt_set_instance_transforms") else INVALID) for k in WITH_ARRAY}
        # ptrt_update_triangles takes NULL with a count of zero as an argument in order
        assert P.lib.ptrt_update_triangles(ctx, 0, None, 0, 0) == NOT_READY
        assert P.lib.ptrt_update_triangles(ctx, 0, None, -1, 0) == INVALID
        out = (C.c_int * 2)(7, 7)
        assert P.lib.ptrt_debug_upload_counts(ctx, out) == OK and tuple(out) == (0, 0)
    finally:
        P.lib.ptrt_destroy(ctx)


def test_after_an_upload(P, desc, dev_xf):
    _, d = desc
    lib = P.lib
    n = d.mesh_count
    ctx = create(P)
    try:
        assert lib.ptrt_upload_geometry(ctx, d.meshes, n, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == OK
        opt = C.c_longlong(-1)
        assert lib.ptrt_get_option(ctx, b"inst_pre_ok", C.byref(opt)) == OK and opt.value == 1
        # (c) a mesh index of -1 and of the mesh count
        for mesh in (-1, n):
            assert run(calls(P, d, dev_xf, mesh=mesh), ctx, WITH_MESH) == {k: INVALID for k in WITH_MESH}, mesh
            # ... the NULL array with it: still PTRT_E_INVALID, whichever check answers
            assert run(calls(P, d, dev_xf, mesh=mesh, null=True), ctx, WITH_MESH) == \
                   {k: INVALID for k in WITH_MESH if k != "ptrt_build_bvh"}, mesh
        # the refused ptrt_build_bvh above marked the first-pass boxes stale all the same
        assert lib.ptrt_get_option(ctx, b"inst_pre_ok", C.byref(opt)) == OK and opt.value == 0
        assert lib.ptrt_refit_tlas(ctx) == OK
        assert lib.ptrt_get_option(ctx, b"inst_pre_ok", C.byref(opt)) == OK and opt.value == 1
        assert lib.ptrt_build_bvh(ctx, n) == INVALID
        assert lib.ptrt_get_option(ctx, b"inst_pre_ok", C.byref(opt)) == OK and opt.value == 0
        # (d) a NULL array
        assert run(calls(P, d, dev_xf, null=True), ctx) == {k: INVALID for k in WITH_ARRAY}
        # counts that are not the upload's
        assert lib.ptrt_update_instances(ctx, d.meshes, n - 1, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == INVALID
        assert lib.ptrt_read_tlas_order(ctx, (C.c_int32 * (d.tlas_index_count + 1))(), d.tlas_index_count + 1) == INVALID
        assert lib.ptrt_read_tlas(ctx, (P.BvhNode * (d.tlas_node_count + 1))(), d.tlas_node_count + 1) == INVALID
        assert lib.ptrt_read_bvh(ctx, 0, (P.BvhNode * (d.meshes[0].node_count + 1))(), d.meshes[0].node_count + 1) == INVALID
        assert b"ptrt_read_bvh" in lib.ptrt_last_error(ctx)
        assert lib.ptrt_update_vertices(ctx, 0, np.zeros(3, np.float32).ctypes.data_as(C.POINTER(C.c_float)), d.meshes[0].vert_count + 1, 0) == INVALID
        assert lib.ptrt_set_instance_transforms(ctx, 0, n + 1, (P.InstanceXform * 1)()) == INVALID
        assert lib.ptrt_set_instance_transforms(ctx, n, 0, (P.InstanceXform * 1)()) == OK       # an empty range at the end is in order
        assert lib.ptrt_set_instance_transforms_device(ctx, n, 0, dev_xf) == OK
        # none of the refused calls was an upload, and the scene is still there
        out = (C.c_int * 2)()
        assert lib.ptrt_debug_upload_counts(ctx, out) == OK and tuple(out) == (1, 0)
        good = run(calls(P, d, dev_xf), ctx)
        assert {k: good[k] for k in ("ptrt_refit", "ptrt_refit_tlas", "ptrt_reorder_tlas", "ptrt_read_tlas", "ptrt_read_tlas_order",
                                     "ptrt_update_instances", "ptrt_set_instance_transforms", "ptrt_update_vertices", "ptrt_read_bvh")} == \
               {k: OK for k in ("ptrt_refit", "ptrt_refit_tlas", "ptrt_reorder_tlas", "ptrt_read_tlas", "ptrt_read_tlas_order",
                                "ptrt_update_instances", "ptrt_set_instance_transforms", "ptrt_update_vertices", "ptrt_read_bvh")}
        assert lib.ptrt_sync(ctx) == OK
    finally:
        lib.ptrt_destroy(ctx)


def test_a_failed_geometry_upload_leaves_the_context_not_ready(P, desc):
    _, d = desc
    lib = P.lib
    n = d.mesh_count
    # the scene again with one face of its last mesh referencing a vertex out of range
    meshes = (P.MeshDesc * n)()
    for m in range(n):
        C.memmove(C.byref(meshes[m]), C.byref(d.meshes[m]), C.sizeof(P.MeshDesc))
    last = meshes[n - 1]
    faces = (P.Tri * last.face_count)()
    C.memmove(faces, last.faces, C.sizeof(faces))
    faces[last.face_count - 1].v2 = last.vert_count
    last.faces = C.cast(faces, C.POINTER(P.Tri))
    rgb = np.zeros(16 * 16 * 3, np.uint8)
    ctx = create(P)
    try:
        assert lib.ptrt_upload_materials(ctx, C.byref(d.materials)) == OK
        assert lib.ptrt_reset_rng(ctx, 1) == OK
        assert lib.ptrt_upload_geometry(ctx, meshes, n, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == INVALID
        assert b"out of range" in lib.ptrt_last_error(ctx)
        assert lib.ptrt_render(ctx, 0, 1, 1, rgb.ctypes.data, 0) == NOT_READY
        assert b"geometry" in lib.ptrt_last_error(ctx)
        assert lib.ptrt_refit(ctx) == NOT_READY
        # the same arrays with the face mended: the context renders
        assert lib.ptrt_upload_geometry(ctx, d.meshes, n, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == OK
        assert lib.ptrt_render(ctx, 0, 1, 1, rgb.ctypes.data, 0) == OK
        # ... and goes on rendering the scene it has when a later upload is refused before anything was freed
        assert lib.ptrt_upload_geometry(ctx, meshes, n, d.tlas_nodes, d.tlas_node_count, d.tlas_mesh_indices, d.tlas_index_count) == INVALID
        assert lib.ptrt_render(ctx, 1, 1, 1, rgb.ctypes.data, 0) == OK
        assert lib.ptrt_sync(ctx) == OK
        out = (C.c_int * 2)()
        assert lib.ptrt_debug_upload_counts(ctx, out) == OK and tuple(out) == (1, 0)
    finally:
        lib.ptrt_destroy(ctx)
