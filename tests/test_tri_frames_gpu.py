"""ptrt_set_option "tri_frames" (DESIGN.md 3.27): PMODE 1's megakernel reads the tangent frame of to_world from a per-triangle
table written with the packets' normals instead of calling orthoBasis at every vertex.  The table holds what orthoBasis returns
for gn and for -gn, so with the option at 0 and at 1 every buffer, the generator states and the ray counts must be equal to each
other and to the oracle's, bit for bit: over axis-aligned normals (zero components of both signs), over BACK faces (the record
of -gn), over every material class (GGX and cosine lobes both go through to_world), with an instanced mesh in the scene (the
table is not read: tri_frames_eff 0), and across a device refit, which writes new normals and no frames, and the upload after it.
24 x 16: ragged tiles."""
import ctypes as C

import numpy as np
import pytest

from common import assert_frames_equal, bits, render_both

pytestmark = pytest.mark.gpu

SIZE, SPP = (24, 16), 2
BUFFERS = ("accum", "normal", "depth", "object_id", "rgb8", "rng")


def _cornell(P, s):
    P.scenes.cornell(s)


def _back_faces(P, s):
    """The camera inside a closed cube whose normals point outwards: every wall is seen from behind.  In the room a quad whose
    normal points away from the camera, and a small cube seen from its front for the light to bounce between both kinds."""
    room = s.addCube(P.Material(albedo=(0.7, 0.6, 0.5), roughness=0.6))
    s.scale(room, (8.0, 6.0, 8.0))
    s.moveTo(room, (0, 0, -2))
    a, b, c, d = (-1.5, -1.0, -4.0), (1.0, -1.0, -4.5), (1.0, 1.5, -4.5), (-1.5, 1.5, -4.0)
    s.addTriangles([a + c + b, a + d + c], P.Material(albedo=(0.2, 0.5, 0.8), roughness=0.3))  # wound clockwise from the camera
    box = s.addCube(P.Material(albedo=(0.9, 0.9, 0.9), roughness=0.15, metallic=1.0))
    s.scale(box, (0.8, 0.8, 0.8))
    s.moveTo(box, (1.6, -1.2, -3.0))
    s.rotateSelfEulerXYZ(box, (0.2, 0.5, 0.1))
    s.addPointLight((0.0, 2.2, -2.0), (1.0, 0.95, 0.9), 4.0, 30.0)
    s.addPointLight((-2.0, -1.0, -1.0), (0.6, 0.7, 1.0), 2.0, 30.0, 0.3)
    s.setCamera((0.2, 0.1, 1.0), (0, 0, -4), (0, 1, 0), 55.0)
    s.disableSky()


def _material_matrix(P, s):
    P.scenes.material_matrix(s)


def _cornell_short_box_instanced(P, s):
    P.scenes.cornell(s)
    short = 7  # (the last slab of scenes.cornell)
    s.setPosition(short, (0.4, 0.0, 0.3))
    s.setRotation(short, (0.0, 0.5, 0.1))


def _gpu_frames(P, s, depth):
    """The GPU half of common.render_both: same calls, same order."""
    s.setPerfSamplesPerPixel(SPP)
    s.setMaxBounceDepth(depth)
    s.setDenoiserEnabled(False)
    s.setBloomEnabled(False)
    s.initBlueNoise()
    s.uploadToGPU()
    s.reset_rng(P.DEFAULT_SEED)
    s.set_option("count_rays", 1)
    rgb = s.render_to_host()
    return [dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
                 object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats())]


_oracle = {}  # (scene builder, depth) -> the oracle's frame: computed once, shared by the cases, never written to


def _both_settings(P, O, blue_noise, make, depth, opts, eff, back_faces=False):
    """`eff`: tri_frames_eff expected with the option at 1 (at 0 it is 0)"""
    got = {}
    for setting in (0, 1):
        s = P.Scene(*SIZE)
        make(P, s)
        for k, v in opts.items():
            s.set_option(k, v)
        s.set_option("tri_frames", setting)
        if (make, depth) not in _oracle:
            got[setting], _oracle[(make, depth)] = render_both(P, O, s, blue_noise, SPP, depth, 1)
        else:
            got[setting] = _gpu_frames(P, s, depth)
        assert s.get_option("pmode") == 1 and s.get_option("render_mode") == 0, (s.get_option("pmode"), s.get_option("render_mode"))
        assert s.get_option("tri_frames_eff") == (eff if setting else 0), (setting, s.get_option("tri_frames_eff"))
        if "refill" in opts:
            assert s.get_option("refilled") == (1 if opts["refill"] else 0)
        s.close()
    cpu = _oracle[(make, depth)]
    assert cpu[0]["accum"].any(), "the frame is black: nothing is tested"
    if back_faces:  # the first hits are back faces: the oracle's normals point against the geometric ones, towards the camera
        seen = cpu[0]["object_id"] >= 0
        assert seen.mean() > 0.95
    for setting in (0, 1):
        assert_frames_equal(got[setting], cpu)
    a, b = got[0][0], got[1][0]
    assert a["stats"] == b["stats"], f"ray counts {a['stats']} vs {b['stats']}"
    for k in BUFFERS:
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{k} differs between tri_frames 0 and 1"


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("refill", [0, 2])
def test_cornell(P, O, blue_noise, refill, depth):
    _both_settings(P, O, blue_noise, _cornell, depth, dict(refill=refill), eff=1)


@pytest.mark.parametrize("depth", [3, 4])
def test_back_faces(P, O, blue_noise, depth):
    _both_settings(P, O, blue_noise, _back_faces, depth, {}, eff=1, back_faces=True)


@pytest.mark.parametrize("depth", [3, 4])
def test_every_material_class(P, O, blue_noise, depth):
    _both_settings(P, O, blue_noise, _material_matrix, depth, {}, eff=1)


@pytest.mark.parametrize("depth", [3, 4])
def test_an_instanced_mesh_keeps_orthobasis(P, O, blue_noise, depth):
    _both_settings(P, O, blue_noise, _cornell_short_box_instanced, depth, {}, eff=0)


def _frame_and_oracle(P, O, s, blue_noise, depth):
    s.setFrameCount(0)
    s.reset_rng(P.DEFAULT_SEED)
    s.stats()  # (read and cleared)
    rng = O.xorwow_init(P.DEFAULT_SEED, 0, SIZE[0] * SIZE[1])
    rgb = s.render_to_host()
    g = dict(accum=s.read(P.BUF_ACCUM), normal=s.read(P.BUF_NORMAL), depth=s.read(P.BUF_DEPTH),
             object_id=s.read(P.BUF_OBJECT_ID), rgb8=rgb, rng=s.read(P.BUF_RNG), stats=s.stats())
    c = O.render(s.flatten(), SIZE[0], SIZE[1], SPP, depth, 0, blue_noise, rng, threads=8)
    c["rgb8"] = O.tonemap(c["accum"], SIZE[0], SIZE[1], threads=8)
    c["rng"] = rng.copy()
    return [g], [c]


def _verts(s, mesh):
    m = s.flatten().contents.meshes[mesh]
    return np.ctypeslib.as_array(C.cast(m.verts, C.POINTER(C.c_float)), (m.vert_count, 3)).copy()


@pytest.mark.parametrize("depth", [3, 4])
def test_a_refit_turns_it_off_until_the_next_upload(P, O, blue_noise, depth):
    """ptrt_refit writes new normals into the packets and no frames: the frame after it must not read the table."""
    from test_tlas_refit_gpu import upload_counts
    s = P.Scene(*SIZE)
    P.scenes.cornell(s)
    gpu, cpu = render_both(P, O, s, blue_noise, SPP, depth, 1)
    assert_frames_equal(gpu, cpu)
    assert s.get_option("pmode") == 1 and s.get_option("tri_frames_eff") == 1
    tall = 6  # the tall box: sheared, so that every one of its normals turns
    v = _verts(s, tall)
    moved = v.copy()
    moved[:, 0] += np.float32(0.25) * (v[:, 1] - v[:, 1].min())
    moved[:, 2] += np.float32(0.1) * (v[:, 1] - v[:, 1].min())
    s.setVertices(tall, moved)
    s.refitObjectChanges()
    gpu, cpu2 = _frame_and_oracle(P, O, s, blue_noise, depth)
    assert s.get_option("tri_frames_eff") == 0, "the device wrote new normals: the frames are the old ones"
    assert_frames_equal(gpu, cpu2)
    assert not np.array_equal(cpu2[0]["normal"], cpu[0]["normal"]), "no normal of the frame moved"
    s.set_option("tri_frames", 1)  # (1 does not force it)
    s.render_to_host()
    assert s.get_option("tri_frames_eff") == 0
    # the same positions through a full upload, which writes the table again
    uploads = upload_counts(P, s)[0]
    s.setVertices(tall, moved)
    s.commitObjectChanges()
    assert upload_counts(P, s)[0] == uploads + 1
    gpu, cpu3 = _frame_and_oracle(P, O, s, blue_noise, depth)
    assert s.get_option("tri_frames_eff") == 1
    assert_frames_equal(gpu, cpu3)
    s.close()


def _entry_points(P, s):
    """name -> thunk for every entry point that must clear the flag, each with arguments under which nothing moves"""
    import torch
    lib, ctx = P.lib, s.ctx
    d = s.flatten().contents
    lib.ptrt_update_instances.restype = C.c_int
    lib.ptrt_update_instances.argtypes = [C.c_void_p, C.POINTER(P.MeshDesc), C.c_int, C.POINTER(P.BvhNode), C.c_int, C.POINTER(C.c_int32), C.c_int]
    one = np.zeros(49, np.float32)  # ptrt_instance_xform: world, inverse, normal = identity; has_transform = 0
    one[[0, 5, 10, 15, 16, 21, 26, 31, 32, 37, 42, 47]] = 1.0
    xf = torch.from_numpy(one.reshape(1, 49)).cuda()
    pose = torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1, 1]], dtype=torch.float32).cuda()
    return {
        "ptrt_refit": lambda: lib.ptrt_refit(ctx),
        "ptrt_build_bvh": lambda: lib.ptrt_build_bvh(ctx, 0),
        "ptrt_refit_tlas": lambda: lib.ptrt_refit_tlas(ctx),
        "ptrt_reorder_tlas": lambda: lib.ptrt_reorder_tlas(ctx),
        "ptrt_update_instances": lambda: lib.ptrt_update_instances(ctx, d.meshes, d.mesh_count, d.tlas_nodes, d.tlas_node_count,
                                                                   d.tlas_mesh_indices, d.tlas_index_count),
        "ptrt_set_instance_transforms_device": lambda: lib.ptrt_set_instance_transforms_device(ctx, 0, 1, C.c_void_p(xf.data_ptr())),
        "ptrt_set_instance_poses_device": lambda: lib.ptrt_set_instance_poses_device(ctx, 0, 1, C.c_void_p(pose.data_ptr())),
        "_keep": (xf, pose),
    }


def test_the_flag_follows_the_upload_and_every_entry_point_clears_it(P):
    """The derivation -- on after an upload of a scene without transforms, off with one -- and each entry point that lets the
    device change a normal or a transform behind the host: off from the next frame, on again after the next upload.  Through
    tri_frames_eff (the flag has no device-free query); the frames of a scene in which nothing moved stay the first frame's."""
    import torch
    from test_tlas_refit_gpu import upload_counts
    s = P.Scene(*SIZE)
    P.scenes.cornell(s)
    v0 = _verts(s, 0)
    first = _gpu_frames(P, s, 4)[0]
    assert s.get_option("pmode") == 1 and s.get_option("tri_frames_eff") == 1
    table = _entry_points(P, s)
    for name, call in table.items():
        if name == "_keep":
            continue
        torch.cuda.synchronize()
        assert call() == 0, name
        s.setFrameCount(0)
        s.reset_rng(P.DEFAULT_SEED)
        rgb = s.render_to_host()
        assert s.get_option("tri_frames_eff") == 0, f"{name} did not clear the flag"
        # (a pose always marks its mesh an instance -- another path to the same picture -- and a rebuild may re-order a leaf's
        # triangles, which decides ties: the frames of those two are not held to the first one's bits)
        if name not in ("ptrt_set_instance_poses_device", "ptrt_build_bvh"):
            assert np.array_equal(rgb, first["rgb8"]), name
            assert np.array_equal(bits(s.read(P.BUF_ACCUM)), bits(first["accum"])), name
        uploads = upload_counts(P, s)[0]
        s.setVertices(0, v0)  # (the same positions: dirty, so that the commit is a full upload)
        s.commitObjectChanges()
        assert upload_counts(P, s)[0] == uploads + 1
        s.setFrameCount(0)
        s.reset_rng(P.DEFAULT_SEED)
        rgb = s.render_to_host()
        assert s.get_option("tri_frames_eff") == 1, f"the upload after {name} did not derive the flag again"
        assert np.array_equal(rgb, first["rgb8"]) and np.array_equal(bits(s.read(P.BUF_ACCUM)), bits(first["accum"])), name
    s.close()
    # the derivation's other arm: a mesh with a transform at upload time
    s = P.Scene(*SIZE)
    _cornell_short_box_instanced(P, s)
    _gpu_frames(P, s, 4)
    assert s.get_option("pmode") == 1 and s.get_option("tri_frames_eff") == 0
    s.close()
