"""The dynamic LDS of every traversal launch (csrc/lds_layout.h, read back with ptrt_lds_layout; DESIGN.md 2, "LDS layouts").
No device needed.

The device carves and the host's byte counts come from one header.  This test holds that header to three things over a grid of
scene sizes and options, no point skipped:
  * every launch passes the bytes it passed before the header existed: the formulas below are the host formulas of the commit
    before it, written out term by term (bare numbers included: they are the record);
  * the PMODE 1 megakernel stages what it staged and picks the workgroup size it picked (pm1_layout of that commit, restated);
  * the regions are sound: inside the total, pairwise disjoint except for the declared aliases, aligned to what they hold, and
    every alias meets the condition that makes it safe wherever the host would admit the scene."""
import ctypes as C
import itertools

import pytest

MESHES = [1, 2, 8, 9, 42, 43, 255]
TRI_SLOTS = [1, 12, 36, 700]
STACKS = [0, 1, 24, 32]
TLAS_LEAF = [1, 17, 32]
TLAS_DEPTH = [0, 1, 12]
LIGHTS = [0, 1, 8, 9]
FULL = [0, 1]
STAGE = list(range(8))
LDS_PAD = [0, 64, 1280]
PM1_WG = [0, 1, 2]
SAMPLE_SYNC = [0, 1]

LOCKSTEP, PAIR1, PAIR2, PAIR3, PAIR4, PM1, NODES, ASYNC, WAVEFRONT = range(9)

# constants of the kernels (pt_kernels.hip.h, pt_render.hip.h, pt_async.hip.h, pt_wavefront.hip.h at the parent commit)
LEAF_PAIR_BYTES = 512 + 1088
PAIR_PAD, TLAS_SLOTS, TLAS_FILL_TARGET, TOP_NODES, AS_RING, WF_RING, LDS_LIGHTS = 2, 1, 64, 7, 128, 256, 8
WAVES_PER_EU, WAVES_PMODE1, WAVES_PMODE1_WG2, LDS_GRANULE = 4, 5, 6, 1280


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("meshes", "tri_slots", "stack_entries", "tlas_leaf", "tlas_depth", "lights", "full",
                                         "stage", "lds_pad", "pm1_wg", "sample_sync")]


class Region(C.Structure):
    _fields_ = [("id", C.c_int32), ("wave", C.c_int32), ("offset", C.c_int64), ("bytes", C.c_int64), ("align", C.c_int32),
                ("in_first", C.c_int32), ("in_last", C.c_int32)]


class Info(C.Structure):
    _fields_ = [("total", C.c_int64), ("waves", C.c_int32), ("lds_flags", C.c_int32), ("lds_extra", C.c_int32),
                ("lds_wave", C.c_int32), ("lds_wave_bytes", C.c_int32), ("wg", C.c_int32), ("pair_cap", C.c_int32),
                ("pair_cap_lo", C.c_int32), ("pair_cap_hi", C.c_int32), ("max_leaf", C.c_int32)]


MAX_REGIONS = 128


@pytest.fixture(scope="module")
def layout(P):
    P.lib.ptrt_lds_layout.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(Region), C.c_int, C.POINTER(Info)]
    P.lib.ptrt_lds_layout.restype = C.c_int
    P.lib.ptrt_lds_region_name.argtypes = [C.c_int]
    P.lib.ptrt_lds_region_name.restype = C.c_char_p
    names = {}
    i = 0
    while P.lib.ptrt_lds_region_name(i):
        names[i] = P.lib.ptrt_lds_region_name(i).decode()
        i += 1
    regions = (Region * MAX_REGIONS)()

    def run(shape, **kw):
        info = Info()
        n = P.lib.ptrt_lds_layout(shape, C.byref(Params(**kw)), regions, MAX_REGIONS, C.byref(info))
        assert 0 <= n <= MAX_REGIONS, (shape, kw, n)
        return [(names[r.id], r.wave, r.offset, r.bytes, r.align, names.get(r.in_first), names.get(r.in_last)) for r in regions[:n]], info

    return run


# ---- the host formulas of the parent commit (ptrt_render.hip.h) ------------------------------------------------------------
def pm1_pair_bytes(meshes):
    return meshes * 128 if meshes * 128 > 1024 else 1024


def merged_pair_cap(meshes, stack):
    rest = meshes * 32 + 512 + 256 + stack * 64 * 8 + LEAF_PAIR_BYTES + 24
    lo, hi = 64 * meshes + 64, 128 * meshes
    cap = (10240 - rest) // 2 // 64 * 64 if rest < 10240 else 0
    cap = lo if cap < lo else cap
    return hi if cap > hi else cap


def pair_lds_bytes(pmode, meshes, tri_slots, stack, tlas_leaf, tlas_depth):
    if pmode == 4:
        return meshes * 32 + 512 + 256 + merged_pair_cap(meshes, stack) * 2 + stack * 64 * 8 + LEAF_PAIR_BYTES + 24
    if pmode == 3:
        return ((tlas_leaf * 64 + TLAS_FILL_TARGET) * 2 + 512 * TLAS_SLOTS + stack * 64 * 8 + (1 if tlas_depth < 1 else tlas_depth) * 512 +
                256 * TLAS_SLOTS + LEAF_PAIR_BYTES + 24)
    common = meshes * (48 if pmode == 1 else 32) + (pm1_pair_bytes(meshes) if pmode == 1 else meshes * 128) + 512
    if pmode == 1:
        return common + tri_slots * 48 + meshes * PAIR_PAD * 16 + 16
    return common + stack * 64 * 8 + LEAF_PAIR_BYTES + 24


def lds_nodes_bytes(meshes, stack):
    return meshes * (32 + TOP_NODES * 64) + 4 * (512 + meshes * 128 + 256 + stack * 512 + LEAF_PAIR_BYTES)


def wavefront_lds_bytes(stack):
    return 4 * (stack * 64 + WF_RING // 2) * 8


def async_lds_bytes(stack):
    return (stack * 64 + AS_RING // 2) * 8 + LEAF_PAIR_BYTES


def waves_per_simd(pmode, full, wg=1):
    return (WAVES_PMODE1_WG2 if wg == 2 else WAVES_PMODE1) if (pmode == 1 and not full) else WAVES_PER_EU


def lds_per_wave(pmode, full, wg=1):
    return 160 * 1024 // (4 * waves_per_simd(pmode, full, wg)) // LDS_GRANULE * LDS_GRANULE


def lds_per_workgroup(pmode, full, wg):
    return 160 * 1024 // (4 * waves_per_simd(pmode, full, wg) // wg) // LDS_GRANULE * LDS_GRANULE


def pm1_layout(meshes, tri_slots, n_lights, full, stage, lds_pad, pm1_wg, sample_sync):
    """-> (bytes, wg, lds_extra, lds_flags, lds_wave, lds_wave_bytes): pm1_layout of the parent commit"""
    shared0 = tri_slots * 48 + meshes * (PAIR_PAD * 16 + 16 + 32)
    lights, mats = n_lights * 64, meshes * (96 if full else 48)
    stage_bn = sample_sync == 0
    K = [0, 0, 0, 0]

    def layout(wg, budget, may_stage=True):
        wave0 = 512 + pm1_pair_bytes(meshes) + 16
        shared = (shared0 + 15) & ~15
        flags = 0
        if shared + wg * wave0 + lds_pad > budget:
            return 0
        extra_at = shared
        wave = wave0
        if may_stage and stage and shared + 128 + wg * (wave0 + (512 if stage_bn else 0)) + lds_pad <= budget:
            flags = 4 | (8 if stage_bn else 0)
            shared += 128
            wave += 512 if stage_bn else 0
            if (stage & 1) and 0 < n_lights <= LDS_LIGHTS and shared + lights + wg * wave + lds_pad <= budget:
                flags |= 1
                shared += lights
            if (stage & 2) and meshes <= 42 and shared + mats + wg * wave + lds_pad <= budget:
                flags |= 2
                shared += mats
        K[:] = [extra_at, flags, shared, wave]
        return shared + wg * wave + lds_pad

    need, wg = 0, 1
    if not full and pm1_wg != 1:
        need = layout(2, lds_per_workgroup(1, False, 2))
    if need:
        wg = 2
    else:
        need = layout(1, lds_per_wave(1, full))
        if not need:
            need = layout(1, 64 * 1024, False)
    return (need, wg, *K)


# ---- what the regions hold (alignment in bytes) and the checks every layout gets --------------------------------------------
HOLDS = {"tris": 16, "meshtab": 16, "meshbox": 16, "topnodes": 16, "lights": 16, "mats": 16,  # float4 / int4
         "jit": 8, "bn": 8, "best": 8, "stack": 8, "tstack": 8, "lkey": 8, "count": 8, "dirty": 8,  # float2, uint2, 64-bit words
         "pairs": 4, "occ": 4, "leafx": 4, "ring": 4, "limits": 4, "park": 4, "owner": 1, "dense_owner": 1, "tail": 1}


def check_regions(regions, info, what):
    total = info.total
    by = {(name, wave): (off, off + size) for name, wave, off, size, *_ in regions}
    assert len(by) == len(regions), what
    plain = []
    for name, wave, off, size, align, first, last in regions:
        assert size > 0 and 0 <= off and off + size <= total, (what, name, wave, off, size, total)
        assert align >= HOLDS[name] and off % align == 0, (what, name, off, align)
        if first is None:
            plain.append((off, off + size, name, wave))
            continue
        # a declared alias: inside the span of the regions it names (of its own wave, or the workgroup's one copy)
        lo = by.get((first, wave), by.get((first, -1)))
        hi = by.get((last, wave), by.get((last, -1)))
        assert lo and hi and lo[0] <= off and off + size <= hi[1], (what, name, wave, off, size, lo, hi)
        if first != last:  # a span is only a span when its regions touch
            assert by[(first, wave)][1] == by[(last, wave)][0], (what, name)
    plain.sort()
    for a, b in zip(plain, plain[1:]):
        assert a[1] <= b[0], (what, "overlap", a, b)
    for wave in range(-1, info.waves):
        lim, occ, best = by.get(("limits", wave)), by.get(("occ", wave)), by.get(("best", wave))
        if lim and occ:  # the any-hit traversals' two planes: never each other's
            assert lim[1] <= occ[0] or occ[1] <= lim[0], what
        if lim:
            assert lim[1] - lim[0] == 256 and lim[0] == best[0], what
    return by


def one(regions, name):
    hit = [r for r in regions if r[0] == name]
    assert len(hit) == 1, (name, regions)
    return hit[0]


def check_owner_list(by, info, waves, what):
    assert info.max_leaf == 17
    for w in waves:
        lo, hi = by[("owner", w)]
        assert hi - lo >= 64 * info.max_leaf, what  # 64 lanes x the largest leaf the host admits to the compacted leaf phase


def check_dense_owner(by, meshes, waves, what):
    for w in waves:
        pairs, own = by[("pairs", w)], by[("dense_owner", w)]
        assert own[0] >= pairs[0] + 32 * meshes * 2, what  # behind the 32 * M 16-bit entries that R <= 32 rays can make
        assert own[1] - own[0] >= 32 and own[1] <= pairs[1], what


# ---- the shapes -------------------------------------------------------------------------------------------------------------
def test_one_wave_pmode1(layout):
    for meshes, tri_slots in itertools.product(MESHES, TRI_SLOTS):
        what = ("pair1", meshes, tri_slots)
        regions, info = layout(PAIR1, meshes=meshes, tri_slots=tri_slots)
        assert info.total == pair_lds_bytes(1, meshes, tri_slots, 0, 0, 0), what
        by = check_regions(regions, info, what)
        assert by[("pairs", 0)][1] - by[("pairs", 0)][0] == pm1_pair_bytes(meshes) >= 1024, what
        if meshes < 1024 and info.total <= 40 * 1024:
            # the wave's totals: 16 bytes in the pad behind the LAST mesh's packets (mesh i's packets start i pads late, so the
            # packets end at most (meshes - 1) pads behind their place in the arena), inside the triangle region
            count = one(regions, "count")
            assert count[5] == "tris" and count[3] == 16 <= PAIR_PAD * 16, what
            assert count[2] >= tri_slots * 48 + (meshes - 1) * PAIR_PAD * 16 and count[2] + 16 <= by[("tris", -1)][1], what
            check_dense_owner(by, meshes, [0], what)
        assert ("park", 0) not in by, what  # (no lane refill in a query)


@pytest.mark.parametrize("pmode", [2, 4])
def test_one_wave_pmode2_and_4(layout, pmode):
    for meshes, stack in itertools.product(MESHES, STACKS):
        what = (pmode, meshes, stack)
        regions, info = layout(pmode, meshes=meshes, stack_entries=stack)
        assert info.total == pair_lds_bytes(pmode, meshes, 0, stack, 0, 0), what
        by = check_regions(regions, info, what)
        if pmode == 4:
            assert info.pair_cap == merged_pair_cap(meshes, stack), what
            assert (info.pair_cap_lo, info.pair_cap_hi) == (64 * meshes + 64, 128 * meshes), what
            assert by[("pairs", 0)][1] - by[("pairs", 0)][0] == 2 * info.pair_cap, what
            assert one(regions, "occ")[5] is None, what  # both kinds of ray at once: flags of their own
        else:
            assert one(regions, "occ")[5] == "best", what
        if meshes < 256 and info.total <= 40 * 1024:
            check_owner_list(by, info, [0], what)


def test_one_wave_pmode3(layout):
    for stack, leaf, depth in itertools.product(STACKS, TLAS_LEAF, TLAS_DEPTH):
        what = ("pair3", stack, leaf, depth)
        regions, info = layout(PAIR3, stack_entries=stack, tlas_leaf=leaf, tlas_depth=depth, meshes=9)
        assert info.total == pair_lds_bytes(3, 0, 0, stack, leaf, depth), what
        by = check_regions(regions, info, what)
        assert ("meshbox", -1) not in by, what
        assert by[("pairs", 0)][1] - by[("pairs", 0)][0] == 2 * (leaf * 64 + TLAS_FILL_TARGET), what
        if leaf <= 32 and info.total <= 40 * 1024:
            check_owner_list(by, info, [0], what)


def test_pmode1_megakernel(layout):
    seen = set()
    for meshes, tri_slots, lights, full, stage, pad, wg, sync in itertools.product(MESHES, TRI_SLOTS, LIGHTS, FULL, STAGE, LDS_PAD,
                                                                                    PM1_WG, SAMPLE_SYNC):
        what = ("pm1", meshes, tri_slots, lights, full, stage, pad, wg, sync)
        regions, info = layout(PM1, meshes=meshes, tri_slots=tri_slots, lights=lights, full=full, stage=stage, lds_pad=pad, pm1_wg=wg,
                               sample_sync=sync)
        need, want_wg, extra, flags, wave, wave_bytes = pm1_layout(meshes, tri_slots, lights, full, stage, pad, wg, sync)
        assert info.total == need, what
        assert (info.wg, info.lds_extra, info.lds_flags, info.lds_wave, info.lds_wave_bytes) == (want_wg, extra, flags, wave, wave_bytes), what
        if not need:  # over 64 KB with nothing staged: never admitted (pair_mode stops at 40 KB), nothing to lay out
            assert not regions and pair_lds_bytes(1, meshes, tri_slots, 0, 0, 0) > 40 * 1024, what
            continue
        seen.add((want_wg, flags, wg == 2 and want_wg == 1, need > lds_per_wave(1, bool(full))))
        assert info.waves == want_wg, what
        by = check_regions(regions, info, what)
        waves = range(want_wg)
        for w in waves:
            assert by[("best", w)][0] == wave + w * wave_bytes, what
            assert by[("count", w)][1] <= wave + (w + 1) * wave_bytes, what
            assert (("bn", w) in by) == bool(flags & 8), what
        assert (("jit", -1) in by) == bool(flags & 4) and (("lights", -1) in by) == bool(flags & 1), what
        assert (("mats", -1) in by) == bool(flags & 2), what
        if flags & 4:
            assert by[("jit", -1)][0] == extra, what
        if pair_lds_bytes(1, meshes, tri_slots, 0, 0, 0) <= 40 * 1024:
            check_dense_owner(by, meshes, waves, what)
            for w in waves:  # the lane refill's six generator planes across the minima and the pair list
                park = by[("park", w)]
                assert park[1] - park[0] == 6 * 256 <= 512 + pm1_pair_bytes(meshes), what
                assert park[0] == by[("best", w)][0] and park[1] <= by[("pairs", w)][1], what
    # the grid reaches both workgroup sizes, both fallbacks and every staging piece
    assert {s[0] for s in seen} == {1, 2} and any(s[2] for s in seen) and any(s[3] and s[1] == 0 for s in seen)
    assert {f for _, f, _, _ in seen} >= {0, 4, 12, 5, 6, 7, 13, 14, 15}


def test_lds_nodes(layout):
    for meshes, stack in itertools.product(MESHES, STACKS):
        what = ("nodes", meshes, stack)
        regions, info = layout(NODES, meshes=meshes, stack_entries=stack)
        assert info.total == lds_nodes_bytes(meshes, stack) and info.waves == 4, what
        by = check_regions(regions, info, what)
        assert one([r for r in regions if r[1] <= 0], "occ")[5] is None, what
        if info.total <= 64 * 1024:
            check_owner_list(by, info, range(4), what)


def test_lockstep_async_wavefront(layout):
    for stack in STACKS:
        regions, info = layout(LOCKSTEP, stack_entries=stack)
        assert info.total == stack * 64 * 8
        check_regions(regions, info, ("lockstep", stack))
        regions, info = layout(ASYNC, stack_entries=stack)
        assert info.total == async_lds_bytes(stack)
        by = check_regions(regions, info, ("async", stack))
        assert by[("ring", 0)][1] - by[("ring", 0)][0] == AS_RING * 4
        check_owner_list(by, info, [0], ("async", stack))
        regions, info = layout(WAVEFRONT, stack_entries=stack)
        assert info.total == wavefront_lds_bytes(stack) and info.waves == 4
        by = check_regions(regions, info, ("wavefront", stack))
        assert all(by[("ring", w)][1] - by[("ring", w)][0] == WF_RING * 4 for w in range(4))


def test_bad_arguments(P, layout):
    info = Info()
    assert P.lib.ptrt_lds_layout(PAIR2, None, None, 0, C.byref(info)) == -1
    assert P.lib.ptrt_lds_layout(99, C.byref(Params(meshes=1)), None, 0, C.byref(info)) == -1
    assert P.lib.ptrt_lds_layout(PAIR2, C.byref(Params(meshes=0)), None, 0, C.byref(info)) == -1
    assert P.lib.ptrt_lds_layout(PAIR2, C.byref(Params(meshes=1, stack_entries=-1)), None, 0, C.byref(info)) == -1
    assert P.lib.ptrt_lds_layout(PAIR2, C.byref(Params(meshes=3)), None, 0, C.byref(info)) > 0  # counting only
