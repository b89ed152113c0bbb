"""orthoBasis's two reciprocals go through the Newton core (pt_device.hip.h: rcp_ieee, neg_rcp_ieee) instead of the compiler's
IEEE divisions.  Every kernel that turns a sample into a normal's frame calls it, so it has to be the same function of its input,
bit for bit: neg_rcp_ieee against `-1.0f / y` for all 2^32 inputs, and orthoBasis against its text with the divisions over 2^22
normals -- unit, axis-aligned with zeros of both signs, len2 on both sides of its 1e-20 threshold, NaN and infinite components,
arbitrary bit patterns.  Both checks ride on ptrt_debug_div3_check (modes 4 and 5): the exported names are pinned."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


def _check(P, s, first, count, mode):
    out = (C.c_uint * 9)()
    P.lib.ptrt_debug_div3_check.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint)]
    assert P.lib.ptrt_debug_div3_check(s.ctx, first, count, mode, out) == 0
    return list(out)


def test_negated_reciprocal_is_the_division_for_every_float(P):
    """neg_rcp_ieee(y) == -1.0f / y, compared as bit patterns (a NaN's sign and payload too), for all 2^32 inputs."""
    s = P.Scene(16, 16)
    out = _check(P, s, 0, 1, 4)
    assert out[0] == 0, f"{out[0]} mismatches, first inputs: {[hex(v) for v in out[1:9]]}"
    s.close()


@pytest.mark.parametrize("seed", [0x1234567, 0x9e3779b9])
def test_orthobasis_through_the_newton_core_is_orthobasis(P, seed):
    """T and B of pt::orthoBasis against the same text with `1.0f / sqrt` and `-1.0f / (s + Nn.z)`, bitwise, 2^21 normals per seed
    (2^22 in all).  out[7], out[8]: normals that took the len2 < 1e-20 arm / whose frame holds a NaN -- both classes are met."""
    n = 1 << 21
    s = P.Scene(16, 16)
    out = _check(P, s, seed, n, 5)
    print(f"seed {seed:#x}: {out[0]} mismatches, {out[7]} normals below the threshold, {out[8]} frames with a NaN")
    assert out[0] == 0, f"{out[0]} mismatching normals, first: {[hex(v) for v in out[1:7]]}"
    # class 5 (an eighth of the normals) straddles the threshold: len2 in [0.25e-20, 2.25e-20]; class 6 and part of 7 give NaN
    assert n // 64 < out[7] < n // 4, out[7]
    assert out[8] > n // 16, out[8]
    s.close()


def test_the_hook_still_refuses_an_unknown_mode(P):
    s = P.Scene(16, 16)
    out = (C.c_uint * 9)()
    P.lib.ptrt_debug_div3_check.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint)]
    assert P.lib.ptrt_debug_div3_check(s.ctx, 0, 1, 6, out) == -1
    s.close()
