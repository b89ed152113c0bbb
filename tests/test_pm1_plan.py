"""The plan behind ptrt_set_option "pm1_lane_groups" (csrc/pm1_plan.h, read back with ptrt_pm1_plan): for
leaves of L triangles, how a tail of n < 64 pairs is cut into sub-batches of g lanes per pair.  No device needed.

For every L and n: the sub-batches cover exactly n pairs, every g divides L, take * g <= 64, and under the plan's own cost model
the tail costs no more than the present rule's single batch (2^sh lanes per pair, ceil(L / 2^sh) iterations and one header).
One thing has to be said about "every g divides L": where 2^sh does not divide L the present rule runs ceil(L / 2^sh)
iterations of the guarded loop in ONE batch, and for some tails no sequence of divisor sub-batches is as cheap at any
positive header cost (L = 7, n = 10: two iterations and a header against 1 + 1 and two headers; the divisors of 7 are 1 and
7).  Such an entry reads g = 0, the kernel runs the present rule for the pairs that are left, and the test holds it to this:
it appears only where 2^sh does not divide L and where an exhaustive search over divisor sequences finds nothing as cheap
for those pairs.  Leaves of 1, 2, 12 and 16 triangles have no such entry."""
import ctypes as C
import functools

import pytest

LEAVES = [1, 2, 7, 12, 16, 17]
SHIFT = 12


def plan(P, L):
    P.lib.ptrt_pm1_plan.argtypes = [C.c_int] + [C.POINTER(C.c_int32)] * 5
    P.lib.ptrt_pm1_plan.restype = C.c_int
    g, take, mul, cost = ((C.c_int32 * 63)() for _ in range(4))
    model = (C.c_int32 * 2)()
    assert P.lib.ptrt_pm1_plan(L, g, take, mul, cost, model) == 1
    return [0] + list(g), [0] + list(take), [0] + list(mul), [0] + list(cost), tuple(model)


def present(L, n):
    """the present rule's single batch: (shift, iterations)"""
    sh = 0
    while (n << (sh + 1)) <= 64 and (2 << sh) <= L:
        sh += 1
    return sh, (L + (1 << sh) - 1) >> sh


def walk(L, g, take, n):
    """the sub-batches of a tail of n pairs: [(g, take, iterations, lanes per pair, pairs left before it)], following the entries as the kernel's loop does"""
    out = []
    while n > 0:
        if g[n] == 0:
            sh, it = present(L, n)
            out.append((0, n, it, 1 << sh, n))
            n = 0
        else:
            out.append((g[n], take[n], L // g[n], g[n], n))
            n -= take[n]
        assert n >= 0 and len(out) <= 63
    return out


@pytest.mark.parametrize("L", LEAVES)
def test_plan(P, L):
    g, take, mul, cost, (body, header) = plan(P, L)
    assert body > 0 and header > 0
    divisors = [d for d in range(1, min(L, 64) + 1) if L % d == 0]

    @functools.lru_cache(None)
    def best_divisor_cost(n):  # the cheapest sequence of divisor sub-batches, by exhaustive recursion
        if n == 0:
            return 0
        return min((L // d) * body + header + best_divisor_cost(n - min(n, 64 // d)) for d in divisors)

    for n in range(1, 64):
        subs = walk(L, g, take, n)
        assert sum(t for _, t, *_ in subs) == n, (L, n, subs)
        sh, it = present(L, n)
        present_cost = it * body + header
        total = 0
        for gg, t, iters, lanes, left in subs:
            assert t >= 1 and t * lanes <= 64, (L, n, subs)
            if gg:
                assert L % gg == 0 and t == min(left, 64 // gg) and iters * gg == L, (L, n, subs)
            else:  # the present rule's batch for what is left: the last one, and only where nothing made of divisors is as cheap
                lsh, lit = present(L, left)
                assert L % (1 << lsh) != 0 and (gg, t, iters, lanes, left) == subs[-1] == (0, left, lit, 1 << lsh, left), (L, n, subs)
                assert best_divisor_cost(left) > lit * body + header, (L, n, left, best_divisor_cost(left))
            total += iters * body + header
        assert total == cost[n], (L, n, total, cost[n])
        assert total <= present_cost, (L, n, total, present_cost)
        assert total <= best_divisor_cost(n), (L, n, total, best_divisor_cost(n))
        if g[n]:
            assert take[n] == min(n, 64 // g[n])
            assert all((lane * mul[n]) >> SHIFT == lane // g[n] for lane in range(64)), (L, n, g[n], mul[n])
    if L in (1, 2, 12, 16):  # every tail of these leaves has a divisor plan
        assert all(g[n] for n in range(1, 64)), [n for n in range(1, 64) if not g[n]]


def test_cornell_plan_is_the_one_in_the_issue(P):
    """12 triangles: up to 5 pairs at 12 lanes (one iteration), 40 pairs as 32 at 2 lanes + 8 at 6 (6 + 2 iterations)"""
    g, take, *_ = plan(P, 12)
    for n in range(1, 6):
        assert (g[n], take[n]) == (12, n)
    assert walk(12, g, take, 40) == [(2, 32, 6, 2, 40), (6, 8, 2, 6, 8)]
    assert walk(12, g, take, 21) == [(3, 21, 4, 3, 21)]


def test_lane_division_constants_are_exact(P):
    P.lib.ptrt_pm1_div_mul.argtypes = [C.c_int]
    P.lib.ptrt_pm1_div_mul.restype = C.c_int
    for g in range(1, 65):  # (the issue asks for g <= 17; the table may hold up to 64)
        m = P.lib.ptrt_pm1_div_mul(g)
        assert m > 0
        for lane in range(64):
            assert (lane * m) >> SHIFT == lane // g, (g, lane, m)
    assert P.lib.ptrt_pm1_div_mul(0) == 0 and P.lib.ptrt_pm1_div_mul(65) == 0


def test_out_of_range_leaf_keeps_the_present_rule(P):
    P.lib.ptrt_pm1_plan.argtypes = [C.c_int] + [C.POINTER(C.c_int32)] * 5
    P.lib.ptrt_pm1_plan.restype = C.c_int
    g, take = (C.c_int32 * 63)(), (C.c_int32 * 63)()
    assert P.lib.ptrt_pm1_plan(256, g, take, None, None, None) == 0
    assert not any(g) and list(take) == list(range(1, 64))
    assert P.lib.ptrt_pm1_plan(0, g, take, None, None, None) == -1
    assert P.lib.ptrt_pm1_plan(12, None, take, None, None, None) == -1
