"""The split of the one-launch decoder backward (psvo_common.h bwd_split_na,
through psvo_debug_bwd_split): of G workgroups the first nA take the
composited samples' (class A's) 16-sample units, the others the loss-only
samples' (class B's).  No GPU: the function is host code too, the same
integers the kernel and the slab sum compute.

The model (rebuilt here on its own): a class split evenly over n workgroups
runs R = ceil(ceil(units / n) / 4) rounds; class A finishes at R_A · a, class B
at R_B · b + b0."""

import pytest

COST = (75, 35, 16)  # kBwdSplitCost: per-round a, b and class B's pre-loop b0


@pytest.fixture(scope="module")
def split():
    from psvo import _lib as L
    lib = L.lib()
    assert lib.psvo_debug_set_bwd_split(0, 0, 0) == 0  # the built-in constants
    yield lambda ua, ub, g: lib.psvo_debug_bwd_split(ua, ub, g)
    lib.psvo_debug_set_bwd_split(0, 0, 0)


def rounds(units, n):
    return -(-(-(-units // n)) // 4)  # ceil(ceil(units / n) / 4) in integers


def finish(ua, ub, g, na, cost=COST):
    a, b, b0 = cost
    return rounds(ua, na) * a, rounds(ub, g - na) * b + b0


def shares(units, n):
    return [(units * w // n, units * (w + 1) // n) for w in range(n)]


def check(split, ua, ub, g, cost=COST):
    na = split(ua, ub, g)
    nb = g - na
    a, b, b0 = cost
    assert 0 <= na <= g
    if ua == 0:
        assert na == 0  # an empty class gets no workgroup
        return na
    if ub == 0:
        assert na == g
        return na
    if g == 1:
        assert na == g  # no split of one workgroup: the host launches twice
        return na
    assert na >= 1 and nb >= 1
    # every unit of either class in exactly one workgroup's [u0, u1)
    for units, n in ((ua, na), (ub, nb)):
        sh = shares(units, n)
        assert sh[0][0] == 0 and sh[-1][1] == units
        assert all(s[1] == t[0] for s, t in zip(sh, sh[1:])) and all(s[0] <= s[1] for s in sh)
        assert max(s[1] - s[0] for s in sh) == -(-units // n)  # what `rounds` assumes of the largest share
    # against the best alternative with uniform shares, i.e. every other nA: no
    # workgroup finishes more than a round of its own class later — and the
    # bisection in fact finds the model's minimum itself.  (Both classes one
    # after the other over all G workgroups can model better on a grid of a
    # few workgroups — 1 + 40 units on 2: 366 against 266 — but the host, which
    # chooses the schedule, does not know the counts.)
    ta, tb = finish(ua, ub, g, na, cost)
    best = min(max(finish(ua, ub, g, n, cost)) for n in range(1, g))
    assert ta <= best + a and tb <= best + b, (ua, ub, g, na, ta, tb, best)
    assert max(ta, tb) == best
    return na


def test_exhaustive_small_range(split):
    for g in range(1, 10):
        for ua in range(41):
            for ub in range(41):
                check(split, ua, ub, g)


@pytest.mark.parametrize("n", [1, 3, 64, 1000, 2750, 7875, 200000])
def test_one_class_empty(split, n):
    assert check(split, 0, n, 256) == 0
    assert check(split, n, 0, 256) == 256


def test_flagship_mix(split):
    """7,875 + 2,750 units on 256 workgroups: 9 class-A rounds on 219
    workgroups (675 k cycles) beside 19 class-B rounds on 37 (681 k) — two
    launches are 8 + 3 rounds (721 k in this model)."""
    na = check(split, 7875, 2750, 256)
    assert na == 219
    assert (rounds(7875, na), rounds(2750, 256 - na)) == (9, 19)
    assert finish(7875, 2750, 256, na) == (675, 681)


@pytest.mark.parametrize("ua,ub,g", [(7875, 2750, 255), (7875, 2750, 304), (1, 1, 256), (1, 100000, 256),
                                     (100000, 1, 256), (5, 3, 2), (123457, 54321, 256), (40000000, 30000000, 256)])
def test_spot_values(split, ua, ub, g):
    check(split, ua, ub, g)


def test_cost_setter_moves_the_split():
    from psvo import _lib as L
    lib = L.lib()
    try:
        base = lib.psvo_debug_bwd_split(7875, 2750, 256)
        assert lib.psvo_debug_set_bwd_split(75, 70, 16) == 0  # class B twice as dear: it gets more workgroups
        dear = lib.psvo_debug_bwd_split(7875, 2750, 256)
        assert dear < base
        assert max(finish(7875, 2750, 256, dear, (75, 70, 16))) == min(
            max(finish(7875, 2750, 256, n, (75, 70, 16))) for n in range(1, 256))
        assert lib.psvo_debug_set_bwd_split(0, 35, 16) != 0  # refused, the model stays
        assert lib.psvo_debug_bwd_split(7875, 2750, 256) == dear
    finally:
        lib.psvo_debug_set_bwd_split(0, 0, 0)
    assert lib.psvo_debug_bwd_split(7875, 2750, 256) == base
    assert lib.psvo_debug_bwd_split(-1, 0, 256) == -1 and lib.psvo_debug_bwd_split(1, 1, 0) == -1
