"""bench_slab's diagnostics: every rank times the same legs in the same order (CPU, no process group).

Each leg ends in one barrier and one all-reduce; ranks that disagree about the list of legs sit in different collectives and the
run hangs.  dist.slab_diagnostic_legs is the list, a pure function of the decomposition."""
import pytest
import torch

from levelsetpy_amd import dist as hjdist
from levelsetpy_amd.dist import HALO, SlabDecomposition, slab_diagnostic_legs

WORLDS = range(1, 9)


def n0_cases(world):
    """24, 65, 513, and an axis that leaves one rank with 7 planes and the others with 6 (fewer than 2*HALO + 1: no interior)."""
    return [n for n in (24, 65, 513, 6 * world + 1) if n // world >= HALO]


def slabs(n0, world, periodic0):
    return [SlabDecomposition(n0, world, r, periodic0, self_exchange=periodic0) for r in range(world)]


def legs_before(slab):
    """{name: [p0, p1]} of the legs the diagnostics ran on this rank before the list became rank-independent."""
    n = slab.n_local
    lo_e = 3 if slab.halo_lo else 0
    hi_b = n - 3 if slab.halo_hi else n
    out = {}
    if hi_b > lo_e:
        out["interior_launch_only"] = [lo_e, hi_b]
    if lo_e > 0:
        out["low_edge_launch_only"] = [0, lo_e]
    if hi_b < n:
        out["high_edge_launch_only"] = [hi_b, n]
    out["whole_slab_launch_only"] = [0, n]
    return out


CASES = [(w, p, n) for w in WORLDS for p in (False, True) for n in n0_cases(w)]


@pytest.mark.parametrize("world,periodic0,n0", CASES)
def test_every_rank_has_the_same_legs_in_the_same_order(world, periodic0, n0):
    names = [[leg[0] for leg in slab_diagnostic_legs(s)] for s in slabs(n0, world, periodic0)]
    assert all(n == names[0] for n in names), names
    assert len(set(names[0])) == len(names[0])
    assert names[0][0] == "interior_launch_only" and names[0][-1] == "whole_slab_launch_only"


@pytest.mark.parametrize("world,periodic0,n0", CASES)
def test_non_empty_ranges_are_the_ranges_of_before(world, periodic0, n0):
    for s in slabs(n0, world, periodic0):
        before = legs_before(s)
        legs = slab_diagnostic_legs(s)
        got = {name: [p0, p1] for name, p0, p1 in legs if p1 > p0}
        assert got == before, (s.rank, legs, before)
        for name, p0, p1 in legs:
            assert 0 <= p0 <= p1 <= s.n_local, (s.rank, name, p0, p1)


@pytest.mark.parametrize("world,periodic0,n0", CASES)
def test_empty_edge_legs_are_on_the_ranks_without_that_halo(world, periodic0, n0):
    for s in slabs(n0, world, periodic0):
        legs = {name: (p0, p1) for name, p0, p1 in slab_diagnostic_legs(s)}
        for name, halo in (("low_edge_launch_only", s.halo_lo), ("high_edge_launch_only", s.halo_hi)):
            if name in legs:
                p0, p1 = legs[name]
                assert (p1 == p0) == (not halo), (s.rank, name, legs[name], halo)
            else:
                assert world == 1 and not s.halo_lo and not s.halo_hi
        p0, p1 = legs["interior_launch_only"]
        assert (p1 == p0) == (s.n_local - HALO * (int(s.halo_lo) + int(s.halo_hi)) <= 0)
        assert legs["whole_slab_launch_only"] == (0, s.n_local)


def test_some_case_has_a_rank_without_interior_beside_one_with():
    """The fourth axis length does what it is there for: an empty interior leg on some ranks only."""
    seen = False
    for world in range(3, 9):
        empty = [dict((n, p1 - p0) for n, p0, p1 in slab_diagnostic_legs(s))["interior_launch_only"] == 0
                 for s in slabs(6 * world + 1, world, True)]
        seen = seen or (any(empty) and not all(empty))
    assert seen


class CountingDist(object):
    """Stands in for torch.distributed: counts the collectives of one rank."""

    class ReduceOp(object):
        MAX = "max"

    def __init__(self):
        self.calls = []

    def barrier(self):
        self.calls.append("barrier")

    def all_reduce(self, tensor, op=None):
        assert op == self.ReduceOp.MAX
        self.calls.append("all_reduce")


@pytest.mark.parametrize("periodic0", [False, True])
@pytest.mark.parametrize("n0", [24, 19])
def test_every_rank_makes_the_same_collectives_at_three_ranks(periodic0, n0):
    world = 3
    calls, launched, results = [], [], []
    for s in slabs(n0, world, periodic0):
        d = CountingDist()
        ran = []

        def timed(fn, d=d):
            return hjdist._timed_collectively(d, torch, "cpu", lambda: None, fn, iters=2)

        def sub(p0, p1, ran=ran):
            return lambda: ran.append((p0, p1))

        results.append(hjdist.run_slab_diagnostic_legs(slab_diagnostic_legs(s), timed, sub, lambda name: {"kernel": "k"}))
        calls.append(d.calls)
        launched.append(ran)
    assert all(c == calls[0] for c in calls), calls
    assert calls[0] == ["barrier", "all_reduce"] * 4
    for s, res, ran in zip(slabs(n0, world, periodic0), results, launched):
        before = legs_before(s)
        assert list(res) == ["interior_launch_only", "low_edge_launch_only", "high_edge_launch_only", "whole_slab_launch_only"]
        for name, entry in res.items():
            assert entry["planes"] == before.get(name, []), (s.rank, name, entry)
            assert set(("this_rank_ms", "max_over_ranks_ms", "min_over_ranks_ms")) <= set(entry)
            assert ("kernel" in entry) == bool(entry["planes"])
        # only the legs with planes launched anything, twice each (iters=2)
        assert ran == [tuple(r) for name in res for r in [before.get(name)] * 2 if r], (s.rank, ran)
    if not periodic0:
        assert results[0]["low_edge_launch_only"]["planes"] == [] and results[2]["high_edge_launch_only"]["planes"] == []
        assert results[1]["low_edge_launch_only"]["planes"] == [0, 3]
