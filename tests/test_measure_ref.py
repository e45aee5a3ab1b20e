"""CPU-only: the restatement tests/measure_ref.py proved on closed forms, so that holding the kernels to it (tests/test_gpu_measure.py)
holds them to the geometry.

  * half-spaces a . x <= c in a box, 1-D to 6-D, against the inclusion-exclusion formula: the interpolant of an affine function is
    the function, so the only error is rounding;
  * balls in 2-D and 3-D: second-order convergence where counting nodes is first order;
  * integer identities: a full grid is exactly cells D! 2^52, a periodic axis measures the full period, a plane through nodes, one cell;
  * the enclosed area / volume of the mesh tests/surface_ref.py extracts from the same interpolant (levelsetpy_amd.level_set_measure);
  * the cases of tests/test_gpu_measure.py have full, empty and cut cells.
"""
import math

import numpy as np
import pytest

import measure_ref as R
import surface_ref as S

HALF_GRIDS = [(7,), (5, 4), (4, 3, 5), (3, 4, 3, 3), (3, 2, 3, 2, 3), (3, 2, 3, 2, 2, 3)]


def box_field(N, fn, lo=-1.0, hi=1.0):
    vs = [np.linspace(lo, hi, n) for n in N]
    dx = [(hi - lo) / (n - 1) for n in N]
    return fn(*np.meshgrid(*vs, indexing="ij")), dx


def volume(data, dx, level=0.0, periodic=()):
    r = R.measure_ref(data, level, periodic)
    return R.volume_of(r["Q"], data.ndim, R.cell_volume(dx)), r


@pytest.mark.parametrize("N", HALF_GRIDS, ids=lambda N: "x".join(map(str, N)))
def test_a_half_space_in_a_box_has_its_closed_form_volume(N):
    """Bound 1e-13 relative (the recursion is cancellation-free: a few roundings per simplex, and sums of integers).  Measured over the
    12 planes per grid below, largest relative error: (7,) 2.4e-16; (5, 4) 4.3e-16; (4, 3, 5) 6.8e-16; (3, 4, 3, 3) 1.3e-15;
    (3, 2, 3, 2, 3) 1.5e-15; (3, 2, 3, 2, 2, 3) 3.5e-15 (the closed form's own alternating sum of 2^D powers is part of that)."""
    D = len(N)
    rng = np.random.default_rng(100 + D)
    worst = 0.0
    for trial in range(12):
        a = rng.uniform(0.3, 1.0, D) * rng.choice([-1.0, 1.0], D)
        c = rng.uniform(-0.4, 0.4)
        phi, dx = box_field(N, lambda *X: sum(a[d] * X[d] for d in range(D)) - c)
        got, r = volume(phi, dx)
        want = R.halfspace_volume(a, c, [-1.0] * D, [1.0] * D)
        assert 0 < want < 2.0 ** D and r["cut"] > 0
        worst = max(worst, abs(got - want) / want)
    print("half-space %s: largest relative error %.2e" % (N, worst))
    assert worst <= 1e-13


@pytest.mark.parametrize("D,sizes", [(2, (11, 21, 41)), (3, (9, 17, 33))], ids=["2d", "3d"])
def test_a_ball_converges_at_second_order(D, sizes):
    """Error ratio per halving of the step between 3.5 and 4.5.  Measured: 2-D 4.04, 4.02 (errors 2.1e-2, 5.3e-3,
    1.3e-3); 3-D 4.02, 4.00 (7.9e-2, 2.0e-2, 4.9e-3)."""
    r0, centre = 0.6, (0.03, -0.02, 0.01)[:D]
    errs = []
    for n in sizes:
        phi, dx = box_field((n,) * D, lambda *X: np.sqrt(sum((X[d] - centre[d]) ** 2 for d in range(D))) - r0)
        got, _ = volume(phi, dx)
        errs.append(abs(got - R.ball_volume(D, r0)))
    ratios = [errs[k] / errs[k + 1] for k in range(2)]
    print("ball %d-D: errors %s ratios %s" % (D, ["%.3e" % e for e in errs], ["%.2f" % q for q in ratios]))
    assert all(3.5 <= q <= 4.5 for q in ratios), ratios


def test_integer_identities():
    # everything inside: exactly cells D! 2^52, and on a periodic axis the full period
    for N, per in R.GRIDS + [((4, 5), (0, 1))]:
        D = len(N)
        r = R.measure_ref(np.full(N, -1.0), 0.0, per)
        assert r["Q"] == r["cells"] * math.factorial(D) * R.Q_ONE == R.cell_count(N, per) * math.factorial(D) * R.Q_ONE
        assert (r["full"], r["cut"], r["invalid"], r["Q_cut"], r["inside"]) == (r["cells"], 0, 0, 0, int(np.prod(N)))
        assert r["lo"] == [0] * D and r["hi"] == [n - 1 for n in N]
        vs, dx, mins, maxs = R.grid_vectors(N, per)
        period = [n * dx[d] if d in per else maxs[d] - mins[d] for d, n in enumerate(N)]
        assert R.volume_of(r["Q"], D, R.cell_volume(dx)) == pytest.approx(math.prod(period), rel=1e-15)
        out = R.measure_ref(np.full(N, 1.0), 0.0, per)
        assert (out["Q"], out["full"], out["cut"], out["inside"], out["lo"], out["hi"]) == (0, 0, 0, 0, list(N), [-1] * D)
    assert R.cell_count((4, 5), (0, 1)) == 20 and R.cell_count((4, 5)) == 12
    # a plane through nodes, x0 <= 0 on 5 nodes per axis: exact zeros at nodes, no cut cell, exactly half the cells
    for D in (1, 2, 3, 4):
        phi, dx = box_field((5,) * D, lambda *X: X[0] + 0.0 * sum(X))
        v, r = volume(phi, dx)
        assert (r["cut"], r["full"]) == (0, 2 * 4 ** (D - 1)) and v == 2.0 ** D / 2
    # a diagonal plane through nodes, x0 + x1 <= 0: cut cells whose simplices are each wholly in or out -- q is 0 or 2^52, never between
    phi, dx = box_field((5, 5), lambda x, y: x + y)
    v, r = volume(phi, dx)
    assert r["cut"] == 4 and r["Q_cut"] == 4 * R.Q_ONE and v == 2.0
    # one cell, (2,)^D, cut through its middle by x0 <= 0: half of it
    for D in range(1, 7):
        phi, dx = box_field((2,) * D, lambda *X: X[0] + 0.0 * sum(X))
        v, r = volume(phi, dx)
        assert (r["cells"], r["cut"]) == (1, 1) and r["Q"] == math.factorial(D) * R.Q_ONE // 2 and v == 2.0 ** D / 2


def test_simplex_q_of_the_small_cases():
    assert R.simplex_q([-1.0, 1.0]) == R.Q_ONE // 2 and R.simplex_q([-1.0, 3.0]) == R.Q_ONE // 4
    assert R.simplex_q([-1.0, 0.0, 1.0]) == R.Q_ONE // 2                       # a zero belongs to neither side
    assert R.simplex_q([0.0, 0.0, -1.0]) == R.Q_ONE and R.simplex_q([0.0, 0.0, 1.0]) == 0 and R.simplex_q([0.0, 0.0]) == R.Q_ONE
    assert R.simplex_q([-1.0, 1.0, 1.0]) == R.Q_ONE // 4 and R.simplex_q([1.0, -1.0, -1.0]) == 3 * R.Q_ONE // 4
    assert R.simplex_q([-1.0, 1.0, 1.0, 1.0]) == R.Q_ONE // 8
    assert [len(R.chains(D)) for D in range(1, 7)] == [1, 2, 6, 24, 120, 720]
    assert R.chains(3)[:2] == [[0, 1, 3, 7], [0, 1, 5, 7]] and R.chains(3) == [c for _, c, _ in S.permutations(3)]


@pytest.mark.parametrize("D", [2, 3])
def test_the_extracted_mesh_encloses_the_same_volume(D):
    """The mesh of tests/surface_ref.py is the boundary of the same piecewise-linear set, so its enclosed area / volume
    (level_set_measure: shoelace / divergence theorem) differs from the measure by rounding alone.  Measured relative difference:
    2-D (23 x 31 ellipse) 1.6e-16, bound ten times that, 1.6e-15; 3-D (17^3 sphere) 0 -- below what two fp64 numbers can differ by,
    so one unit in the last place, 2.2e-16, stands for the measured value and the bound is 2.2e-15."""
    from levelsetpy_amd import level_set_measure
    case = S.ellipse() if D == 2 else S.sphere(17)
    verts, faces = S.extract(case)
    _, enclosed = level_set_measure(verts, faces)
    got, r = volume(np.array(case["phi"]), case["dx"], case["level"])
    rel = abs(got - enclosed) / enclosed
    print("mesh %d-D: measure %.17g enclosed %.17g relative difference %.2e" % (D, got, enclosed, rel))
    assert r["cut"] > 20 and rel <= (1.6e-15 if D == 2 else 2.2e-15)


def test_the_gpu_cases_have_full_empty_and_cut_cells():
    """Seed 20261020: between 1 and 77 cut cells each, all three classes present on every grid but the one-cell one."""
    for N, per in R.GRIDS:
        r = R.measure_ref(R.field(N, per), 0.0, per)
        empty = r["cells"] - r["full"] - r["cut"] - r["invalid"]
        if r["cells"] > 1:
            assert r["full"] > 0 and empty > 0 and 1 <= r["cut"] <= 77 and r["invalid"] == 0, (N, r)
        else:
            assert r["cut"] == 1
    for i in (1, 3, 5):                                            # the second set of the comparisons overlaps the first only partly
        N, per = R.GRIDS[i]
        a, b = R.field(N, per) <= 0, R.field_b(N, per) <= 0
        assert (a & ~b).any() and (b & ~a).any() and (a & b).any()
