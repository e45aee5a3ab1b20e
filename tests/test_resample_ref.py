"""The NumPy restatement of the resampling rule (tests/resample_ref.py) proved on closed forms -- no device.  The maps are the
front end's own (levelsetpy_amd.resample.shiftMap / rotateMap: host arithmetic), so what is proved here is what
tests/test_gpu_resample.py then holds the kernels to, bit for bit."""
import numpy as np
import pytest

import resample_ref as R
from levelsetpy_amd import resample as M

EPS = np.finfo(np.float64).eps


def _mesh(g):
    return np.meshgrid(*g.vs, indexing='ij')


@pytest.mark.parametrize("src,dst", [((9, 8), (12, 7)), ((13, 11, 9), (9, 12, 10)), ((7, 6, 8, 5, 9), (6, 7, 5, 6, 8))])
def test_affine_function_migrates_exactly(src, dst):
    """Multilinear interpolation reproduces c0 + c . x.  Bound: 4 eps times the magnitude |c0| + sum |c_d| max |x_d| the terms
    reach (a weight carries about eps |x| / dx of rounding, which the slope c dx turns into eps |c x|; the sums add the like).
    Measured 0.56, 0.89 and 1.50 eps of that magnitude at 2-D, 3-D and 5-D."""
    D = len(src)
    smin, smax, dmin, dmax = R.pair_bounds(src, ())
    gO, gN = R.RefGrid(smin, smax, src), R.RefGrid(dmin, dmax, dst)
    c, c0 = np.array([0.7, -1.3, 0.45, 2.1, -0.6])[:D], 0.25

    def f(xs):
        return c0 + sum(c[d] * xs[d] for d in range(D))
    out, counts = R.resample_ref(gO, f(_mesh(gO)), gN, fill='nan')
    inside = ~np.isnan(out)
    assert counts == inside.sum() and 0.1 < inside.mean() < 0.9
    scale = abs(c0) + sum(abs(c[d]) * max(abs(smin[d]), abs(smax[d])) for d in range(D))
    err = np.abs(out - f(_mesh(gN)))[inside].max()
    print("affine %d-D: %.2f eps" % (D, err / (EPS * scale)))
    assert err <= 4 * EPS * scale


@pytest.mark.parametrize("nodes", [1, 3, -2, 8, 11])
def test_whole_node_shift_along_a_periodic_axis_is_roll(nodes):
    """Dyadic coordinates (dx = 0.25) keep every operation exact: the weights are exactly 0, one corner is read."""
    g = R.RefGrid([-1.0, -1.0], [0.75, 1.0], [8, 9], pd=(0,))
    data = R.field(g, 3)
    A, b = M.shiftMap(g, [nodes * 0.25], (0,))
    out, counts = R.resample_ref(g, data, g, A, b, fill='nan')
    assert counts == data.size
    assert np.array_equal(out, np.roll(data, nodes, axis=0))


def test_rotation_there_and_back_is_second_order():
    """A Gaussian bump (sigma 0.5) on [-2, 2]^2 rotated by 0.4 and back, compared where |x| < 1.2 (both images stay inside the
    grid there).  One multilinear interpolation errs by at most dx^2 / 8 times the sum over the axes of max |f_dd| = 1 / sigma^2,
    and interpolation does not amplify the first pass's error: the bound of two passes is dx^2 / (2 sigma^2).
    Measured: 1.550e-02 at 41 nodes per axis (bound 2.0e-02), 4.164e-03 at 81 (bound 5.0e-03), ratio 3.72; second order is 4."""
    errs = []
    for n in (41, 81):
        g = R.RefGrid([-2, -2], [2, 2], [n, n])
        X = _mesh(g)
        f = np.exp(-(X[0] ** 2 + X[1] ** 2) / (2 * 0.5 ** 2))
        A, b = M.rotateMap(g, 0.4, (0, 1))
        there, _ = R.resample_ref(g, f, g, A, b, fill=0.0)
        A, b = M.rotateMap(g, -0.4, (0, 1))
        back, _ = R.resample_ref(g, there, g, A, b, fill=0.0)
        err = np.abs(back - f)[X[0] ** 2 + X[1] ** 2 < 1.2 ** 2].max()
        print("rotation there and back, %d nodes: %.3e" % (n, err))
        assert err <= g.dx[0] ** 2 / (2 * 0.5 ** 2)
        errs.append(err)
    assert 3.0 < errs[0] / errs[1] < 5.0


@pytest.mark.parametrize("reduce", ['min', 'max'])
def test_fold_is_the_masked_reduction_of_the_stack(reduce):
    gO, gN = R.ref_pair(1)
    data = R.field(gO, 5)
    rng = np.random.default_rng(7)
    K = 6
    A = np.stack([M.rotateMap(gO, t, (0, 1), 2)[0] for t in rng.uniform(-1, 1, K)])
    b = rng.uniform(-0.4, 0.4, (K, 3))
    v, inside, batched, stacked = R.members_ref(gO, data, gN, A, b)
    assert batched and not stacked and inside.any(axis=0).mean() > 0.1 and (~inside.any(axis=0)).mean() > 0.1
    assert (inside.sum(axis=0) > 1).any()
    neutral = np.inf if reduce == 'min' else -np.inf
    op = np.minimum if reduce == 'min' else np.maximum
    want = op.reduce(np.where(inside, v[:, 0, :], neutral), axis=0)
    want[~inside.any(axis=0)] = np.nan
    out, counts = R.resample_ref(gO, data, gN, A, b, reduce=reduce, fill='nan')
    assert np.array_equal(out.ravel(), want, equal_nan=True)
    assert counts == inside.any(axis=0).sum()
    stack, each = R.resample_ref(gO, data, gN, A, b, fill='nan')
    assert stack.shape == (K,) + R.shape_of(gN) and np.array_equal(each, inside.sum(axis=1))


def test_fill_max_takes_the_largest_transferred_value_and_skips_nan():
    gO, gN = R.ref_pair(0)
    data = R.field(gO, 2)
    data[3, 4] = np.nan
    data[5, 2] = -np.inf
    out, counts = R.resample_ref(gO, data, gN, fill='max')
    plain, same = R.resample_ref(gO, data, gN, fill='nan')
    inside = R.members_ref(gO, data, gN)[1][0].reshape(out.shape)
    assert counts == same == inside.sum() and np.isnan(plain[inside]).any()           # a stored NaN is inside, and counted
    top = np.nanmax(plain[inside])
    assert np.isfinite(top) and np.all(out[~inside] == top)
    assert np.array_equal(out[inside], plain[inside], equal_nan=True)
    nothing, zero = R.resample_ref(gO, data, gN, b=np.array([100.0, 0.0]), fill='max')
    assert zero == 0 and np.isnan(nothing).all()


@pytest.mark.parametrize("pair", range(5))
def test_shared_cases_fill_and_leave_at_least_a_tenth(pair):
    """What tests/test_gpu_resample.py relies on: with every map of maps_for, every two-grid pair has nodes on both sides
    (the identity gives 14 % at 6-D to 65 % at 3-D; the 1-D pair 84 %).  The (2, 2, 2, 2, 2) grid onto itself cannot: the
    identity fills all of it."""
    gO, gN = R.ref_pair(pair)
    for name, (A, b) in R.maps_for(gO.dim, gO).items():
        out, counts = R.resample_ref(gO, R.field(gO, pair), gN, A, b, fill='nan')
        assert 0.1 <= counts / out.size <= 0.9, (name, counts / out.size)
