"""Value-function queries on the device (levelsetpy_amd/query.py, libhj_query.so) against tests/query_ref.py, against the
host loop hji_solver._eval_point, against computeGradients + eval_u, against NumPy, against the reference's own eval_u
(tests/golden/query.npz) -- and guarded-buffer runs and a census of the new library's kernels.

Grids are the smallest on which the kernels can go wrong, and non-cubic so that a swapped axis shows: 2-D 7x6, 3-D 7x6x9,
4-D 5x6x4x7, with periodic sets none, {0}, {last}, {1,2}, all.  The state sets (query_ref.state_set) hold exact nodes, the
first and last node of extrapolated axes, points in the first and the last cell (ghost stencils), points outside (NaN), points
several periods away and points in the wrap cell.

PINNED to the reference: test_eval_u_golden_on_the_device.  Everything else is UNPINNED (the reference returns one value for
many states, raises on periodic axes >= 1 and for every proj; it has no costate query) and is held to the restatement.

Kernel -> test that launches it (each test asserts the name through hjq_last_kernel; test_census_of_the_query_library checks
the table against `nm -D libhj_query.so`):
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import eval_u, eval_costate, proj  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _ffi, _marshal, _qffi, query  # noqa: E402
from levelsetpy_amd.hji_solver import _eval_point  # noqa: E402
from levelsetpy_amd.opt_traj import find_earliest_BRS_ind  # noqa: E402

import query_ref as Q  # noqa: E402
from guarded_pool import GuardedPool, run_case  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query.npz")
EPS = 2.0 ** -52
TD = {"float64": torch.float64, "float32": torch.float32}
CT = {"float64": "double", "float32": "float"}
MS = (1, 63, 64, 65, 1000)
SCHEMES = {"ENO2": (L.upwindFirstENO2, 0), "ENO3": (L.upwindFirstENO3, 1), "WENO5_ASSHIPPED": (L.upwindFirstWENO5, 3)}

# kernel (as hjq_last_kernel names it) -> the test that launches it and asserts that name
CENSUS = {
    "interp_points_kernel<double>": "test_eval_u_bitwise",
    "interp_points_kernel<float>": "test_eval_u_bitwise",
    "costate_points_kernel<double, 0>": "test_eval_costate_is_gradients_then_eval_u",
    "costate_points_kernel<double, 1>": "test_eval_costate_is_gradients_then_eval_u",
    "costate_points_kernel<double, 3>": "test_eval_costate_is_gradients_then_eval_u",
    "costate_points_kernel<float, 0>": "test_eval_costate_is_gradients_then_eval_u",
    "costate_points_kernel<float, 1>": "test_eval_costate_is_gradients_then_eval_u",
    "costate_points_kernel<float, 3>": "test_eval_costate_is_gradients_then_eval_u",
    "project_minmax_kernel<double, false>": "test_proj_minmax_bitwise",
    "project_minmax_kernel<double, true>": "test_proj_minmax_bitwise",
    "project_minmax_kernel<float, false>": "test_proj_minmax_bitwise",
    "project_minmax_kernel<float, true>": "test_proj_minmax_bitwise",
}
__doc__ += "\n".join("  %-40s %s" % kv for kv in sorted(CENSUS.items())) + "\n"


def launched(kernel, test):
    """The calling thread's last launch ran `kernel`, and the census credits it to `test`."""
    assert _qffi.last_kernel() == kernel, (_qffi.last_kernel(), kernel)
    assert CENSUS[kernel] == test


def dev(a, dtype="float64"):
    return torch.as_tensor(np.array(a), device="cuda").to(TD[dtype])        # (a copy: the shared cases are read-only)


def same(a, b):
    """Bit for bit, NaN equal to NaN (whatever its payload)."""
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def smooth(g, seed, noise=0.05):
    """A bent distance-like function plus noise: finite, no two stencil values tie."""
    rng = np.random.default_rng(seed)
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in g.vs], indexing='ij')
    r = np.sqrt(sum((x - 0.1 * d) ** 2 for d, x in enumerate(xs))) - 0.9
    return r + 0.2 * np.sin(2 * xs[0]) * np.cos(xs[-1]) + noise * rng.standard_normal(r.shape)


_REFS = {}


def case(nd, pd):
    """(grid, oracle grid, N(0,1) data, smooth data, 1000 states, eval_u_ref of both): computed once, never modified."""
    key = (nd, pd)
    if key not in _REFS:
        g, og = Q.make_grids(Q.SHAPES[nd], pd)
        data = np.random.default_rng(nd * 10 + len(pd)).standard_normal(Q.SHAPES[nd])
        xs = Q.state_set(g, 1000)
        for a in (data, xs):
            a.setflags(write=False)
        _REFS[key] = (g, og, data, xs, Q.eval_u_ref(g, data, xs))
    return _REFS[key]


# ------------------------------------------------------------------------------------------ 1. eval_u
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nd", [2, 3, 4])
def test_eval_u_bitwise(nd, dtype):
    """fp64: bit for bit eval_u_ref and the host loop _eval_point; fp32: within one fp32 ulp of max|data| of the fp64
    restatement on the fp32-rounded data (the sum is carried in fp64 and rounded once); NaN positions identical."""
    for pd in Q.periodic_sets(nd):
        g, og, data, xs, ref = case(nd, pd)
        d_t = dev(data, dtype)
        if dtype == "float32":
            ref = Q.eval_u_ref(g, data.astype(np.float32), xs)
        for M in MS:
            x = xs[:M] if M > 1 else xs[-1:]
            r = ref[:M] if M > 1 else ref[-1:]
            got = eval_u(g, d_t, dev(x))
            launched("interp_points_kernel<%s>" % CT[dtype], "test_eval_u_bitwise")
            assert torch.is_tensor(got) and got.is_cuda and got.dtype == TD[dtype] and tuple(got.shape) == (M,)
            got = got.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(r)), (pd, M)
            ok = ~np.isnan(r)
            if dtype == "float64":
                assert np.array_equal(got[ok], r[ok]), (pd, M, np.max(np.abs(got[ok] - r[ok])))
            else:
                ulp = float(np.spacing(np.float32(np.max(np.abs(data)))))
                err = np.max(np.abs(got[ok].astype(np.float64) - r[ok])) if ok.any() else 0.0
                print("fp32 eval_u nd=%d pd=%s M=%d: err %.3e, one ulp of max|data| %.3e" % (nd, pd, M, err, ulp))
                assert err <= ulp, (pd, M, err, ulp)
        if not all(Q.periodic_axes(g)):
            assert np.isnan(ref).any()
        if dtype == "float64":
            host = np.array([_eval_point(g, data, x) for x in xs[:120]])          # NumPy data: the Python loop
            assert same(eval_u(g, d_t, dev(xs[:120])), host), pd
            assert _eval_point(g, d_t, xs[70]) == host[70] or np.isnan(host[70])  # a device tensor: through the kernel
            # NumPy in -> NumPy out, all M values
            out = eval_u(g, data, xs[:65])
            assert isinstance(out, np.ndarray) and same(out, ref[:65])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_eval_u_call_forms_stacks_and_strides(dtype):
    g, og, data, xs, ref = case(3, (1, 2))
    if dtype == "float32":
        data = data.astype(np.float32).astype(np.float64)
    x65 = dev(xs[:65])
    one = eval_u(g, dev(data, dtype), x65)
    stack = np.stack([data, 2 * data - 1, data[::-1].copy()])
    # a time-first stack, many states: (T, M), each row the array's own result
    got = eval_u(g, dev(stack, dtype), x65)
    assert tuple(got.shape) == (3, 65) and same(got[0], one)
    assert same(got[2], eval_u(g, dev(stack[2], dtype), x65))
    # option 2: a list / a stack and ONE state -> one value per array
    v2 = eval_u(g, [dev(a, dtype) for a in stack], xs[5])
    assert tuple(v2.shape) == (3,) and same(v2, got[:, 5])
    assert same(eval_u(g, dev(stack, dtype), dev(xs[5])), got[:, 5])
    # option 3: lists of grids, arrays and states
    g2, _, data2, xs2, ref2 = case(2, (0,))
    v3 = eval_u([g, g2], [stack[1], data2], [xs[7], xs2[9]])
    assert isinstance(v3, np.ndarray) and v3.shape == (2,)
    assert v3[1] == ref2[9] and v3[0] == Q.eval_u_ref(g, stack[1], xs[7:8])[0]
    # a transposed (non-contiguous) array is made contiguous, never read with its base's strides
    base = dev(np.ascontiguousarray(data.transpose(2, 0, 1)), dtype)
    view = base.permute(1, 2, 0)
    assert not view.is_contiguous() and tuple(view.shape) == Q.SHAPES[3]
    assert same(eval_u(g, view, x65), one)
    # states as columns are transposed (the column count is not g.dim); the caller's states are not modified
    xt = dev(xs[:65].T.copy())
    keep = xt.clone()
    assert same(eval_u(g, dev(data, dtype), xt), one) and torch.equal(xt, keep)
    assert same(eval_u(g, dev(data, dtype), xt.T), one)          # a non-contiguous view of the states


def test_eval_u_golden_on_the_device():
    """PINNED: the unmodified reference's eval_u, every case it ran (non-periodic grids; axis 0 periodic, also in the wrap
    cell), within (2^D + D + 2) eps max|data| -- 2^D weighted terms summed in another order."""
    G = dict(np.load(GOLDEN))
    n = 0
    for name, nd in (("g2", 2), ("g3", 3), ("g4", 4)):
        data = G[name + "_data"]
        bound = (2 ** nd + nd + 2) * EPS * float(np.max(np.abs(data)))
        for pd in Q.periodic_sets(nd):
            key = "%s_p%s" % (name, "".join(str(d) for d in pd) or "none")
            ok = ~G[key + "_raised"]
            if not ok.any():
                continue                                            # the reference raised: unpinned
            g, og = Q.make_grids(Q.SHAPES[nd], pd)
            got = eval_u(g, dev(data), dev(G[key + "_xs"])).cpu().numpy()
            err = np.max(np.abs(got[ok] - G[key + "_vals"][ok]))
            assert err <= bound, (key, err, bound)
            n += int(ok.sum())
    assert n >= 60


# ------------------------------------------------------------------------------------------ 2. eval_costate
def gradients_then_eval_u(g, d_t, x_t, fn):
    dC, dL, dR = L.computeGradients(g, d_t, derivFunc=fn)
    return [torch.stack([eval_u(g, a[d], x_t) for d in range(g.dim)], dim=-1) for a in (dC, dL, dR)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("nd", [2, 3, 4])
def test_eval_costate_is_gradients_then_eval_u(nd, scheme, dtype):
    """BIT FOR BIT eval_u applied to computeGradients' derivC arrays of the same data (the same upwind<> source, the same
    interpolation), for every M; in fp64 also against costate_ref (the oracle's derivatives) at the tolerance of
    test_compute_gradients_vs_oracle: 1e-11 max(1, max|ref|)."""
    fn, sid = SCHEMES[scheme]
    kernel = "costate_points_kernel<%s, %d>" % (CT[dtype], sid)
    for pd in Q.periodic_sets(nd):
        g, og, _, xs, _ = case(nd, pd)
        data = smooth(g, 7 + nd)
        d_t, x_t = dev(data, dtype), dev(xs)
        expC, expL, expR = gradients_then_eval_u(g, d_t, x_t, fn)
        for M in MS:
            sl = slice(0, M) if M > 1 else slice(999, 1000)
            got = eval_costate(g, d_t, x_t[sl], fn)
            launched(kernel, "test_eval_costate_is_gradients_then_eval_u")
            assert tuple(got.shape) == (M, nd) and got.dtype == TD[dtype]
            assert same(got, expC[sl]), (pd, M, float((got - expC[sl]).abs().nan_to_num().max()))
        # the one-sided values and V itself from the same gather
        cs, dl, dr, val = query.costate_states(g, d_t, x_t, sid, want_lr=True, want_value=True)
        assert same(cs[0], expC) and same(dl[0], expL) and same(dr[0], expR) and same(val[0], eval_u(g, d_t, x_t))
        if dtype == "float64":
            ref = Q.costate_ref(og, data, xs, scheme)
            got = eval_costate(g, data, xs, fn)                          # NumPy in -> NumPy out
            assert isinstance(got, np.ndarray) and same(got, expC)
            ok = ~np.isnan(ref)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            scale = max(1.0, float(np.max(np.abs(ref[ok]))))
            err = float(np.max(np.abs(got[ok] - ref[ok])))
            assert err <= 1e-11 * scale, (pd, err, scale)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_eval_costate_fallbacks_stack_dims_and_nonfinite(dtype):
    g, og, _, xs, _ = case(3, (2,))
    data = smooth(g, 21)
    d_t, x_t = dev(data, dtype), dev(xs[:200])
    # the intended WENO5 (grid-wide epsilon) and a foreign derivative function take computeGradients, then the interpolation kernel
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    for fn in (L.upwindFirstWENO5Intended, foreign):
        got = eval_costate(g, d_t, x_t, fn)
        assert _qffi.last_kernel() == "interp_points_kernel<%s>" % CT[dtype]
        assert same(got, gradients_then_eval_u(g, d_t, x_t, fn)[0])
    assert same(eval_costate(g, d_t, x_t, foreign), eval_costate(g, d_t, x_t, L.upwindFirstENO3))
    # derivFunc defaults to upwindFirstWENO5; a dims mask leaves NaN columns; a time-first stack is its arrays one by one
    dflt = eval_costate(g, d_t, x_t)
    assert same(dflt, eval_costate(g, d_t, x_t, L.upwindFirstWENO5))
    part = eval_costate(g, d_t, x_t, dims=[1, 0, 1])
    assert same(part[:, [0, 2]], dflt[:, [0, 2]]) and bool(torch.isnan(part[:, 1]).all())
    stack = torch.stack([d_t, 2 * d_t + 1])
    st = eval_costate(g, stack, x_t)
    assert tuple(st.shape) == (2, 200, 3) and same(st[0], dflt) and same(st[1], eval_costate(g, stack[1].clone(), x_t))
    # an inf block and a NaN in the data: as computeGradients (1e6 in the neighbours' stencils, NaN / inf at the node), then eval_u
    bad = data.copy()
    bad[2:4, 1:3, 4:7] = np.inf
    bad[5, 4, 1] = np.nan
    bad[0, 0, 8] = -np.inf
    b_t = dev(bad, dtype)
    for fn in (L.upwindFirstENO2, L.upwindFirstENO3, L.upwindFirstWENO5):
        got = eval_costate(g, b_t, dev(xs), fn)
        exp = gradients_then_eval_u(g, b_t, dev(xs), fn)[0]
        assert same(got, exp), fn.__name__
        assert bool(torch.isinf(got).any()) and bool(torch.isnan(got).any()) and bool(torch.isfinite(got).any())


# ------------------------------------------------------------------------------------------ 3. proj
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nd", [3, 4])
def test_proj_minmax_bitwise(nd, dtype):
    """'min' / 'max' bit for bit NumPy's: every non-empty proper subset of removed axes in 3-D, a sample in 4-D; a NaN in a
    reduced set gives NaN; the time-first stack equals per-time calls."""
    g, og, data, _, _ = case(nd, (nd - 1,))
    npdt = np.float32 if dtype == "float32" else np.float64
    data = data.astype(npdt)
    d_t = dev(data, dtype)
    masks = range(1, (1 << nd) - 1) if nd == 3 else (0b0001, 0b1000, 0b0110, 0b1010, 0b0111, 0b1110, 0b1011)
    for mask in masks:
        rem = [(mask >> d) & 1 for d in range(nd)]
        axes = tuple(d for d in range(nd) if rem[d])
        for op, red in (('min', np.amin), ('max', np.amax)):
            gOut, out = proj(g, d_t, rem, op)
            launched("project_minmax_kernel<%s, %s>" % (CT[dtype], "true" if rem[-1] else "false"), "test_proj_minmax_bitwise")
            assert torch.is_tensor(out) and out.dtype == TD[dtype]
            assert same(out, red(data, axis=axes)), (rem, op)
            assert gOut.dim == nd - len(axes) and [int(n) for n in np.ravel(gOut.N)] == [Q.SHAPES[nd][d] for d in range(nd) if not rem[d]]
            assert [f.__name__ for f in gOut.bdry] == [g.bdry[d].__name__ for d in range(nd) if not rem[d]]
            assert np.array_equal(np.ravel(gOut.min), np.ravel(g.min)[[d for d in range(nd) if not rem[d]]])
    assert same(proj(g, d_t, [1] + [0] * (nd - 1))[1], np.amin(data, axis=0))          # xs defaults to 'min'
    bad = data.copy()
    bad[(1,) * nd] = np.nan
    for rem in ([0] * (nd - 1) + [1], [1] + [0] * (nd - 1)):
        for op, red in (('min', np.amin), ('max', np.amax)):
            out = proj(g, dev(bad, dtype), rem, op)[1]
            assert same(out, red(bad, axis=rem.index(1))) and int(torch.isnan(out).sum()) == 1
    stack = np.stack([data, -data, bad])
    for rem in ([0] * (nd - 1) + [1], [1, 1] + [0] * (nd - 2)):
        out = proj(g, dev(stack, dtype), rem, 'max')[1]
        for t in range(3):
            assert same(out[t], proj(g, dev(stack[t], dtype), rem, 'max')[1])
    gOut, out = proj(g, data.astype(np.float64), [0] * (nd - 1) + [1], 'min')           # NumPy in -> NumPy out
    assert isinstance(out, np.ndarray) and same(out, np.amin(data.astype(np.float64), axis=nd - 1))


def test_proj_slices_and_resampling_bitwise():
    """Slices and NOut resampling in fp64: bit for bit proj_ref (UNPINNED: the reference's proj raises)."""
    for nd, pd in ((3, (2,)), (3, ()), (4, (0, 3))):
        g, og, data, _, _ = case(nd, pd)
        vs = [np.asarray(v).ravel() for v in g.vs]
        dx = np.asarray(g.dx).ravel()
        d_t = dev(data)
        stack = np.stack([data, data ** 2])
        for mask in ((0b100, 0b001, 0b101, 0b110) if nd == 3 else (0b1000, 0b1001, 0b0110)):
            rem = [(mask >> d) & 1 for d in range(nd)]
            gone = [d for d in range(nd) if rem[d]]
            for kind in ("node", "between", "far"):
                pt = [{"node": vs[d][2], "between": vs[d][1] + 0.37 * dx[d],
                       "far": vs[d][1] + 0.37 * dx[d] + (5 * Q.SHAPES[nd][d] * dx[d] if d in pd else 0.0)}[kind] for d in gone]
                gOut, out = proj(g, d_t, rem, pt)
                assert same(out, Q.proj_ref(g, data, rem, pt)), (pd, rem, kind)
                assert list(out.shape) == [int(n) for n in np.ravel(gOut.N)] == [Q.SHAPES[nd][d] for d in range(nd) if not rem[d]]
            pt = [vs[d][1] + 0.6 * dx[d] for d in gone]
            assert same(proj(g, dev(stack), rem, pt)[1], Q.proj_ref(g, stack, rem, pt))          # time first
            nk = nd - len(gone)
            NOut = [11, 4, 9][:nk]
            gOut, out = proj(g, d_t, rem, pt, NOut=NOut)
            assert tuple(out.shape) == tuple(NOut) and same(out, Q.proj_ref(g, data, rem, pt, NOut=NOut))
            assert [int(n) for n in np.ravel(gOut.N)] == NOut
            assert same(proj(g, d_t, rem, 'min', NOut=NOut)[1], Q.proj_ref(g, data, rem, 'min', NOut=NOut))
            assert same(proj(g, dev(stack), rem, 'max', NOut=5)[1], Q.proj_ref(g, stack, rem, 'max', NOut=5))
        gOut, out = proj(g, d_t, [0] * (nd - 1) + [1], [float(vs[-1][0])], process=False)
        assert not hasattr(gOut, "vs") and same(out, Q.proj_ref(g, data, [0] * (nd - 1) + [1], [float(vs[-1][0])]))


# ------------------------------------------------------------------------------------------ 4. computeOptTraj, stopInit
class _Plant(object):
    """xddot = u, |u| <= 1 (the dynSys protocol of computeOptTraj)."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)

    def get_opt_u(self, t, deriv, uMode, x):
        s = np.sign(deriv[1]) if deriv[1] != 0 else 1.0
        return -s if uMode == 'min' else s

    def update_state(self, u, dt, x, d=None):
        k = lambda z: np.array([z[1], u])                                   # noqa: E731
        k1 = k(x); k2 = k(x + .5 * dt * k1); k3 = k(x + .5 * dt * k2); k4 = k(x + dt * k3)
        self.x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        return self.x


def parent_opt_traj(g, data, tau, plant, subSamples):
    """The algorithm computeOptTraj had before the query kernels: host bisection over _eval_point, computeGradients over the
    whole grid, the costate from D more _eval_point calls -- all interpolation in the Python loop on NumPy arrays."""
    host = data.cpu().numpy() if torch.is_tensor(data) else np.asarray(data)

    def earliest(x, upper, lower):
        while upper > lower:
            mid = (upper + lower + 1) // 2
            if _eval_point(g, host[mid], x) < 1e-4:
                lower = mid
            else:
                upper = mid - 1
        return upper
    n = len(tau)
    dt = (tau[1] - tau[0]) / subSamples
    traj = np.full((g.dim, n), np.nan)
    traj[:, 0] = plant.x
    tE, it = 0, 0
    while it < n - 1:
        tE = earliest(np.asarray(plant.x).ravel(), n - 1, tE)
        if tE == n - 1:
            break
        Deriv, _, _ = L.computeGradients(g, data[tE])
        Deriv = [a.cpu().numpy() if torch.is_tensor(a) else a for a in Deriv]
        for _ in range(subSamples):
            x = np.asarray(plant.x, dtype=np.float64).ravel()
            deriv = [_eval_point(g, Deriv[d], x) for d in range(g.dim)]
            plant.update_state(plant.get_opt_u(tau[tE], deriv, 'min', x), dt, x, None)
        it += 1
        traj[:, it] = plant.x
    return traj[:, :it + 1], tau[:it + 1]


_SOLVE = {}


def double_integrator_solve():
    if not _SOLVE:
        n = 41
        g = L.createGrid(np.array([[-1.], [-1.]]), np.array([[1.], [1.]]), np.array([[n], [n]]), None)
        data0 = L.shapeSphere(g, np.zeros((2, 1)), .15)
        sys_ = L.DoubleIntegrator(g, 1)
        sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationGLF,
                           derivFunc=L.upwindFirstENO3))
        tau = np.linspace(0, 1.0, 21)
        data, _, _ = L.HJIPDE_solve(data0, tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, flipOutput=True)))
        _SOLVE.update(g=g, sd=sd, tau=tau, data=np.asarray(data), data0=data0)
    return _SOLVE


@pytest.mark.parametrize("where", ["numpy", "device", "device32"])
def test_compute_opt_traj_equals_the_parent_algorithm(where):
    """The trajectory and the returned tau, bit for bit, against a restatement of the parent's algorithm."""
    S = double_integrator_solve()
    g, tau = S["g"], S["tau"]
    data = {"numpy": lambda: S["data"], "device": lambda: dev(S["data"]), "device32": lambda: dev(S["data"], "float32")}[where]()
    pa, pb = _Plant([0.25, 0.05]), _Plant([0.25, 0.05])
    traj, ttau = L.computeOptTraj(g, data, tau, pa, L.Bundle(dict(uMode='min', subSamples=4)))
    rtraj, rtau = parent_opt_traj(g, data, tau, pb, 4)
    assert traj.shape == rtraj.shape and traj.shape[1] >= 5, (traj.shape, rtraj.shape)
    assert np.array_equal(ttau, rtau) and np.array_equal(traj, rtraj), float(np.max(np.abs(traj - rtraj)))
    # the bisection over one launch picks the index the host bisection picks, also on non-monotone data
    jumble = S["data"][np.random.default_rng(5).permutation(len(tau))]
    for x in ([0.4, 0.05], [0.1, -0.2], [0.9, 0.9], [2.0, 0.0]):
        want = find_earliest_BRS_ind(g, jumble, np.array(x))
        assert find_earliest_BRS_ind(g, dev(jumble), np.array(x)) == want
        assert find_earliest_BRS_ind(g, dev(jumble), np.array(x), 17, 3) == find_earliest_BRS_ind(g, jumble, np.array(x), 17, 3)


def test_stop_init_stops_at_the_step_of_the_host_evaluation():
    S = double_integrator_solve()
    g, sd, tau = S["g"], S["sd"], S["tau"]
    full, _, _ = L.HJIPDE_solve(S["data0"], tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True)))
    full = np.asarray(full)
    x = np.array([0.2, -0.1])
    vals = [_eval_point(g, full[i], x) for i in range(len(tau))]              # NumPy side: the Python loop
    assert vals[0] > 0 and vals[-1] < 0
    first = next(i for i, v in enumerate(vals) if v <= 0)
    d, t, out = L.HJIPDE_solve(S["data0"], tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, stopInit=x)))
    assert out.stoptau == tau[first] and len(t) == first + 1
    assert np.array_equal(np.asarray(d), full[:first + 1])
    for i in (first - 1, first):
        assert _eval_point(g, dev(full[i]), x) == vals[i]                     # device side: one launch, the same bits


# ------------------------------------------------------------------------------------------ 5. bounds
_POOLS = {}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", 400 * 1000)
    return _POOLS[dtype]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nd", [2, 3, 4])
def test_kernels_stay_inside_their_arrays(nd, dtype):
    """The three kernels on views carved from tests/guarded_pool.py's pool, at element offsets 0-3 and with guards of NaN and
    +-1e30: guards intact, inputs unchanged, every output element written, the same bits as on fresh arrays."""
    lib = _qffi.lib()
    pd = (nd - 1,)
    g, og, _, xs, _ = case(nd, pd)
    desc, N = _marshal.descriptor(g, dtype)
    stack = torch.stack([dev(smooth(g, 3), dtype), dev(smooth(g, 4), dtype)])
    M = 130
    x_t = dev(xs[:M])
    P = pool(dtype)

    def states(alloc):
        # the states are fp64 whatever the pool's dtype: guarded on the fp64 pool, plain otherwise
        return alloc.inp("xs", x_t).view if dtype == "float64" else x_t

    def interp(alloc):
        a = alloc.inp("data", stack)
        x = states(alloc)
        o = alloc.out("out", (2, M))
        alloc.arm()
        _qffi.check(lib.hjq_interp_points(C.byref(desc), a.ptr, 2, stack[0].numel(), C.c_void_p(x.data_ptr()), M, o.ptr, 0, _stream()))
        return {"kernel": _qffi.last_kernel()}

    def costate(sid):
        def op(alloc):
            a = alloc.inp("data", stack)
            x = states(alloc)
            outs = [alloc.out(k, (2, M, nd)) for k in ("costate", "derivL", "derivR")]
            v = alloc.out("value", (2, M))
            alloc.arm()
            _qffi.check(lib.hjq_costate_points(C.byref(desc), sid, a.ptr, 2, stack[0].numel(), C.c_void_p(x.data_ptr()), M,
                                               outs[0].ptr, outs[1].ptr, outs[2].ptr, v.ptr, 0, _stream()))
            return {"kernel": _qffi.last_kernel()}
        return op

    def project(mask, op_id):
        keep = tuple(n for d, n in enumerate(N) if not (mask >> d) & 1)

        def op(alloc):
            a = alloc.inp("data", stack)
            o = alloc.out("out", (2,) + keep)
            alloc.arm()
            _qffi.check(lib.hjq_project_minmax(C.byref(desc), a.ptr, 2, stack[0].numel(), mask, op_id, o.ptr, _stream()))
            return {"kernel": _qffi.last_kernel()}
        return op

    ref, _ = run_case(interp, P, what="interp")
    assert ref["kernel"] == "interp_points_kernel<%s>" % CT[dtype]
    for sid in (0, 1, 3):
        ref, _ = run_case(costate(sid), P, what="costate %d" % sid)
        assert ref["kernel"] == "costate_points_kernel<%s, %d>" % (CT[dtype], sid)
    for mask in (1 << (nd - 1), 1, (1 << nd) - 2):
        ref, _ = run_case(project(mask, mask & 1), P, what="project %#x" % mask)
        assert ref["kernel"] == "project_minmax_kernel<%s, %s>" % (CT[dtype], "true" if mask >> (nd - 1) else "false")


def test_entry_points_refuse_bad_arguments():
    lib = _qffi.lib()
    g, og, data, xs, _ = case(3, ())
    desc, N = _marshal.descriptor(g, "float64")
    d_t, x_t, o = dev(data), dev(xs[:4]), torch.empty(12, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.hjq_costate_points(C.byref(desc), _ffi.WENO5, p(d_t), 1, d_t.numel(), p(x_t), 4, p(o), None, None, None, 0, None) == -3
    assert b"scheme" in lib.hjq_last_error()
    with pytest.raises(_ffi.Unsupported):
        query.costate_states(g, d_t, x_t, _ffi.WENO5)
    assert lib.hjq_interp_points(C.byref(desc), None, 1, d_t.numel(), p(x_t), 4, p(o), 0, None) == -1
    assert lib.hjq_interp_points(C.byref(desc), p(d_t), 2, 5, p(x_t), 4, p(o), 0, None) == -1        # stride below the grid
    assert lib.hjq_project_minmax(C.byref(desc), p(d_t), 1, d_t.numel(), 0, 0, p(o), None) == -1
    assert lib.hjq_project_minmax(C.byref(desc), p(d_t), 1, d_t.numel(), 7, 0, p(o), None) == -1
    with pytest.raises(ValueError):
        eval_u(g, dev(data[:-1]), x_t)
    with pytest.raises(ValueError):
        eval_u(g, d_t, dev(xs[:4, :2]))


# ------------------------------------------------------------------------------------------ 6. census
def test_census_of_the_query_library():
    """Every __device_stub__ of `nm -D libhj_query.so` is in CENSUS, and every entry names a test of this file that asserts
    the launch through hjq_last_kernel (the `launched(kernel, test)` calls)."""
    out = subprocess.check_output(["nm", "-D", "-C", _qffi.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+<[^>]*>)\(", out))
    assert stubs, "no kernels found in %s" % _qffi.LIB_PATH
    assert stubs == set(CENSUS), (sorted(stubs - set(CENSUS)), sorted(set(CENSUS) - stubs))
    src = open(os.path.abspath(__file__)).read()
    for kernel, test in CENSUS.items():
        fn = globals().get(test)
        assert callable(fn), test
        body = src[src.index("def %s(" % test):]
        body = body[:body.index("\n\n\n")]
        assert 'launched(' in body and '"%s"' % test in body, test
