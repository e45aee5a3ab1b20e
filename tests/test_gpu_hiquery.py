"""Queries and rollouts on 5-D and 6-D grids (libhj_hiquery.so through levelsetpy_amd/query.py and rollout.py) against the
NumPy restatements tests/query_ref.py and tests/rollout_ref.py, against computeGradients + eval_u, against NumPy's amin / amax,
against the 3-D library on data that does not depend on the trailing axes, against computeOptTraj -- and guarded-buffer runs.

Grids (tests/hidim_cases.py): (7, 6, 8, 5, 9) periodic in axis 2, (6, 5, 7, 5, 6, 8) periodic in axes 2 and 5, and
(5, 5, 6, 5, 70) for the wavefront form of the projection.  Data with noise, so that no ENO choice ties.  States from
query_ref.state_set (nodes, first and last cells, the last node, outside an extrapolated axis, several periods away, the wrap
cell) plus a NaN state.  UNPINNED throughout, as the <= 4-D queries are: the reference has none of this at any dimension.

Tolerances.  eval_u, proj, eval_costate against computeGradients: exact.  eval_costate against the oracle: exact for ENO2 / ENO3,
1e-11 max(1, max|ref|) for the as-shipped WENO5 (the suite's fp64 rule, tests/test_gpu_hidim.py).  Rollout states: 1e-12, the
tolerance of tests/test_gpu_rollout.py where the device's sin / cos enter (its docstring has the derivation).

Kernel -> test that launches it (each asserts the name through hjx_last_kernel; tests/test_hiquery_host.py checks the census
against `nm -D libhj_hiquery.so`):
  hi_interp_points_kernel<T>               test_eval_u_bitwise
  hi_costate_points_kernel<T, ND, SCHEME>  test_eval_costate_is_gradients_then_eval_u
  hi_project_minmax_kernel<T, WAVE>        test_proj_minmax_bitwise
  hi_rollout_kernel<T, SCHEME, PLANT>      test_one_control_step_on_every_plant_and_scheme
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import eval_u, eval_costate, proj, computeOptTraj, computeOptTrajs  # noqa: E402
from levelsetpy_amd import _ffi, _marshal, _qffi, _rffi, query, rollout  # noqa: E402
from levelsetpy_amd import _xffi as X  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd.decomp import sepGrid  # noqa: E402

import hidim_cases as HC  # noqa: E402
import hiquery_cases as XC  # noqa: E402
import query_ref as Q  # noqa: E402
import rollout_ref as R  # noqa: E402
from guarded_pool import GuardedPool, PlainAlloc, run_case  # noqa: E402

TD = {"float64": torch.float64, "float32": torch.float32}
ND = {"float64": np.float64, "float32": np.float32}
SCHEMES = {"ENO2": (L.upwindFirstENO2, 0), "ENO3": (L.upwindFirstENO3, 1), "WENO5_ASSHIPPED": (L.upwindFirstWENO5, 3)}
NAMES = ("plane5d", "pair6d")
MS = (1, 7, 64, 65, 203)                    # 8 (5-D) / 4 (6-D) states fill a workgroup of the costate kernel: 7, 65 and 203 do not
TOL = 1e-12

CENSUS_TEST = {"hi_interp_points_kernel": "test_eval_u_bitwise", "hi_costate_points_kernel": "test_eval_costate_is_gradients_then_eval_u",
               "hi_project_minmax_kernel": "test_proj_minmax_bitwise", "hi_rollout_kernel": "test_one_control_step_on_every_plant_and_scheme"}


def launched(kernel, test):
    """The calling thread's last launch of the library ran `kernel`, and the census credits it to `test`."""
    assert X.last_kernel() == kernel, (X.last_kernel(), kernel)
    assert CENSUS_TEST[kernel.split("<")[0]] == test


def dev(a, dtype="float64"):
    return torch.as_tensor(np.array(a), device="cuda").to(TD[dtype])        # (a copy: the shared cases are read-only)


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    """Bit for bit, NaN equal to NaN (whatever its payload)."""
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


_REFS = {}


def case(name):
    """(grid, oracle grid, noisy data, 203 states with a NaN state among them, eval_u_ref): computed once, never modified."""
    if name not in _REFS:
        g, og = XC.grids(name)
        data = XC.noisy(name)
        xs = Q.state_set(g, 203)
        xs[100, 0] = np.nan                                                 # (an extrapolated axis: no cell holds such a state)
        for a in (data, xs):
            a.setflags(write=False)
        _REFS[name] = (g, og, data, xs, Q.eval_u_ref(g, data, xs))
    return _REFS[name]


# ------------------------------------------------------------------------------------------ 1. eval_u
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_eval_u_bitwise(name, dtype):
    """fp64: bit for bit eval_u_ref; fp32: within one fp32 ulp of max|data| of the fp64 restatement on the fp32-rounded data
    (the sum is carried in fp64 and rounded once: the rule of tests/test_gpu_query.py); NaN positions identical."""
    g, og, data, xs, ref = case(name)
    d_t = dev(data, dtype)
    if dtype == "float32":
        ref = Q.eval_u_ref(g, data.astype(np.float32), xs)
    assert np.isnan(ref).sum() >= 4 and np.isnan(ref[100])
    for M in MS:
        x = xs[:M] if M > 1 else xs[-1:]
        r = ref[:M] if M > 1 else ref[-1:]
        got = eval_u(g, d_t, dev(x))
        launched(X.interp_kernel_name(dtype), "test_eval_u_bitwise")
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == TD[dtype] and tuple(got.shape) == (M,)
        got = got.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(r)), M
        ok = ~np.isnan(r)
        if dtype == "float64":
            assert np.array_equal(got[ok], r[ok]), (M, np.max(np.abs(got[ok] - r[ok])))
        else:
            ulp = float(np.spacing(np.float32(np.max(np.abs(data)))))
            err = np.max(np.abs(got[ok].astype(np.float64) - r[ok])) if ok.any() else 0.0
            print("fp32 eval_u %s M=%d: err %.3e, one ulp of max|data| %.3e" % (name, M, err, ulp))
            assert err <= ulp, (M, err, ulp)
    if dtype == "float64":
        out = eval_u(g, data, xs[:65])                                       # NumPy in -> NumPy out, all M values
        assert isinstance(out, np.ndarray) and same(out, ref[:65])
        view = eval_u(g, L.lazy.HostView(d_t), xs[:65])                      # a HostView in -> a tensor out
        assert torch.is_tensor(view) and view.is_cuda and same(view, ref[:65])
        from levelsetpy_amd.hji_solver import _eval_point
        assert _eval_point(g, d_t, xs[70]) == ref[70] == _eval_point(g, data, xs[70])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_eval_u_call_forms_and_stacks(name, dtype):
    g, og, data, xs, _ = case(name)
    if dtype == "float32":
        data = data.astype(np.float32).astype(np.float64)
    x65 = dev(xs[:65])
    one = eval_u(g, dev(data, dtype), x65)
    stack = np.stack([data, 2 * data - 1, data[::-1].copy()])
    ref = Q.eval_u_ref(g, stack, xs[:65])
    # a time-first stack, many states: (T, M), each row the array's own result
    got = eval_u(g, dev(stack, dtype), x65)
    assert tuple(got.shape) == (3, 65) and same(got[0], one) and same(got[2], eval_u(g, dev(stack[2], dtype), x65))
    if dtype == "float64":
        assert same(got, ref)
    # option 2: a list / a stack and ONE state -> one value per array
    v2 = eval_u(g, [dev(a, dtype) for a in stack], xs[5])
    assert tuple(v2.shape) == (3,) and same(v2, got[:, 5]) and same(eval_u(g, dev(stack, dtype), dev(xs[5])), got[:, 5])
    # option 3: lists of grids, arrays and states -- a 5-D / 6-D grid next to a 2-D one
    g2, _ = Q.make_grids(Q.SHAPES[2], (0,))
    d2 = np.random.default_rng(3).standard_normal(Q.SHAPES[2])
    x2 = Q.state_set(g2, 1)[0]
    v3 = eval_u([g, g2], [stack[1], d2], [xs[7], x2])
    assert isinstance(v3, np.ndarray) and v3.shape == (2,)
    assert v3[0] == Q.eval_u_ref(g, stack[1], xs[7:8])[0] and v3[1] == Q.eval_u_ref(g2, d2, x2[None])[0]
    # states as columns are transposed; the caller's states are not modified; a non-contiguous array is made contiguous
    xt = dev(xs[:65].T.copy())
    keep = xt.clone()
    assert same(eval_u(g, dev(data, dtype), xt), one) and torch.equal(xt, keep)
    perm = list(range(1, g.dim)) + [0]
    base = dev(np.ascontiguousarray(data.transpose(perm)), dtype)
    view = base.permute([g.dim - 1] + list(range(g.dim - 1)))
    assert not view.is_contiguous() and tuple(view.shape) == data.shape and same(eval_u(g, view, x65), one)
    with pytest.raises(ValueError):
        eval_u(g, dev(data[:-1]), x65)
    with pytest.raises(ValueError):
        eval_u(g, dev(data), dev(xs[:4, :3]))


# ------------------------------------------------------------------------------------------ 2. eval_costate
def gradients_then_eval_u(g, d_t, x_t, fn):
    dC, dL, dR = L.computeGradients(g, d_t, derivFunc=fn)
    return [torch.stack([eval_u(g, a[d], x_t) for d in range(g.dim)], dim=-1) for a in (dC, dL, dR)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("name", NAMES)
def test_eval_costate_is_gradients_then_eval_u(name, scheme, dtype):
    """BIT FOR BIT eval_u applied to computeGradients' derivC arrays of the same data (hidim_upwind_kernel: the same upwind<>
    source, the same interpolation), for every M; the one-sided values and V from the same gather; in fp64 also against
    costate_ref (the oracle's derivatives): exactly for ENO2 / ENO3, within 1e-11 max(1, max|ref|) for the as-shipped WENO5."""
    fn, sid = SCHEMES[scheme]
    g, og, data, xs, _ = case(name)
    kernel = X.costate_kernel_name(dtype, g.dim, sid)
    d_t, x_t = dev(data, dtype), dev(xs)
    expC, expL, expR = gradients_then_eval_u(g, d_t, x_t, fn)
    for M in MS:
        sl = slice(0, M) if M > 1 else slice(202, 203)
        got = eval_costate(g, d_t, x_t[sl], fn)
        launched(kernel, "test_eval_costate_is_gradients_then_eval_u")
        assert tuple(got.shape) == (M, g.dim) and got.dtype == TD[dtype]
        assert same(got, expC[sl]), (M, float((got - expC[sl]).abs().nan_to_num().max()))
    cs, dl, dr, val = query.costate_states(g, d_t, x_t, sid, want_lr=True, want_value=True)
    assert same(cs[0], expC) and same(dl[0], expL) and same(dr[0], expR) and same(val[0], eval_u(g, d_t, x_t))
    assert bool(torch.isnan(cs[0, 100]).all()) and bool(torch.isnan(val[0, 100]))
    if dtype == "float64":
        ref = Q.costate_ref(og, data, xs, scheme)
        got = eval_costate(g, data, xs, fn)                              # NumPy in -> NumPy out
        assert isinstance(got, np.ndarray) and same(got, expC)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        scale = max(1.0, float(np.max(np.abs(ref[ok]))))
        err = float(np.max(np.abs(got[ok] - ref[ok])))
        print("eval_costate %s %s: max|device - oracle| %.3e (scale %.3g)" % (name, scheme, err, scale))
        if scheme.startswith("ENO"):
            assert np.array_equal(got[ok], ref[ok]), err
        else:
            assert err <= 1e-11 * scale, (err, scale)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_eval_costate_fallbacks_stack_dims_and_nonfinite(name, dtype):
    g, og, data, xs, _ = case(name)
    d_t, x_t = dev(data, dtype), dev(xs[:130])
    # a foreign derivative function takes computeGradients, then the interpolation kernel
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    got = eval_costate(g, d_t, x_t, foreign)
    assert X.last_kernel() == X.interp_kernel_name(dtype)
    assert same(got, gradients_then_eval_u(g, d_t, x_t, foreign)[0]) and same(got, eval_costate(g, d_t, x_t, L.upwindFirstENO3))
    # derivFunc defaults to upwindFirstWENO5; a dims mask leaves NaN columns; a time-first stack is its arrays one by one
    dflt = eval_costate(g, d_t, x_t)
    assert same(dflt, eval_costate(g, d_t, x_t, L.upwindFirstWENO5))
    mask = [1, 0, 1, 1, 0, 1][:g.dim]
    on, off = [d for d in range(g.dim) if mask[d]], [d for d in range(g.dim) if not mask[d]]
    part = eval_costate(g, d_t, x_t, dims=mask)
    assert same(part[:, on], dflt[:, on]) and bool(torch.isnan(part[:, off]).all())
    part = eval_costate(g, d_t, x_t, foreign, dims=mask)
    assert same(part[:, on], got[:, on]) and bool(torch.isnan(part[:, off]).all())
    stack = torch.stack([d_t, 2 * d_t + 1])
    st = eval_costate(g, stack, x_t)
    assert tuple(st.shape) == (2, 130, g.dim) and same(st[0], dflt) and same(st[1], eval_costate(g, stack[1].clone(), x_t))
    # an inf block, a NaN and a -inf in the data: as computeGradients (1e6 in the neighbours' stencils, NaN / inf at the node)
    bad = data.copy()
    bad[(slice(2, 4), slice(1, 3), slice(4, 7)) + (slice(1, 3),) * (g.dim - 3)] = np.inf
    bad[(5, 4, 1) + (2,) * (g.dim - 3)] = np.nan
    bad[(0, 0, 6) + (0,) * (g.dim - 3)] = -np.inf
    b_t = dev(bad, dtype)
    # states in the cells next to the three kinds of node, besides the shared ones
    vs, dx = [np.asarray(v).ravel() for v in g.vs], np.asarray(g.dx).ravel()
    at = lambda idx, s: np.array([vs[d][i] + s * dx[d] for d, i in enumerate(idx)])      # noqa: E731
    near = np.stack([at((5, 4, 1) + (2,) * (g.dim - 3), -0.3), at((0, 0, 6) + (0,) * (g.dim - 3), 0.3), at((3, 2, 5) + (2,) * (g.dim - 3), -0.4),
                     at((4, 1, 4) + (1,) * (g.dim - 3), 0.3)])        # NaN node, -inf node, inside the inf block, beside it
    x_b = dev(np.concatenate([near, xs]))
    plain = eval_costate(g, d_t, x_b, L.upwindFirstENO2)
    for fn in (L.upwindFirstENO2, L.upwindFirstENO3, L.upwindFirstWENO5):
        got = eval_costate(g, b_t, x_b, fn)
        assert same(got, gradients_then_eval_u(g, b_t, x_b, fn)[0]), fn.__name__
        assert bool(torch.isnan(got[0]).all()) and bool(torch.isinf(got[1:3]).all()) and bool(torch.isfinite(got[3]).all())
        assert bool(torch.isfinite(plain[:4]).all()) and bool(torch.isfinite(got).any())


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("trailing", [2, 3])
def test_data_without_trailing_axes_gives_the_3d_librarys_bits(trailing, scheme):
    """Independent of the restatements: a 3-D array broadcast along two (5-D) and three (6-D) trailing axes, states on nodes of
    those axes.  eval_u equals what libhj_query.so gives on the 3-D grid bit for bit -- the corners off the trailing nodes have
    weight 0 and are skipped --, and the trailing costate columns are exactly 0.  The first three costate columns equal the 3-D
    library's bit for bit with the as-shipped WENO5, where both libraries run upwind<>.  With ENO2 / ENO3 they cannot: at
    5-D / 6-D computeGradients rounds every ENO operation on its own (hidim_upwind_kernel, upwind_lr_exact) and eval_costate is
    held to ITS bits (test_eval_costate_is_gradients_then_eval_u), while the 3-D library contracts dx D2 + D1 into one FMA, as
    the 3-D computeGradients does.  The two differ by the roundings of at most three products per side, each below eps times the
    largest first divided difference of the data, through 0.5 (L + R) and a convex combination of eight corners: held to
    16 eps max|D1| (a wrong stencil or stride is off by 1e-2 and more)."""
    fn, sid = SCHEMES[scheme]
    name = "plane5d" if trailing == 2 else "pair6d"
    g, og = XC.grids(name)
    gmin, gmax, N, pd = HC.limits(name)
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    g3 = L.createGrid(col(gmin[:3], np.float64), col(gmax[:3], np.float64), col(N[:3], np.int64), [2])
    for d in range(3):
        assert np.array_equal(np.asarray(g3.vs[d]).ravel(), np.asarray(g.vs[d]).ravel())
    rng = np.random.default_rng(17)
    xs3d = np.meshgrid(*[np.asarray(v).ravel() for v in g3.vs], indexing='ij')
    d3 = np.sqrt(xs3d[0] ** 2 + 1.2 * xs3d[1] ** 2 + 0.01) - 1 + 0.1 * np.sin(xs3d[2]) + 0.02 * rng.standard_normal(xs3d[0].shape)
    dn = np.ascontiguousarray(np.broadcast_to(d3.reshape(d3.shape + (1,) * trailing), tuple(N)))
    x3 = Q.state_set(g3, 150)
    # nodes of the trailing axes that the cell search places exactly (weight 0, or 1 at the last node): node 0 always is one;
    # vs[k] and vs[0] + k dx may differ in the last place for the others, and such a node is a state beside a node
    lo, w, _ = Q.locate(g, np.stack([np.asarray(v).ravel()[np.arange(max(N)) % len(np.asarray(v).ravel())] for v in g.vs], axis=1))
    nodes = []
    for d in range(3, g.dim):
        v = np.asarray(g.vs[d]).ravel()
        exact = [k for k in range(v.size) if w[d][k] == 0.0 or (w[d][k] == 1.0 and k == v.size - 1 and d not in pd)]
        assert 0 in exact and len(exact) >= 2, (d, exact)
        nodes.append(v[exact])
    pick = np.stack([v[rng.integers(0, v.size, 150)] for v in nodes], axis=1)
    pick[:5] = [v[-1] for v in nodes]
    xn = np.concatenate([x3, pick], axis=1)
    v3, vn = eval_u(g3, dev(d3), dev(x3)), eval_u(g, dev(dn), dev(xn))
    assert _qffi.last_kernel() == "interp_points_kernel<double>" and X.last_kernel() == X.interp_kernel_name("float64")
    assert same(vn, v3) and int(torch.isnan(v3).sum()) >= 2
    c3, cn = eval_costate(g3, dev(d3), dev(x3), fn), eval_costate(g, dev(dn), dev(xn), fn)
    assert _qffi.last_kernel() == "costate_points_kernel<double, %d>" % sid and X.last_kernel() == X.costate_kernel_name("float64", g.dim, sid)
    inside = ~torch.isnan(c3[:, 0])
    if scheme == "WENO5_ASSHIPPED":
        assert same(cn[:, :3], c3)
    else:
        assert bool(torch.equal(torch.isnan(cn[:, :3]), torch.isnan(c3)))
        per = Q.periodic_axes(g3)
        wrapped = [np.concatenate([d3, np.take(d3, [0], axis=d)], axis=d) if per[d] else d3 for d in range(3)]
        d1 = max(float(np.max(np.abs(np.diff(wrapped[d], axis=d)))) / float(np.ravel(g3.dx)[d]) for d in range(3))
        err = float((cn[inside][:, :3] - c3[inside]).abs().max())
        print("%s, %d trailing axes: max|5-D / 6-D costate - 3-D costate| %.3e, bound %.3e" % (scheme, trailing, err, 16 * 2.0 ** -52 * d1))
        assert err <= 16 * 2.0 ** -52 * d1, (err, d1)
    assert bool((cn[inside][:, 3:] == 0).all()) and bool(torch.isnan(cn[~inside][:, 3:]).all())


# ------------------------------------------------------------------------------------------ 3. proj
# removed-axes masks (bit d = axis d) by class: last axis kept; last axis removed; one axis removed; all but one removed
MASKS = {5: (0b00001, 0b01010, 0b00111, 0b10000, 0b10100, 0b11010, 0b01111, 0b11110, 0b11101),
         6: (0b000001, 0b001010, 0b010111, 0b100000, 0b100100, 0b110101, 0b011111, 0b111110, 0b111011)}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["plane5d", "pair6d", "plane5d_long"])
def test_proj_minmax_bitwise(name, dtype):
    """'min' / 'max' bit for bit NumPy's over every class of removed axes: the last axis kept (a thread per output node), the
    last axis removed and shorter than a wavefront (9 and 8 nodes) or longer (70), one axis removed, all but one removed; a
    NaN in a reduced set gives NaN; a time-first stack and a list equal per-array calls."""
    g, og = XC.grids(name)
    nd = g.dim
    shape = tuple(int(n) for n in np.ravel(g.N))
    data = XC.noisy(name).astype(ND[dtype])
    d_t = dev(data, dtype)
    for mask in MASKS[nd]:
        rem = [(mask >> d) & 1 for d in range(nd)]
        axes = tuple(d for d in range(nd) if rem[d])
        for op, red in (('min', np.amin), ('max', np.amax)):
            gOut, out = proj(g, d_t, rem, op)
            launched(X.project_kernel_name(dtype, rem[-1]), "test_proj_minmax_bitwise")
            assert torch.is_tensor(out) and out.dtype == TD[dtype]
            assert same(out, red(data, axis=axes)), (rem, op)
            assert gOut.dim == nd - len(axes) and [int(n) for n in np.ravel(gOut.N)] == [shape[d] for d in range(nd) if not rem[d]]
            assert [f.__name__ for f in gOut.bdry] == [g.bdry[d].__name__ for d in range(nd) if not rem[d]]
    assert same(proj(g, d_t, [1] + [0] * (nd - 1))[1], np.amin(data, axis=0))          # xs defaults to 'min'
    bad = data.copy()
    bad[(1,) * nd] = np.nan
    bad[(2,) * (nd - 1) + (shape[-1] - 1,)] = np.nan
    for rem in ([0] * (nd - 1) + [1], [1] + [0] * (nd - 1), [1] * (nd - 1) + [0], [0] + [1] * (nd - 1)):
        axes = tuple(d for d in range(nd) if rem[d])
        for op, red in (('min', np.amin), ('max', np.amax)):
            out = proj(g, dev(bad, dtype), rem, op)[1]
            assert same(out, red(bad, axis=axes)) and 1 <= int(torch.isnan(out).sum()) <= 2
    stack = np.stack([data, -data, bad])
    for rem in ([0] * (nd - 1) + [1], [1, 1] + [0] * (nd - 2)):
        out = proj(g, dev(stack, dtype), rem, 'max')[1]
        lst = proj(g, [dev(a, dtype) for a in stack], rem, 'max')[1]
        assert same(out, lst)
        for t in range(3):
            assert same(out[t], proj(g, dev(stack[t], dtype), rem, 'max')[1])
    gOut, out = proj(g, data.astype(np.float64), [0] * (nd - 1) + [1], 'min')           # NumPy in -> NumPy out
    assert isinstance(out, np.ndarray) and same(out, np.amin(data.astype(np.float64), axis=nd - 1))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_proj_in_two_launches_has_the_single_launchs_bits(dtype, monkeypatch):
    """With fewer output nodes than query.PROJ_STAGE_NODES the leading removed axes go first, the rest is removed from that
    result (on a grid of fewer axes: libhj_query.so below five).  The threshold is lowered to the test grid's size: the same
    bits as NumPy and as the single launch, NaN planes included, for one array and a stack."""
    g, og, data, _, _ = case("pair6d")
    data = data.astype(ND[dtype])
    bad = data.copy()
    bad[1, 1, 1, 1, 1, 1] = np.nan
    bad[2, 0, 3, 4, 5, 7] = np.nan
    stack = np.stack([data, bad, -bad])
    ct = "double" if dtype == "float64" else "float"
    # (removed axes, threshold, kernel of this library's last launch, kernel of libhj_query.so's last launch or None)
    cases = [([2, 3, 4, 5], 200, X.project_kernel_name(dtype, False), "project_minmax_kernel<%s, true>" % ct),     # {2,3,4} then {5}
             ([0, 1, 2, 3], 200, X.project_kernel_name(dtype, False), "project_minmax_kernel<%s, false>" % ct),    # {0,1,2} then {3}
             ([1, 2, 3, 5], 3000, X.project_kernel_name(dtype, True), None),                                        # {1}, then {2,3,5} at 5-D
             ([0, 5], 200, X.project_kernel_name(dtype, True), None)]                                              # enough nodes: one launch
    for gone, thresh, mine, theirs in cases:
        rem = [1 if d in gone else 0 for d in range(6)]
        for op, red in (('min', np.amin), ('max', np.amax)):
            monkeypatch.setattr(query, "PROJ_STAGE_NODES", 1)
            single = proj(g, dev(stack, dtype), rem, op)[1]
            monkeypatch.setattr(query, "PROJ_STAGE_NODES", thresh)
            before = _qffi.last_kernel()
            out = proj(g, dev(stack, dtype), rem, op)[1]
            assert X.last_kernel() == mine and _qffi.last_kernel() == (theirs or before), (gone, X.last_kernel(), _qffi.last_kernel())
            assert same(out, red(stack, axis=tuple(1 + d for d in gone))) and same(out, single), (gone, op)
            assert int(torch.isnan(out).sum()) >= 2
            assert same(proj(g, dev(bad, dtype), rem, op)[1], out[1])


@pytest.mark.parametrize("name", NAMES)
def test_proj_slices_and_resampling_bitwise(name):
    """Slices and NOut resampling in fp64: bit for bit proj_ref.  The kept grid of a resampled min / max may itself be 5-D."""
    g, og, data, _, _ = case(name)
    nd = g.dim
    shape = data.shape
    pd = HC.SHAPES[name][1]
    vs = [np.asarray(v).ravel() for v in g.vs]
    dx = np.asarray(g.dx).ravel()
    d_t = dev(data)
    stack = np.stack([data, data ** 2])
    for mask in ((0b10100, 0b00011, 0b11110) if nd == 5 else (0b100100, 0b011011, 0b000001)):
        rem = [(mask >> d) & 1 for d in range(nd)]
        gone = [d for d in range(nd) if rem[d]]
        nk = nd - len(gone)
        for kind in ("node", "between", "far"):
            pt = [{"node": vs[d][2], "between": vs[d][1] + 0.37 * dx[d],
                   "far": vs[d][1] + 0.37 * dx[d] + (5 * shape[d] * dx[d] if d in pd else 0.0)}[kind] for d in gone]
            gOut, out = proj(g, d_t, rem, pt)
            assert same(out, Q.proj_ref(g, data, rem, pt)), (rem, kind)
            assert list(out.shape) == [int(n) for n in np.ravel(gOut.N)] == [shape[d] for d in range(nd) if not rem[d]]
        pt = [vs[d][1] + 0.6 * dx[d] for d in gone]
        assert same(proj(g, dev(stack), rem, pt)[1], Q.proj_ref(g, stack, rem, pt))          # time first
        NOut = [5, 4, 6, 3, 4][:nk]
        gOut, out = proj(g, d_t, rem, pt, NOut=NOut)
        assert tuple(out.shape) == tuple(NOut) and same(out, Q.proj_ref(g, data, rem, pt, NOut=NOut))
        assert [int(n) for n in np.ravel(gOut.N)] == NOut
        assert same(proj(g, d_t, rem, 'min', NOut=NOut)[1], Q.proj_ref(g, data, rem, 'min', NOut=NOut))
        if nk == 5:
            assert X.last_kernel() == X.interp_kernel_name("float64")            # the 5-D kept grid: resampled by this library
        assert same(proj(g, dev(stack), rem, 'max', NOut=3)[1], Q.proj_ref(g, stack, rem, 'max', NOut=3))
    gOut, out = proj(g, d_t, [0] * (nd - 1) + [1], [float(vs[-1][0])], process=False)
    assert not hasattr(gOut, "vs") and same(out, Q.proj_ref(g, data, [0] * (nd - 1) + [1], [float(vs[-1][0])]))


def test_sep_grid_on_the_6d_grid():
    g, og, data, _, _ = case("pair6d")
    d_t = dev(data)
    gs, ds = sepGrid(g, [[0, 1, 2], [3, 4, 5], [0, 1, 3, 4, 5]], d_t, 'min')
    assert [gi.dim for gi in gs] == [3, 3, 5]
    assert same(ds[0], np.amin(data, axis=(3, 4, 5))) and same(ds[1], np.amin(data, axis=(0, 1, 2))) and same(ds[2], np.amin(data, axis=2))
    gs, ds = sepGrid(g, [[0, 1, 2], [3, 4, 5]], data, [0.3, -0.2, 1.0])
    assert same(ds[0], Q.proj_ref(g, data, [0, 0, 0, 1, 1, 1], [0.3, -0.2, 1.0])) and same(ds[1], Q.proj_ref(g, data, [1, 1, 1, 0, 0, 0], [0.3, -0.2, 1.0]))


# ------------------------------------------------------------------------------------------ 4. rollouts
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("name", NAMES)
def test_one_control_step_on_every_plant_and_scheme(name, scheme, dtype):
    """T = 2 with data[1] = data[0] + 1, so tE = 0 is forced and the step is two sub-samples of {costate, controls, RK4} on
    smooth analytic data, for 203 states (nodes, first / last cells, outside, periods away, the wrap cell, a NaN state): states
    within 1e-12 of the restatement, lengths, status, tEarliest and NaN patterns equal."""
    fn, sid = SCHEMES[scheme]
    g, og, _, xs, _ = case(name)
    kernel = X.rollout_kernel_name(dtype, sid, XC.PLANT_ID[name])
    tau = np.array([0.0, 0.1])
    base = XC.smooth(g, 1).astype(ND[dtype])
    data = np.stack([base, base + ND[dtype](1)])
    system, par = XC.system(name, g), XC.PLANT_PAR[name]
    for uMode, dMode in (('max', 'min'), ('min', 'max')):
        rtraj, rlen, rte, rstat, fragile = R.rollout_ref(og, data, tau, name, par, xs, uMode, dMode, 2, scheme)
        args = L.Bundle(dict(uMode=uMode, dMode=dMode, subSamples=2, derivFunc=fn, tEarliest=True))
        trajs, lengths, _, outs = computeOptTrajs(g, dev(data, dtype), tau, system, dev(xs), args)
        launched(kernel, "test_one_control_step_on_every_plant_and_scheme")
        assert outs.path == kernel == rollout.last_path()
        got = host(trajs)
        assert (rlen == 2).all() and same(lengths, rlen) and same(outs.tEarliest, rte) and same(outs.status, rstat)
        assert same(got[:, :, 0], xs)
        assert np.array_equal(np.isnan(got), np.isnan(rtraj)), uMode
        ok = ~np.isnan(rtraj)
        err = float(np.max(np.abs(got[ok] - rtraj[ok])))
        print("%s %s %s %s/%s: max|state - restatement| %.3e, %d fragile, %d NaN trajectories" % (
            name, scheme, dtype, uMode, dMode, err, int(fragile.sum()), int(np.isnan(rtraj[:, 0, 1]).sum())))
        assert err <= TOL, (uMode, err)
    assert np.isnan(rtraj[:, :, 1]).any() and (rstat == R.LEFT_GRID).any()


_HORIZON = {}


def horizon():
    """The pursuit game of DubinsPair6D on (6, 5, 7, 5, 6, 8): a store-all HJIPDE_solve with ENO2 over five time stamps,
    flipped (index 0 the full horizon), and 64 joint states.  tests/hiquery_cases.py fixes the inputs; with them the restatement
    meets no fragile decision, 17 trajectories leave the grid and the lengths 1, 2, 4 and 5 occur (checked on the CPU with the
    oracle's solve of the same problem)."""
    if not _HORIZON:
        g, og = XC.grids("pair6d")
        pair = L.DubinsPair6D(g, *XC.HORIZON_PAR)
        sd = L.Bundle(dict(grid=g, hamFunc=pair.hamiltonian, partialFunc=pair.dissipation, dissFunc=L.artificialDissipationGLF,
                           derivFunc=L.upwindFirstENO2))
        stack, tau, _ = L.HJIPDE_solve(XC.horizon_target(og), XC.HORIZON_TAU, sd, 'minVOverTime', L.Bundle(dict(quiet=True)))
        stack = np.asarray(stack)
        assert stack.shape == (5,) + og.shape and np.array_equal(tau, XC.HORIZON_TAU)
        data = np.ascontiguousarray(stack[::-1])
        xs = XC.horizon_states(og)
        for a in (data, xs):
            a.setflags(write=False)
        ref = R.rollout_ref(og, data, XC.HORIZON_TAU, "pair6d", XC.HORIZON_PAR, xs, 'max', 'min', 4, "ENO2")
        _HORIZON.update(g=g, og=og, data=data, xs=xs, ref=ref, tau=XC.HORIZON_TAU)
    return _HORIZON


@pytest.mark.parametrize("where", ["numpy", "tensor"])
def test_pursuit_whole_horizon(where):
    """Within 1e-12 of the restatement, lengths and NaN patterns equal.  A trajectory is set aside only if the restatement met a
    switching function with 0 < |s| < 1e-6 or a bisection value within 1e-6 of 1e-4; at most 4 of 64.  Then every trajectory
    against computeOptTraj with a copy of the system."""
    H = horizon()
    g, og, data, xs, tau = H["g"], H["og"], H["data"], H["xs"], H["tau"]
    rtraj, rlen, rte, rstat, fragile = H["ref"]
    keep = ~fragile
    print("restatement: %d of 64 fragile, lengths %s, %d leave the grid" % (
        int(fragile.sum()), sorted(set(rlen.tolist())), int((rstat == R.LEFT_GRID).sum())))
    assert fragile.sum() <= 4 and (rstat == R.LEFT_GRID).any() and len(set(rlen.tolist())) >= 2
    system = L.DubinsPair6D(g, *XC.HORIZON_PAR)
    args = L.Bundle(dict(uMode='max', dMode='min', subSamples=4, derivFunc=L.upwindFirstENO2, tEarliest=True))
    d_in, x_in = (data, xs) if where == "numpy" else (dev(data), dev(xs))
    trajs, lengths, _, outs = computeOptTrajs(g, d_in, tau, system, x_in, args)
    assert X.last_kernel() == "hi_rollout_kernel<double, 0, 51>" == outs.path
    for a in (trajs, lengths, outs.status, outs.tEarliest):
        assert (torch.is_tensor(a) and a.is_cuda) if where == "tensor" else isinstance(a, np.ndarray)
    got = host(trajs)
    ok = ~np.isnan(rtraj[keep])
    err = float(np.max(np.abs(got[keep][ok] - rtraj[keep][ok])))
    print("%s: max|state - restatement| %.3e over %d trajectories" % (where, err, int(keep.sum())))
    assert np.array_equal(host(lengths)[keep], rlen[keep])
    assert np.array_equal(np.isnan(got[keep]), np.isnan(rtraj[keep]))
    assert np.array_equal(host(outs.status)[keep], rstat[keep]) and np.array_equal(host(outs.tEarliest)[keep], rte[keep])
    assert err <= TOL, err
    # uMode / dMode as the host loop resolves them when extraArgs names neither: 'min', and get_opt_v's own default
    a = computeOptTrajs(g, d_in, tau, system, x_in[:9], L.Bundle(dict(derivFunc=L.upwindFirstENO2)))
    b = computeOptTrajs(g, d_in, tau, system, x_in[:9], L.Bundle(dict(uMode='min', dMode='min', derivFunc=L.upwindFirstENO2)))
    assert len(a) == 3 and same(a[0], b[0]) and same(a[1], b[1])
    if where == "tensor":
        return
    one = L.Bundle(dict(uMode='max', dMode='min', subSamples=4, derivFunc=L.upwindFirstENO2))
    worst = 0.0
    for m in np.nonzero(keep)[0]:
        sys_m = L.DubinsPair6D(g, *XC.HORIZON_PAR)
        sys_m.x = xs[m].copy()
        traj, t1 = computeOptTraj(g, dev(data), tau, sys_m, one)
        assert traj.shape[1] == rlen[m] and np.array_equal(t1, tau[:rlen[m]]), (m, traj.shape, rlen[m])
        mine = got[m][:, :rlen[m]]
        assert np.array_equal(np.isnan(traj), np.isnan(mine)), m
        fin = ~np.isnan(mine)
        worst = max(worst, float(np.max(np.abs(traj[fin] - mine[fin]))) if fin.any() else 0.0)
    print("max|computeOptTraj - kernel| %.3e" % worst)
    assert worst <= TOL, worst


class _Lazy(L.DubinsPair6D):
    """A subclass that overrides a protocol method: not the kernel's plant any more."""

    def get_opt_u(self, t, deriv, uMode, x):
        return 0.5 * L.DubinsPair6D.get_opt_u(self, t, deriv, uMode, x)


def test_other_systems_take_the_host_loop():
    H = horizon()
    g, data, xs, tau = H["g"], H["data"], H["xs"], H["tau"]
    pick = xs[[0, 9, 20, 33]]
    args = L.Bundle(dict(uMode='max', dMode='min', subSamples=2, derivFunc=L.upwindFirstENO2, status=True))
    plant = _Lazy(g, *XC.HORIZON_PAR)
    plant.x = np.full(6, 7.0)
    trajs, lengths, _, outs = computeOptTrajs(g, dev(data), tau, plant, dev(pick), args)
    assert outs.path.startswith("host loop: ") and "_Lazy" in outs.path and rollout.last_path() == outs.path
    assert np.array_equal(plant.x, np.full(6, 7.0)) and torch.is_tensor(trajs) and tuple(trajs.shape) == (4, 6, 5)
    for m in range(4):
        one = _Lazy(g, *XC.HORIZON_PAR)
        one.x = pick[m].copy()
        traj, _ = computeOptTraj(g, dev(data), tau, one, args)
        assert int(host(lengths)[m]) == traj.shape[1] and same(host(trajs)[m][:, :traj.shape[1]], traj), m
    # a derivative function without a point kernel, and a 5-D system on the 6-D grid
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO2(grid, a, dim)        # noqa: E731
    kern = computeOptTrajs(g, dev(data), tau, L.DubinsPair6D(g, *XC.HORIZON_PAR), dev(pick), args)
    assert kern[3].path == "hi_rollout_kernel<double, 0, 51>"
    args_f = L.Bundle(dict(uMode='max', dMode='min', subSamples=2, derivFunc=foreign, status=True))
    loop = computeOptTrajs(g, dev(data), tau, L.DubinsPair6D(g, *XC.HORIZON_PAR), dev(pick[:2]), args_f)
    assert loop[3].path.startswith("host loop: derivFunc") and same(host(loop[1]), host(kern[1])[:2])
    fin = ~np.isnan(host(kern[0])[:2])
    assert np.array_equal(np.isnan(host(loop[0])), ~fin) and float(np.max(np.abs(host(loop[0])[fin] - host(kern[0])[:2][fin]))) <= TOL


# ------------------------------------------------------------------------------------------ 5. bounds
_POOLS = {}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", 700 * 1000)
    return _POOLS[dtype]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_guarded(op, what):
    """tests/test_gpu_rollout.py's run_guarded: op(F, S, arm) carves the fp64 arrays from F and the four-byte ones (an fp32
    stack; the int32 outputs, as views of the fp32 pool, which compares bits) from S."""
    P32 = pool("float32")

    def both(a):
        b = P32.begin(a.fill, a.offset_elems) if isinstance(a, GuardedPool) else PlainAlloc(torch.float32, "cuda")
        res = dict(op(a, b, lambda: (a.arm(), b.arm())))
        if isinstance(a, GuardedPool):
            b.check()
        else:
            torch.cuda.synchronize()
        res.update(("s " + k, v) for k, v in b.results().items())
        return res
    return run_case(both, pool("float64"), what=what)[0]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_kernels_stay_inside_their_arrays(name, dtype):
    """The four entry points on views carved from tests/guarded_pool.py's pools, at element offsets 0-3 (a view at an odd
    element offset among them) and with guards of NaN and +-1e30, an odd number of states, the optional outputs included:
    guards intact, inputs unchanged, every output element written, the same bits as on fresh arrays."""
    lib = X.lib()
    g, og, _, xs, _ = case(name)
    nd = g.dim
    desc, N = _marshal.descriptor_hi(g, dtype)
    n = int(np.prod(N))
    rows = (2 * N[0], n // N[0])                    # the stack as 2 N[0] planes: the guards are four such planes, not four fields
    stack = torch.stack([dev(XC.noisy(name, 3), dtype), dev(XC.noisy(name, 4), dtype)]).reshape(rows)
    M = 131
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
        X.check(lib.hjx_interp_points(C.byref(desc), a.ptr, 2, n, C.c_void_p(x.data_ptr()), M, o.ptr, 0, _stream()))
        return {"kernel": X.last_kernel()}

    def costate(sid):
        def op(alloc):
            a = alloc.inp("data", stack)
            x = states(alloc)
            outs = [alloc.out(k, (2, M, nd)) for k in ("costate", "derivL", "derivR")]
            v = alloc.out("value", (2, M))
            alloc.arm()
            X.check(lib.hjx_costate_points(C.byref(desc), sid, a.ptr, 2, n, C.c_void_p(x.data_ptr()), M,
                                           outs[0].ptr, outs[1].ptr, outs[2].ptr, v.ptr, 0, _stream()))
            return {"kernel": X.last_kernel()}
        return op

    def project(mask, op_id):
        keep = tuple(k for d, k in enumerate(N) if not (mask >> d) & 1)

        def op(alloc):
            a = alloc.inp("data", stack)
            o = alloc.out("out", (2,) + keep)
            alloc.arm()
            X.check(lib.hjx_project_minmax(C.byref(desc), a.ptr, 2, n, mask, op_id, o.ptr, _stream()))
            return {"kernel": X.last_kernel()}
        return op

    ref, _ = run_case(interp, P, what="interp")
    assert ref["kernel"] == X.interp_kernel_name(dtype)
    for sid in (0, 1, 3):
        ref, _ = run_case(costate(sid), P, what="costate %d" % sid)
        assert ref["kernel"] == X.costate_kernel_name(dtype, nd, sid)
    for mask in (1 << (nd - 1), 1, (1 << nd) - 2, (1 << (nd - 1)) - 1):
        ref, _ = run_case(project(mask, mask & 1), P, what="project %#x" % mask)
        assert ref["kernel"] == X.project_kernel_name(dtype, mask >> (nd - 1))

    # the rollout: one control step from every state, slices `n + 3` elements apart with gaps that would change the result
    base = XC.smooth(g, 2)
    data = np.stack([base, base + 1]).reshape(2, -1)
    stride = n + 3
    buf = torch.full((stride + n,), -1e30, dtype=TD[dtype], device="cuda")
    buf[:n], buf[stride:] = dev(data[0], dtype), dev(data[1], dtype)
    plant = _rffi.plant_descriptor(XC.PLANT_ID[name], 1, 0, list(XC.PLANT_PAR[name]))

    def roll(F, S, arm):
        a = (F if dtype == "float64" else S).inp("data", buf)
        x = F.inp("x0", x_t)
        traj = F.out("traj", (M, nd, 2))
        length, te, status = S.out("length", (M,)), S.out("t_earliest", (M, 2)), S.out("status", (M,))
        arm()
        X.check(lib.hjx_rollout(C.byref(desc), 3, a.ptr, 2, stride, x.ptr, M, 2, 0.05, C.byref(plant), traj.ptr,
                                length.ptr, te.ptr, status.ptr, _stream()))
        return {"kernel": X.last_kernel()}
    assert run_guarded(roll, "rollout")["kernel"] == X.rollout_kernel_name(dtype, 3, XC.PLANT_ID[name])
    # the strided stack gives what the contiguous one gives through the front end; t_earliest is optional
    dense = rollout.rollout_states(g, dev(data.reshape((2,) + tuple(N)), dtype), x_t, 3, 2, 0.05, plant, True)
    traj = torch.empty((M, nd, 2), dtype=torch.float64, device="cuda")
    length, status = (torch.empty((M,), dtype=torch.int32, device="cuda") for _ in range(2))
    X.check(lib.hjx_rollout(C.byref(desc), 3, C.c_void_p(buf.data_ptr()), 2, stride, C.c_void_p(x_t.data_ptr()), M, 2, 0.05,
                            C.byref(plant), C.c_void_p(traj.data_ptr()), C.c_void_p(length.data_ptr()), None,
                            C.c_void_p(status.data_ptr()), _stream()))
    assert same(traj, dense[0]) and same(length, dense[1]) and same(status, dense[3])


def test_the_front_end_refuses_what_the_library_refuses():
    g, og, data, xs, _ = case("plane5d")
    with pytest.raises(_ffi.Unsupported):
        query.costate_states(g, dev(data), dev(xs[:4]), _ffi.WENO5)
    g7 = L.createGrid(np.zeros((7, 1)), np.ones((7, 1)), 3 * np.ones((7, 1), dtype=np.int64))
    with pytest.raises(ValueError, match="more than 6 dimensions"):
        eval_u(g7, np.zeros((3,) * 7), np.zeros((1, 7)))
    with pytest.raises(ValueError, match="more than 6 dimensions"):
        proj(g7, np.zeros((3,) * 7), [1] + [0] * 6)
    # the descriptor of the tools that stop at four axes still refuses
    with pytest.raises(ValueError, match="more than 4 dimensions"):
        _marshal.descriptor(g, "float64")
