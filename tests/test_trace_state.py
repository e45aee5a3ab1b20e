"""CPU: state the traced callbacks read, changed after the trace, must reach the fused kernel (levelsetpy_amd/trace_ham.py).

A traced plan does not call hamFunc / partialFunc at every step: it runs an expression whose parameters and tables were read from Python
state when the pair was traced.  Every lookup of the plan must therefore notice when that state has changed -- wherever it lives -- or refuse
the pair at trace time.  And the tracer must put a real array among the operands on the axis NumPy / torch broadcasting puts it on.

Both are checked against the callbacks themselves: after every change, the parameters and the expression the traced system reports must be
those of a fresh trace, and that expression, evaluated in NumPy (Traced.evaluate), must equal the callbacks on real arrays."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import trace_ham as TH  # noqa: E402

N = (22, 20, 24)
V0, W = 1.3, 0.7
# non-integer speeds before and after each change (integers up to 16 become literals, not parameters)
V1, V2 = 2.15, 0.85


def grid(n=N):
    return L.createGrid(np.array([[-2., -2., -np.pi]]).T, np.array([[2., 2., np.pi * (1 - 2 / n[2])]]).T, np.array(n, dtype=np.int64).reshape(-1, 1), 2)


def _is_t(a):
    return type(a).__module__.startswith("torch")


def _as(v, like):
    """v in the array type of `like` (NumPy for the oracle, device tensors for the split path; a symbolic array takes anything)."""
    if _is_t(v) and isinstance(like, np.ndarray):
        return v.numpy()
    if _is_t(like) and (isinstance(v, np.ndarray) or (_is_t(v) and v.device != like.device)):
        return torch.as_tensor(v, device=like.device)
    return v


def _x(g, d, like):
    return _as(g.xs[d], like)


def ham(v, g, p, c2=None):
    """The Dubins-like system of every case: v (p0 cos x2 + p1 sin x2) + w |p2|."""
    v = _as(v, p[0])
    x2 = _x(g, 2, p[0])
    xp = torch if _is_t(p[0]) else np
    c2 = xp.cos(x2) if c2 is None else _as(c2, p[0])
    return v * (p[0] * c2 + p[1] * xp.sin(x2)) + W * abs(p[2])


def diss(v, g, data, dim, c2=None):
    like = data if data is not None else np.zeros(1)
    v = _as(v, like)
    x2 = _x(g, 2, like)
    xp = torch if _is_t(like) else np
    c2 = xp.cos(x2) if c2 is None else _as(c2, like)
    return [abs(v * c2), abs(v * xp.sin(x2)), W][dim]


# ---------------------------------------------------------------------------------------------- the holders
class Attr(object):
    def __init__(self, g):
        self.grid, self.v = g, V0

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.v, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.v, self.grid, data, dim)


class DictAttr(Attr):
    def __init__(self, g):
        self.grid, self.cfg = g, {"v": V0, "name": "car"}

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.cfg["v"], self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.cfg["v"], self.grid, data, dim)


class NestedDict(Attr):
    def __init__(self, g):
        self.grid, self.cfg = g, {"car": {"speeds": {"v": V0}}}

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.cfg["car"]["speeds"]["v"], self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.cfg["car"]["speeds"]["v"], self.grid, data, dim)


class LongList(Attr):
    def __init__(self, g):
        self.grid, self.speeds = g, [0.05 + 0.1 * k for k in range(20)]
        self.speeds[13] = V0

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.speeds[13], self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.speeds[13], self.grid, data, dim)


class Speeds(object):
    __slots__ = ("v", "unused")

    def __init__(self, v):
        self.v = v


class SlotsHolder(Attr):
    def __init__(self, g):
        self.grid, self.par = g, Speeds(V0)

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.par.v, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.par.v, self.grid, data, dim)


class SlotsSystem(object):
    __slots__ = ("grid", "v", "__weakref__")

    def __init__(self, g):
        self.grid, self.v = g, V0

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.v, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.v, self.grid, data, dim)


GLOBAL_NS = SimpleNamespace(v=V0)
GLOBAL_CFG = {"v": V0}


class GlobalNamespace(Attr):
    def hamiltonian(self, t, data, p, sd=None):
        return ham(GLOBAL_NS.v, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(GLOBAL_NS.v, self.grid, data, dim)


class GlobalDict(Attr):
    def hamiltonian(self, t, data, p, sd=None):
        return ham(GLOBAL_CFG["v"], self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(GLOBAL_CFG["v"], self.grid, data, dim)


class TensorAttr(Attr):
    """A filled tensor of more than 8192 elements (22 x 20 x 24), changed in place."""

    def __init__(self, g):
        self.grid, self.vt = g, torch.full(tuple(g.shape), V0, dtype=torch.float64)

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.vt, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.vt, self.grid, data, dim)


class FilledArray(Attr):
    """A filled NumPy array of more than 8192 elements, changed in place."""

    def __init__(self, g):
        self.grid, self.va = g, np.full(tuple(g.shape), V0)

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.va, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.va, self.grid, data, dim)


class StoredTable(Attr):
    """cos(x2) stored as a full-grid NumPy array before the call (a one-axis table), changed in place: a new expression."""

    def __init__(self, g):
        self.grid, self.v, self.c2 = g, V0, np.cos(np.asarray(g.xs[2])).copy()

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.v, self.grid, p, self.c2)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.v, self.grid, data, dim, self.c2)


class FilledArrayThroughNumPy(FilledArray):
    """The same filled array, reaching the symbolic arguments only through real NumPy operations (temporaries made at every call)."""

    def hamiltonian(self, t, data, p, sd=None):
        return ham(2.0 * self.va / 2.0, self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(np.abs(self.va), self.grid, data, dim)


class HeadingThroughNumPy(Attr):
    """A stored full-grid heading, cos() of it taken at every call: the table the expression holds is a temporary."""

    def __init__(self, g):
        self.grid, self.v, self.heading = g, V0, np.asarray(g.xs[2]).copy()

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.v, self.grid, p, np.cos(self.heading))

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.v, self.grid, data, dim, np.cos(self.heading))


class ScalarOfArray(FilledArray):
    """A NumPy scalar read out of the stored array."""

    def hamiltonian(self, t, data, p, sd=None):
        return ham(self.va[0, 0, 0], self.grid, p)

    def dissipation(self, t, data, lo, hi, sd, dim):
        return diss(self.va[0, 0, 0], self.grid, data, dim)


class Case(object):
    """A schemeData around one holder, and change(k) for the k-th change in place (k = 1, 2)."""

    def __init__(self, g, hamFunc, partialFunc, change, **extra):
        self.grid = g
        self.sd = L.Bundle(dict(grid=g, hamFunc=hamFunc, partialFunc=partialFunc, dissFunc=L.artificialDissipationGLF,
                                CoStateCalc=L.upwindFirstWENO5, **extra))
        self.change = change


def _obj_case(cls, setter):
    def make(g):
        o = cls(g)
        return Case(g, o.hamiltonian, o.dissipation, lambda k: setter(o, k))
    return make


def _closure_case(g):
    cfg = {"v": V0}
    c = Case(g, lambda t, d, p, sd: ham(cfg["v"], g, p), lambda t, d, lo, hi, sd, dim: diss(cfg["v"], g, d, dim),
             lambda k: cfg.__setitem__("v", (V1, V2)[k - 1]))
    c.cfg = cfg
    return c


def _partial_ham(t, data, p, sd, cfg=None, g=None):
    return ham(cfg["v"], g, p)


def _partial_diss(t, data, lo, hi, sd, dim, cfg=None, g=None):
    return diss(cfg["v"], g, data, dim)


def _partial_case(g):
    cfg = {"v": V0}
    return Case(g, functools.partial(_partial_ham, cfg=cfg, g=g), functools.partial(_partial_diss, cfg=cfg, g=g),
                lambda k: cfg.__setitem__("v", (V1, V2)[k - 1]))


def _sd_ham(t, data, p, sd):
    return ham(sd.speeds["v"], sd.grid, p)


def _sd_diss(t, data, lo, hi, sd, dim):
    return diss(sd.speeds["v"], sd.grid, data, dim)


def _schemedata_case(g):
    c = Case(g, _sd_ham, _sd_diss, None, speeds={"v": V0})
    c.change = lambda k: c.sd.speeds.__setitem__("v", (V1, V2)[k - 1])
    return c


def _global_ns_case(g):
    GLOBAL_NS.v = V0
    return _obj_case(GlobalNamespace, lambda o, k: setattr(GLOBAL_NS, "v", (V1, V2)[k - 1]))(g)


def _global_dict_case(g):
    GLOBAL_CFG["v"] = V0
    return _obj_case(GlobalDict, lambda o, k: GLOBAL_CFG.__setitem__("v", (V1, V2)[k - 1]))(g)


def _tensor_change(o, k):
    if k == 1:
        o.vt.fill_(V1)
    else:
        o.vt.mul_(V2 / V1)


def _array_change(o, k):
    if k == 1:
        o.va[...] = V1
    else:
        o.va *= V2 / V1


def _table_change(o, k):
    o.c2 *= (1.25, 0.5)[k - 1]


def _heading_change(o, k):
    o.heading *= (1.25, 0.5)[k - 1]


CASES = {
    "attribute (control)": _obj_case(Attr, lambda o, k: setattr(o, "v", (V1, V2)[k - 1])),
    "dict attribute": _obj_case(DictAttr, lambda o, k: o.cfg.__setitem__("v", (V1, V2)[k - 1])),
    "nested dict": _obj_case(NestedDict, lambda o, k: o.cfg["car"]["speeds"].__setitem__("v", (V1, V2)[k - 1])),
    "list of 20 floats": _obj_case(LongList, lambda o, k: o.speeds.__setitem__(13, (V1, V2)[k - 1])),
    "__slots__ holder": _obj_case(SlotsHolder, lambda o, k: setattr(o.par, "v", (V1, V2)[k - 1])),
    "__slots__ system": _obj_case(SlotsSystem, lambda o, k: setattr(o, "v", (V1, V2)[k - 1])),
    "module-global namespace": _global_ns_case,
    "module-global dict": _global_dict_case,
    "closure dict": _closure_case,
    "partial keyword dict": _partial_case,
    "schemeData dict": _schemedata_case,
    "tensor > 8192, fill_ / mul_": _obj_case(TensorAttr, _tensor_change),
    "filled array > 8192": _obj_case(FilledArray, _array_change),
    "stored table > 8192": _obj_case(StoredTable, _table_change),
    "filled array > 8192 through NumPy": _obj_case(FilledArrayThroughNumPy, _array_change),
    "NumPy scalar of an array > 8192": _obj_case(ScalarOfArray, _array_change),
    "heading > 8192, cos() at every call": _obj_case(HeadingThroughNumPy, _heading_change),
}
NEW_TEXT = ("stored table > 8192", "heading > 8192, cos() at every call")
SAME_TEXT = sorted(k for k in CASES if k not in NEW_TEXT)


@pytest.fixture
def fresh_registry(monkeypatch):
    monkeypatch.setattr(TH, "_REG_BY_SOURCE", {})
    monkeypatch.setattr(TH, "_BAD_SOURCES", set())
    monkeypatch.setattr(TH, "_CHURN", {})


def real_arrays(g, seed=4):
    rng = np.random.default_rng(seed)
    X = np.meshgrid(*[np.asarray(v).ravel() for v in g.vs], indexing="ij")
    p = [rng.standard_normal(tuple(g.shape)) for _ in range(g.dim)]
    return X, p, [-1.5, -0.75, -2.0, -1.0][:g.dim], [1.25, 2.5, 0.5, 1.0][:g.dim]


def check_current(system, case):
    """The traced system's parameters and expression are a fresh trace's, and that expression computes what the callbacks compute now."""
    sd, g = case.sd, case.grid
    par = system.params()
    fresh = TH.trace_callbacks(g, sd.hamFunc, sd.partialFunc, sd)
    assert par == fresh.params
    # the registration the plan launches is the fresh expression: evaluating that expression with the plan's parameters is evaluating the kernel
    assert system.reg is not TH._NoReg and system.reg.traced_key == TH._key_of(fresh) == system._key
    X, p, lo, hi = real_arrays(g)
    H, al = fresh.evaluate(X, p, lo, hi, params=par)
    Hr = sd.hamFunc(0., None, p, sd)
    np.testing.assert_allclose(np.broadcast_to(H, g.shape), Hr, rtol=1e-14, atol=1e-14)
    for d in range(g.dim):
        ar = np.broadcast_to(np.asarray(sd.partialFunc(0., None, lo, hi, sd, d), dtype=np.float64), g.shape)
        np.testing.assert_allclose(np.broadcast_to(al[d], g.shape), ar, rtol=1e-14, atol=1e-14)
    return fresh


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_changed_in_place_reaches_the_traced_parameters(name, fresh_registry):
    g = grid()
    case = CASES[name](g)
    nat = TH.traced_native(case.sd)
    assert nat is not None, "refused at trace time"
    system = nat[0]
    first = check_current(system, case)
    assert first.params[:2] == [V0, W] or name in NEW_TEXT
    for k in (1, 2):
        case.change(k)
        tr = check_current(system, case)
        if name in SAME_TEXT:
            assert TH._key_of(tr) == TH._key_of(first) and tr.params[0] != first.params[0]
        else:
            assert TH._key_of(tr) != TH._key_of(first)
        # the plan-cache entry point re-reads the same
        assert L.dynamics.native_again(system) == (system.reg.ham_id, tr.params)


def test_holders_of_one_speed_share_one_expression(fresh_registry):
    """The GPU half compiles one kernel for all of them."""
    g = grid()
    keys = set()
    for name in SAME_TEXT:
        case = CASES[name](g)
        keys.add(TH._key_of(TH.trace_callbacks(g, case.sd.hamFunc, case.sd.partialFunc, case.sd)))
    assert len(keys) == 1, keys


def test_a_stored_numpy_array_too_large_to_recheck_is_refused(fresh_registry, monkeypatch):
    g = grid()
    monkeypatch.setattr(TH._Consumed, "MAX_CHECKED", 4096)
    case = _obj_case(FilledArray, _array_change)(g)
    with pytest.raises(TH.TraceError, match="too large to re-check"):
        TH.trace_callbacks(g, case.sd.hamFunc, case.sd.partialFunc, case.sd)
    assert TH.traced_native(case.sd) is None
    e = L.explain_plan(case.sd)
    assert e["path"] == "split" and "too large to re-check" in e["reason"]
    # a temporary the callbacks make of the same size is made again from the state at every call: not kept, not refused
    tmp = lambda t, d, p, sd: np.full(tuple(g.shape), V0) * p[0]  # noqa: E731
    TH.trace_callbacks(g, tmp, lambda t, d, lo, hi, sd, dim: 1.0, None)
    # a temporary made from a stored array that is too large to re-check: refused as well
    case = _obj_case(FilledArrayThroughNumPy, _array_change)(g)
    monkeypatch.setattr(TH._Consumed, "MAX_CHECKED", 1 << 16)
    case.sd.hamFunc.__self__.extra = np.zeros((300, 300))
    with pytest.raises(TH.TraceError, match="too large to re-check"):
        TH.trace_callbacks(g, case.sd.hamFunc, case.sd.partialFunc, case.sd)
    assert "too large to re-check" in L.explain_plan(case.sd)["reason"]


def test_state_beyond_the_fingerprint_bounds_is_reported(fresh_registry, monkeypatch):
    g = grid()
    case = _obj_case(LongList, lambda o, k: None)(g)
    o = case.sd.hamFunc.__self__
    o.history = [np.zeros(3)] * 300                           # a list of 300 arrays: not walked
    o.deep = SimpleNamespace(a=SimpleNamespace(b=SimpleNamespace(c=[1.0, [2.0]])))
    e = L.explain_plan(case.sd)
    assert e["path"] == "traced"
    assert any(u.startswith("self[\'history\']") or "history" in u for u in e["unchecked"]), e["unchecked"]
    assert any("deep" in u and "too deep" in u for u in e["unchecked"]), e["unchecked"]
    monkeypatch.setenv("HJ_TRACE_VERBOSE", "1")
    with pytest.warns(UserWarning, match="would not be seen"):
        TH.traced_native(case.sd)


# ---------------------------------------------------------------------------------------------- broadcasting
def cube(dim, n):
    lo = [-2.0, -1.0, -3.0, -0.5][:dim]
    hi = [1.0, 2.5, 0.5, 1.5][:dim]
    return L.createGrid(np.array([lo]).T, np.array([hi]).T, np.full((dim, 1), n, dtype=np.int64), None)


def one_axis_shapes(dim, n):
    """Every shape of 1 to dim axes with exactly one of length n: (n,), (n,1), (1,n), (n,1,1), ..."""
    out = []
    for k in range(1, dim + 1):
        for j in range(k):
            out.append(tuple(n if i == j else 1 for i in range(k)))
    return out


BROADCAST = [(dim, n, s, what) for dim, n in ((2, 12), (3, 10), (4, 7)) for s in one_axis_shapes(dim, n) for what in ("gain", "coordinate")]


@pytest.mark.parametrize("lib", ["numpy", "torch"])
@pytest.mark.parametrize("dim,n,shape,what", BROADCAST, ids=["%dd-%s-%s" % (d, "x".join(map(str, s)), w) for d, n, s, w in BROADCAST])
def test_operands_go_to_the_axis_broadcasting_gives_them(dim, n, shape, what, lib):
    g = cube(dim, n)
    axis = dim - len(shape) + shape.index(n)           # NumPy: the shape aligned to the right
    if what == "gain":
        vals = 1.0 + np.random.default_rng(len(shape) * 10 + shape.index(n)).random(n)
    else:
        vals = np.asarray(g.vs[0]).ravel() if axis != 0 else np.asarray(g.vs[dim - 1]).ravel()   # another axis' coordinates
    op = vals.reshape(shape)
    if lib == "torch":
        op = torch.as_tensor(op)
    h = lambda t, d, p, sd: op * p[0] + p[1] * 0.5  # noqa: E731
    a = lambda t, d, lo, hi, sd, k: abs(op) + 0.25 if k == 0 else 1.0  # noqa: E731
    tr = TH.trace_callbacks(g, h, a, None)
    assert tr.tables and all(d == axis for d, _ in tr.tables), ([d for d, _ in tr.tables], axis)
    X, p, lo, hi = real_arrays(g, seed=dim)
    H, al = tr.evaluate(X, p, lo, hi)
    pp = [torch.as_tensor(q) for q in p] if lib == "torch" else p
    Hr = np.asarray(h(0., None, pp, None))
    np.testing.assert_allclose(np.broadcast_to(H, g.shape), Hr, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(np.broadcast_to(al[0], g.shape), np.broadcast_to(np.asarray(a(0., None, lo, hi, None, 0)), g.shape),
                               rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("lib", ["numpy", "torch"])
@pytest.mark.parametrize("shape,axis", [((12,), None), ((12, 1), 1), ((14,), 2), ((10, 1, 1), 0), ((10, 1), None), ((10,), None),
                                        ((1, 12, 14), None), ((2, 10, 1, 1), None)])
def test_non_cube_grid_operands_broadcast_or_are_refused(shape, axis, lib):
    g = grid((10, 12, 14))
    vals = 1.0 + np.random.default_rng(2).random(int(np.prod(shape)))
    op = vals.reshape(shape)
    if lib == "torch":
        op = torch.as_tensor(op)
    h = lambda t, d, p, sd: op * p[0]  # noqa: E731
    a = lambda t, d, lo, hi, sd, k: 1.0  # noqa: E731
    if axis is None:
        # NumPy refuses to broadcast these against (10, 12, 14): so must the tracer, rather than pick an axis of the same length
        with pytest.raises(TH.TraceError):
            TH.trace_callbacks(g, h, a, None)
        return
    tr = TH.trace_callbacks(g, h, a, None)
    assert tr.tables[0][0] == axis
    X, p, lo, hi = real_arrays(g)
    H, _ = tr.evaluate(X, p, lo, hi)
    pp = [torch.as_tensor(q) for q in p] if lib == "torch" else p
    np.testing.assert_allclose(np.broadcast_to(H, g.shape), np.asarray(h(0., None, pp, None)).reshape(g.shape), rtol=1e-14, atol=1e-14)
