"""What tests/test_hidim_trace_host.py and tests/test_gpu_hidim_trace.py share: systems written ONLY as hamFunc / partialFunc callbacks -- NumPy
style, one operation per statement, nothing registered -- for the tracer on 5-D and 6-D grids (levelsetpy_amd/trace_ham.py, set_hidim_trace).

  PlanePair, DubinsPair      Plane5D over stored cos / sin tables and DubinsPair6D with np.cos(grid.xs[2]) ... inside the callbacks, in the operation
                             order of include/hj_hidim.h (that of tests/hidim_user_cases.py's PLANE_SRC / PAIR_SRC): traced, they must give the
                             built-in kernels' bits under ENO2 / ENO3.  (A speed times a STORED table is NumPy arithmetic the tracer never sees: it
                             would meet v_e cos x2 as a table of its own.  The pair therefore takes its trig from the coordinates.)
  QuadTables, QuadInline     the planar quadrotor of tests/hidim_user_cases.py, statement for statement its quad_ham / quad_diss: sin phi / cos phi
                             from tables stored at construction, or np.sin(grid.xs[4]) / np.cos(grid.xs[4]) inside the callbacks
  FiveTables                 a 5-D pair that reads five stored tables (more than the kernel's four slots)
  RangeReader, DataReader, TimeReader, Fickle
                             pairs the tracer must leave on the split path: alpha from derivMin / derivMax, H from data, H from t, and a
                             hamFunc that computes something else from its second call on (hidden Python state)
  random_pair                seeded random expressions at 5-D

Every callback runs on NumPy arrays and on device tensors (the split path): coordinates and tables are made by NumPy on the host and converted
to the array type of the costates, anew at every call (a table changed in place is seen by the next call).
Grids, data and parameters are tests/hidim_cases.py's and tests/hidim_user_cases.py's: (7, 6, 8, 5, 9), (6, 5, 7, 5, 6, 8), (5, 6, 5, 7, 8, 6).
"""
import numpy as np


def like(a, ref):
    """A NumPy array in the array type of `ref` (a device tensor on the split path; anything else -- NumPy, the tracer's stand-ins -- as is)."""
    if type(ref).__module__.split(".")[0] == "torch":
        import torch
        return torch.as_tensor(np.ascontiguousarray(a), dtype=ref.dtype, device=ref.device)
    return a


def along(v, axis, nd):
    return np.asarray(v, dtype=np.float64).ravel().reshape([-1 if d == axis else 1 for d in range(nd)])


def one(v, nd):
    """A number as a one-element array that broadcasts against the grid."""
    return np.full([1] * nd, float(v))


def select(keep, k):
    """k where keep, else 0."""
    if type(k).__module__.split(".")[0] == "torch":
        import torch
        return torch.where(keep, k, torch.zeros_like(k))
    return np.where(keep, k, 0)


# ------------------------------------------------------------------------------------------ Plane5D
class PlanePair(object):
    """H = p0 (x3 cos x2) + p1 (x3 sin x2) + p2 x4 + s (a_max |p3|) + s (alpha_max |p4|), left to right; the trig from stored tables."""
    AXES = (2, 2)

    def __init__(self, grid, a_max=1.0, alpha_max=1.0, u_mode='min'):
        self.grid, self.a_max, self.alpha_max = grid, float(a_max), float(alpha_max)
        self.s = -1.0 if u_mode == 'min' else 1.0
        self.cos2 = along(np.cos(np.asarray(grid.vs[2], dtype=np.float64).ravel()), 2, 5)
        self.sin2 = along(np.sin(np.asarray(grid.vs[2], dtype=np.float64).ravel()), 2, 5)

    def hamiltonian(self, t, data, p, sd=None):
        x = self.grid.xs
        x3 = like(x[3], p[0])
        x4 = like(x[4], p[0])
        vc = x3 * like(self.cos2, p[0])
        vs = x3 * like(self.sin2, p[0])
        t0 = p[0] * vc
        t1 = p[1] * vs
        t2 = p[2] * x4
        a3 = self.a_max * abs(p[3])
        t3 = self.s * a3
        a4 = self.alpha_max * abs(p[4])
        t4 = self.s * a4
        h = t0 + t1
        h = h + t2
        h = h + t3
        h = h + t4
        return h

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        x = self.grid.xs
        if dim == 0:
            return abs(like(x[3], data) * like(self.cos2, data))
        if dim == 1:
            return abs(like(x[3], data) * like(self.sin2, data))
        if dim == 2:
            return abs(like(x[4], data))
        return self.a_max if dim == 3 else self.alpha_max


# ------------------------------------------------------------------------------------------ DubinsPair6D
class DubinsPair(object):
    """H = -( p0 (v_e cos x2) + p1 (v_e sin x2) + p3 (v_p cos x5) + p4 (v_p sin x5) + w_e |p2| - w_p |p5| ), left to right; the trig is
    np.cos(grid.xs[2]) etc. inside the callbacks (made by NumPy on the host, whatever the array type): the tracer hoists the four into tables."""
    AXES = (2, 2, 5, 5)

    def __init__(self, grid, v_e=5, v_p=5, w_e=5, w_p=5):
        self.grid, self.v_e, self.v_p, self.w_e, self.w_p = grid, float(v_e), float(v_p), float(w_e), float(w_p)

    def _a(self, ref):
        x = self.grid.xs
        a0 = self.v_e * like(np.cos(x[2]), ref)
        a1 = self.v_e * like(np.sin(x[2]), ref)
        a3 = self.v_p * like(np.cos(x[5]), ref)
        a4 = self.v_p * like(np.sin(x[5]), ref)
        return a0, a1, a3, a4

    def hamiltonian(self, t, data, p, sd=None):
        a0, a1, a3, a4 = self._a(p[0])
        t0 = p[0] * a0
        t1 = p[1] * a1
        t3 = p[3] * a3
        t4 = p[4] * a4
        t2 = self.w_e * abs(p[2])
        t5 = self.w_p * abs(p[5])
        h = t0 + t1
        h = h + t3
        h = h + t4
        h = h + t2
        h = h - t5
        return -h

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        if dim == 2:
            return self.w_e
        if dim == 5:
            return self.w_p
        a0, a1, a3, a4 = self._a(data)
        return abs({0: a0, 1: a1, 3: a3, 4: a4}[dim])


# ------------------------------------------------------------------------------------------ the planar quadrotor
class QuadTables(object):
    """tests/hidim_user_cases.py's quadrotor (par = { m, I, l, Cv, Cphi, g, Tmax, s }), statement for statement its quad_ham / quad_diss
    (the order of QUAD_SRC): parameter arithmetic in Python floats, the two divisors m and I as one-element arrays (torch divides by a Python
    scalar by multiplying with its reciprocal, which rounds differently).  Four tables along phi are made at construction, in fp64: sin phi,
    cos phi and alpha's (2 Tmax / m) |sin phi|, (2 Tmax / m) |cos phi| -- whatever the callbacks compute from stored arrays ALONE is NumPy
    arithmetic the tracer never sees, so it is done once here and rounded once to the caller's floating type, as the kernel's tables are."""
    AXES = (4, 4, 4, 4)          # in the order the expression first reads them: cos phi (ka = p3 cos phi), sin phi, u1, u3
    TRIG_INSIDE = False

    def __init__(self, grid, params):
        self.grid, self.params = grid, [float(v) for v in params]
        v4 = np.asarray(grid.vs[4], dtype=np.float64).ravel()
        self.sin4, self.cos4 = along(np.sin(v4), 4, 6), along(np.cos(v4), 4, 6)
        tmm = 2.0 * self.params[6] / self.params[0]
        self.u1, self.u3 = tmm * abs(self.sin4), tmm * abs(self.cos4)

    def trig(self, ref):
        """(sin phi, cos phi, (2 Tmax / m) |sin phi|, (2 Tmax / m) |cos phi|) in the array type of ref."""
        return like(self.sin4, ref), like(self.cos4, ref), like(self.u1, ref), like(self.u3, ref)

    def hamiltonian(self, t, data, p, sd=None):
        m, I, l, Cv, Cphi, g, Tmax, s = self.params
        x = self.grid.xs
        vx, vz, w = like(x[1], p[0]), like(x[3], p[0]), like(x[5], p[0])
        m_, I_ = like(one(m, 6), p[0]), like(one(I, 6), p[0])
        sn, cs, _, _ = self.trig(p[0])
        cvm = Cv / m
        cpi = Cphi / I
        ka = p[3] * cs
        kb = p[1] * sn
        kk = ka - kb
        k = kk / m_
        q = p[5] * l
        r = q / I_
        kp = k + r
        km = k - r
        op = select((kp < 0) if s < 0 else (kp > 0), kp)
        om = select((km < 0) if s < 0 else (km > 0), km)
        t0 = p[0] * vx
        d1 = cvm * vx
        t1 = p[1] * d1
        t2 = p[2] * vz
        d3 = cvm * vz
        e3 = d3 + g
        t3 = p[3] * e3
        t4 = p[4] * w
        d5 = cpi * w
        t5 = p[5] * d5
        t6 = Tmax * op
        t7 = Tmax * om
        h = t0 - t1
        h = h + t2
        h = h - t3
        h = h + t4
        h = h - t5
        h = h + t6
        h = h + t7
        return h

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        m, I, l, Cv, Cphi, g, Tmax, s = self.params
        x = self.grid.xs
        vx, vz, w = like(x[1], data), like(x[3], data), like(x[5], data)
        _, _, u1, u3 = self.trig(data)
        cvm = Cv / m
        cpi = Cphi / I
        if dim == 0:
            return abs(vx)
        if dim == 1:
            return abs(cvm * vx) + u1
        if dim == 2:
            return abs(vz)
        if dim == 3:
            return abs(cvm * vz + g) + u3
        if dim == 4:
            return abs(w)
        lt = l * Tmax
        lti = lt / I
        return abs(cpi * w) + lti


class QuadInline(QuadTables):
    """The same with np.sin(grid.xs[4]) / np.cos(grid.xs[4]) inside the callbacks (made by NumPy on the host, whatever the array type)."""
    TRIG_INSIDE = True
    AXES = (4, 4)                # cos phi, sin phi: hoisted; their abs() and the product with 2 Tmax / m stay device arithmetic

    def __init__(self, grid, params):
        self.grid, self.params = grid, [float(v) for v in params]

    def sincos(self, ref):
        phi = self.grid.xs[4]
        return like(np.sin(phi), ref), like(np.cos(phi), ref)

    def trig(self, ref):
        sn, cs = self.sincos(ref)
        tmm = 2.0 * self.params[6] / self.params[0]
        return sn, cs, tmm * abs(sn), tmm * abs(cs)


class QuadInlineDeviceTrig(QuadInline):
    """For the timing tool: the trig in the caller's array type (torch.sin / torch.cos of a device copy of x4 on the split path)."""

    def sincos(self, ref):
        phi = like(self.grid.xs[4], ref)
        if type(phi).__module__.split(".")[0] == "torch":
            return phi.sin(), phi.cos()
        return np.sin(phi), np.cos(phi)


# ------------------------------------------------------------------------------------------ pairs the tracer refuses
class FiveTables(PlanePair):
    """Five stored tables: one along every axis."""

    def __init__(self, grid, **kw):
        PlanePair.__init__(self, grid, **kw)
        self.gain = [along(1.0 + 0.1 * np.arange(int(n)) ** 2, d, 5) for d, n in enumerate(np.asarray(grid.N).ravel())]

    def hamiltonian(self, t, data, p, sd=None):
        h = p[0] * like(self.gain[0], p[0])
        for d in range(1, 5):
            h = h + p[d] * like(self.gain[d], p[0])
        return h

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        return abs(like(self.gain[dim], data))


class RangeReader(PlanePair):
    """alpha_3 from the costate range, as the reference's artificialDissipationGLF hands it over."""

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        if dim == 3:
            return self.a_max + 0.01 * abs(derivMax[3] - derivMin[3])
        return PlanePair.dissipation(self, t, data, derivMin, derivMax, sd, dim)


class DataReader(PlanePair):
    def hamiltonian(self, t, data, p, sd=None):
        return PlanePair.hamiltonian(self, t, data, p, sd) + 0.1 * data


class TimeReader(PlanePair):
    def hamiltonian(self, t, data, p, sd=None):
        return PlanePair.hamiltonian(self, t, data, p, sd) * (1.0 + 0.5 * t)


class Fickle(PlanePair):
    """The first call (the trace) is Plane5D; every later call has p0's term doubled -- state the tracer cannot see (a class-level counter
    behind a method the fingerprint does not walk).  The kernel traced from the first call disagrees with what the callbacks compute."""
    _calls = {}

    def hamiltonian(self, t, data, p, sd=None):
        n = Fickle._calls[id(self)] = Fickle._calls.get(id(self), 0) + 1
        # (an expression of its own: a kernel is checked once per process, expression and floating type, and PlanePair's has been)
        h = PlanePair.hamiltonian(self, t, data, p, sd) + 0.125 * p[1]
        if n > 1:
            h = h + p[0] * like(self.grid.xs[3], p[0])
        return h


# ------------------------------------------------------------------------------------------ random expressions
_UN = [np.abs, np.cos, np.sin, np.tanh, np.square, lambda v: np.sqrt(np.abs(v) + 0.5), lambda v: np.exp(-np.abs(v))]
_BIN = [np.add, np.subtract, np.multiply, np.maximum, np.minimum, lambda a, b: a / (1.5 + np.abs(b))]


def _random_program(rng, nleaf, nops):
    """A straight-line program over `nleaf` leaves: (unary index, a) or (binary index, a, b) per step; the value of the last step is the result."""
    prog = []
    for k in range(nops):
        n = nleaf + k
        if rng.random() < 0.4:
            prog.append((int(rng.integers(len(_UN))), int(rng.integers(n))))
        else:
            prog.append((int(rng.integers(len(_BIN))), int(rng.integers(n)), n - 1 if k else int(rng.integers(n))))
    return prog


def _run(prog, leaves):
    v = list(leaves)
    for st in prog:
        v.append(_UN[st[0]](v[st[1]]) if len(st) == 2 else _BIN[st[0]](v[st[1]], v[st[2]]))
    return v[-1]


class RandomPair(object):
    """H = f(x, p, c) and alpha_d = |g_d(x, c)| for seeded random straight-line programs f, g_d; c three floats."""

    def __init__(self, grid, seed):
        rng = np.random.default_rng(seed)
        self.grid, self.nd = grid, int(grid.dim)
        self.c = [float(v) for v in rng.uniform(0.3, 1.7, 3)]
        self.hprog = _random_program(rng, 2 * self.nd + 3, int(rng.integers(6, 14)))
        self.aprog = [_random_program(rng, self.nd + 3, int(rng.integers(2, 6))) for _ in range(self.nd)]

    def hamiltonian(self, t, data, p, sd=None):
        return _run(self.hprog, list(self.grid.xs) + list(p) + self.c) + 0 * p[0]

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        return np.abs(_run(self.aprog[dim], list(self.grid.xs) + self.c)) + 0 * data


def random_pair(grid, seed):
    return RandomPair(grid, seed)


# ------------------------------------------------------------------------------------------ QuadTables written by hand
def quad_hand_registration():
    """(device expression, aux_axes, parameters) of QuadTables as somebody would hand it to register_hidim_hamiltonian: QUAD_SRC of
    tests/hidim_user_cases.py with the callbacks' parameter arithmetic (Cv / m, Cphi / I and l Tmax / I arrive as parameters, computed in Python
    floats as the callbacks compute them; QUAD_SRC divides in the element type, which is the same number in fp64 only), alpha's two tables and
    the sign s = -1 resolved as the callbacks resolve it.  par = { m, I, l, Cv / m, Cphi / I, g, Tmax, l Tmax / I }; aux = cos, sin, u1, u3."""
    import hidim_user_cases as UC
    m, I, l, Cv, Cphi, g, Tmax, s = UC.QUAD_PAR
    assert s < 0
    src = "    const T SN = aux[1];\n    const T CS = aux[0];" + UC._QUAD_BODY
    for old, new in (("par[3] / par[0]", "par[3]"), ("par[4] / par[1]", "par[4]"),
                     ("par[7] < T(0) ? (kp < T(0) ? kp : T(0)) : (kp > T(0) ? kp : T(0))", "kp < T(0) ? kp : T(0)"),
                     ("par[7] < T(0) ? (km < T(0) ? km : T(0)) : (km > T(0) ? km : T(0))", "km < T(0) ? km : T(0)"),
                     ("const T u1 = tmm * fabs(SN);", "const T u1 = aux[2];"), ("const T u3 = tmm * fabs(CS);", "const T u3 = aux[3];"),
                     ("const T lti = lt / par[1];", "const T lti = par[7];")):
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    return src, (4, 4, 4, 4), [m, I, l, Cv / m, Cphi / I, g, Tmax, l * Tmax / I]
