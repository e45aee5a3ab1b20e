"""What tests/test_hidim_user_host.py and tests/test_gpu_hidim_user.py share: three systems as device expressions for
register_hidim_hamiltonian (levelsetpy_amd/hidim_ham.py).

  PLANE_SRC, PAIR_SRC   Plane5D and DubinsPair6D over tables, in the operation order of include/hj_hidim.h: under ENO2 / ENO3 they
                        must give the built-in kernels' bits.  Grids, data and parameters are tests/hidim_cases.py's.
  QUAD_SRC              a planar quadrotor, the case no built-in kernel can serve, with its NumPy restatement (quad_ham /
                        quad_diss, in the oracle's style; they also run on device tensors, for the split path).
                        State (x, vx, z, vz, phi, omega), thrusts T1, T2 in [0, Tmax] chosen by the sign s:
                            k+- = (p3 cos phi - p1 sin phi) / m +- p5 l / I
                            H = p0 vx - p1 (Cv/m) vx + p2 vz - p3 ((Cv/m) vz + g) + p4 omega - p5 (Cphi/I) omega
                                + Tmax opt_s(k+) + Tmax opt_s(k-)              opt_s = min(., 0) for s < 0, max(., 0) otherwise
                            alpha = { |vx|, |(Cv/m) vx| + (2 Tmax/m) |sin phi|, |vz|, |(Cv/m) vz + g| + (2 Tmax/m) |cos phi|,
                                      |omega|, |(Cphi/I) omega| + l Tmax / I }
                        Every sum runs left to right, one operation per statement in both restatements; sin phi and cos phi are
                        tables NumPy makes from grid.vs[4] (QUAD_TRIG_SRC: the same with device sin / cos instead).
"""
import numpy as np

from oracle import hj_oracle as O
import hidim_cases as HC

PLANE_SRC = """
    const T vc = x[3] * aux[0];
    const T vs = x[3] * aux[1];
    const T t0 = p[0] * vc;
    const T t1 = p[1] * vs;
    const T t2 = p[2] * x[4];
    const T a3 = par[0] * fabs(p[3]);
    const T t3 = par[2] * a3;
    const T a4 = par[1] * fabs(p[4]);
    const T t4 = par[2] * a4;
    T h = t0 + t1;
    h = h + t2;
    h = h + t3;
    h = h + t4;
    H = h;
    alpha[0] = fabs(vc);
    alpha[1] = fabs(vs);
    alpha[2] = fabs(x[4]);
    alpha[3] = par[0];
    alpha[4] = par[1];
"""
PLANE_AXES = (2, 2)             # aux0 = cos(vs[2]), aux1 = sin(vs[2])

PAIR_SRC = """
    const T a0 = par[0] * aux[0];
    const T a1 = par[0] * aux[1];
    const T a3 = par[1] * aux[2];
    const T a4 = par[1] * aux[3];
    const T t0 = p[0] * a0;
    const T t1 = p[1] * a1;
    const T t3 = p[3] * a3;
    const T t4 = p[4] * a4;
    const T t2 = par[2] * fabs(p[2]);
    const T t5 = par[3] * fabs(p[5]);
    T h = t0 + t1;
    h = h + t3;
    h = h + t4;
    h = h + t2;
    h = h - t5;
    H = -h;
    alpha[0] = fabs(a0);
    alpha[1] = fabs(a1);
    alpha[2] = par[2];
    alpha[3] = fabs(a3);
    alpha[4] = fabs(a4);
    alpha[5] = par[3];
"""
PAIR_AXES = (2, 2, 5, 5)        # cos(vs[2]), sin(vs[2]), cos(vs[5]), sin(vs[5])


def builtin_tables(vs):
    """The tables of PLANE_SRC / PAIR_SRC: what hidim.HiGrid makes for the built-in kernels."""
    t = [np.cos(vs[2]), np.sin(vs[2])]
    if len(vs) == 6:
        t += [np.cos(vs[5]), np.sin(vs[5])]
    return t


# ------------------------------------------------------------------------------------------ the quadrotor
# par = { m, I, l, Cv, Cphi, g, Tmax, s }
QUAD_PAR = [1.3, 0.15, 0.25, 0.4, 0.02, 9.81, 9.0, -1.0]
QUAD_AXES = (4, 4)              # aux0 = sin(vs[4]), aux1 = cos(vs[4])
_QUAD_BODY = """
    const T cvm = par[3] / par[0];
    const T cpi = par[4] / par[1];
    const T ka = p[3] * CS;
    const T kb = p[1] * SN;
    const T kk = ka - kb;
    const T k = kk / par[0];
    const T q = p[5] * par[2];
    const T r = q / par[1];
    const T kp = k + r;
    const T km = k - r;
    const T op = par[7] < T(0) ? (kp < T(0) ? kp : T(0)) : (kp > T(0) ? kp : T(0));
    const T om = par[7] < T(0) ? (km < T(0) ? km : T(0)) : (km > T(0) ? km : T(0));
    const T t0 = p[0] * x[1];
    const T d1 = cvm * x[1];
    const T t1 = p[1] * d1;
    const T t2 = p[2] * x[3];
    const T d3 = cvm * x[3];
    const T e3 = d3 + par[5];
    const T t3 = p[3] * e3;
    const T t4 = p[4] * x[5];
    const T d5 = cpi * x[5];
    const T t5 = p[5] * d5;
    const T t6 = par[6] * op;
    const T t7 = par[6] * om;
    T h = t0 - t1;
    h = h + t2;
    h = h - t3;
    h = h + t4;
    h = h - t5;
    h = h + t6;
    h = h + t7;
    H = h;
    const T tm = T(2) * par[6];
    const T tmm = tm / par[0];
    const T u1 = tmm * fabs(SN);
    const T u3 = tmm * fabs(CS);
    const T lt = par[2] * par[6];
    const T lti = lt / par[1];
    alpha[0] = fabs(x[1]);
    alpha[1] = fabs(d1) + u1;
    alpha[2] = fabs(x[3]);
    alpha[3] = fabs(e3) + u3;
    alpha[4] = fabs(x[5]);
    alpha[5] = fabs(d5) + lti;
"""
QUAD_SRC = "    const T SN = aux[0];\n    const T CS = aux[1];" + _QUAD_BODY
QUAD_TRIG_SRC = "    const T SN = sin(x[4]);\n    const T CS = cos(x[4]);" + _QUAD_BODY

QUAD_N, QUAD_PERIODIC = (5, 6, 5, 7, 8, 6), [4]


def quad_limits():
    gmin, gmax = [-2.0, -1.5, -2.2, -1.8, 0.0, -2.5], [2.1, 1.6, 2.0, 1.7, HC.TWO_PI * (1.0 - 1.0 / QUAD_N[4]), 2.4]
    return gmin, gmax, list(QUAD_N), list(QUAD_PERIODIC)


def quad_oracle_grid():
    gmin, gmax, N, pd = quad_limits()
    return O.Grid(gmin, gmax, N, pd)


def quad_data(og, seed=7):
    """hidim_cases.data's recipe (its 6-D base and its noise) on the quadrotor's grid."""
    return HC.data(og, seed)


def quad_tables(vs):
    v4 = np.asarray(vs[4], dtype=np.float64).ravel()
    return [np.sin(v4), np.cos(v4)]


def _like(a, like):
    """A NumPy array in the array type of `like` (a device tensor on the split path)."""
    if type(like).__module__.split(".")[0] == "torch":
        import torch
        return torch.as_tensor(np.ascontiguousarray(a), dtype=like.dtype, device=like.device)
    return a


def _coords(self, like):
    """vx, vz, omega, sin phi, cos phi broadcastable against the grid, made by NumPy on the host, and the two divisors m and I as one-element
    arrays (torch divides by a Python scalar by multiplying with its reciprocal, which rounds differently); cached per array type."""
    key = (type(like).__module__.split(".")[0], str(getattr(like, "device", "")))
    cache = self.__dict__.setdefault("_quad_coords", {})
    if key not in cache:
        nd = 6

        def along(v, ax):
            return np.asarray(v, dtype=np.float64).ravel().reshape([-1 if d == ax else 1 for d in range(nd)])
        vs = self.grid.vs
        phi = np.asarray(vs[4], dtype=np.float64).ravel()
        one = lambda v: np.full([1] * nd, float(v))      # noqa: E731
        c = (along(vs[1], 1), along(vs[3], 3), along(vs[5], 5), along(np.sin(phi), 4), along(np.cos(phi), 4), one(self.params[0]), one(self.params[1]))
        cache[key] = tuple(_like(a, like) for a in c)
    return cache[key]


def _select(keep, k):
    """k where keep, else 0: opt_s written as the kernel's selection (min(k, 0) is keep = k < 0, max(k, 0) is keep = k > 0)."""
    if isinstance(k, np.ndarray):
        return np.where(keep, k, 0.0)
    import torch
    return torch.where(keep, k, torch.zeros_like(k))


def quad_ham(self, t, data, p, sd=None):
    m, I, l, Cv, Cphi, g, Tmax, s = self.params
    vx, vz, w, sn, cs, m_, I_ = _coords(self, p[0])
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
    op = _select((kp < 0) if s < 0 else (kp > 0), kp)
    om = _select((km < 0) if s < 0 else (km > 0), km)
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


def quad_diss(self, t, data, derivMin, derivMax, sd, dim):
    m, I, l, Cv, Cphi, g, Tmax, s = self.params
    vx, vz, w, sn, cs, m_, I_ = _coords(self, data)
    cvm = Cv / m
    cpi = Cphi / I
    tm = 2.0 * Tmax
    tmm = tm / m
    if dim == 0:
        return abs(vx)
    if dim == 1:
        return abs(cvm * vx) + tmm * abs(sn)
    if dim == 2:
        return abs(vz)
    if dim == 3:
        return abs(cvm * vz + g) + tmm * abs(cs)
    if dim == 4:
        return abs(w)
    lt = l * Tmax
    lti = lt / I
    return abs(cpi * w) + lti


class QuadOracle(object):
    """The quadrotor for the NumPy oracle: the restated callbacks on an oracle grid."""

    def __init__(self, grid, params=QUAD_PAR):
        self.grid, self.params = grid, [float(v) for v in params]

    def hamiltonian(self, t, data, p, sd=None):
        return quad_ham(self, t, data, p, sd)

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        return quad_diss(self, t, data, derivMin, derivMax, sd, dim)
