"""What tests/test_plant_host.py and tests/test_gpu_plant.py share -- TEST INFRASTRUCTURE, NOT PRODUCT: plants as device statements for
register_plant (levelsetpy_amd/plant.py) and their NumPy restatements for tests/rollout_ref.py, whose PLANTS table is extended here, at
import (rollout_ref passes c0 / c1 through untouched: a tuple of controls and a tuple of disturbances fit).

  BUILTIN     the five built-in plants again, in the operation order of include/hj_rollout.h / include/hj_hiquery.h (csrc/hj_rollout.hip,
              csrc/hj_hiquery.hip): user_rollout_kernel around them must give rollout_kernel's / hi_rollout_kernel's bits.  Their
              restatements are rollout_ref's and hiquery_cases'.
  QUAD_*      the planar quadrotor of tests/hidim_user_cases.py (quad_ham), the case no built-in kernel serves.  State (x, vx, z, vz, phi,
              omega), thrusts T1, T2 in [0, Tmax], par = QUAD_PAR (its last slot, the Hamiltonian's sign, is not read: the rollout takes
              uMode from its caller).  H = p . f with
                  f = (vx, -(Cv/m) vx - (T1 + T2) sin phi / m, vz, -((Cv/m) vz + g) + (T1 + T2) cos phi / m, omega, -(Cphi/I) omega + l (T1 - T2) / I)
              so the thrusts enter as T1 k+ + T2 k-, k+- = (p3 cos phi - p1 sin phi) / m +- p5 l / I (quad_ham's kp / km, in its
              operation order), and T1 = (Tmax / 2) (1 -+ sgn(k+)) for uMode 'min' / 'max', T2 the same with k-: through sgn, so a NaN
              costate gives NaN thrusts.
  LIN_*       four states, three controls, two disturbances, linear, no trigonometry: it exists to exercise the control vector.
                  u0 = b0 sgn(p0), u1 = b1 sgn(p1), u2 = b2 sgn(p3), d0 = e0 sgn(p2), d1 = e1 sgn(p0 + p3)    ('max'; negated for 'min')
                  f = ((x1 + u0) + d1, u1 - 0.5 x0, x3 + d0, (u2 + d1) - 0.25 x2)
"""
import numpy as np

import hidim_user_cases as UC
import hiquery_cases as XC                      # noqa: F401  (adds plane5d / pair6d to rollout_ref.PLANTS)
import rollout_ref as R

# name -> (dim, controls_src, dynamics_src, ncontrols, ndisturbances, nparams)
BUILTIN = {
    "dubins": (3, """
        const double w = par[2];
        const double s1 = p[0] * x[1];
        const double s2 = p[1] * x[0];
        double s = s1 - s2;
        s = s - p[2];
        u[0] = w * sgn(s);
        if (!u_max) u[0] = -u[0];
        dst[0] = w * sgn(p[2]);
        if (!d_max) dst[0] = -dst[0];
    """, """
        const double ve = par[0], vp = par[1];
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        const double vc = vp * c;
        const double drift = -ve + vc;
        const double ax2 = u[0] * x[1];
        dx[0] = drift + ax2;
        const double vs = vp * s;
        const double ax1 = u[0] * x[0];
        dx[1] = vs - ax1;
        dx[2] = dst[0] - u[0];
    """, 1, 1, 3),
    "integrator": (2, """
        u[0] = par[0] * sgn(p[1]);
        if (!u_max) u[0] = -u[0];
    """, """
        dx[0] = x[1];
        dx[1] = u[0];
    """, 1, 0, 1),
    "pendulum": (4, """
        u[0] = par[0] * sgn(p[1]);
        u[1] = par[0] * sgn(p[3]);
        if (!u_max) { u[0] = -u[0]; u[1] = -u[1]; }
    """, """
        constexpr double G = 9.8, L1 = 1.0, L2 = 1.0, M1 = 1.0, M2 = 1.0;
        const double w1 = x[1], w2 = x[3];
        const double s1 = sin(x[0]), c1 = cos(x[0]), s2 = sin(x[2]), c2 = cos(x[2]);
        const double a0 = s2 * c1, a1 = c2 * s1;
        const double sd = a0 - a1;
        const double b0 = c2 * c1, b1 = s2 * s1;
        const double cd = b0 + b1;
        const double m12 = M1 + M2;
        double t = M2 * L1; t = t * cd; t = t * cd;
        const double den1 = m12 * L1 - t;
        double q1 = M2 * L1; q1 = q1 * w1; q1 = q1 * w1; q1 = q1 * sd; q1 = q1 * cd;
        double q2 = M2 * G; q2 = q2 * s2; q2 = q2 * cd;
        double q3 = M2 * L2; q3 = q3 * w2; q3 = q3 * w2; q3 = q3 * sd;
        double q4 = m12 * G; q4 = q4 * s1;
        double n1 = q1 + q2; n1 = n1 + q3; n1 = n1 - q4;
        const double f1 = n1 / den1;
        const double den2 = (L2 / L1) * den1;
        double r1 = -M2 * L2; r1 = r1 * w2; r1 = r1 * w2; r1 = r1 * sd; r1 = r1 * cd;
        double r2 = m12 * G; r2 = r2 * s1; r2 = r2 * cd;
        double r3 = m12 * L1; r3 = r3 * w1; r3 = r3 * w1; r3 = r3 * sd;
        double r4 = m12 * G; r4 = r4 * s2;
        double n3 = r1 + r2; n3 = n3 - r3; n3 = n3 - r4;
        const double f3 = n3 / den2;
        dx[0] = w1;
        dx[1] = f1 + u[0];
        dx[2] = w2;
        dx[3] = f3 + u[1];
    """, 2, 0, 1),
    "plane5d": (5, """
        u[0] = par[0] * sgn(p[3]);
        u[1] = par[1] * sgn(p[4]);
        if (!u_max) { u[0] = -u[0]; u[1] = -u[1]; }
    """, """
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        dx[0] = x[3] * c;
        dx[1] = x[3] * s;
        dx[2] = x[4];
        dx[3] = u[0];
        dx[4] = u[1];
    """, 2, 0, 2),
    "pair6d": (6, """
        u[0] = par[2] * sgn(p[2]);
        if (!u_max) u[0] = -u[0];
        dst[0] = par[3] * sgn(p[5]);
        if (!d_max) dst[0] = -dst[0];
    """, """
        const double ve = par[0], vp = par[1];
        const double c2 = cos(x[2]);
        const double s2 = sin(x[2]);
        const double c5 = cos(x[5]);
        const double s5 = sin(x[5]);
        dx[0] = ve * c2;
        dx[1] = ve * s2;
        dx[2] = u[0];
        dx[3] = vp * c5;
        dx[4] = vp * s5;
        dx[5] = dst[0];
    """, 1, 1, 4),
}
BUILTIN_ID = {"dubins": 0, "integrator": 1, "pendulum": 2, "plane5d": 50, "pair6d": 51}
# the restatement's parameters: what test_gpu_rollout.plant_of / hiquery_cases.PLANT_PAR use
BUILTIN_PAR = {"dubins": (0.75, 0.75, 1.5), "integrator": (0.8,), "pendulum": (1.25,), "plane5d": XC.PLANT_PAR["plane5d"],
               "pair6d": XC.PLANT_PAR["pair6d"]}


def register_builtin(name):
    import levelsetpy_amd as L
    dim, ctl, dyn, nu, nd, npar = BUILTIN[name]
    return L.register_plant(name + "_again", dim, ctl, dyn, nu, nd, npar)


def builtin_system(name, g, par=None):
    """The package's own system (the restatement's parameters)."""
    import levelsetpy_amd as L
    par = BUILTIN_PAR[name] if par is None else par
    if name == "dubins":
        assert par[0] == par[1]
        return L.DubinsVehicleRel(g, par[0], par[2])
    if name == "integrator":
        return L.DoubleIntegrator(g, par[0])
    if name == "pendulum":
        return L.DoublePendulum4D(g, par[0])
    return L.Plane5D(g, par[0], par[1]) if name == "plane5d" else L.DubinsPair6D(g, *par)


def wrapped(reg, system, par):
    """A PlantSystem whose Python callables are the built-in system's own methods: the host loop runs THEM, the kernel the registration."""
    return reg(par, dynamics=lambda s, t, x, u, d: system.dynamics(t, x, u, d), get_opt_u=lambda s, t, p, m, x: system.get_opt_u(t, p, m, x),
               get_opt_v=lambda s, t, p, m, x: system.get_opt_v(t, p, m, x))


# ------------------------------------------------------------------------------------------ the quadrotor
QUAD_PAR = list(UC.QUAD_PAR)
QUAD_CONTROLS = """
    const double cs = cos(x[4]);
    const double sn = sin(x[4]);
    const double ka = p[3] * cs;
    const double kb = p[1] * sn;
    const double kk = ka - kb;
    const double k = kk / par[0];
    const double q = p[5] * par[2];
    const double r = q / par[1];
    const double kp = k + r;
    const double km = k - r;
    const double half = 0.5 * par[6];
    const double sp = sgn(kp);
    const double sm = sgn(km);
    const double hp = u_max ? 1.0 + sp : 1.0 - sp;
    const double hm = u_max ? 1.0 + sm : 1.0 - sm;
    u[0] = half * hp;
    u[1] = half * hm;
"""
QUAD_DYNAMICS = """
    const double cvm = par[3] / par[0];
    const double cpi = par[4] / par[1];
    const double cs = cos(x[4]);
    const double sn = sin(x[4]);
    const double tt = u[0] + u[1];
    const double tm = tt / par[0];
    const double d1 = cvm * x[1];
    const double a1 = tm * sn;
    dx[0] = x[1];
    dx[1] = -d1 - a1;
    dx[2] = x[3];
    const double d3 = cvm * x[3];
    const double e3 = d3 + par[5];
    const double a3 = tm * cs;
    dx[3] = a3 - e3;
    dx[4] = x[5];
    const double d5 = cpi * x[5];
    const double td = u[0] - u[1];
    const double lt = par[2] * td;
    const double li = lt / par[1];
    dx[5] = li - d5;
"""


def quad_controls(par, P, X, uMode, dMode):
    m, I, l, Cv, Cphi, g, Tmax = par[:7]
    cs = np.cos(X[:, 4])
    sn = np.sin(X[:, 4])
    ka = P[:, 3] * cs
    kb = P[:, 1] * sn
    kk = ka - kb
    k = kk / m
    q = P[:, 5] * l
    r = q / I
    kp = k + r
    km = k - r
    half = 0.5 * Tmax
    sp, sm = R.sgn(kp), R.sgn(km)
    hp = (1.0 + sp) if uMode == 'max' else (1.0 - sp)
    hm = (1.0 + sm) if uMode == 'max' else (1.0 - sm)
    return (half * hp, half * hm), (), [kp, km]


def quad_f(par, X, u, d):
    m, I, l, Cv, Cphi, g, Tmax = par[:7]
    cvm = Cv / m
    cpi = Cphi / I
    cs = np.cos(X[:, 4])
    sn = np.sin(X[:, 4])
    tt = u[0] + u[1]
    tm = tt / m
    d1 = cvm * X[:, 1]
    a1 = tm * sn
    f1 = -d1 - a1
    d3 = cvm * X[:, 3]
    e3 = d3 + g
    a3 = tm * cs
    f3 = a3 - e3
    d5 = cpi * X[:, 5]
    td = u[0] - u[1]
    lt = l * td
    li = lt / I
    f5 = li - d5
    return np.stack([X[:, 1], f1, X[:, 3], f3, X[:, 5], f5], axis=1)


def quad_get_opt_u(self, t, deriv, uMode, x):
    """The restatement at one state: what a user would write as the object's own method."""
    c, _, _ = quad_controls(self.params, np.asarray(deriv, dtype=np.float64).reshape(1, 6), np.asarray(x, dtype=np.float64).reshape(1, 6), uMode, None)
    return float(c[0][0]), float(c[1][0])


def quad_dynamics(self, t, x, u, d=None):
    return quad_f(self.params, np.asarray(x, dtype=np.float64).reshape(1, 6), (np.array([float(u[0])]), np.array([float(u[1])])), ())[0]


class Quadrotor(object):
    """A user's own class: the callback protocol of the solver (hamiltonian / dissipation: hidim_user_cases' restatement) AND the dynSys
    protocol of computeOptTraj.  Both registrations can be attached to one instance."""
    x = None

    def __init__(self, grid, params=None):
        self.grid, self.params = grid, [float(v) for v in (QUAD_PAR if params is None else params)]

    def hamiltonian(self, t, data, p, sd=None):
        return UC.quad_ham(self, t, data, p, sd)

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        return UC.quad_diss(self, t, data, derivMin, derivMax, sd, dim)

    def dynamics(self, t, x, u, d=None):
        return quad_dynamics(self, t, x, u, d)

    def get_opt_u(self, t, deriv, uMode, x):
        return quad_get_opt_u(self, t, deriv, uMode, x)

    def get_opt_v(self, t, deriv, dMode, x):
        return None

    def update_state(self, u, dt, x, d=None):
        from levelsetpy_amd.dynamics import _rk4
        self.x = _rk4(lambda z: self.dynamics(None, z, u), x, dt)
        return self.x


def register_quad_hamiltonian():
    import levelsetpy_amd as L
    return L.register_hidim_hamiltonian("planar_quad", 6, UC.QUAD_SRC, nparams=8, aux_axes=UC.QUAD_AXES)


def quadrotor(g):
    """One object, both registrations attached: it solves fused and rolls out fused."""
    q = Quadrotor(g)
    register_quad_hamiltonian().attach(q, params=lambda o: o.params, tables=UC.quad_tables(g.vs))
    register_quad().attach(q, params=lambda o: o.params)
    return q


def register_quad():
    import levelsetpy_amd as L
    return L.register_plant("planar_quad", 6, QUAD_CONTROLS, QUAD_DYNAMICS, ncontrols=2, nparams=8)


def quad_grids():
    import levelsetpy_amd as L
    gmin, gmax, N, pd = UC.quad_limits()
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd), UC.quad_oracle_grid()


# the whole-horizon case: reach a disc in the (x, z) plane, the thrusts minimising (QUAD_PAR's sign), ENO2, five time stamps
QUAD_TAU = np.linspace(0.0, 0.16, 5)


def quad_target(og):
    """A disc of radius 1.1 around (0.2, -0.1) in (x, z), with hidim_cases' kind of noise so that no ENO choice ties."""
    x = og.xs
    rng = np.random.default_rng(13)
    return np.sqrt((x[0] - 0.2) ** 2 + (x[2] + 0.1) ** 2 + 0.01) - 1.1 + 0.02 * rng.standard_normal(og.shape)


def quad_states(og, M=64):
    """M states from a fixed seed, positions within 1.9 of the disc's centre; the first eight next to the upper edge of the x axis,
    moving towards it (those leave the grid)."""
    rng = np.random.default_rng(21)
    lo = np.array([float(np.asarray(v).ravel()[0]) for v in og.vs])
    hi = np.array([float(np.asarray(v).ravel()[-1]) for v in og.vs])
    xs = lo + (0.15 + 0.7 * rng.random((M, 6))) * (hi - lo)
    xs[:8, 0] = hi[0] - 0.01 * (1 + np.arange(8))
    xs[:8, 1] = 0.6 + 0.1 * np.arange(8)
    return xs


R.PLANTS.update({"quad": (quad_controls, quad_f, 6)})


# ------------------------------------------------------------------------------------------ three controls, two disturbances
LIN_PAR = (0.7, 1.1, 0.4, 0.9, 0.3)
LIN_CONTROLS = """
    u[0] = par[0] * sgn(p[0]);
    u[1] = par[1] * sgn(p[1]);
    u[2] = par[2] * sgn(p[3]);
    if (!u_max) { u[0] = -u[0]; u[1] = -u[1]; u[2] = -u[2]; }
    const double s = p[0] + p[3];
    dst[0] = par[3] * sgn(p[2]);
    dst[1] = par[4] * sgn(s);
    if (!d_max) { dst[0] = -dst[0]; dst[1] = -dst[1]; }
"""
LIN_DYNAMICS = """
    const double t0 = x[1] + u[0];
    dx[0] = t0 + dst[1];
    const double a = 0.5 * x[0];
    dx[1] = u[1] - a;
    dx[2] = x[3] + dst[0];
    const double t3 = u[2] + dst[1];
    const double b = 0.25 * x[2];
    dx[3] = t3 - b;
"""


def lin_controls(par, P, X, uMode, dMode):
    u = [par[0] * R.sgn(P[:, 0]), par[1] * R.sgn(P[:, 1]), par[2] * R.sgn(P[:, 3])]
    if uMode == 'min':
        u = [-v for v in u]
    s = P[:, 0] + P[:, 3]
    d = [par[3] * R.sgn(P[:, 2]), par[4] * R.sgn(s)]
    if dMode == 'min':
        d = [-v for v in d]
    return tuple(u), tuple(d), [P[:, 0], P[:, 1], P[:, 3], P[:, 2], s]


def lin_f(par, X, u, d):
    t0 = X[:, 1] + u[0]
    f0 = t0 + d[1]
    a = 0.5 * X[:, 0]
    f1 = u[1] - a
    f2 = X[:, 3] + d[0]
    t3 = u[2] + d[1]
    b = 0.25 * X[:, 2]
    f3 = t3 - b
    return np.stack([f0, f1, f2, f3], axis=1)


def register_lin():
    import levelsetpy_amd as L
    return L.register_plant("lin_3u2d", 4, LIN_CONTROLS, LIN_DYNAMICS, ncontrols=3, ndisturbances=2, nparams=5)


R.PLANTS.update({"lin": (lin_controls, lin_f, 4)})
