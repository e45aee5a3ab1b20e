"""Problem callbacks with a native (fused-kernel) implementation:
DubinsVehicleRel (reference DynamicalSystems/dubins_relative.py:12), DoubleIntegrator
(double_integrator.py:9), the build-defined DoublePendulum4D (BASELINE config C5), and the 5-D / 6-D systems
Plane5D and DubinsPair6D, whose kernels live in libhj_hidim.so (include/hj_hidim.h, hidim.py).

Each class keeps the reference's callback protocol -- `.hamiltonian(t, data, derivs, sd)` and
`.dissipation(t, data, derivMin, derivMax, sd, dim)` work on NumPy arrays or torch tensors, for
use with foreign terms / dissipation functions -- and additionally advertises `native()` =
(ham_id, params): termLaxFriedrichs and odeCFLn then run the fused HIP kernels instead of
calling back into Python.

Each class also implements the dynSys protocol of computeOptTraj -- attribute `x`, dynamics(t, x, u, d),
get_opt_u(t, deriv, uMode, x), get_opt_v(t, deriv, dMode, x), update_state(u, dt, x, d) -- with the dynamics its own
Hamiltonian is the optimum of.  One state at a time, in fp64, one operation per statement: rollout_kernel
(csrc/hj_rollout.hip) restates these methods, so computeOptTrajs and computeOptTraj give the same bits.
"""
import numpy as np

from . import _ffi, _hffi
from .context import is_tensor

__all__ = ["DubinsVehicleRel", "DoubleIntegrator", "DoublePendulum4D", "Plane5D", "DubinsPair6D", "native_of", "native_again", "native_plant",
           "native_plant_hi"]


def native_again(system):
    """(ham_id, params) of a system object as of NOW (its speeds / parameters may have been changed in place), None if it
    is not native any more: what a cached plan is re-validated with (term.native_plan)."""
    att = getattr(system, "_hj_native", None)
    if att is not None:
        par = att.params(system)            # (a traced pair re-traces here and may change its registration: the id is read after)
        return att.reg.ham_id, par
    return system.native()


def _sgn(s):
    """+1 for s >= 0, -1 for s < 0, NaN for NaN: an exact zero is deterministic, a NaN costate poisons the state."""
    s = float(s)
    return 1.0 if s >= 0 else (-1.0 if s < 0 else float('nan'))


def _mode(mode, default=None):
    if mode is None and default is not None:
        mode = default
    if mode not in ('min', 'max'):
        raise ValueError("mode must be 'min' or 'max', not %r" % (mode,))
    return mode


def _state(x):
    return np.asarray(x, dtype=np.float64).ravel()


def _rk4(f, x, dt):
    """One classical RK4 step of xdot = f(x): h = .5 dt, k2 = f(x + h k1), ..., x + dt/6 (k1 + 2 k2 + 2 k3 + k4) left to
    right.  f returns an fp64 array; every array operation here is one rounding per element."""
    x = _state(x)
    h = .5 * dt
    k1 = f(x)
    k2 = f(x + h * k1)
    k3 = f(x + h * k2)
    k4 = f(x + dt * k3)
    return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def _xs(grid, i, like):
    """grid.xs[i] in the array type of `like`."""
    x = grid.xs[i]
    if is_tensor(like):
        import torch
        cache = grid.__dict__.setdefault("_hj_xs_t", {})
        key = (i, like.device, like.dtype)
        if key not in cache:
            cache[key] = torch.as_tensor(np.asarray(x), dtype=like.dtype, device=like.device)
        return cache[key]
    return np.asarray(x)


def _abs(a):
    return a.abs() if is_tensor(a) else np.abs(a)


def _cos(a):
    return a.cos() if is_tensor(a) else np.cos(a)


def _sin(a):
    return a.sin() if is_tensor(a) else np.sin(a)


class DubinsVehicleRel(object):
    """Two Dubins vehicles in relative coordinates (dubins_relative.py:13-61 for the speed
    conventions: v(u)=u*u_bound, w(u)=u*w_bound; scalar bounds give v_e=v_p, w_e=w_p)."""

    def __init__(self, grid, u_bound=5, w_bound=5, x=None):
        self.grid = grid
        self.cur_state = x if x is not None else grid.xs
        self.v = lambda u: u * u_bound
        self.w = lambda w: w * w_bound
        if not np.isscalar(u_bound) and len(u_bound) > 1:
            self.v_e, self.v_p = self.v(1), self.v(-1)
        else:
            self.v_e = self.v_p = self.v(1)
        if not np.isscalar(w_bound) and len(w_bound) > 1:
            self.w_e, self.w_p = self.w(1), self.w(-1)
        else:
            self.w_e = self.w_p = self.w(1)
        self._scalar = np.isscalar(u_bound) and np.isscalar(w_bound)

    def native(self):
        if not self._scalar or self.grid.dim != 3:
            return None
        return _ffi.HAM_DUBINS_REL, [float(self.v_e), float(self.v_p), float(self.w(1)),
                                     float(self.w_e + self.w_p)]

    def hamiltonian(self, t, data, value_derivs, finite_diff_bundle=None):
        """dubins_relative.py:83-90."""
        p1, p2, p3 = value_derivs[0], value_derivs[1], value_derivs[2]
        x1, x2, x3 = (_xs(self.grid, i, p1) for i in range(3))
        p1_coeff = self.v_e - self.v_p * _cos(x3)
        p2_coeff = self.v_p * _sin(x3)
        return (p1 * p1_coeff - p2 * p2_coeff - self.w(1) * _abs(p1 * x2 - p2 * x1 - p3)
                + self.w(1) * _abs(p3))

    def dissipation(self, t, data, derivMin, derivMax, schemeData, dim):
        """dubins_relative.py:104-111."""
        assert dim >= 0 and dim < 3, "Dubins vehicle dimension has to between 0 and 2 inclusive."
        if dim == 0:
            return _abs(self.v_e - self.v_p * _cos(_xs(self.grid, 2, data))) + _abs(self.w(1) * _xs(self.grid, 1, data))
        if dim == 1:
            return _abs(self.v_p * _sin(_xs(self.grid, 2, data))) + _abs(self.w(1) * _xs(self.grid, 0, data))
        return self.w_e + self.w_p

    # ---- the dynSys protocol (scalar bounds): u = a, the evader's turn rate; d = b, the pursuer's.  H = -max_a min_b p.f
    x = None

    def _need_scalar(self):
        if not self._scalar:
            raise ValueError('DubinsVehicleRel: the dynSys protocol needs scalar u_bound and w_bound')

    def dynamics(self, t, x, u, d):
        self._need_scalar()
        x = _state(x)
        a, b = float(u), float(d)
        x1, x2, x3 = float(x[0]), float(x[1]), float(x[2])
        ve, vp = float(self.v_e), float(self.v_p)
        vc = vp * float(np.cos(x3))
        drift = -ve + vc
        ax2 = a * x2
        f1 = drift + ax2
        vs = vp * float(np.sin(x3))
        ax1 = a * x1
        f2 = vs - ax1
        f3 = b - a
        return np.array([f1, f2, f3])

    def get_opt_u(self, t, deriv, uMode, x):
        self._need_scalar()
        x = _state(x)
        p1, p2, p3 = float(deriv[0]), float(deriv[1]), float(deriv[2])
        s1 = p1 * float(x[1])
        s2 = p2 * float(x[0])
        s = s1 - s2
        s = s - p3
        a = float(self.w(1)) * _sgn(s)
        return a if _mode(uMode) == 'max' else -a

    def get_opt_v(self, t, deriv, dMode, x):
        """dMode None: 'min', the pursuer of the class's own Hamiltonian."""
        self._need_scalar()
        b = float(self.w(1)) * _sgn(deriv[2])
        return b if _mode(dMode, 'min') == 'max' else -b

    def update_state(self, u, dt, x, d=None):
        d = 0.0 if d is None else d
        self.x = _rk4(lambda z: self.dynamics(None, z, u, d), x, dt)
        return self.x


class DoubleIntegrator(object):
    """double_integrator.py:9: xddot = u, |u| <= u_bound."""

    def __init__(self, grid, u_bound=1):
        self.grid = grid
        self.control_law = u_bound

    def native(self):
        if self.grid.dim != 2 or not np.isscalar(self.control_law):
            return None
        return _ffi.HAM_DOUBLE_INTEGRATOR, [float(self.control_law), 0.0, 0.0, 0.0]

    @property
    def switching_curve(self):
        x2 = np.asarray(self.grid.xs[1])
        return -.5 * x2 * np.abs(x2)                       # :44-47

    def hamiltonian(self, t, data, value_derivs, finite_diff_bundle=None):
        x2 = _xs(self.grid, 1, value_derivs[0])
        return -(value_derivs[0] * x2 - _abs(value_derivs[1]) * self.control_law)   # :71-74

    def dissipation(self, t, data, derivMin, derivMax, schemeData, dim):
        return [_abs(_xs(self.grid, 1, data)), abs(self.control_law)][dim]           # :84-89

    def mttr(self):
        """Closed-form minimum time to reach the origin (double_integrator.py:91-119)."""
        x1, x2 = np.asarray(self.grid.xs[0]), np.asarray(self.grid.xs[1])
        gamma = self.switching_curve
        above, below, on = x1 > gamma, x1 < gamma, x1 == gamma
        t1 = (x2 + np.emath.sqrt(4 * x1 + 2 * x2 ** 2)) * above
        t2 = (-x2 + np.emath.sqrt(-4 * x1 + 2 * x2 ** 2)) * below
        t3 = np.abs(x2) * on
        return (t1 + t2 + t3).real

    # ---- the dynSys protocol: f = (x2, u), no disturbance
    x = None

    def dynamics(self, t, x, u, d=None):
        x = _state(x)
        return np.array([float(x[1]), float(u)])

    def get_opt_u(self, t, deriv, uMode, x):
        u = float(self.control_law) * _sgn(deriv[1])
        return u if _mode(uMode) == 'max' else -u

    def get_opt_v(self, t, deriv, dMode, x):
        return None

    def update_state(self, u, dt, x, d=None):
        self.x = _rk4(lambda z: self.dynamics(None, z, u), x, dt)
        return self.x


class DoublePendulum4D(object):
    """Build-defined 4-D Hamiltonian (the reference ships none; BASELINE config C5).  State
    (th1, w1, th2, w2); drift of the frictionless double pendulum with unit masses and lengths,
    g = 9.8 (the dynamics written out in the reference's Tests/double_pendulum.py:29-51), torque
    control |u| <= u_max on both angular accelerations:
        H = sum_i p_i f_i(x) + u_max(|p_2| + |p_4|),   alpha_i = |f_i| + u_max [i in {1,3}]."""
    G, L1, L2, M1, M2 = 9.8, 1.0, 1.0, 1.0, 1.0

    def __init__(self, grid, u_max=1.0):
        self.grid = grid
        self.u_max = u_max

    def native(self):
        if self.grid.dim != 4:
            return None
        return _ffi.HAM_DOUBLE_PENDULUM, [float(self.u_max), 0.0, 0.0, 0.0]

    def _drift(self, like):
        th1, w1, th2, w2 = (_xs(self.grid, i, like) for i in range(4))
        G, L1, L2, M1, M2 = self.G, self.L1, self.L2, self.M1, self.M2
        s1, c1, s2, c2 = _sin(th1), _cos(th1), _sin(th2), _cos(th2)
        sd, cd = s2 * c1 - c2 * s1, c2 * c1 + s2 * s1
        den1 = (M1 + M2) * L1 - M2 * L1 * cd * cd
        f1 = (M2 * L1 * w1 * w1 * sd * cd + M2 * G * s2 * cd + M2 * L2 * w2 * w2 * sd
              - (M1 + M2) * G * s1) / den1
        den2 = (L2 / L1) * den1
        f3 = (-M2 * L2 * w2 * w2 * sd * cd + (M1 + M2) * G * s1 * cd
              - (M1 + M2) * L1 * w1 * w1 * sd - (M1 + M2) * G * s2) / den2
        return [w1 + 0 * th1, f1, w2 + 0 * th1, f3]

    def hamiltonian(self, t, data, p, sd=None):
        f = self._drift(p[0])
        return (p[0] * f[0] + p[1] * f[1] + p[2] * f[2] + p[3] * f[3]
                + self.u_max * (_abs(p[1]) + _abs(p[3])))

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        return _abs(self._drift(data)[dim]) + (self.u_max if dim in (1, 3) else 0.0)

    # ---- the dynSys protocol: f = drift(x) + (0, u1, 0, u2), u = (u1, u2), no disturbance
    x = None

    def dynamics(self, t, x, u, d=None):
        """The drift at ONE state, in the expression order of _drift (products and sums left to right)."""
        x = _state(x)
        th1, w1, th2, w2 = float(x[0]), float(x[1]), float(x[2]), float(x[3])
        G, L1, L2, M1, M2 = self.G, self.L1, self.L2, self.M1, self.M2
        s1, c1, s2, c2 = float(np.sin(th1)), float(np.cos(th1)), float(np.sin(th2)), float(np.cos(th2))
        sd, cd = s2 * c1 - c2 * s1, c2 * c1 + s2 * s1
        den1 = (M1 + M2) * L1 - M2 * L1 * cd * cd
        f1 = (M2 * L1 * w1 * w1 * sd * cd + M2 * G * s2 * cd + M2 * L2 * w2 * w2 * sd
              - (M1 + M2) * G * s1) / den1
        den2 = (L2 / L1) * den1
        f3 = (-M2 * L2 * w2 * w2 * sd * cd + (M1 + M2) * G * s1 * cd
              - (M1 + M2) * L1 * w1 * w1 * sd - (M1 + M2) * G * s2) / den2
        return np.array([w1, f1 + float(u[0]), w2, f3 + float(u[1])])

    def get_opt_u(self, t, deriv, uMode, x):
        u1 = float(self.u_max) * _sgn(deriv[1])
        u2 = float(self.u_max) * _sgn(deriv[3])
        return (u1, u2) if _mode(uMode) == 'max' else (-u1, -u2)

    def get_opt_v(self, t, deriv, dMode, x):
        return None

    def update_state(self, u, dt, x, d=None):
        self.x = _rk4(lambda z: self.dynamics(None, z, u), x, dt)
        return self.x


class Plane5D(object):
    """A planar vehicle with speed and turn rate as states: (x, y, theta, v, omega) with xdot = v cos theta,
    ydot = v sin theta, thetadot = omega, vdot = a, omegadot = alpha, |a| <= a_max, |alpha| <= alpha_max.  u_mode 'min':
    the controls minimise (s = -1), 'max': they maximise (s = +1):
        H = p0 (x3 cos x2) + p1 (x3 sin x2) + p2 x4 + s (a_max |p3|) + s (alpha_max |p4|)      summed left to right
        alpha = { |x3 cos x2|, |x3 sin x2|, |x4|, a_max, alpha_max }
    hidim_substep_kernel<T, HamPlane5D, SCHEME> (csrc/hj_hidim.hip) restates these expressions operation by operation."""

    def __init__(self, grid, a_max=1.0, alpha_max=1.0, u_mode='min'):
        self.grid = grid
        self.a_max = a_max
        self.alpha_max = alpha_max
        self.u_mode = _mode(u_mode)

    def _s(self):
        return -1.0 if self.u_mode == 'min' else 1.0

    def native(self):
        if self.grid.dim != 5 or not (np.isscalar(self.a_max) and np.isscalar(self.alpha_max)) or self.u_mode not in ('min', 'max'):
            return None
        return _hffi.HAM_PLANE5D, [float(self.a_max), float(self.alpha_max), self._s(), 0.0]

    def hamiltonian(self, t, data, value_derivs, finite_diff_bundle=None):
        p = value_derivs
        x2, x3, x4 = (_xs(self.grid, i, p[0]) for i in (2, 3, 4))
        s = self._s()
        return (p[0] * (x3 * _cos(x2)) + p[1] * (x3 * _sin(x2)) + p[2] * x4 + s * (self.a_max * _abs(p[3]))
                + s * (self.alpha_max * _abs(p[4])))

    def dissipation(self, t, data, derivMin, derivMax, schemeData, dim):
        assert 0 <= dim < 5, "Plane5D has dimensions 0 to 4."
        if dim == 0:
            return _abs(_xs(self.grid, 3, data) * _cos(_xs(self.grid, 2, data)))
        if dim == 1:
            return _abs(_xs(self.grid, 3, data) * _sin(_xs(self.grid, 2, data)))
        if dim == 2:
            return _abs(_xs(self.grid, 4, data))
        return self.a_max if dim == 3 else self.alpha_max

    # ---- the dynSys protocol: u = (a, alpha), no disturbance
    x = None

    def dynamics(self, t, x, u, d=None):
        x = _state(x)
        th, v, om = float(x[2]), float(x[3]), float(x[4])
        return np.array([v * float(np.cos(th)), v * float(np.sin(th)), om, float(u[0]), float(u[1])])

    def get_opt_u(self, t, deriv, uMode, x):
        a = float(self.a_max) * _sgn(deriv[3])
        al = float(self.alpha_max) * _sgn(deriv[4])
        return (a, al) if _mode(uMode, self.u_mode) == 'max' else (-a, -al)

    def get_opt_v(self, t, deriv, dMode, x):
        return None

    def update_state(self, u, dt, x, d=None):
        self.x = _rk4(lambda z: self.dynamics(None, z, u), x, dt)
        return self.x


class DubinsPair6D(object):
    """Two Dubins vehicles in ABSOLUTE coordinates: evader (x0, x1, x2), pursuer (x3, x4, x5), speeds v_e / v_p, turn rates
    |u| <= w_e / |d| <= w_p.  The convention of the reference's Dubins game (dubins_relative.py:63-111): the evader
    maximises, the pursuer minimises, H is the negated optimum:
        H = -( p0 (v_e cos x2) + p1 (v_e sin x2) + p3 (v_p cos x5) + p4 (v_p sin x5) + w_e |p2| - w_p |p5| )   left to right
        alpha = { |v_e cos x2|, |v_e sin x2|, w_e, |v_p cos x5|, |v_p sin x5|, w_p }
    hidim_substep_kernel<T, HamDubinsPair6D, SCHEME> (csrc/hj_hidim.hip) restates these expressions operation by operation."""

    def __init__(self, grid, v_e=5, v_p=5, w_e=5, w_p=5):
        self.grid = grid
        self.v_e, self.v_p, self.w_e, self.w_p = v_e, v_p, w_e, w_p

    def native(self):
        if self.grid.dim != 6 or not all(np.isscalar(v) for v in (self.v_e, self.v_p, self.w_e, self.w_p)):
            return None
        return _hffi.HAM_DUBINS_PAIR6D, [float(self.v_e), float(self.v_p), float(self.w_e), float(self.w_p)]

    def hamiltonian(self, t, data, value_derivs, finite_diff_bundle=None):
        p = value_derivs
        x2, x5 = _xs(self.grid, 2, p[0]), _xs(self.grid, 5, p[0])
        return -(p[0] * (self.v_e * _cos(x2)) + p[1] * (self.v_e * _sin(x2)) + p[3] * (self.v_p * _cos(x5))
                 + p[4] * (self.v_p * _sin(x5)) + self.w_e * _abs(p[2]) - self.w_p * _abs(p[5]))

    def dissipation(self, t, data, derivMin, derivMax, schemeData, dim):
        assert 0 <= dim < 6, "DubinsPair6D has dimensions 0 to 5."
        if dim == 0:
            return _abs(self.v_e * _cos(_xs(self.grid, 2, data)))
        if dim == 1:
            return _abs(self.v_e * _sin(_xs(self.grid, 2, data)))
        if dim == 3:
            return _abs(self.v_p * _cos(_xs(self.grid, 5, data)))
        if dim == 4:
            return _abs(self.v_p * _sin(_xs(self.grid, 5, data)))
        return self.w_e if dim == 2 else self.w_p

    # ---- the dynSys protocol: u the evader's turn rate, d the pursuer's
    x = None

    def dynamics(self, t, x, u, d):
        x = _state(x)
        ve, vp = float(self.v_e), float(self.v_p)
        return np.array([ve * float(np.cos(x[2])), ve * float(np.sin(x[2])), float(u),
                         vp * float(np.cos(x[5])), vp * float(np.sin(x[5])), float(d)])

    def get_opt_u(self, t, deriv, uMode, x):
        """uMode None: 'max', the evader of the class's own Hamiltonian."""
        a = float(self.w_e) * _sgn(deriv[2])
        return a if _mode(uMode, 'max') == 'max' else -a

    def get_opt_v(self, t, deriv, dMode, x):
        """dMode None: 'min', the pursuer of the class's own Hamiltonian."""
        b = float(self.w_p) * _sgn(deriv[5])
        return b if _mode(dMode, 'min') == 'max' else -b

    def update_state(self, u, dt, x, d=None):
        d = 0.0 if d is None else d
        self.x = _rk4(lambda z: self.dynamics(None, z, u, d), x, dt)
        return self.x


def native_of(hamFunc, partialFunc):
    """(system, ham_id, params) when hamFunc/partialFunc are the bound methods of ONE of the
    systems above (so the fused kernel computes exactly what the callbacks would), else None.
    A subclass that overrides hamiltonian() / dissipation() / native() is NOT native: the methods are
    compared with the ones of the class that owns the kernel, not with type(self)'s."""
    sys_h = getattr(hamFunc, "__self__", None)
    sys_p = getattr(partialFunc, "__self__", None)
    if sys_h is None or sys_h is not sys_p:
        return None
    att = getattr(sys_h, "_hj_native", None)
    if att is not None:
        # a Hamiltonian registered at run time (user_ham.py): the methods must be the ones the registration saw
        if getattr(hamFunc, "__func__", None) is not att.ham_func or getattr(partialFunc, "__func__", None) is not att.diss_func:
            return None
        return sys_h, att.reg.ham_id, att.params(sys_h)
    owner = next((k for k in (DubinsVehicleRel, DoubleIntegrator, DoublePendulum4D, Plane5D, DubinsPair6D) if isinstance(sys_h, k)), None)
    if owner is None:
        return None
    if getattr(hamFunc, "__func__", None) is not owner.hamiltonian:
        return None
    if getattr(partialFunc, "__func__", None) is not owner.dissipation:
        return None
    if type(sys_h).native is not owner.native:
        return None
    nat = sys_h.native()
    if nat is None:
        return None
    return sys_h, nat[0], nat[1]


_PROTOCOL = ("native", "dynamics", "get_opt_u", "get_opt_v", "update_state")


def native_plant(dynSys):
    """(ham_id, params) when rollout_kernel computes exactly what dynSys's dynSys-protocol methods would: an instance of
    one of the systems above whose native() and protocol methods are the ones of the class that owns the kernel (the
    identity rule of native_of: a subclass that overrides one of them is NOT native), with scalar bounds.  Else None."""
    owner = next((k for k in (DubinsVehicleRel, DoubleIntegrator, DoublePendulum4D) if isinstance(dynSys, k)), None)
    if owner is None or getattr(dynSys, "_hj_native", None) is not None:
        return None
    for name in _PROTOCOL:
        if getattr(type(dynSys), name, None) is not getattr(owner, name) or name in getattr(dynSys, "__dict__", {}):
            return None
    return dynSys.native()


def native_plant_hi(dynSys):
    """native_plant for the 5-D / 6-D systems and hi_rollout_kernel (libhj_hiquery.so): (plant id, the four parameters of
    include/hj_hiquery.h's table) under the same identity rule, else None.  Plane5D's sign slot is not a plant parameter: the
    rollout takes uMode from its caller, as get_opt_u does."""
    owner = next((k for k in (Plane5D, DubinsPair6D) if isinstance(dynSys, k)), None)
    if owner is None or getattr(dynSys, "_hj_native", None) is not None:
        return None
    for name in _PROTOCOL:
        if getattr(type(dynSys), name, None) is not getattr(owner, name) or name in getattr(dynSys, "__dict__", {}):
            return None
    nat = dynSys.native()
    if nat is None:
        return None
    return nat[0], (nat[1][:2] + [0.0, 0.0] if owner is Plane5D else list(nat[1]))
