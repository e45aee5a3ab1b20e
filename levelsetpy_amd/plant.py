"""A user's own system in computeOptTrajs' one launch (C ABI: hjp_plant_register, include/hj_plant.h).

computeOptTrajs (rollout.py) runs a whole batch of trajectories in one kernel for the five built-in systems; every other dynSys takes
one computeOptTraj per state.  `register_plant` closes that gap the way register_native_hamiltonian / register_hidim_hamiltonian close
it for the solve: write the optimal controls and the dynamics ONCE more, as device statements; user_rollout_kernel is compiled around
them with hipRTC (libhj_plant.so), and a dynSys that carries the registration runs as the built-in systems do -- selected by the identity of
its protocol methods (the rule of dynamics.native_plant).

    Quad = register_plant("planar_quad", 6, controls_src='''
        const double k = (p[3] * cos(x[4]) - p[1] * sin(x[4])) / par[0];
        const double r = p[5] * par[2] / par[1];
        u[0] = 0.5 * par[6] * (u_max ? 1.0 + sgn(k + r) : 1.0 - sgn(k + r));
        u[1] = 0.5 * par[6] * (u_max ? 1.0 + sgn(k - r) : 1.0 - sgn(k - r));
    ''', dynamics_src='''
        dx[0] = x[1];  dx[1] = -(par[3] / par[0]) * x[1] - sin(x[4]) * (u[0] + u[1]) / par[0];  ...
    ''', ncontrols=2, nparams=8)
    sys_ = Quad(params, dynamics=py_f, get_opt_u=py_u)        # a new dynSys around Python callables (they serve the host loop)
    Quad.attach(obj, params=...)                              # or: an EXISTING object with the dynSys protocol -- also one a
                                                              # Hamiltonian registration is attached to: it solves AND rolls out fused
    Quad.check("ENO3", "float64")                             # compiles now, no GPU needed
    Quad.compare(sys_, g, data, tau, x0s[:16], extraArgs)     # kernel against host loop on the same states

In controls_src: p[d] the costate, x[d] the state, par[k] parameters (at most 16), the booleans u_max / d_max (uMode / dMode is 'max'),
sgn() (+1 for s >= 0, -1 for s < 0, NaN for NaN) and the device math functions; assign u[i] (ncontrols of them) and dst[j] (ndisturbances).
In dynamics_src: x[d], u[i], dst[j], par[k]; assign dx[d].  Both are fp64 with contraction off: one operation per statement rounds where
NumPy does.  No t, no value, no tables.  2 to 6 states, at most 8 controls and disturbances together.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi, _pffi
from .dynamics import _rk4
from .user_ham import HERE, _hiprtc_path

__all__ = ["register_plant", "PlantRegistration", "PlantSystem", "plant_kernel_cache_stats", "plant_of"]

_PROTOCOL = ("dynamics", "get_opt_u", "get_opt_v", "update_state")


class _PlantAttached(object):
    """What plant_of needs to recognise an object's protocol methods: the registration, the functions the methods must be, and where
    the parameters come from (a list, or a callable of the object: re-read at every call)."""

    def __init__(self, reg, params, funcs):
        self.reg, self._params, self.funcs = reg, params, funcs

    def params(self, obj):
        p = self._params(obj) if callable(self._params) else self._params
        p = [float(v) for v in p]
        if len(p) != self.reg.nparams:
            raise ValueError("plant '%s' takes %d parameters, got %d" % (self.reg.name, self.reg.nparams, len(p)))
        return p


def plant_of(dynSys):
    """(registration, parameters) when user_rollout_kernel computes what dynSys's protocol methods would: a registration is attached
    and the methods are the ones it saw -- none replaced in the class since, none shadowed in the instance.  Else None."""
    att = getattr(dynSys, "_hj_plant", None)
    if att is None:
        return None
    for name in _PROTOCOL:
        if getattr(type(dynSys), name, None) is not att.funcs[name] or name in getattr(dynSys, "__dict__", {}):
            return None
    return att.reg, att.params(dynSys)


class PlantSystem(object):
    """A dynSys around a registration: the protocol computeOptTraj calls (x, get_opt_u, get_opt_v, update_state; dynamics) from the
    Python callables given -- each is called with the system first, which has .params -- plus the registered plant."""
    x = None

    def __init__(self, reg, params, dynamics=None, get_opt_u=None, get_opt_v=None):
        self.params = [float(v) for v in params]
        self._py_dyn, self._py_u, self._py_v = dynamics, get_opt_u, get_opt_v
        self._hj_plant = _PlantAttached(reg, lambda s: s.params, dict((n, getattr(PlantSystem, n)) for n in _PROTOCOL))
        self._hj_plant.params(self)             # validates the count now

    def _need(self, fn, what):
        if fn is None:
            raise NotImplementedError("no Python %s was given for '%s': it only runs in the kernel" % (what, self._hj_plant.reg.name))
        return fn

    def dynamics(self, t, x, u, d=None):
        return self._need(self._py_dyn, "dynamics")(self, t, x, u, d)

    def get_opt_u(self, t, deriv, uMode, x):
        return self._need(self._py_u, "get_opt_u")(self, t, deriv, uMode, x)

    def get_opt_v(self, t, deriv, dMode, x):
        return None if self._py_v is None else self._py_v(self, t, deriv, dMode, x)

    def update_state(self, u, dt, x, d=None):
        self.x = _rk4(lambda z: np.asarray(self.dynamics(None, z, u, d), dtype=np.float64), x, dt)
        return self.x


class PlantRegistration(object):
    def __init__(self, name, dim, controls_src, dynamics_src, ncontrols, ndisturbances=0, nparams=0):
        self.name, self.dim, self.nparams = str(name), int(dim), int(nparams)
        self.ncontrols, self.ndisturbances = int(ncontrols), int(ndisturbances)
        self.controls_src, self.dynamics_src = str(controls_src), str(dynamics_src)
        if not _pffi.MIN_DIM <= self.dim <= _pffi.MAX_DIM:
            raise ValueError("plant '%s': dim must be %d..%d, got %d" % (self.name, _pffi.MIN_DIM, _pffi.MAX_DIM, self.dim))
        if not 0 <= self.nparams <= _pffi.PAR_SLOTS:
            raise ValueError("plant '%s': at most %d parameters (HJP_PAR_SLOTS), got %d" % (self.name, _pffi.PAR_SLOTS, self.nparams))
        if self.ncontrols < 0 or self.ndisturbances < 0 or not 1 <= self.ncontrols + self.ndisturbances <= _pffi.MAX_CONTROLS:
            raise ValueError("plant '%s': 1..%d controls and disturbances together (HJP_MAX_CONTROLS), got %d + %d"
                             % (self.name, _pffi.MAX_CONTROLS, self.ncontrols, self.ndisturbances))
        if '"' in self.name or "'" in self.name:
            raise ValueError("the name of a plant must not contain quotes: %r" % self.name)
        pid = C.c_int()
        rtc = _hiprtc_path()
        _pffi.check(_pffi.lib().hjp_plant_register(self.name.encode(), self.dim, self.ncontrols, self.ndisturbances, self.nparams,
                                                   self.controls_src.encode(), self.dynamics_src.encode(), os.path.join(HERE, "csrc").encode(),
                                                   rtc.encode() if rtc else None, C.byref(pid)))
        self.plant_id = int(pid.value)

    def check(self, scheme="WENO5_ASSHIPPED", dtype="float64", kind="rollout"):
        """Compile the kernel of (scheme, dtype) now (no GPU needed): raises ValueError with the compiler's message, which points into the
        body at fault as name:line, if one is wrong.  kind: 'rollout' (user_rollout_kernel: computeOptTrajs), 'noisy' (computeStochTrajs),
        'filtered' (computeSafeTrajs) or 'decide' (safeControls) -- the last three run under extraArgs.plantKernel."""
        if kind not in _pffi.KINDS:
            raise ValueError("kind must be 'rollout', 'noisy', 'filtered' or 'decide' (got %r)" % (kind,))
        _pffi.check(_pffi.lib().hjp_plant_compile_kind(self.plant_id, _pffi.KINDS[kind], _ffi.SCHEME_IDS[scheme],
                                                       _ffi.F64 if dtype == "float64" else _ffi.F32))
        return self

    def source(self):
        """The translation unit hipRTC is given (hjp_plant_source), for a look at it or an offline hipcc."""
        n = len(self.controls_src.encode()) + len(self.dynamics_src.encode()) + 16384
        buf = C.create_string_buffer(n)
        _pffi.check(_pffi.lib().hjp_plant_source(self.plant_id, buf, n))
        return buf.value.decode()

    def __call__(self, params=(), dynamics=None, get_opt_u=None, get_opt_v=None):
        return PlantSystem(self, params, dynamics, get_opt_u, get_opt_v)

    def attach(self, obj, params=()):
        """Mark an existing dynSys (its class has dynamics / get_opt_u / update_state, and get_opt_v or none): computeOptTrajs then runs it
        in the kernel as long as those methods are the ones seen now.  params: a list, or a callable of the object.  The mark is its own
        attribute: a Hamiltonian registration attached to the same object stays as it is."""
        cls = type(obj)
        funcs = dict((n, getattr(cls, n, None)) for n in _PROTOCOL)
        missing = [n for n in _PROTOCOL if funcs[n] is None and n != "get_opt_v"]
        if missing:
            raise ValueError("the object's class needs the dynSys protocol: no %s()" % "(), ".join(missing))
        shadowed = [n for n in _PROTOCOL if n in getattr(obj, "__dict__", {})]
        if shadowed:
            raise ValueError("the object shadows %s in its own attributes: the kernel could not stand for it" % ", ".join(shadowed))
        att = _PlantAttached(self, params, funcs)
        att.params(obj)                      # validates the count now
        obj._hj_plant = att
        return obj

    def compare(self, dynSys, g, data, tau, x0s, extraArgs=None):
        """The kernel and the host loop (computeOptTraj with dynSys's own methods, once per state) on the same states:
        -> (the largest deviation of a recorded state, the number of trajectories whose lengths differ, the number whose statuses differ).
        States are compared over the columns both recorded; a NaN against a number counts as inf.  No threshold: the caller judges."""
        from . import rollout
        from .query import states_2d
        from .utilities import Bundle
        if plant_of(dynSys) is None or plant_of(dynSys)[0] is not self:
            raise ValueError("plant '%s' is not attached to this object (or its protocol methods have changed since)" % self.name)
        args = Bundle(dict(extraArgs.__dict__ if extraArgs is not None else {}))
        args.status = True
        trajs, lengths, _, outs = rollout.computeOptTrajs(g, data, tau, dynSys, x0s, args)
        if outs.path.startswith("host loop"):
            raise ValueError("computeOptTrajs took the %s" % outs.path)
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)     # noqa: E731
        x0 = states_2d(g, x0s)
        x0 = np.asarray(host(x0), dtype=np.float64)
        tau = np.asarray(tau, dtype=np.float64).ravel()
        want_te = False
        rt, rl, _, rs = rollout._host_loop(g, data, tau, dynSys, x0, extraArgs, want_te)
        kt, kl, ks = host(trajs), host(lengths), host(outs.status)
        worst = 0.0
        for m in range(x0.shape[0]):
            n = int(min(kl[m], rl[m]))
            a, b = kt[m][:, :n], rt[m][:, :n]
            na, nb = np.isnan(a), np.isnan(b)
            if (na != nb).any():
                worst = np.inf
            elif (~na).any():
                worst = max(worst, float(np.max(np.abs(a[~na] - b[~na]))))
        return worst, int((kl != rl).sum()), int((ks != rs).sum())


def plant_kernel_cache_stats():
    """(rollout kernels compiled with hipRTC, kernels loaded from the on-disk cache) in this process; the cache is
    user_ham.kernel_cache_stats's."""
    a, b = C.c_int(), C.c_int()
    _pffi.check(_pffi.lib().hjp_plant_cache_stats(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def register_plant(name, dim, controls_src, dynamics_src, ncontrols, ndisturbances=0, nparams=0):
    """Register a system's optimal controls and dynamics as device statements (module docstring); returns a PlantRegistration: call it to
    make a dynSys, or .attach() it to an existing one."""
    return PlantRegistration(name, dim, controls_src, dynamics_src, ncontrols, ndisturbances, nparams)
