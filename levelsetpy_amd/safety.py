"""computeSafeTrajs and safeControls: the least-restrictive safety filter on a stored value function.

    outs = computeSafeTrajs(g, data, tau, dynSys, x0s, nominal, extraArgs)
    dec  = safeControls(g, data, dynSys, xs, uNom, extraArgs)

A nominal controller runs while V(x) is on the safe side of `level` by more than `margin`; the value function's optimal control
takes over once the margin is used up (the least-restrictive supervisor of Fisac, Bansal, Chen and Tomlin).  With gap = V(x) -
level for uMode 'max' (an avoid tube: the control keeps V up) and level - V(x) for 'min', a sub-step acts -- applies the optimal
control -- unless gap > margin; a NaN gap acts.  include/hj_filter.h states a filtered trajectory operation by operation: it is
computeOptTrajs' trajectory (rollout.py) that never stops early and chooses its controls this way at every RK4 sub-step.

`data`, `tau`, `dynSys` and `x0s` are computeStochTrajs' (montecarlo.py): the time-first stack, its time stamps, the system and one
initial state per row.  `data` may also be ONE field of g.shape with policy 'static': a converged value function that serves every
time stamp; it is passed as it is, no copy per time stamp is made.  `nominal` is the controller being filtered:
  * an array (M, T-1, NU), or (T-1, NU) for every state: the nominal controls of every column, held over its sub-steps and applied
    as given (keeping them inside the bounds the value function was solved for is the caller's); NU is the number of controls
    (1: DubinsVehicleRel's turn rate, DoubleIntegrator's u; 2: DoublePendulum4D's torques);
  * Bundle(data=..., uMode=...): a second value function on the same grid, (T,) + g.shape or g.shape, whose optimal control (for
    its own uMode, default extraArgs.uMode) is the nominal one -- e.g. a reach tube steering to a goal inside an avoid tube.  It is
    brought to the element type of `data`.

extraArgs: uMode, dMode, subSamples, derivFunc as computeOptTrajs reads them; margin (0.0; +inf always acts, -inf never does); level
(0.0); policy 'clock' (slice `it` at column `it`: the default) or 'static' (one slice, extraArgs.slice, default 0, throughout);
disturbance 'worst' (the optimal disturbance: the default) or 'zero'; keepTrajs (True); keepControls (False).

outs: trajs (M, dim, T) or None; final (M, dim); gapMin (M,) the NaN-propagating minimum of the gap over every sub-step's state and
the last; valueEnd (M,); interventions (M,) the number of acting sub-steps; firstIntervention (M,) the first one's index, -1 if none;
status (M,) SAFE / VIOLATED (gapMin is not above 0) / LEFT_GRID (a recorded state is outside an extrapolated axis or not finite);
length (M,), always T; active (M, (T-1) subSamples) bool and controls (M, (T-1) subSamples, 2), the two values every sub-step held
(the control and the disturbance, or the two controls), with keepControls, else None; tau; path: the kernel that ran, or 'host loop:
<why>'.  NumPy in -> NumPy out; a device tensor or HostView (data or x0s) in -> device tensors out.

safeControls answers the runtime question for M states `xs` and the controls `uNom` (M, NU) or (NU,) one would like to apply: `data`
is one field of g.shape, or a stack with extraArgs.slice; extraArgs as above without the rollout's.  dec: controls (M, 2), active (M,)
bool, value (M,), gap (M,), costate (M, dim).  It is exactly the decision of a filtered trajectory's sub-step.

With a built-in 2-D .. 4-D system (native_plant's identity rule) and upwindFirstENO2 / ENO3 / WENO5 (as shipped) computeSafeTrajs is
ONE launch of filtered_rollout_kernel (libhj_filter.so) per split over states, and safeControls one of decide_points_kernel.
Plane5D / DubinsPair6D, a registered plant, a foreign dynSys or a derivative function without a point kernel take a host loop on
dynSys.get_opt_u / get_opt_v / update_state with the same output contract (controls then holds the system's u then d, flattened,
padded with 0.0 to two), and say so in an info line.

extraArgs.plantKernel=True (a bool, default False) sends two more kinds of system to a kernel, after the built-in rule: a registered plant
(plant.register_plant; plant_of's identity rule, the registration's dimension, a derivative function with a point kernel) and Plane5D /
DubinsPair6D, which the package registers itself at their first use (plant_builtin.py).  libhj_plant.so compiles
user_filtered_rollout_kernel / user_decide_points_kernel around the plant at run time; the contract is the one above with the plant's
controls u[0 .. NU) in the nominal's place (a table's last axis is NU = the registration's ncontrols), every dst[j] zeroed by disturbance
'zero', and controls W = max(2, NU + NDST) wide: u then dst, padded with 0.0 -- the host loop's layout.  Whatever is not eligible under the
flag keeps the host loop and its info line.
Parity UNPINNED: the reference has no counterpart.
"""
import copy
import ctypes as C

import numpy as np

from . import _fffi, _pffi, _rffi, plant_builtin
from .context import is_tensor, require_gpu
from .dynamics import native_plant, native_plant_hi
from .query import interp_states, costate_states, point_scheme, states_2d
from .rollout import _get, _outside
from .spatial import upwindFirstWENO5
from .utilities import Bundle, error, info, isfield
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, device_data as _device_data,
                       device_states as _device_states, stream as _stream, ptr as _ptr, descriptor as _descriptor,
                       dtype_name as _dtype_name, is_hi as _is_hi, descriptor_hi as _descriptor_hi)
from .plant import PlantRegistration

__all__ = ["computeSafeTrajs", "safeControls", "SAFE", "VIOLATED", "LEFT_GRID"]

SAFE, VIOLATED, LEFT_GRID = _fffi.SAFE, _fffi.VIOLATED, _fffi.LEFT_GRID

_MODES = {'min': _rffi.MODE_MIN, 'max': _rffi.MODE_MAX}
# threads one launch may hold (hj_tool_host.h's blocks_for refuses 2^32 - 255 and more); a call over more is split over states
LAUNCH_THREADS = 2 ** 32 - 256
_last_path = ""


def last_path():
    """What the calling process's last computeSafeTrajs or safeControls ran: the kernel's name, or 'host loop: <why>'."""
    return _last_path


def _why_host(dynSys, derivFunc, g, plantKernel=False):
    """(plant, None) when a kernel covers this call, else (None, the reason for the host loop).  plant: native_plant's (id, parameters),
    or under plantKernel (registration, parameters) of a plant libhj_plant.so compiles a kernel around -- the built-in rule comes first."""
    if plantKernel and native_plant(dynSys) is None:
        user, why = plant_builtin.route(dynSys, derivFunc, g)
        if user is not None or why is not None:
            return user, why
    if _is_hi(g):
        return None, "%s has no filter kernel on a %d-D grid" % (type(dynSys).__name__, g.dim)
    nat = native_plant(dynSys)
    if nat is None:
        if native_plant_hi(dynSys) is not None:
            return None, "%s has no filter kernel (5-D / 6-D systems are out of its scope)" % type(dynSys).__name__
        from .plant import plant_of
        if plant_of(dynSys) is not None:
            return None, "%s is a registered plant: it has no filter kernel" % type(dynSys).__name__
        return None, "%s has no native plant" % type(dynSys).__name__
    if _fffi.PLANT_DIMS.get(nat[0]) != g.dim:
        return None, "%s has no native plant on a %d-D grid" % (type(dynSys).__name__, g.dim)
    if point_scheme(derivFunc) is None:
        return None, "derivFunc %s has no point kernel" % getattr(derivFunc, "__name__", derivFunc)
    return nat, None


def _number(extraArgs, name, default, nan_text):
    v = _get(extraArgs, name, default)
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        error('extraArgs.%s must be a number (got %r)' % (name, v))
    v = float(v)
    if v != v:
        error('extraArgs.%s must not be NaN%s' % (name, nan_text))
    return v


def _common(extraArgs):
    """The arguments both calls read, checked: uMode, dMode, derivFunc, margin, level, disturbance."""
    uMode = _get(extraArgs, 'uMode', 'min')
    dMode = _get(extraArgs, 'dMode', None)
    derivFunc = _get(extraArgs, 'derivFunc', upwindFirstWENO5)
    if uMode not in _MODES or (dMode is not None and dMode not in _MODES):
        error("uMode / dMode must be 'min' or 'max'")
    margin = _number(extraArgs, 'margin', 0.0, ' (+inf always acts, -inf never does)')
    level = _number(extraArgs, 'level', 0.0, '')
    if not np.isfinite(level):
        error('extraArgs.level must be finite (got %r)' % (level,))
    dstb = _get(extraArgs, 'disturbance', 'worst')
    if dstb not in _fffi.DISTURBANCES:
        error("extraArgs.disturbance must be 'worst' or 'zero' (got %r)" % (dstb,))
    return uMode, dMode, derivFunc, margin, level, dstb


def _index(extraArgs, name, n):
    k = _get(extraArgs, name, 0)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < n:
        error('extraArgs.%s must be an integer in 0 .. %d (got %r)' % (name, n - 1, k))
    return int(k)


def _table(u, lead, M, what):
    """The nominal controls as an (M,) + lead + (NU,) array or tensor: a table without the state axis serves every state."""
    u = _unlazy(u)
    if not is_tensor(u):
        u = np.asarray(u, dtype=np.float64)
    shape = tuple(int(v) for v in u.shape)
    if len(shape) == len(lead) + 1 and shape[:-1] == lead:
        u = u.expand((M,) + shape) if is_tensor(u) else np.broadcast_to(u, (M,) + shape)
    elif not (len(shape) == len(lead) + 2 and shape[:-1] == (M,) + lead):
        error('%s must have shape %s or %s with NU the number of controls, got %s'
              % (what, (M,) + lead + ('NU',), lead + ('NU',), shape))
    if u.shape[-1] < 1:
        error('%s holds no control' % what)
    return u


def _entry(plant, g, name):
    """(binding, entry point, descriptor function) for a built-in plant's descriptor or a registered plant's (_pffi.Plant)."""
    if isinstance(plant, _pffi.Plant):
        hi = _is_hi(g)
        return _pffi, getattr(_pffi.lib(), "hjp_" + name + ("_hi" if hi else "")), (_descriptor_hi if hi else _descriptor)
    return _fffi, getattr(_fffi.lib(), "hjf_" + ("rollout" if name == "filtered_rollout" else name)), _descriptor


def filtered_rollout_states(g, data, T, xs, scheme, subSamples, dtSmall, plant, policy, k, u_nom, nom, nom_mode, level, margin,
                            dstb, keep, keep_controls, width=2):
    """hjf_rollout (hjp_filtered_rollout / _hi for a _pffi.Plant, `width` its W) on device tensors: `data` a contiguous (T,) + g.shape stack or one g.shape field (stride 0), `xs` an (M, dim)
    fp64 tensor, `u_nom` an (M, T-1, NU) fp64 tensor or None, `nom` None or a stack / field of data's dtype.
    -> final, gap_min, value_end, interventions, first, length, status, traj or None, active or None, applied or None."""
    torch = require_gpu()
    ffi, call, describe = _entry(plant, g, "filtered_rollout")
    desc, N = describe(g, _dtype_name(data))
    total = int(np.prod(N))
    stride = 0 if tuple(data.shape) == tuple(N) else total
    M, nd = int(xs.shape[0]), g.dim
    nsteps = (T - 1) * subSamples
    dev = data.device
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)        # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)          # noqa: E731
    final, gmin, vend, count, first, length, status = f64(M, nd), f64(M), f64(M), i32(M), i32(M), i32(M), i32(M)
    traj = f64(M, nd, T) if keep else None
    active = torch.empty((M, nsteps), dtype=torch.uint8, device=dev) if keep_controls else None
    applied = f64(M, nsteps, width) if keep_controls else None
    nom_T = 0 if nom is None else (1 if tuple(nom.shape) == tuple(N) else int(nom.shape[0]))
    with torch.cuda.device(dev):
        ffi.check(call(
            C.byref(desc), int(scheme), _ptr(data), T, stride, _ptr(xs), M, int(subSamples), float(dtSmall), C.byref(plant), int(policy),
            int(k), _fffi.NOMINAL_TABLE if nom is None else _fffi.NOMINAL_VALUE, _ptr(u_nom), _ptr(nom), nom_T, total, int(nom_mode),
            float(level), float(margin), int(dstb), _ptr(final), _ptr(gmin), _ptr(vend), _ptr(count), _ptr(first), _ptr(length),
            _ptr(status), _ptr(traj), _ptr(active), _ptr(applied), _stream(torch, dev)))
    return final, gmin, vend, count, first, length, status, traj, active, applied


def decide_states(g, data, k, xs, scheme, plant, u_nom, level, margin, dstb, width=2):
    """hjf_decide (hjp_decide / _hi for a _pffi.Plant, `width` its W) on device tensors -> applied (M, width), active (M,) uint8, value,
    gap (M,), costate (M, dim)."""
    torch = require_gpu()
    ffi, call, describe = _entry(plant, g, "decide")
    desc, N = describe(g, _dtype_name(data))
    total = int(np.prod(N))
    F = 1 if tuple(data.shape) == tuple(N) else int(data.shape[0])
    M, dev = int(xs.shape[0]), data.device
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)        # noqa: E731
    applied, value, gap, costate = f64(M, width), f64(M), f64(M), f64(M, g.dim)
    active = torch.empty((M,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ffi.check(call(C.byref(desc), int(scheme), _ptr(data), F, total, int(k), _ptr(xs), M, C.byref(plant),
                       _ptr(u_nom), float(level), float(margin), int(dstb), _ptr(applied), _ptr(active),
                       _ptr(value), _ptr(gap), _ptr(costate), _stream(torch, dev)))
    return applied, active, value, gap, costate


# ---------------------------------------------------------------------------------------------- the host loop
def _flat(u):
    return [] if u is None else [float(v) for v in np.ravel(np.asarray(u, dtype=np.float64))]


class _HostField(object):
    """V and grad V of the slices of a stack (or of one field) at one state: the device's point queries where the derivative
    function has one, computeGradients' tables otherwise -- as computeOptTraj."""

    def __init__(self, g, data, derivFunc):
        self.g, self.data, self.derivFunc = g, data, derivFunc
        self.t = _device_data(data)
        self.single = tuple(self.t.shape) == tuple(g.shape)
        self.sid = point_scheme(derivFunc)
        self.tables = {}

    def field(self, k):
        return self.t if self.single else self.t[k]

    def value(self, k, x):
        xs = _device_states(x.reshape(1, -1), self.t.device)
        return float(interp_states(self.g, self.field(k), xs, out_f64=True)[0, 0])

    def costate(self, k, x):
        if self.sid is not None:
            xs = _device_states(x.reshape(1, -1), self.t.device)
            return costate_states(self.g, self.field(k), xs, self.sid, out_f64=True)[0][0, 0].cpu().numpy().tolist()
        from .gradients import computeGradients
        from .hji_solver import _eval_point
        k = 0 if self.single else k
        if k not in self.tables:
            src = _unlazy(self.data)
            src = src.detach().cpu().numpy() if is_tensor(src) else np.asarray(src)
            self.tables[k] = computeGradients(self.g, src if self.single else src[k], derivFunc=self.derivFunc)[0]
        return [_eval_point(self.g, self.tables[k][d], x) for d in range(self.g.dim)]


def _host_decision(plant, t, x, v, deriv, uMode, dMode, level, margin, zero, nominal_u):
    """One sub-step's decision on the system's own methods -> act, gap, u, d."""
    gap = v - level if uMode == 'max' else level - v
    act = not (gap > margin)
    u = plant.get_opt_u(t, deriv, uMode, x) if act else nominal_u()
    d = plant.get_opt_v(t, deriv, dMode, x) if hasattr(plant, 'get_opt_v') else None
    if zero and d is not None:
        d = np.zeros_like(np.asarray(d, dtype=np.float64)) if np.ndim(d) else 0.0
    return act, gap, u, d


def _nmin(a, b):
    return np.nan if (a != a or b != b) else (b if b < a else a)


def _as_control(row):
    return float(row[0]) if len(row) == 1 else tuple(float(v) for v in row)


def _host_loop(g, data, tau, dynSys, x0, u_nom, nom, nomMode, uMode, dMode, subSamples, derivFunc, level, margin, zero, clock, k, keep,
               keep_controls):
    """The trajectories one by one on dynSys's own protocol methods, to the kernel's output contract (NumPy)."""
    M, T, nd = x0.shape[0], len(tau), g.dim
    nsteps = (T - 1) * subSamples
    dtSmall = (tau[1] - tau[0]) / subSamples
    V = _HostField(g, data, derivFunc)
    Vn = _HostField(g, nom, derivFunc) if nom is not None else None
    final, gmin, vend = np.empty((M, nd)), np.empty(M), np.empty(M)
    count, first, status = np.zeros(M, dtype=np.int32), np.full(M, -1, dtype=np.int32), np.empty(M, dtype=np.int32)
    trajs = np.empty((M, nd, T)) if keep else None
    active = np.zeros((M, nsteps), dtype=bool) if keep_controls else None
    rows = []
    for m in range(M):
        plant = copy.copy(dynSys)
        x = np.array(x0[m], dtype=np.float64)
        if keep:
            trajs[m, :, 0] = x
        left = bool(_outside(g, x.reshape(-1, 1))[0])
        gm, held = None, []
        for it in range(T - 1):
            sl = it if clock else k
            for s in range(subSamples):
                plant.x = x
                deriv = V.costate(sl, x)

                def nominal_u():
                    if Vn is None:
                        return _as_control(u_nom[m, it])
                    return plant.get_opt_u(tau[sl], Vn.costate(0 if Vn.single else it, x), nomMode, x)
                act, gap, u, d = _host_decision(plant, tau[sl], x, V.value(sl, x), deriv, uMode, dMode, level, margin, zero, nominal_u)
                gm = gap if gm is None else _nmin(gm, gap)
                step = it * subSamples + s
                if act:
                    if count[m] == 0:
                        first[m] = step
                    count[m] += 1
                if keep_controls:
                    active[m, step] = act
                    held.append(_flat(u) + _flat(d))
                xt = plant.update_state(u, dtSmall, x, d)
                x = np.array(xt if xt is not None else plant.x, dtype=np.float64).ravel()
            left = left or bool(_outside(g, x.reshape(-1, 1))[0])
            if keep:
                trajs[m, :, it + 1] = x
        v = V.value(T - 1 if clock else k, x)
        gm = _nmin(gm, v - level if uMode == 'max' else level - v)
        final[m], gmin[m], vend[m] = x, gm, v
        status[m] = LEFT_GRID if left else (VIOLATED if not (gm > 0) else SAFE)
        rows.append(held)
    applied = None
    if keep_controls:
        width = max([2] + [len(h) for held in rows for h in held])
        applied = np.zeros((M, nsteps, width))
        for m, held in enumerate(rows):
            for step, h in enumerate(held):
                applied[m, step, :len(h)] = h
    return final, gmin, vend, count, first, np.full(M, T, dtype=np.int32), status, trajs, active, applied


# ---------------------------------------------------------------------------------------------- the front ends
def _kernel_plant(nat, uMode, dMode):
    """-> (plant descriptor, NU, W, the binding whose last_kernel names the launch) of _why_host's plant."""
    if isinstance(nat[0], PlantRegistration):
        reg = nat[0]
        return (_pffi.plant_descriptor(reg.plant_id, _MODES[uMode], _MODES[dMode or 'min'], nat[1]), reg.ncontrols,
                max(2, reg.ncontrols + reg.ndisturbances), _pffi)
    return _rffi.plant_descriptor(nat[0], _MODES[uMode], _MODES[dMode or 'min'], nat[1]), _fffi.PLANT_NU[nat[0]], 2, _fffi


def _out_device(torch, data, xs):
    d = _unlazy(data)
    return d.device if is_tensor(d) and d.is_cuda else (xs.device if is_tensor(xs) and xs.is_cuda else "cuda")


def computeSafeTrajs(g, data, tau, dynSys, x0s, nominal, extraArgs=None):
    global _last_path
    uMode, dMode, derivFunc, margin, level, dstb = _common(extraArgs)
    subSamples = int(_get(extraArgs, 'subSamples', 4))
    policy = _get(extraArgs, 'policy', 'clock')
    keep = bool(_get(extraArgs, 'keepTrajs', True))
    keep_controls = bool(_get(extraArgs, 'keepControls', False))
    tau = np.asarray(tau, dtype=np.float64).ravel()
    if np.any(np.diff(tau) < 0):
        error('Time stamps must be in ascending order!')
    if len(tau) < 2:
        error('a trajectory needs at least two time stamps')
    if subSamples < 1:
        error('subSamples must be positive')
    if policy not in _fffi.POLICIES:
        error("extraArgs.policy must be 'clock' or 'static' (got %r)" % (policy,))
    T = len(tau)
    single = tuple(data.shape) == tuple(g.shape)
    if single:
        if policy != 'static':
            error("data holds one value function: only policy 'static' reads one field at every time stamp (policy 'clock' needs one "
                  "per time stamp)")
    elif data.shape[0] != T or tuple(data.shape[1:]) != tuple(g.shape):
        error('data must hold one value function per time stamp (time first), or one field of g.shape with policy static')
    k = _index(extraArgs, 'slice', 1 if single else T) if policy == 'static' else 0
    tensors = _wants_tensor(data) or _wants_tensor(x0s)
    x0 = states_2d(g, x0s)
    M = int(x0.shape[0])
    nom, nomMode, u_nom = None, uMode, None
    if isinstance(nominal, Bundle):
        if not isfield(nominal, 'data'):
            error('a value-function nominal is Bundle(data=..., uMode=...)')
        nom = nominal.data
        nomMode = _get(nominal, 'uMode', uMode)
        if nomMode not in _MODES:
            error("nominal.uMode must be 'min' or 'max'")
        if tuple(nom.shape) != tuple(g.shape) and tuple(nom.shape) != (T,) + tuple(g.shape):
            error('nominal.data must be a value function on the grid of data: shape %s or %s, got %s'
                  % (tuple(g.shape), (T,) + tuple(g.shape), tuple(nom.shape)))
    else:
        u_nom = _table(nominal, (T - 1,), M, 'nominal')
    nat, why = _why_host(dynSys, derivFunc, g, plant_builtin.flag(extraArgs))
    if why is None:
        plant, NU, W, ffi = _kernel_plant(nat, uMode, dMode)
        if u_nom is not None and int(u_nom.shape[-1]) != NU:
            error('nominal holds %d controls per column, %s has %d' % (int(u_nom.shape[-1]), type(dynSys).__name__, NU))
        torch = require_gpu()
        t = _device_data(data)
        xs = _device_states(x0, t.device)
        un = _device_states(u_nom, t.device) if u_nom is not None else None
        nt = _device_data(nom).to(device=t.device, dtype=t.dtype).contiguous() if nom is not None else None
        dtSmall = (tau[1] - tau[0]) / subSamples                     # exactly as computeOptTraj forms it
        per = max(1, LAUNCH_THREADS >> g.dim)                        # states one launch holds
        parts = []
        for a in range(0, max(M, 1), per):
            b = min(M, a + per)
            parts.append(filtered_rollout_states(g, t, T, xs[a:b], point_scheme(derivFunc), subSamples, dtSmall, plant,
                                                 _fffi.POLICIES[policy], k, un[a:b] if un is not None else None, nt, _MODES[nomMode],
                                                 level, margin, _fffi.DISTURBANCES[dstb], keep, keep_controls, W))
        _last_path = ffi.last_kernel() if M else ""
        outs = [parts[0][i] if len(parts) == 1 else (torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None)
                for i in range(10)]
        if outs[8] is not None:
            outs[8] = outs[8].bool()
        if not tensors:
            outs = [o.cpu().numpy() if o is not None else None for o in outs]
    else:
        _last_path = "host loop: " + why
        info('computeSafeTrajs: ' + _last_path)
        x0 = x0.detach().cpu().numpy() if is_tensor(x0) else x0
        un = u_nom.detach().cpu().numpy() if is_tensor(u_nom) else u_nom
        outs = list(_host_loop(g, data, tau, dynSys, np.asarray(x0, dtype=np.float64), un, nom, nomMode, uMode, dMode, subSamples,
                               derivFunc, level, margin, dstb == 'zero', policy == 'clock', k, keep, keep_controls))
        if tensors:
            torch = require_gpu()
            dev = _out_device(torch, data, x0s)
            outs = [torch.as_tensor(o, device=dev) if o is not None else None for o in outs]
    final, gmin, vend, count, first, length, status, trajs, active, applied = outs
    return Bundle(dict(trajs=trajs, final=final, gapMin=gmin, valueEnd=vend, interventions=count, firstIntervention=first,
                       status=status, length=length, active=active, controls=applied, tau=tau, path=_last_path))


def safeControls(g, data, dynSys, xs, uNom, extraArgs=None):
    global _last_path
    uMode, dMode, derivFunc, margin, level, dstb = _common(extraArgs)
    single = tuple(data.shape) == tuple(g.shape)
    if not single and (len(data.shape) != g.dim + 1 or tuple(data.shape[1:]) != tuple(g.shape) or data.shape[0] < 1):
        error('data must be one value function of g.shape, or a stack of them (time first) with extraArgs.slice')
    k = _index(extraArgs, 'slice', 1 if single else int(data.shape[0]))
    tensors = _wants_tensor(data) or _wants_tensor(xs)
    x = states_2d(g, xs)
    M = int(x.shape[0])
    u_nom = _table(uNom, (), M, 'uNom')
    nat, why = _why_host(dynSys, derivFunc, g, plant_builtin.flag(extraArgs))
    if why is None:
        plant, NU, W, ffi = _kernel_plant(nat, uMode, dMode)
        if int(u_nom.shape[-1]) != NU:
            error('uNom holds %d controls per state, %s has %d' % (int(u_nom.shape[-1]), type(dynSys).__name__, NU))
        t = _device_data(data)
        outs = list(decide_states(g, t, k, _device_states(x, t.device), point_scheme(derivFunc), plant, _device_states(u_nom, t.device),
                                  level, margin, _fffi.DISTURBANCES[dstb], W))
        _last_path = ffi.last_kernel() if M else ""
        outs[1] = outs[1].bool()
        if not tensors:
            outs = [o.cpu().numpy() for o in outs]
    else:
        _last_path = "host loop: " + why
        info('safeControls: ' + _last_path)
        xh = np.asarray(x.detach().cpu().numpy() if is_tensor(x) else x, dtype=np.float64)
        un = u_nom.detach().cpu().numpy() if is_tensor(u_nom) else u_nom
        V = _HostField(g, data, derivFunc)
        held, active, value, gap, costate = [], np.zeros(M, dtype=bool), np.empty(M), np.empty(M), np.empty((M, g.dim))
        for m in range(M):
            plant = copy.copy(dynSys)
            plant.x = xh[m]
            deriv = V.costate(k, xh[m])
            value[m] = V.value(k, xh[m])
            active[m], gap[m], u, d = _host_decision(plant, 0.0, xh[m], value[m], deriv, uMode, dMode, level, margin, dstb == 'zero',
                                                     lambda: _as_control(un[m]))
            costate[m] = deriv
            held.append(_flat(u) + _flat(d))
        applied = np.zeros((M, max([2] + [len(h) for h in held])))
        for m, h in enumerate(held):
            applied[m, :len(h)] = h
        outs = [applied, active, value, gap, costate]
        if tensors:
            torch = require_gpu()
            dev = _out_device(torch, data, xs)
            outs = [torch.as_tensor(o, device=dev) for o in outs]
    applied, active, value, gap, costate = outs
    return Bundle(dict(controls=applied, active=active, value=value, gap=gap, costate=costate, path=_last_path))
