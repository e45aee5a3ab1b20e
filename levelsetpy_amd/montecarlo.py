"""computeStochTrajs: Monte Carlo rollouts of dx = f(x, u*, d*) dt + G dW through a stored value function, and
reachProbability on their results.

    outs = computeStochTrajs(g, data, tau, dynSys, x0s, sigma, extraArgs)
    p, stderr = reachProbability(outs, level=0.0, kind='end')

`data`, `tau`, `dynSys` and `x0s` are computeOptTrajs' (rollout.py): the time-first stack ordered like the toolbox's
`dataTraj = flip(data)`, its time stamps, the system and one initial state per row.  `sigma` is what HJIPDE_solve takes as
extraArgs.addGaussianNoiseStandardDeviation (stochastic.check_sigma), a g.dim x g.dim matrix of numbers only: a cell matrix or
a callable -- a sigma that varies with state or time -- is refused by name.  The solver's PDE phi_t + H = trace(sigma^T D^2phi
sigma) has no 1/2, so the diffusion of the rollout is G = sqrt(2) sigma (G G^T = 2 sigma sigma^T).

Every realisation is the trajectory of computeOptTrajs with x <- x + sqrt(dt_small) (G xi) after every RK4 sub-step, xi the
standard normals of (realisation, step): include/hj_mc.h states it operation by operation.  outs holds, per initial state m and
realisation k: final (M, R, dim) the last recorded state, length and status (M, R) as computeOptTrajs', valueEnd (M, R) the
target function V[T-1] at the last recorded state, valueMin (M, R) its NaN-propagating minimum over all recorded states;
trajs (M, R, dim, T) and tEarliest (M, R, T) with keepTrajs, else None; tau, seed, and path: the kernel that ran, or
'host loop: <why>'.  NumPy in -> NumPy out; a device tensor (data or x0s) in -> device tensors out.

extraArgs: uMode, dMode, subSamples, derivFunc as computeOptTrajs reads them; realisations (R, default 1); seed (0 .. 2^64-1,
default 0); policy 'earliest' (computeOptTraj's bisection: stop inside the last stored set; the default) or 'clock' (slice `it`
at column `it`, the time-consistent policy of a compMethod='none' solve: with it E[l(x_T)] = V(x0, 0) up to discretisation);
keepTrajs (default False); normals, an (M, R, (T-1) subSamples, dim) fp64 array that replaces the generator (bit-for-bit tests,
common random numbers); firstRealisation, the global index of realisation 0 of state 0 (default 0).  Realisation k of state m has
the global index firstRealisation + m R + k, and its normals depend on (seed, index, step) alone -- Philox4x32-10 as a counter --
so a call over states [a:b] with firstRealisation = a R gives the slice of the full call, and a call is split over states
wherever one launch would not hold it.

With a built-in 2-D .. 4-D system (native_plant's identity rule) and upwindFirstENO2 / ENO3 / WENO5 (as shipped) a call is ONE
launch of noisy_rollout_kernel (libhj_mc.so) per split.  Plane5D / DubinsPair6D, a registered plant, a foreign dynSys or a
derivative function without a point kernel take a host loop on dynSys.get_opt_u / get_opt_v / update_state with the same
generator (hjn_normals_host) and the same output contract, and say so in an info line.

extraArgs.plantKernel=True (a bool, default False) sends two more kinds of system to a kernel, after the built-in rule: a registered plant
(plant.register_plant; plant_of's identity rule, the registration's dimension, a derivative function with a point kernel) and Plane5D /
DubinsPair6D, which the package registers itself at their first use (plant_builtin.py).  libhj_plant.so compiles
user_noisy_rollout_kernel around the plant at run time, under the contract above word for word; whatever is not eligible under the flag
keeps the host loop and its info line.

reachProbability forms its sums with torch / NumPy on the returned arrays: the kernel uses no float atomics.
Parity UNPINNED: the reference has no counterpart (its computeOptTraj cannot run).
"""
import copy
import ctypes as C

import numpy as np

from . import _nffi, _pffi, _rffi, plant_builtin
from .context import is_tensor, require_gpu
from .dynamics import native_plant, native_plant_hi
from .query import interp_states, costate_states, point_scheme, states_2d
from .rollout import _get, _outside, REACHED, EXHAUSTED, LEFT_GRID
from .spatial import upwindFirstWENO5
from .stochastic import check_sigma
from .utilities import Bundle, error, info
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, device_data as _device_data,
                       device_states as _device_states, stream as _stream, ptr as _ptr, fields as _fields,
                       descriptor as _descriptor, dtype_name as _dtype_name, is_hi as _is_hi, descriptor_hi as _descriptor_hi)
from .plant import PlantRegistration

__all__ = ["computeStochTrajs", "reachProbability"]

_MODES = {'min': _rffi.MODE_MIN, 'max': _rffi.MODE_MAX}
# threads one launch may hold (hj_tool_host.h's blocks_for refuses 2^32 - 255 and more); a call over more is split over states
LAUNCH_THREADS = 2 ** 32 - 256
_last_path = ""


def last_path():
    """What the calling process's last computeStochTrajs ran: the kernel's name, or 'host loop: <why>'."""
    return _last_path


def _why_host(dynSys, derivFunc, g, plantKernel=False):
    """(plant, None) when a kernel covers this call, else (None, the reason for the host loop).  plant: native_plant's (id, parameters),
    or under plantKernel (registration, parameters) of a plant libhj_plant.so compiles a kernel around -- the built-in rule comes first."""
    nat = native_plant(dynSys)
    if plantKernel and nat is None:
        user, why = plant_builtin.route(dynSys, derivFunc, g)
        if user is not None or why is not None:
            return user, why
    if nat is None:
        if native_plant_hi(dynSys) is not None:
            return None, "%s has no noisy rollout kernel (5-D / 6-D systems are out of its scope)" % type(dynSys).__name__
        from .plant import plant_of
        if plant_of(dynSys) is not None:
            return None, "%s is a registered plant: it has no noisy rollout kernel" % type(dynSys).__name__
        return None, "%s has no native plant" % type(dynSys).__name__
    if _nffi.PLANT_DIMS.get(nat[0]) != g.dim:
        return None, "%s has no native plant on a %d-D grid" % (type(dynSys).__name__, g.dim)
    if point_scheme(derivFunc) is None:
        return None, "derivFunc %s has no point kernel" % getattr(derivFunc, "__name__", derivFunc)
    return nat, None


def noisy_rollout_states(g, data, xs, scheme, subSamples, dtSmall, plant, G, sq, R, first, seed, normals, policy, keep):
    """hjn_rollout (hjp_noisy_rollout / _hi for a _pffi.Plant) on device tensors: `data` a contiguous (T,) + g.shape stack, `xs` an (M, dim) fp64 tensor, `normals` None or an
    (M, R, (T-1) subSamples, dim) fp64 device tensor, `G` a (dim, dim) float64 NumPy array.
    -> final, length, status, value_end, value_min, traj or None, t_earliest or None."""
    torch = require_gpu()
    if isinstance(plant, _pffi.Plant):
        hi = _is_hi(g)
        ffi, call, describe = _pffi, (_pffi.lib().hjp_noisy_rollout_hi if hi else _pffi.lib().hjp_noisy_rollout), (_descriptor_hi if hi else _descriptor)
    else:
        ffi, call, describe = _nffi, _nffi.lib().hjn_rollout, _descriptor
    desc, N = describe(g, _dtype_name(data))
    T, stride = _fields(data, N)
    M, nd = int(xs.shape[0]), g.dim
    dev = data.device
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)        # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)          # noqa: E731
    final, length, status, vend, vmin = f64(M, R, nd), i32(M, R), i32(M, R), f64(M, R), f64(M, R)
    traj, te = (f64(M, R, nd, T), i32(M, R, T)) if keep else (None, None)
    Gm = np.ascontiguousarray(G, dtype=np.float64)
    with torch.cuda.device(dev):
        ffi.check(call(C.byref(desc), int(scheme), _ptr(data), T, stride, _ptr(xs), M, int(R), int(first),
                       int(seed), _ptr(normals), Gm.ctypes.data, float(sq), int(policy), int(subSamples),
                       float(dtSmall), C.byref(plant), _ptr(final), _ptr(length), _ptr(status), _ptr(vend),
                       _ptr(vmin), _ptr(traj), _ptr(te), _stream(torch, dev)))
    return final, length, status, vend, vmin, traj, te


def _nmin(a, b):
    return np.nan if (a != a or b != b) else (b if b < a else a)


def _host_loop(g, data, tau, dynSys, x0, G, sq, R, first, seed, normals, policy, uMode, dMode, subSamples, derivFunc, keep):
    """The realisations one by one on dynSys's own protocol methods, to the kernel's output contract (NumPy).  The values and
    the costates are the device's point queries, as in computeOptTraj."""
    from .gradients import computeGradients
    from .hji_solver import _eval_point
    M, T, nd = x0.shape[0], len(tau), g.dim
    nsteps = (T - 1) * subSamples
    dtSmall = (tau[1] - tau[0]) / subSamples
    t = _device_data(data)
    sid = point_scheme(derivFunc)
    tables = {}
    final = np.empty((M, R, nd))
    length, status = np.empty((M, R), dtype=np.int32), np.empty((M, R), dtype=np.int32)
    vend, vmin = np.empty((M, R)), np.empty((M, R))
    trajs = np.full((M, R, nd, T), np.nan) if keep else None
    te = np.full((M, R, T), -1, dtype=np.int32) if keep else None

    def values(x):                                  # V of every stored set at x, fp64
        return interp_states(g, t, _device_states(x.reshape(1, -1), t.device), out_f64=True)[:, 0].cpu().numpy()

    def costate(k, x):
        if sid is not None:
            xs = _device_states(x.reshape(1, -1), t.device)
            return costate_states(g, t[k], xs, sid, out_f64=True)[0][0, 0].cpu().numpy().tolist()
        if k not in tables:
            tables[k] = computeGradients(g, data[k], derivFunc=derivFunc)[0]
        return [_eval_point(g, tables[k][d], x) for d in range(nd)]

    for m in range(M):
        for k in range(R):
            q = m * R + k
            xi = np.asarray(normals[m, k], dtype=np.float64) if normals is not None else \
                _nffi.normals_host(seed, first + q, 1, 0, nsteps, nd)[0]
            plant = copy.copy(dynSys)
            x = np.array(x0[m], dtype=np.float64)
            if keep:
                trajs[m, k, :, 0] = x
            vals = values(x)
            ve = vm = float(vals[T - 1])
            left = bool(_outside(g, x.reshape(-1, 1))[0])
            tE, n, reached = 0, 1, False
            for it in range(T - 1):
                if policy == _nffi.POLICY_CLOCK:
                    tE = it
                else:
                    lower, upper = tE, T - 1
                    while upper > lower:
                        mid = (upper + lower + 1) // 2
                        if vals[mid] < 1e-4:
                            lower = mid
                        else:
                            upper = mid - 1
                    tE = upper
                    if tE == T - 1:
                        reached = True
                if keep:
                    te[m, k, it] = tE
                if reached:
                    break
                for s in range(subSamples):
                    plant.x = x
                    deriv = costate(tE, x)
                    u = plant.get_opt_u(tau[tE], deriv, uMode, x)
                    d = plant.get_opt_v(tau[tE], deriv, dMode, x) if hasattr(plant, 'get_opt_v') else None
                    xt = plant.update_state(u, dtSmall, x, d)
                    x = np.array(xt if xt is not None else plant.x, dtype=np.float64).ravel()
                    z = xi[it * subSamples + s]
                    step = np.empty(nd)
                    for i in range(nd):
                        acc = G[i, 0] * z[0]
                        for j in range(1, nd):
                            acc = acc + G[i, j] * z[j]
                        step[i] = sq * acc
                    x = x + step
                n = it + 2
                left = left or bool(_outside(g, x.reshape(-1, 1))[0])
                vals = values(x)
                ve = float(vals[T - 1])
                vm = _nmin(vm, ve)
                if keep:
                    trajs[m, k, :, it + 1] = x
            final[m, k] = x
            length[m, k] = n
            status[m, k] = LEFT_GRID if left else (REACHED if reached else EXHAUSTED)
            vend[m, k], vmin[m, k] = ve, vm
    return final, length, status, vend, vmin, trajs, te


def computeStochTrajs(g, data, tau, dynSys, x0s, sigma, extraArgs=None):
    global _last_path
    uMode = _get(extraArgs, 'uMode', 'min')
    dMode = _get(extraArgs, 'dMode', None)
    subSamples = int(_get(extraArgs, 'subSamples', 4))
    derivFunc = _get(extraArgs, 'derivFunc', upwindFirstWENO5)
    R = _get(extraArgs, 'realisations', 1)
    seed = _get(extraArgs, 'seed', 0)
    policy = _get(extraArgs, 'policy', 'earliest')
    keep = bool(_get(extraArgs, 'keepTrajs', False))
    normals = _get(extraArgs, 'normals', None)
    first = _get(extraArgs, 'firstRealisation', 0)
    tau = np.asarray(tau, dtype=np.float64).ravel()
    if np.any(np.diff(tau) < 0):
        error('Time stamps must be in ascending order!')
    if len(tau) < 2:
        error('a trajectory needs at least two time stamps')
    if data.shape[0] != len(tau) or tuple(data.shape[1:]) != tuple(g.shape):
        error('data must hold one value function per time stamp (time first)')
    if subSamples < 1:
        error('subSamples must be positive')
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or R < 1:
        error('extraArgs.realisations must be a positive integer (got %r)' % (R,))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        error('extraArgs.seed must be an integer in 0 .. 2^64-1 (got %r)' % (seed,))
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or not 0 <= int(first) < 2 ** 64:
        error('extraArgs.firstRealisation must be an integer in 0 .. 2^64-1 (got %r)' % (first,))
    if policy not in _nffi.POLICIES:
        error("extraArgs.policy must be 'earliest' or 'clock' (got %r)" % (policy,))
    if uMode not in _MODES or (dMode is not None and dMode not in _MODES):
        error("uMode / dMode must be 'min' or 'max'")
    R, seed, first = int(R), int(seed), int(first)
    kind, S = check_sigma(sigma, g.dim)
    if kind != 'numbers':
        error('computeStochTrajs: sigma is a %s: only a %d x %d matrix of numbers is rolled out (a sigma that varies with '
              'state or time is out of scope)' % ('cell matrix' if kind == 'cell' else 'callable', g.dim, g.dim))
    G = np.sqrt(2.0) * S
    tensors = _wants_tensor(data) or _wants_tensor(x0s) or _wants_tensor(normals)
    x0 = states_2d(g, x0s)
    M, T = int(x0.shape[0]), len(tau)
    nsteps = (T - 1) * subSamples
    if normals is not None:
        normals = _unlazy(normals)
        if tuple(normals.shape) != (M, R, nsteps, g.dim):
            error('extraArgs.normals must have shape (M, realisations, (len(tau) - 1) * subSamples, g.dim) = %s, got %s'
                  % ((M, R, nsteps, g.dim), tuple(normals.shape)))
    dtSmall = (tau[1] - tau[0]) / subSamples                     # exactly as computeOptTraj forms it
    sq = float(np.sqrt(np.float64(dtSmall)))
    pol = _nffi.POLICIES[policy]
    plantKernel = plant_builtin.flag(extraArgs)
    if plantKernel or not _is_hi(g):                             # (a built-in plant on a 5-D / 6-D grid is refused by its dimension there)
        nat, why = _why_host(dynSys, derivFunc, g, plantKernel)
    else:
        nat, why = None, "%s has no noisy rollout kernel on a %d-D grid" % (type(dynSys).__name__, g.dim)
    if why is None:
        user = isinstance(nat[0], PlantRegistration)
        ffi = _pffi if user else _nffi
        t = _device_data(data)
        xs = _device_states(x0, t.device)
        nz = _device_states(normals, t.device) if normals is not None else None
        plant = (_pffi.plant_descriptor(nat[0].plant_id, _MODES[uMode], _MODES[dMode or 'min'], nat[1]) if user
                 else _rffi.plant_descriptor(nat[0], _MODES[uMode], _MODES[dMode or 'min'], nat[1]))
        per = max(1, (LAUNCH_THREADS >> g.dim) // R)             # states one launch holds
        parts = []
        for a in range(0, max(M, 1), per):
            b = min(M, a + per)
            parts.append(noisy_rollout_states(g, t, xs[a:b], point_scheme(derivFunc), subSamples, dtSmall, plant, G, sq, R,
                                              (first + a * R) % 2 ** 64, seed, nz[a:b] if nz is not None else None, pol, keep))
        _last_path = ffi.last_kernel() if M else ""
        torch = require_gpu()
        outs = [parts[0][i] if len(parts) == 1 else (torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None)
                for i in range(7)]
        if not tensors:
            outs = [o.cpu().numpy() if o is not None else None for o in outs]
    else:
        _last_path = "host loop: " + why
        info('computeStochTrajs: ' + _last_path)
        x0 = x0.detach().cpu().numpy() if is_tensor(x0) else x0
        nz = normals.detach().cpu().numpy() if is_tensor(normals) else normals
        outs = list(_host_loop(g, data, tau, dynSys, np.asarray(x0, dtype=np.float64), G, sq, R, first, seed, nz, pol, uMode, dMode,
                               subSamples, derivFunc, keep))
        if tensors:
            torch = require_gpu()
            d = _unlazy(data)
            dev = d.device if is_tensor(d) and d.is_cuda else (x0s.device if is_tensor(x0s) and x0s.is_cuda else "cuda")
            outs = [torch.as_tensor(o, device=dev) if o is not None else None for o in outs]
    final, length, status, vend, vmin, trajs, te = outs
    return Bundle(dict(final=final, length=length, status=status, valueEnd=vend, valueMin=vmin, trajs=trajs, tEarliest=te,
                       tau=tau, seed=seed, path=_last_path))


def reachProbability(outs, level=0.0, kind='end'):
    """(p, stderr) per initial state: the share of its realisations whose valueEnd (kind 'end': the state at the end is in the
    level set of the target function) or valueMin (kind 'min': the path entered it at a recorded time) is below `level`, and
    sqrt(p (1 - p) / R).  A NaN value (the realisation left the grid) counts as a miss.  Arrays of the type of outs' own."""
    if kind not in ('end', 'min'):
        error("reachProbability: kind must be 'end' or 'min' (got %r)" % (kind,))
    v = outs.valueEnd if kind == 'end' else outs.valueMin
    R = int(v.shape[1])
    if is_tensor(v):
        torch = require_gpu()
        p = (v < level).to(torch.float64).sum(dim=1) / R
        return p, torch.sqrt(p * (1.0 - p) / R)
    p = (np.asarray(v) < level).astype(np.float64).sum(axis=1) / R
    return p, np.sqrt(p * (1.0 - p) / R)
