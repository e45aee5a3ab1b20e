"""computeOptTrajs: computeOptTraj (opt_traj.py) for many initial states at once.

    trajs, lengths, tau = computeOptTrajs(g, data, tau, dynSys, x0s, extraArgs)
    trajs, lengths, tau, extraOuts = computeOptTrajs(..., extraArgs with tEarliest=True or status=True)

`data` and `tau` are computeOptTraj's: the time-first stack ordered like the toolbox's `dataTraj = flip(data)` and its
time stamps.  `x0s` holds one initial state per row.  trajs is (M, g.dim, len(tau)): trajectory m is
trajs[m, :, :lengths[m]] -- what computeOptTraj returns for x0s[m] --, the columns past lengths[m] hold NaN.
extraOuts.status is one of REACHED / EXHAUSTED / LEFT_GRID per trajectory (LEFT_GRID: one of its recorded states is
outside an extrapolated axis or not finite; such a trajectory runs to full length with NaN states, as computeOptTraj
returns it), extraOuts.tEarliest (M, len(tau)) the index the bisection settled on at every column (-1 where none ran),
extraOuts.path the kernel that ran, or 'host loop: <why>'.  NumPy in -> NumPy out; a device tensor (data or x0s) in ->
device tensors out.  extraArgs: uMode, dMode, subSamples and derivFunc as computeOptTraj reads them.  dynSys.x is not
touched.

With one of the built-in systems (dynamics.py) and upwindFirstENO2 / ENO3 / WENO5 (as shipped) the whole horizon of every
trajectory -- the bisection over the stored sets, the costates, the controls, the RK4 sub-steps -- is ONE launch of
rollout_kernel (libhj_rollout.so, include/hj_rollout.h), and the result equals computeOptTraj's with that system's own
methods bit for bit up to the device's sin / cos.  Plane5D and DubinsPair6D on a 5-D / 6-D grid take the same path in
hi_rollout_kernel (libhj_hiquery.so, include/hj_hiquery.h), which compiles the trajectory's source at six axes; uMode and dMode
are resolved as computeOptTraj resolves them.  A dynSys with a registered plant (plant.register_plant) runs in user_rollout_kernel
(libhj_plant.so, include/hj_plant.h), the same trajectory compiled at run time around the user's controls and dynamics.  Any other
dynSys -- a foreign class, a subclass that overrides a protocol method, non-scalar bounds -- or derivative function takes a
host loop: computeOptTraj on copy.copy(dynSys) once per state, padded the same way.

Parity UNPINNED: the reference's computeOptTraj cannot run (opt_traj.py), and it has no batched form.
"""
import copy
import ctypes as C

import numpy as np

from . import _ffi, _hffi, _pffi, _rffi, _xffi
from .context import grid_bc, is_tensor, require_gpu
from .dynamics import native_plant, native_plant_hi
from .opt_traj import computeOptTraj, find_earliest_BRS_ind
from .query import point_scheme, states_2d
from .spatial import upwindFirstWENO5
from .utilities import Bundle, error, info, isfield
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, device_data as _device_data,
                       device_states as _device_states, stream as _stream, ptr as _ptr, fields as _fields,
                       descriptor as _descriptor, dtype_name as _dtype_name, descriptor_hi as _descriptor_hi, is_hi as _is_hi)

__all__ = ["computeOptTrajs", "REACHED", "EXHAUSTED", "LEFT_GRID"]

REACHED, EXHAUSTED, LEFT_GRID = _rffi.REACHED, _rffi.EXHAUSTED, _rffi.LEFT_GRID

_MODES = {'min': _rffi.MODE_MIN, 'max': _rffi.MODE_MAX}
_last_path = ""


def last_path():
    """What the calling process's last computeOptTrajs ran: the kernel's name, or 'host loop: <why>'."""
    return _last_path


def _get(extraArgs, name, default):
    return getattr(extraArgs, name) if extraArgs is not None and isfield(extraArgs, name) and getattr(extraArgs, name) is not None else default


def _why_host(dynSys, derivFunc, g):
    """None when the kernel covers this call, else the reason for the host loop."""
    nat = native_plant(dynSys) or native_plant_hi(dynSys)
    if nat is None:
        from .plant import plant_of
        user = plant_of(dynSys)                          # (registration, parameters): a plant registered at run time
        if user is None:
            return None, "%s has no native plant" % type(dynSys).__name__
        if user[0].dim != g.dim:
            return None, "%s has no native plant on a %d-D grid" % (type(dynSys).__name__, g.dim)
        if point_scheme(derivFunc) is None:
            return None, "derivFunc %s has no point kernel" % getattr(derivFunc, "__name__", derivFunc)
        return user, None
    if (_hffi.HAM_DIMS if nat[0] in _hffi.HAM_DIMS else _rffi.PLANT_DIMS).get(nat[0]) != g.dim:
        return None, "%s has no native plant on a %d-D grid" % (type(dynSys).__name__, g.dim)
    if point_scheme(derivFunc) is None:
        return None, "derivFunc %s has no point kernel" % getattr(derivFunc, "__name__", derivFunc)
    return nat, None


def rollout_states(g, data, xs, scheme, subSamples, dtSmall, plant, want_te=False):
    """hjr_rollout on device tensors: `data` a contiguous (T,) + g.shape stack, `xs` an (M, dim) fp64 tensor, `plant` an
    _rffi.Plant, or a _pffi.Plant for hjp_rollout / hjp_rollout_hi.
    -> (traj (M, dim, T) fp64, length (M,) int32, tEarliest (M, T) int32 or None, status (M,) int32)."""
    torch = require_gpu()
    hi = _is_hi(g)                                   # 5-D / 6-D: hjx_rollout (libhj_hiquery.so), the same call on hjh_grid
    desc, N = (_descriptor_hi if hi else _descriptor)(g, _dtype_name(data))
    if isinstance(plant, _pffi.Plant):
        ffi, call = _pffi, (_pffi.lib().hjp_rollout_hi if hi else _pffi.lib().hjp_rollout)
    else:
        ffi, call = (_xffi, _xffi.lib().hjx_rollout) if hi else (_rffi, _rffi.lib().hjr_rollout)
    T, stride = _fields(data, N)
    if xs.dim() != 2 or xs.shape[1] != g.dim:
        error('states must be an (M, %d) array' % g.dim)
    M = int(xs.shape[0])
    traj = torch.empty((M, g.dim, T), dtype=torch.float64, device=data.device)
    length = torch.empty((M,), dtype=torch.int32, device=data.device)
    status = torch.empty((M,), dtype=torch.int32, device=data.device)
    te = torch.empty((M, T), dtype=torch.int32, device=data.device) if want_te else None
    with torch.cuda.device(data.device):
        ffi.check(call(C.byref(desc), int(scheme), _ptr(data), T, stride, _ptr(xs), M, int(subSamples),
                       float(dtSmall), C.byref(plant), _ptr(traj), _ptr(length), _ptr(te), _ptr(status),
                       _stream(torch, data.device)))
    return traj, length, te, status


def _outside(g, cols):
    """Per column of a (dim, n) array: outside an extrapolated axis, or not finite."""
    bc, _ = grid_bc(g)
    bad = ~np.isfinite(cols).all(axis=0)
    with np.errstate(invalid='ignore'):
        for d in range(g.dim):
            if bc[d] != _ffi.BC_PERIODIC:
                v = np.asarray(g.vs[d], dtype=np.float64).ravel()
                bad |= (cols[d] < v[0]) | (cols[d] > v[-1])
    return bad


def _host_loop(g, data, tau, dynSys, x0, extraArgs, want_te):
    """computeOptTraj once per state, padded to the kernel's output contract (NumPy)."""
    M, T = x0.shape[0], len(tau)
    trajs = np.full((M, g.dim, T), np.nan)
    lengths = np.zeros(M, dtype=np.int32)
    status = np.zeros(M, dtype=np.int32)
    te = np.full((M, T), -1, dtype=np.int32) if want_te else None
    args = extraArgs if extraArgs is not None else Bundle({})
    for m in range(M):
        plant = copy.copy(dynSys)
        plant.x = x0[m].copy()
        traj, _ = computeOptTraj(g, data, tau, plant, args)
        n = traj.shape[1]
        trajs[m, :, :n] = traj
        lengths[m] = n
        status[m] = LEFT_GRID if _outside(g, traj).any() else (REACHED if n < T else EXHAUSTED)
        if want_te:
            cur = 0
            for it in range(min(n, T - 1)):          # the columns at which computeOptTraj bisected
                cur = find_earliest_BRS_ind(g, data, traj[:, it], T - 1, cur)
                te[m, it] = cur
    return trajs, lengths, te, status


def computeOptTrajs(g, data, tau, dynSys, x0s, extraArgs=None):
    global _last_path
    uMode = _get(extraArgs, 'uMode', 'min')
    dMode = _get(extraArgs, 'dMode', None)
    subSamples = int(_get(extraArgs, 'subSamples', 4))
    derivFunc = _get(extraArgs, 'derivFunc', upwindFirstWENO5)
    want_te = bool(_get(extraArgs, 'tEarliest', False))
    want_outs = want_te or bool(_get(extraArgs, 'status', False))
    tau = np.asarray(tau, dtype=np.float64).ravel()
    if np.any(np.diff(tau) < 0):
        error('Time stamps must be in ascending order!')
    if len(tau) < 2:
        error('a trajectory needs at least two time stamps')
    if data.shape[0] != len(tau) or tuple(data.shape[1:]) != tuple(g.shape):
        error('data must hold one value function per time stamp (time first)')
    if subSamples < 1:
        error('subSamples must be positive')
    tensors = _wants_tensor(data) or _wants_tensor(x0s)
    x0 = states_2d(g, x0s)
    nat, why = _why_host(dynSys, derivFunc, g)
    if why is None:
        if uMode not in _MODES or (dMode is not None and dMode not in _MODES):
            error("uMode / dMode must be 'min' or 'max'")
        t = _device_data(data)
        xs = _device_states(x0, t.device)
        user = not isinstance(nat[0], int)
        if user:
            plant = _pffi.plant_descriptor(nat[0].plant_id, _MODES[uMode], _MODES[dMode or 'min'], nat[1])
        else:
            plant = _rffi.plant_descriptor(nat[0], _MODES[uMode], _MODES[dMode or 'min'], nat[1])
        dtSmall = (tau[1] - tau[0]) / subSamples                 # exactly as computeOptTraj forms it
        trajs, lengths, te, status = rollout_states(g, t, xs, point_scheme(derivFunc), subSamples, dtSmall, plant, want_te)
        _last_path = (_pffi if user else (_xffi if _is_hi(g) else _rffi)).last_kernel()
        if not tensors:
            trajs, lengths, status = (a.cpu().numpy() for a in (trajs, lengths, status))
            te = te.cpu().numpy() if te is not None else None
    else:
        _last_path = "host loop: " + why
        info('computeOptTrajs: ' + _last_path)
        x0 = x0.detach().cpu().numpy() if is_tensor(x0) else x0
        trajs, lengths, te, status = _host_loop(g, data, tau, dynSys, np.asarray(x0, dtype=np.float64), extraArgs, want_te)
        if tensors:
            torch = require_gpu()
            d = _unlazy(data)
            dev = d.device if is_tensor(d) and d.is_cuda else (x0s.device if is_tensor(x0s) and x0s.is_cuda else "cuda")
            trajs, lengths, status = (torch.as_tensor(a, device=dev) for a in (trajs, lengths, status))
            te = torch.as_tensor(te, device=dev) if te is not None else None
    if not want_outs:
        return trajs, lengths, tau
    outs = Bundle(dict(status=status, path=_last_path))
    if want_te:
        outs.tEarliest = te
    return trajs, lengths, tau, outs
