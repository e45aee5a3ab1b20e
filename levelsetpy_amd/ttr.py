"""Time-to-reach functions on the device: postTimeStepTTR (reference Helper/post_ttr.py:8) and TD2TTR (helperOC's
TD2TTR.m) -- for every node, the time at which the sublevel set {y <= level} first (or last) swept over it, +inf where
it never did: the minimum-time value function that time-optimal controllers read.

All of it runs in libhj_ttr.so (include/hj_ttr.h): `ttr_init_kernel`, `ttr_update_kernel` (one step of the
recurrence, in place) and `ttr_from_stack_kernel` (a stored time-first stack folded in one pass: every value read
once, the result written once).  The recurrence, in fp64, every operation rounded on its own:

    a = last_y - level;  b = y - level
    changed = (y <= level) & (last_y > level)            a NaN compares false: a NaN node never changes
    'first' crossing:  changed &= (ttr == +inf)
    tc = t_last - ((t - t_last) * a) / (b - a)           or t when interpolation is off
    ttr[changed] = tc[changed];  last_y = y

With crossing 'last' (the toolbox's postTimestepTTR) every inward crossing overwrites; 'first' keeps the earliest one,
which is the minimum time to reach (helperOC's TD2TTR).  Times are fp64 whatever the data's dtype.  A node that comes
from +inf interpolates to inf / inf = NaN, as the formula says; such nodes keep their meaning with interpolate=False.

NumPy in -> NumPy out for TD2TTR; a device tensor or HostView in -> a tensor on the same device.  The state that
postTimeStepTTR keeps in schemeData lives on the device: tensors for a tensor caller, HostViews (materialised by
np.asarray) for a NumPy caller.

Parity.  PINNED to the reference (tests/golden/ttr.npz): the initialisation branch of its postTimeStepTTR -- the only
branch of it that runs.  UNPINNED, checked against the NumPy restatement tests/ttr_ref.py: the update (the shipped
reference takes np.logical_and of two np.nonzero index vectors and applies scalar `@` to an array: it raises on the
second call), the 'first' rule, levels other than 0, TD2TTR and HJIPDE_solve's computeTTR.  The restatement follows the
toolbox semantics that the reference's docstring describes.
"""
import copy

import numpy as np

from . import _ffi, _tffi
from .context import is_tensor, require_gpu
from .lazy import HostView
from .utilities import isfield, error
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, device_data as _device_data,
                       stream as _stream, ptr as _ptr, fields as _fields)

__all__ = ["postTimeStepTTR", "TD2TTR"]


def mode_bits(crossing, interpolate):
    if crossing not in ('first', 'last'):
        error('crossing must be \'first\' or \'last\' (got %r)' % (crossing,))
    return (_tffi.FIRST if crossing == 'first' else 0) | (0 if interpolate else _tffi.NO_INTERP)


def _dtype_id(torch, t):
    return _ffi.F32 if t.dtype == torch.float32 else _ffi.F64


# ------------------------------------------------------------------------------------------ the three launches
def ttr_init(y, t, level=0.0):
    """(ttr, last_y) for the contiguous device tensor y at time t: new tensors of y's shape, fp64 and y's dtype."""
    torch = require_gpu()
    ttr = torch.empty(y.shape, dtype=torch.float64, device=y.device)
    last = torch.empty_like(y)
    with torch.cuda.device(y.device):
        _tffi.check(_tffi.lib().hjt_ttr_init(_dtype_id(torch, y), _ptr(y), y.numel(), float(t), float(level), _ptr(ttr),
                                             _ptr(last), _stream(torch, y.device)))
    return ttr, last


def ttr_update(y, t, t_last, ttr, last, level=0.0, mode=0):
    """One step of the recurrence, IN PLACE on the device tensors ttr (fp64) and last (y's dtype)."""
    torch = require_gpu()
    if tuple(ttr.shape) != tuple(y.shape) or tuple(last.shape) != tuple(y.shape) or last.dtype != y.dtype:
        error('ttr / ttrLastY do not agree with the state in shape or dtype')
    with torch.cuda.device(y.device):
        _tffi.check(_tffi.lib().hjt_ttr_update(_dtype_id(torch, y), _ptr(y), y.numel(), float(t), float(t_last), float(level),
                                               int(mode), _ptr(ttr), _ptr(last), _stream(torch, y.device)))


def ttr_from_stack(data, nslices, field_stride, n, tau, level=0.0, mode=0):
    """The recurrence over `nslices` slices of n elements, field_stride apart, of the contiguous device tensor `data`;
    tau: the slices' times (host).  Returns a flat fp64 tensor of n elements."""
    torch = require_gpu()
    tau_dev = torch.as_tensor(np.ascontiguousarray(tau, dtype=np.float64)).to(data.device)
    out = torch.empty(int(n), dtype=torch.float64, device=data.device)
    with torch.cuda.device(data.device):
        _tffi.check(_tffi.lib().hjt_ttr_from_stack(_dtype_id(torch, data), _ptr(data), int(nslices), int(field_stride), int(n),
                                                   _ptr(tau_dev), float(level), int(mode), _ptr(out),
                                                   _stream(torch, data.device)))
    return out


def _check_tau(tau, nslices):
    tau = np.asarray(_unlazy(tau).detach().cpu().numpy() if is_tensor(_unlazy(tau)) else tau, dtype=np.float64).ravel()
    if tau.size != nslices:
        error('tau must hold one time per slice of data (%d times for %d slices)' % (tau.size, nslices))
    if np.any(np.diff(tau) < 0):
        error('tau must be non-decreasing')
    return tau


# ------------------------------------------------------------------------------------------ postTimeStepTTR
def _state_tensor(a, dtype, device):
    """A field of schemeData as a contiguous device tensor: the tensor itself when it already is one (updated in place)."""
    torch = require_gpu()
    a = _unlazy(a)
    if is_tensor(a):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def postTimeStepTTR(t, yIn, schemeDataIn):
    """post_ttr.py:8: postTimeStep routine that records the time to reach.  Use it as
    odeCFLset(postTimeStep=postTimeStepTTR), and call it once yourself with the initial data and time before the
    integration starts (the integrators call it after the first step).

    yOut is yIn, unmodified and not copied.  schemeDataOut is a shallow copy of schemeDataIn with

      .ttr        time to reach, in the shape of yIn (fp64); +inf at nodes never reached
      .ttrLastY   the data of the last call        .ttrLastT   its time

    The first call (no .ttr field) initialises: t inside the sublevel set, +inf outside.  Later calls require the other
    two fields and apply one step of the recurrence (module docstring) IN PLACE on the device arrays behind .ttr and
    .ttrLastY -- as the reference's update, the arrays are shared with schemeDataIn.  Read when present:
    schemeData.ttrLevel (default 0) and schemeData.ttrCrossing ('last', the toolbox's rule and the default, or 'first').

    The fields live on the device: tensors when yIn is a tensor, HostViews (np.asarray materialises them) when yIn is a
    HostView or an ndarray.  Inside the device integrator's loop with a tensor state nothing crosses to the host."""
    sd = copy.copy(schemeDataIn)
    level = float(sd.ttrLevel) if isfield(sd, 'ttrLevel') else 0.0
    mode = mode_bits(sd.ttrCrossing if isfield(sd, 'ttrCrossing') else 'last', True)
    y = _device_data(yIn)
    if isfield(sd, 'ttr'):
        assert isfield(sd, 'ttrLastY'), 'schemeData has .ttr but no .ttrLastY'
        assert isfield(sd, 'ttrLastT'), 'schemeData has .ttr but no .ttrLastT'
        torch = require_gpu()
        ttr = _state_tensor(sd.ttr, torch.float64, y.device)
        last = _state_tensor(sd.ttrLastY, y.dtype, y.device)
        if last.data_ptr() == y.data_ptr():
            last = last.clone()
        ttr_update(y, t, float(sd.ttrLastT), ttr, last, level, mode)
    else:
        ttr, last = ttr_init(y, t, level)
    wrap = (lambda a: a) if is_tensor(yIn) else HostView
    sd.ttr = wrap(ttr)
    sd.ttrLastY = wrap(last)
    sd.ttrLastT = float(t)
    return yIn, sd


# ------------------------------------------------------------------------------------------ TD2TTR
def TD2TTR(g, data, tau, level=0.0, crossing='first', interpolate=False):
    """The time-to-reach function of a stored solve: `data` is a time-first stack on grid g (one array counts as a stack of
    one), tau its times (non-decreasing, one per slice).  Equal to postTimeStepTTR's recurrence applied slice by slice
    with the same options, computed by ttr_from_stack_kernel in one pass over the stack.  Defaults as helperOC's TD2TTR:
    the earliest crossing, stamped with the time of the slice that found the node inside.  Returns an array of g.shape
    (fp64): NumPy for NumPy data, a tensor for a tensor or HostView.  Parity UNPINNED (the reference has no such function)."""
    mode = mode_bits(crossing, interpolate)
    N = tuple(int(v) for v in np.asarray(g.N).ravel())
    t = _device_data(data)
    F, stride = _fields(t, N)
    tau = _check_tau(tau, F)
    out = ttr_from_stack(t, F, stride, stride, tau, level, mode).reshape(N)
    if _wants_tensor(data):
        p = _unlazy(data)
        return out if (not is_tensor(p) or p.is_cuda) else out.to(p.device)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ HJIPDE_solve's recorder
class Recorder(object):
    """What HJIPDE_solve(computeTTR=True) keeps: the running ttr and the last recorded state, on the device."""

    def __init__(self, level=0.0, crossing='first', interpolate=False):
        self.level, self.mode = float(level), mode_bits(crossing, interpolate)
        self.ttr = self.last = self.t_last = None

    def fold(self, stack, tau):
        """A given history: time-first slices at times tau."""
        t = _device_data(stack)
        T = int(t.shape[0])
        tau = _check_tau(tau, T)
        n = t[0].numel()
        self.ttr = ttr_from_stack(t, T, n, n, tau, self.level, self.mode)
        self.last = t[-1].reshape(-1).clone()
        self.t_last = float(tau[-1])

    def record(self, y, t):
        y = _device_data(y).reshape(-1)
        if self.ttr is None:
            self.ttr, self.last = ttr_init(y, t, self.level)
        else:
            if self.last.dtype != y.dtype:
                self.last = self.last.to(y.dtype)
            ttr_update(y, t, self.t_last, self.ttr, self.last, self.level, self.mode)
        self.t_last = float(t)

    def result(self, shape, proto):
        out = self.ttr.reshape(tuple(shape))
        return out if is_tensor(proto) else out.cpu().numpy()
