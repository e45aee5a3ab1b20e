"""Stochastic reachability: HJIPDE_solve's extraArgs.addGaussianNoiseStandardDeviation (reference ValueFuncs/hji_solver.py:449-471).

With the option set to a matrix sigma the PDE becomes  phi_t + H(x, grad phi) = trace(sigma^T D^2phi sigma):  the reference
wraps its scheme in termSum,
    schemeFunc = termSum
    innerFunc  = [the deterministic schemeFunc, termTraceHessian]
    innerData  = [its data, Bundle(grid, L = sigma^T, R = sigma, hessianFunc = hessianSecond)]
and so does HJIPDE_solve here (noise_scheme).  There is no factor 1/2 in front of the trace (the reference and helperOC write it
so): for the diffusion  dx = f dt + s dW  whose generator is 1/2 trace(s s^T D^2phi), pass sigma = s / sqrt(2).

sigma is an nd x nd matrix of numbers (NumPy array or nested list), a cell matrix with array entries, or a callable
(t, data, schemeData) -> one of these: the forms termTraceHessian takes for L and R (check_sigma).  A vector is refused.

Two routes compute the solve, with the same answers (extraOuts.path / last_path() say which ran and why):

  * the fused route (solve): one launch of stoch_substep_kernel (libhj_stoch.so, include/hj_stoch.h) per Runge-Kutta stage and a
    whole tau interval as one native call, planned on the host -- the step bounds of the built-in systems and of a constant sigma
    ignore the data.  Taken when classify() finds the solve eligible: a grid of 2 to 4 dimensions, hamFunc / partialFunc the
    bound methods of one built-in system (native_of's identity rule), upwindFirstENO2 / ENO3 / WENO5 as shipped, global
    Lax-Friedrichs dissipation, sigma all numbers, compMethod none / zero / minWithZero / min|maxVOverTime / min|maxVWithV0 /
    min|maxVWithL|Target, static or time-varying targets and obstacles, and no stopping set, stopInit, discounting, SDModFunc,
    computeTTR or history in data0;
  * the generic route: the termSum wiring above through HJIPDE_solve's own integrator loop, made only of the kernels of
    termLaxFriedrichs / termRestrictUpdate, termTraceHessian and the stage expressions.  Every option of HJIPDE_solve keeps
    its meaning there.
    (On a 1-D grid HJIPDE_solve stops at its own shape checks with or without the option: nothing changes there.)

With termRestrictUpdate (minWithZero / zero) the state is an (N,) vector and the restricted term comes back as one, while
termTraceHessian returns an (N, 1) column (the reference's sum of the two would broadcast to (N, N)): the second inner function
is then termTraceHessian with its column flattened (_trace_hessian_vector).

Parity: UNPINNED like termTraceHessian itself (the shipped term does not run); held to the NumPy restatement tests/stoch_ref.py
and, for ENO2 / ENO3 bit for bit, to the generic route.
"""
import ctypes as C

import numpy as np

from . import _bffi, _ffi, _wffi
from .context import grid_bc, is_tensor, require_gpu
from .curvature import hessianSecond, termSum, _number
from .dissipation import artificialDissipationGLF
from .dynamics import native_of
from .lazy import HostView
from .spatial import scheme_id_of, upwindFirstWENO5
from .term import termLaxFriedrichs, termRestrictUpdate
from .trace_hessian import termTraceHessian
from .utilities import Bundle, error, info, iscell, isfield, realmax
from ._marshal import unlazy as _unlazy, stream as _stream, ptr as _ptr, descriptor as _descriptor

__all__ = ["NOISE", "check_sigma", "noise_scheme", "classify", "solve", "step_bound", "substep", "integrate", "last_path"]

NOISE = 'addGaussianNoiseStandardDeviation'
SMALL = 1e-4            # HJIPDE_solve's `while tNow < tau[i] - small` (hji_solver.py:185)
FACTOR_CFL = 0.8        # its integratorOptions

_last_path = ""


def last_path():
    """What the calling process's last HJIPDE_solve with the noise option ran: 'fused: <kernel>' or 'generic: <why>'."""
    return _last_path


def _set_path(p):
    global _last_path
    _last_path = p
    return p


def _get(b, name, default=None):
    return getattr(b, name) if (b is not None and isfield(b, name)) else default


# ------------------------------------------------------------------------------------------ sigma
def _is_array(e):
    return is_tensor(e) or (isinstance(e, np.ndarray) and e.dtype != object and e.ndim > 0)


def check_sigma(sigma, nd):
    """extraArgs.addGaussianNoiseStandardDeviation -> (kind, sigma): ('numbers', (nd, nd) float64 array), ('cell', nd x nd list
    of lists with at least one array entry) or ('callable', the callable).  Anything else is refused by name."""
    if callable(sigma):
        return 'callable', sigma
    if is_tensor(sigma):
        sigma = sigma.detach().cpu().numpy()
    if isinstance(sigma, np.ndarray) and sigma.dtype != object:
        M = sigma
    else:
        if _number(sigma):
            M = np.asarray(float(sigma))
        elif iscell(sigma) or isinstance(sigma, (tuple, np.ndarray)):
            rows = list(sigma)
            if rows and all(iscell(r) or isinstance(r, (tuple, np.ndarray)) for r in rows) \
                    and any(_is_array(e) for r in rows for e in r):
                # a cell matrix with array entries: the shape and the numbers are checked here, the arrays' sizes where they are used
                rows = [list(r) for r in rows]
                if len(rows) != nd or any(len(r) != nd for r in rows):
                    error('extraArgs.%s must be a %d x %d matrix (got %d rows of lengths %s)'
                          % (NOISE, nd, nd, len(rows), [len(r) for r in rows]))
                for i, r in enumerate(rows):
                    for j, e in enumerate(r):
                        if isinstance(e, np.ndarray) and e.ndim == 0:
                            r[j] = e = e.item()
                        if _number(e):
                            if not np.isfinite(e):
                                error('extraArgs.%s[%d][%d] is not finite' % (NOISE, i, j))
                        elif not _is_array(e):
                            error('extraArgs.%s entries must be numbers or arrays the size of data' % NOISE)
                return 'cell', rows
            try:
                M = np.asarray(rows, dtype=np.float64)
            except (TypeError, ValueError):
                error('extraArgs.%s must be a %d x %d matrix of numbers, a cell matrix or a callable' % (NOISE, nd, nd))
        else:
            error('extraArgs.%s must be a %d x %d matrix of numbers, a cell matrix or a callable' % (NOISE, nd, nd))
    try:
        M = np.asarray(M, dtype=np.float64)
    except (TypeError, ValueError):
        error('extraArgs.%s must be a %d x %d matrix of numbers, a cell matrix or a callable' % (NOISE, nd, nd))
    if M.ndim == 1 and M.shape[0] == nd and nd > 1:
        error('extraArgs.%s is a vector of length %d: it must be the %d x %d matrix sigma; for independent noise per state '
              'pass np.diag(vector)' % (NOISE, nd, nd, nd))
    if M.ndim == 0 and nd == 1:
        M = M.reshape(1, 1)
    if M.shape != (nd, nd):
        error('extraArgs.%s must be a %d x %d matrix, got shape %s' % (NOISE, nd, nd, tuple(M.shape)))
    if not np.all(np.isfinite(M)):
        i, j = [int(v) for v in np.argwhere(~np.isfinite(M))[0]]
        error('extraArgs.%s[%d][%d] is not finite' % (NOISE, i, j))
    return 'numbers', np.ascontiguousarray(M)


def _transposed(kind, sigma):
    if kind == 'numbers':
        return np.ascontiguousarray(sigma.T)
    if kind == 'cell':
        n = len(sigma)
        return [[sigma[j][i] for j in range(n)] for i in range(n)]

    def left(t, data, schemeData):
        M = sigma(t, data, schemeData)
        if isinstance(M, np.ndarray) and M.dtype != object:
            return M.T if M.ndim == 2 else M
        if is_tensor(M) and M.dim() == 2:
            return M.T
        if iscell(M) and all(iscell(r) for r in M):
            return [[M[j][i] for j in range(len(M))] for i in range(len(M[0]))]
        return M
    return left


def _trace_hessian_vector(t, y, schemeData):
    """termTraceHessian with its (N, 1) column flattened to the (N,) vector termRestrictUpdate returns."""
    ydot, stepBound, schemeData = termTraceHessian(t, y, schemeData)
    return ydot.reshape(-1), stepBound, schemeData


def noise_scheme(kind, sigma, grid, schemeFunc, schemeData):
    """The reference's wiring (hji_solver.py:449-471): (termSum, its schemeData) around the deterministic (schemeFunc, schemeData)."""
    trace = _trace_hessian_vector if schemeFunc is termRestrictUpdate else termTraceHessian
    noise = Bundle(dict(grid=grid, L=_transposed(kind, sigma), R=sigma, hessianFunc=hessianSecond))
    return termSum, Bundle(dict(innerFunc=[schemeFunc, trace], innerData=[schemeData, noise]))


# ------------------------------------------------------------------------------------------ which route
_NONE = (None, 'none', 'set')
_ZERO = ('zero', 'minWithZero')
_PREV = {'minVOverTime': _ffi.POST_MIN_PREV, 'maxVOverTime': _ffi.POST_MAX_PREV}
_V0 = {'minVWithV0': _bffi.ARR_MIN, 'maxVWithV0': _bffi.ARR_MAX}
_TARGET = {'minVWithL': _bffi.ARR_MIN, 'minVwithL': _bffi.ARR_MIN, 'minVWithTarget': _bffi.ARR_MIN,
           'maxVWithL': _bffi.ARR_MAX, 'maxVwithL': _bffi.ARR_MAX, 'maxVWithTarget': _bffi.ARR_MAX}
# extraArgs that send a solve to the generic route, and what the reason calls them
_DISQUALIFIERS = (('stopInit', 'a stopping condition'), ('stopSetInclude', 'a stopping condition'),
                  ('stopSetIntersect', 'a stopping condition'), ('discountFactor', 'discounting'),
                  ('SDModFunc', 'an SDModFunc'), ('computeTTR', 'computeTTR'))


def _deriv_func(sd):
    # as HJIPDE_solve: CoStateCalc, else derivFunc, else upwindFirstWENO5 (hji_solver.py)
    if isfield(sd, 'CoStateCalc'):
        return sd.CoStateCalc
    return sd.derivFunc if isfield(sd, 'derivFunc') else upwindFirstWENO5


def classify(data0, schemeData, compMethod=None, extraArgs=None):
    """(setup, None) when the fused route covers the solve, else (None, reason).  Touches no device.
    setup: Bundle(grid, ham, scheme, params, sigma, restrict_sign)."""
    sd = schemeData
    for f in ('grid', 'hamFunc', 'partialFunc'):
        if not isfield(sd, f):
            return None, 'schemeData has no %s' % f
    g = sd.grid
    nd = int(g.dim)
    if nd < 2 or nd > 4:
        return None, 'a grid of %d dimension%s (the fused kernel covers 2 to 4)' % (nd, '' if nd == 1 else 's')
    try:
        grid_bc(g)
    except ValueError:
        return None, 'the grid has a boundary function without a device implementation'
    nat = native_of(sd.hamFunc, sd.partialFunc)
    if nat is None:
        return None, 'hamFunc / partialFunc are not the methods of a built-in system'
    if nat[1] >= _ffi.HAM_USER_BASE:
        return None, 'a registered Hamiltonian'
    if _wffi.HAM_DIMS.get(nat[1]) != nd:
        return None, '%s has no kernel on a %d-D grid' % (type(nat[0]).__name__, nd)
    if nat[0].grid is not g:
        return None, 'the system lives on another grid object than its schemeData'
    fn = _deriv_func(sd)
    sid = scheme_id_of(fn) if fn is not None else None
    if sid is None:
        return None, 'the derivative function is not one of upwindFirstENO2 / ENO3 / WENO5'
    if sid == _ffi.SCHEME_IDS["WENO5"]:
        return None, 'the intended WENO5 needs a grid-wide epsilon'
    if sid not in _wffi.SCHEMES:
        return None, 'scheme %s has no stochastic kernel' % getattr(fn, '__name__', fn)
    if isfield(sd, 'dissFunc') and sd.dissFunc is not artificialDissipationGLF:
        return None, 'the dissipation is not artificialDissipationGLF'
    kind, sigma = check_sigma(_get(extraArgs, NOISE), nd)
    if kind != 'numbers':
        return None, 'sigma %s' % ('has an array entry' if kind == 'cell' else 'is a callable')
    if compMethod not in _NONE and compMethod not in _ZERO and compMethod not in _PREV and compMethod not in _V0 \
            and compMethod not in _TARGET:
        return None, 'compMethod %r' % (compMethod,)
    for name, what in _DISQUALIFIERS:
        v = _get(extraArgs, name)
        if v is None or v is False:
            continue
        if name == 'discountFactor' and not v:
            continue
        return None, 'extraArgs.%s (%s)' % (name, what)
    src = _unlazy(data0)
    nd0 = src.dim() if is_tensor(src) else np.ndim(src)
    if nd0 != nd:
        return None, 'data0 carries a time history'
    for what in ('targetFunction', 'obstacleFunction'):
        a = _get(extraArgs, what)
        if a is not None and np.ndim(_unlazy(a)) not in (nd, nd + 1):
            return None, 'extraArgs.%s has neither the grid\'s dimensions nor a time axis more' % what
    p = [float(v) for v in nat[2]]
    return Bundle(dict(grid=g, ham=nat[1], scheme=sid, params=p + [0.0] * (_bffi.PAR_SLOTS - len(p)), sigma=sigma,
                       restrict_sign=-1 if compMethod in _ZERO else 0)), None


# ------------------------------------------------------------------------------------------ the native calls
def _darr(values):
    return np.ascontiguousarray(values, dtype=np.float64)


def _pd(a):
    return a.ctypes.data_as(_wffi._pd)


class _Call(object):
    """What every native call of one solve shares: the descriptor, the tables, the parameters, sigma and the stream."""

    def __init__(self, g, ham, scheme, params, sigma, torch, device, form=_wffi.FORM_AUTO):
        from .batch import tables
        self.torch, self.device = torch, device
        self.desc, self.N = _descriptor(g, "float64")
        self.tab = tables(g, torch, device)
        self.ham, self.scheme, self.form = int(ham), int(scheme), int(form)
        p = [float(v) for v in params]
        self.params = _darr(p + [0.0] * (_bffi.PAR_SLOTS - len(p)))
        self.sigma = _darr(sigma).reshape(-1)

    def stream(self):
        return _stream(self.torch, self.device)

    def step_bound(self):
        keys = self.torch.empty((4,), dtype=self.torch.int64, device=self.device)
        sb = np.zeros(3, dtype=np.float64)
        _wffi.check(_wffi.lib().hjw_step_bound(C.byref(self.desc), C.byref(self.tab), self.ham, _pd(self.params), _pd(self.sigma),
                                               _ptr(keys), _pd(sb), self.stream()))
        return float(sb[0]), float(sb[1]), float(sb[2])

    def substep(self, stage, src, dst, y0=None, dt=0.0, restrict_sign=0, post_prev=0, op_a=0, post_a=None, op_b=0, post_b=None):
        e = _wffi.Entry(src=src.data_ptr(), y0=y0.data_ptr() if y0 is not None else None, dst=dst.data_ptr(),
                        post_a=post_a.data_ptr() if post_a is not None else None,
                        post_b=post_b.data_ptr() if post_b is not None else None, dt=float(dt), active=1,
                        post_prev=int(post_prev), op_a=int(op_a), op_b=int(op_b))
        _wffi.check(_wffi.lib().hjw_substep(C.byref(self.desc), C.byref(self.tab), self.scheme, self.ham, int(stage), int(restrict_sign),
                                            _pd(self.params), _pd(self.sigma), self.form, C.byref(e), self.stream()))

    def integrate(self, sb, y_in, buf_a, buf_b, work, t0, tf, order=3, restrict_sign=0, post_prev=0, op_a=0, post_a=None, op_b=0,
                  post_b=None, factorCFL=FACTOR_CFL, maxStep=realmax, stop_tol=SMALL):
        p = _bffi.Problem(y_in=y_in.data_ptr(), buf_a=buf_a.data_ptr(), buf_b=buf_b.data_ptr(),
                          work=work.data_ptr() if work is not None else None,
                          post_a=post_a.data_ptr() if post_a is not None else None,
                          post_b=post_b.data_ptr() if post_b is not None else None, op_a=int(op_a), op_b=int(op_b))
        t, steps, where = C.c_double(), C.c_int64(), C.c_int32()
        _wffi.check(_wffi.lib().hjw_integrate(
            C.byref(self.desc), C.byref(self.tab), self.scheme, self.ham, int(order), int(restrict_sign), int(post_prev),
            _pd(self.params), _pd(self.sigma), self.form, float(sb), C.byref(p), float(t0), float(tf), float(factorCFL),
            float(maxStep), float(stop_tol), C.byref(t), C.byref(steps), C.byref(where), self.stream()))
        return float(t.value), int(steps.value), int(where.value)


def _device_of(torch, *arrays):
    for a in arrays:
        a = _unlazy(a)
        if is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(torch, a, device):
    a = _unlazy(a)
    if is_tensor(a):
        return a.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float64)).to(device)


def _back(t, like, shape):
    t = t.reshape(shape)
    return t if (is_tensor(like) or isinstance(like, HostView)) else t.cpu().numpy()


def step_bound(grid, ham, params, sigma):
    """(stepBound, stepBound of the Lax-Friedrichs term, stepBound of the trace term): hjw_step_bound."""
    torch = require_gpu()
    device = _device_of(torch)
    with torch.cuda.device(device):
        return _Call(grid, ham, _ffi.ENO2, params, check_sigma(sigma, int(grid.dim))[1], torch, device).step_bound()


def substep(grid, scheme, ham, params, sigma, stage, y, y0=None, dt=0.0, restrict_sign=0, form=_wffi.FORM_AUTO, post_prev=0,
            op_a=0, post_a=None, op_b=0, post_b=None):
    """One stage through hjw_substep: a new array of y's kind and shape (NumPy in -> NumPy out, tensor in -> tensor out)."""
    torch = require_gpu()
    device = _device_of(torch, y)
    with torch.cuda.device(device):
        call = _Call(grid, ham, scheme, params, check_sigma(sigma, int(grid.dim))[1], torch, device, form)
        dev = lambda a: _to_device(torch, a, device).reshape(-1) if a is not None else None   # noqa: E731
        src = dev(y)
        dst = torch.empty_like(src)
        call.substep(stage, src, dst, dev(y0), dt, restrict_sign, post_prev, op_a, dev(post_a), op_b, dev(post_b))
        return _back(dst, y, tuple(y.shape))


def integrate(grid, scheme, ham, params, sigma, y, t0, tf, order=3, restrict_sign=0, form=_wffi.FORM_AUTO, post_prev=0, op_a=0,
              post_a=None, op_b=0, post_b=None, factorCFL=FACTOR_CFL, maxStep=realmax, stop_tol=SMALL):
    """One interval through hjw_step_bound and hjw_integrate: (t, y of the input's kind and shape, steps)."""
    torch = require_gpu()
    device = _device_of(torch, y)
    with torch.cuda.device(device):
        call = _Call(grid, ham, scheme, params, check_sigma(sigma, int(grid.dim))[1], torch, device, form)
        dev = lambda a: _to_device(torch, a, device).reshape(-1) if a is not None else None   # noqa: E731
        src = dev(y)
        a, b, w = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
        sb = call.step_bound()[0]
        t, steps, where = call.integrate(sb, src, a, b, w, t0, tf, order, restrict_sign, post_prev, op_a, dev(post_a), op_b,
                                         dev(post_b), factorCFL, maxStep, stop_tol)
        out = (src.clone(), a, b)[where]
        return t, _back(out, y, tuple(y.shape)), steps


# ------------------------------------------------------------------------------------------ the fused solve
def solve(setup, data0, tau, compMethod=None, extraArgs=None):
    """HJIPDE_solve for a solve classify() found eligible: (data, tau, extraOuts), as HJIPDE_solve returns them.  extraOuts.steps[i]
    is the number of time steps taken in the interval tau[i] .. tau[i+1], extraOuts.tNow the time reached in the last one."""
    from .hji_solver import _trim
    torch = require_gpu()
    extraArgs = extraArgs if extraArgs is not None else Bundle({})
    extraOuts = Bundle({})
    g = setup.grid
    nd = int(g.dim)
    quiet = bool(_get(extraArgs, 'quiet', False))
    keepLast = bool(_get(extraArgs, 'keepLast', False))
    lowMemory = bool(_get(extraArgs, 'lowMemory', False))
    flipOutput = bool(_get(extraArgs, 'flipOutput', False))
    stopConverge = bool(_get(extraArgs, 'stopConverge', False))
    convergeThreshold = _get(extraArgs, 'convergeThreshold', 1e-5)
    ignoreBoundary = bool(_get(extraArgs, 'ignoreBoundary', False))
    targets = _get(extraArgs, 'targetFunction')
    obstacles = _get(extraArgs, 'obstacleFunction')
    targ_tv = targets is not None and np.ndim(_unlazy(targets)) == nd + 1
    obs_tv = obstacles is not None and np.ndim(_unlazy(obstacles)) == nd + 1
    src = _unlazy(data0)
    tensors = is_tensor(src) or isinstance(data0, HostView)
    device = _device_of(torch, src)
    shape = tuple(int(v) for v in g.shape)
    if tuple(int(v) for v in src.shape) != shape:
        error('data0 does not agree in array size with grid')
    store_all = not keepLast and not lowMemory
    with torch.cuda.device(device):
        call = _Call(g, setup.ham, setup.scheme, setup.params, setup.sigma, torch, device)
        sb = call.step_bound()[0]
        y_init = _to_device(torch, src, device).reshape(-1)              # only ever read
        n = y_init.numel()
        S = torch.empty((3, n), dtype=torch.float64, device=device)
        W = torch.empty((n,), dtype=torch.float64, device=device)
        slot = -1                                                        # where the state is: -1 = y_init
        data = None
        if store_all:
            data = np.zeros((len(tau),) + shape, dtype=np.float64)
            data[0] = y_init.cpu().numpy().reshape(shape)
        post_prev = _PREV.get(compMethod, _ffi.POST_NONE)
        extraOuts.steps, extraOuts.tNow = np.zeros(len(tau) - 1, dtype=np.int64), float(tau[0])
        path = "fused: %s (no step taken)" % _wffi.kernel_name(setup.ham, setup.scheme, not np.any(setup.sigma - np.diag(np.diag(setup.sigma))))
        for i in range(1, len(tau)):
            if not quiet:
                info('Computing value function at time tau[%d]: %.4f' % (i, tau[i]))
            y = y_init if slot < 0 else S[slot]
            target_i = _to_device(torch, targets[i] if targ_tv else targets, device).reshape(-1) if targets is not None else None
            obstacle_i = _to_device(torch, obstacles[i] if obs_tv else obstacles, device).reshape(-1) if obstacles is not None else None
            op_a, arr_a = 0, None
            if compMethod in _V0:
                op_a, arr_a = _V0[compMethod], y_init
            elif compMethod in _TARGET:
                if target_i is None:
                    error('Need to define target function l(x)!')
                op_a, arr_a = _TARGET[compMethod], target_i
            op_b, arr_b = (_bffi.ARR_MAX_NEG, obstacle_i) if obstacle_i is not None else (0, None)
            free = [k for k in range(3) if k != slot]
            extraOuts.tNow, steps, where = call.integrate(sb, y, S[free[0]], S[free[1]], W, tau[i - 1], tau[i], 3, setup.restrict_sign, post_prev,
                                             op_a, arr_a, op_b, arr_b)
            extraOuts.steps[i - 1] = steps
            y_start = y
            if where:
                slot = free[where - 1]
                path = "fused: " + _wffi.last_kernel().split(';')[-1]
            cur = y_init if slot < 0 else S[slot]
            if steps and bool(torch.isnan(cur).any()):
                error('Nans encountered in the integrated result of HJI PDE data')   # hji_solver.py:544-545
            if store_all:
                data[i] = cur.cpu().numpy().reshape(shape)
            if stopConverge:                                             # hji_solver.py:661-672, 706-722
                a, b = cur.reshape(shape), y_start.reshape(shape)
                if ignoreBoundary:
                    a, b = _trim(g, a), _trim(g, b)
                change = float(abs(a - b).max()) if a.numel() else 0.0
                if not quiet:
                    info('Max change since last iteration: %s' % change)
                if change < convergeThreshold:
                    extraOuts.stoptau = tau[i]
                    tau = tau[:i + 1]
                    if store_all:
                        data = data[:i + 1]
                    break
        if not store_all:
            cur = (y_init if slot < 0 else S[slot]).clone().reshape(shape)
            data = cur if tensors else cur.cpu().numpy()
        elif tensors:
            data = torch.as_tensor(data, device=device)
        if flipOutput and store_all:
            data = data.flip(0) if is_tensor(data) else np.flip(data, 0).copy()
    extraOuts.path = _set_path(path)
    return data, tau, extraOuts
