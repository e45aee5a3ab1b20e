"""HJIPDE_solve_batch: HJIPDE_solve (hji_solver.py) for many problems on one grid at once.

    data, tau, extraOuts = HJIPDE_solve_batch(data0s, tau, schemeDatas, compMethod, extraArgs)

`data0s` is (B,) + g.shape, `schemeDatas` a list of B schemeData Bundles -- or ONE Bundle with `extraArgs.systems`, a
list of B system objects whose hamiltonian / dissipation methods take the place of the Bundle's hamFunc / partialFunc.
data[b] is what HJIPDE_solve(data0s[b], tau, schemeDatas[b], compMethod, extraArgs_b) returns: (B,) + g.shape with
extraArgs.keepLast (or lowMemory), (B, len(tau)) + g.shape otherwise.  extraArgs.targetFunction / obstacleFunction are
static arrays on the grid, shared by the problems, or (B,) + g.shape with one per problem.  NumPy in -> NumPy out; a
device tensor in -> a device tensor out.  As in HJIPDE_solve the solve itself runs in fp64 whatever the input's type.
extraOuts.steps[b, i] is the number of time steps problem b took in the interval tau[i] .. tau[i+1], extraOuts.tNow[b]
the time it reached in the last one, extraOuts.path what ran (also last_path()).

The device path advances all B value functions together: every Runge-Kutta stage is ONE launch of batch_substep_kernel
(libhj_batch.so, include/hj_batch.h) for all problems, and a whole tau interval is one native call.  The problems' CFL
bounds differ, so they need different numbers of steps per interval; alpha of the built-in systems ignores the data, so
every problem's step sizes are known before the interval starts (plan_interval) and a problem that has arrived sits the
remaining launches out.  It is taken when
  * all problems share one grid (equal N, min, max, boundary kinds);
  * hamFunc / partialFunc are the bound methods of instances of ONE built-in system class (dynamics.py), native by
    native_of's identity rule;
  * the derivative function is upwindFirstENO2 / ENO3 / WENO5 as shipped, the dissipation artificialDissipationGLF;
  * compMethod is None / 'none' / 'set', min|maxVOverTime, min|maxVWithV0 or min|maxVWithL / Target;
  * there is no stopping condition, discounting, SDModFunc, computeTTR or time-varying target / obstacle.
Anything else takes a host loop over HJIPDE_solve with the same outputs (extraOuts.steps / tNow are then None:
HJIPDE_solve does not report them) and an info line saying why.  Where a single solve raises, the batch raises and
names the problems.

Parity: nothing new is pinned -- each problem is an existing solve, and the batch is held to it bit for bit.
"""
import copy
import ctypes as C

import numpy as np

from . import _bffi, _ffi
from .context import grid_bc, is_tensor, require_gpu
from .dissipation import artificialDissipationGLF
from .dynamics import native_of
from .hji_solver import HJIPDE_solve
from .lazy import HostView, DeviceArray
from .spatial import scheme_id_of, upwindFirstWENO5
from .utilities import Bundle, error, info, isfield, realmax
from ._marshal import unlazy as _unlazy, stream as _stream, ptr as _ptr, descriptor as _descriptor

__all__ = ["HJIPDE_solve_batch", "plan_interval", "plan_schedule"]

SMALL = 1e-4            # HJIPDE_solve's `while tNow < tau[i] - small` (hji_solver.py:185)
FACTOR_CFL = 0.8        # its integratorOptions
_EPS = 2.220446049250313e-16

_last_path = ""


def last_path():
    """What the calling process's last HJIPDE_solve_batch ran: the kernel's name, or 'host loop: <why>'."""
    return _last_path


# ------------------------------------------------------------------------------------------ the schedule
def plan_interval(step_bound, t0, tf, factorCFL=FACTOR_CFL, maxStep=realmax, stop_tol=SMALL, order=3):
    """The time steps ONE problem takes from t0 towards tf: ([deltaT per step], [time after each step]).

    A pure function: the native systems' stepBound ignores the data, so deltaT = min(factorCFL * stepBound, tf - t,
    maxStep) (ode_cfl_3.py:142) and the time expressions of odeCFL1/2/3 give the whole sequence without a device.
    stop_tol >= 0: HJIPDE_solve's loop `while t < tf - stop_tol`; stop_tol < 0: the integrators' own
    `while tf - t >= 100 eps |tf|`.  The same expressions, in the same order, as hjb_plan / hj_rk_integrate."""
    sb, t, tf = float(step_bound), float(t0), float(tf)
    if not sb > 0.0:
        error('the step bound must be positive (got %r)' % step_bound)
    dts, ts = [], []
    while (tf - t >= 100 * _EPS * abs(tf)) if stop_tol < 0 else (t < tf - stop_tol):
        dt = min(factorCFL * sb, tf - t, maxStep)
        if order == 1:
            tn = t + dt
        else:
            t1 = t + dt
            t2 = t1 + dt
            if order == 2:
                tn = 0.5 * (t + t2)
            else:
                tHalf = 0.25 * (3 * t + t2)
                tThreeHalf = tHalf + dt
                tn = (1 / 3) * (t + 2 * tThreeHalf)
        if not tn > t:
            error('time step underflow at t=%g (dt=%g)' % (t, dt))
        dts.append(dt)
        ts.append(tn)
        t = tn
    return dts, ts


def plan_schedule(step_bounds, tau, factorCFL=FACTOR_CFL, maxStep=realmax, stop_tol=SMALL, order=3):
    """HJIPDE_solve's time loop for every problem: (times, steps) with times[b][i] the list of times problem b passes
    through in the interval tau[i] .. tau[i+1] (every interval starts from tau[i] itself) and steps an integer array
    (B, len(tau) - 1) of their lengths."""
    tau = np.asarray(tau, dtype=np.float64).ravel()
    times = [[plan_interval(sb, tau[i], tau[i + 1], factorCFL, maxStep, stop_tol, order)[1] for i in range(len(tau) - 1)]
             for sb in step_bounds]
    steps = np.array([[len(iv) for iv in row] for row in times], dtype=np.int64).reshape(len(times), len(tau) - 1)
    return times, steps


# ------------------------------------------------------------------------------------------ which path
_NONE = (None, 'none', 'set')
_PREV = {'minVOverTime': _ffi.POST_MIN_PREV, 'maxVOverTime': _ffi.POST_MAX_PREV}
_V0 = {'minVWithV0': _bffi.ARR_MIN, 'maxVWithV0': _bffi.ARR_MAX}
_TARGET = {'minVWithL': _bffi.ARR_MIN, 'minVwithL': _bffi.ARR_MIN, 'minVWithTarget': _bffi.ARR_MIN,
           'maxVWithL': _bffi.ARR_MAX, 'maxVwithL': _bffi.ARR_MAX, 'maxVWithTarget': _bffi.ARR_MAX}
# extraArgs the device path understands; any other field sends the batch to the host loop
_KNOWN_ARGS = ('quiet', 'keepLast', 'lowMemory', 'targetFunction', 'obstacleFunction', 'systems')
_REASONS = {'stopInit': 'a stopping condition', 'stopSetInclude': 'a stopping condition', 'stopSetIntersect': 'a stopping condition',
            'stopConverge': 'a stopping condition', 'stopLevel': 'a stopping condition', 'convergeThreshold': 'a stopping condition',
            'ignoreBoundary': 'a stopping condition', 'discountFactor': 'discounting', 'discountMode': 'discounting',
            'discountAnneal': 'discounting', 'SDModFunc': 'an SDModFunc', 'SDModParams': 'an SDModFunc',
            'addGaussianNoiseStandardDeviation': 'noise: the batched kernel has no diffusion term',
            'computeTTR': 'computeTTR', 'ttrLevel': 'computeTTR', 'ttrCrossing': 'computeTTR', 'ttrInterpolate': 'computeTTR'}


def _get(b, name, default=None):
    return getattr(b, name) if (b is not None and isfield(b, name)) else default


def _same_grid(a, b):
    if a is b:
        return True
    if int(a.dim) != int(b.dim):
        return False
    for f in ('N', 'min', 'max'):
        if not np.array_equal(np.asarray(getattr(a, f)).ravel(), np.asarray(getattr(b, f)).ravel()):
            return False
    try:
        return grid_bc(a) == grid_bc(b)
    except ValueError:
        return False


def _deriv_func(sd):
    # as HJIPDE_solve: CoStateCalc, else derivFunc, else upwindFirstWENO5 (hji_solver.py)
    if isfield(sd, 'CoStateCalc'):
        return sd.CoStateCalc
    return sd.derivFunc if isfield(sd, 'derivFunc') else upwindFirstWENO5


def _per_problem(a, gdim, B, what):
    """A target / obstacle argument -> (kind, array): 'none', 'shared' (g.shape), 'each' ((B,) + g.shape) or 'timed'."""
    if a is None:
        return 'none', None
    nd = a.dim() if is_tensor(a) else np.ndim(_unlazy(a))
    if nd == gdim:
        return 'shared', a
    if nd == gdim + 1:
        if int(a.shape[0]) != B:
            error('extraArgs.%s with a leading axis must hold one array per problem (%d), got %d' % (what, B, int(a.shape[0])))
        return 'each', a
    if nd == gdim + 2 and int(a.shape[0]) == B:
        return 'timed', a
    error('Inconsistent %s dimensions!' % ('target' if what == 'targetFunction' else 'obstacle'))


def classify(data0s, schemeDatas, compMethod=None, extraArgs=None):
    """(setup, None) when the device path covers the call, else (None, reason).  Touches no device.
    setup: Bundle(grid, ham, scheme, params (B lists), systems)."""
    B = len(schemeDatas)
    sd0 = schemeDatas[0]
    for b, sd in enumerate(schemeDatas):
        for f in ('grid', 'hamFunc', 'partialFunc'):
            if not isfield(sd, f):
                return None, 'schemeData of problem %d has no %s' % (b, f)
    g = sd0.grid
    for b, sd in enumerate(schemeDatas):
        if not _same_grid(g, sd.grid):
            return None, 'problem %d lives on another grid' % b
    try:
        grid_bc(g)
    except ValueError:
        return None, 'the grid has a boundary function without a device implementation'
    nd0 = data0s.dim() if is_tensor(data0s) else np.ndim(_unlazy(data0s))
    if nd0 != g.dim + 1:
        return None, 'data0s carries a time history per problem'
    ham, owner, scheme, params = None, None, None, []
    for b, sd in enumerate(schemeDatas):
        nat = native_of(sd.hamFunc, sd.partialFunc)
        if nat is None:
            return None, 'hamFunc / partialFunc of problem %d are not the methods of a built-in system' % b
        if nat[1] >= _ffi.HAM_USER_BASE:
            return None, 'problem %d runs a registered Hamiltonian' % b
        if nat[0].grid is not sd.grid:
            return None, 'the system of problem %d lives on another grid object than its schemeData' % b
        if ham is None:
            ham, owner = nat[1], type(nat[0])
        elif nat[1] != ham or type(nat[0]) is not owner:
            return None, 'problem %d is a %s, problem 0 a %s' % (b, type(nat[0]).__name__, owner.__name__)
        if _bffi.HAM_DIMS.get(ham) != g.dim:
            return None, '%s has no kernel on a %d-D grid' % (owner.__name__, g.dim)
        fn = _deriv_func(sd)
        sid = scheme_id_of(fn) if fn is not None else None
        if sid is None:
            return None, 'the derivative function of problem %d is not one of upwindFirstENO2 / ENO3 / WENO5' % b
        if sid == _ffi.SCHEME_IDS["WENO5"]:
            return None, 'the intended WENO5 needs a grid-wide epsilon per problem'
        if sid not in _bffi.SCHEMES:
            return None, 'scheme %s has no batched kernel' % getattr(fn, '__name__', fn)
        if scheme is None:
            scheme = sid
        elif sid != scheme:
            return None, 'problem %d uses another derivative function than problem 0' % b
        if isfield(sd, 'dissFunc') and sd.dissFunc is not artificialDissipationGLF:
            return None, 'the dissipation of problem %d is not artificialDissipationGLF' % b
        p = [float(v) for v in nat[2]]
        params.append(p + [0.0] * (_bffi.PAR_SLOTS - len(p)))
    if compMethod not in _NONE and compMethod not in _PREV and compMethod not in _V0 and compMethod not in _TARGET:
        return None, 'compMethod %r' % (compMethod,)
    for name in sorted(getattr(extraArgs, '__dict__', {})):
        if name in _KNOWN_ARGS or name.startswith('_'):
            continue
        v = getattr(extraArgs, name)
        if v is None or v is False:
            continue
        return None, 'extraArgs.%s (%s)' % (name, _REASONS.get(name, 'not known to the batched path'))
    for what in ('targetFunction', 'obstacleFunction'):
        kind, _ = _per_problem(_get(extraArgs, what), g.dim, B, what)
        if kind == 'timed':
            return None, 'extraArgs.%s varies in time' % what
    return Bundle(dict(grid=g, ham=ham, scheme=scheme, params=params)), None


# ------------------------------------------------------------------------------------------ the two paths
def _scheme_datas(schemeDatas, extraArgs, B):
    systems = _get(extraArgs, 'systems')
    if isinstance(schemeDatas, (list, tuple)):
        if systems is not None:
            error('extraArgs.systems goes with ONE schemeData Bundle, not with a list')
        sds = list(schemeDatas)
    else:
        if systems is None:
            error('schemeDatas must be a list of schemeData Bundles, or one Bundle with extraArgs.systems')
        sds = []
        for s in systems:
            sd = copy.copy(schemeDatas)
            sd.hamFunc, sd.partialFunc = s.hamiltonian, s.dissipation
            sds.append(sd)
    if len(sds) != B:
        error('data0s holds %d problems, schemeDatas %d' % (B, len(sds)))
    return sds


def _args_of(extraArgs, b, kinds):
    """extraArgs of problem b for HJIPDE_solve: per-problem targets / obstacles unpacked, `systems` dropped."""
    a = Bundle(dict(getattr(extraArgs, '__dict__', {})))
    a.__dict__.pop('systems', None)
    for what, (kind, arr) in kinds.items():
        if kind in ('each', 'timed'):
            setattr(a, what, arr[b])
    return a


def _host_loop(data0s, tau, sds, compMethod, extraArgs, kinds, tensors):
    B = len(sds)
    outs, tau_out, failed = [], tau, []
    for b in range(B):
        try:
            d, tau_out, _ = HJIPDE_solve(data0s[b], tau, sds[b], compMethod, _args_of(extraArgs, b, kinds))
            outs.append(d)
        except ValueError as e:
            failed.append((b, str(e)))
    if failed:
        error('%s in problems %s' % (failed[0][1], [b for b, _ in failed]))
    if tensors:
        torch = require_gpu()
        data = torch.stack([torch.as_tensor(_unlazy(d)) for d in outs])
    else:
        data = np.stack([np.asarray(d) for d in outs])
    return data, tau_out


def tables(g, torch, device, dtype_name="float64"):
    """hjb_tables of a grid on a device: the coordinate vectors, and the trig tables computed by NumPy exactly as
    context.DeviceGrid computes the solver's (fp64 values, rounded once for an fp32 grid)."""
    cache = g.__dict__.get("_hj_batch_tables")
    if cache is None:
        cache = {}
        object.__setattr__(g, "_hj_batch_tables", cache)
    key = (dtype_name, device.type, device.index)
    if key not in cache:
        vs = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in g.vs]
        aux = []
        if g.dim == 3:
            aux = [np.cos(vs[2]), np.sin(vs[2])]
        elif g.dim == 4:
            aux = [np.sin(vs[0]), np.cos(vs[0]), np.sin(vs[2]), np.cos(vs[2])]
        tdtype = torch.float64 if dtype_name == "float64" else torch.float32
        keep = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(tdtype).to(device) for a in vs + aux]
        tab = _bffi.Tables()
        for d in range(g.dim):
            tab.coord[d] = keep[d].data_ptr()
        for s in range(len(aux)):
            tab.aux[s] = keep[g.dim + s].data_ptr()
        cache[key] = (tab, keep)
    return cache[key][0]


def upload_entries(ent, torch, device):
    """A NumPy array of _bffi.ENTRY records -> the bytes on the device (keep the tensor alive while launches read it)."""
    return torch.from_numpy(np.ascontiguousarray(ent).view(np.uint8).copy()).to(device)


def _to_device(torch, a, device):
    a = _unlazy(a)
    if is_tensor(a):
        return a.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float64)).to(device)


def integrate_batch(g, tab, desc, scheme, ham, par_dev, sbs, probs, t0, tf, order=3, post_prev=0, restrict_sign=0,
                    factorCFL=FACTOR_CFL, maxStep=realmax, stop_tol=SMALL, torch=None, device=None):
    """hjb_integrate for B problems: `probs` an _bffi.Problem array.  -> (t (B,), steps (B,), where (B,)) as NumPy."""
    B = len(probs)
    nmax = max(len(plan_interval(sb, t0, tf, factorCFL, maxStep, stop_tol, order)[0]) for sb in sbs)
    table = torch.empty((max(1, nmax * order * B * _bffi.ENTRY.itemsize),), dtype=torch.uint8, device=device)
    t = np.zeros(B, dtype=np.float64)
    steps = np.zeros(B, dtype=np.int64)
    where = np.zeros(B, dtype=np.int32)
    sb = np.ascontiguousarray(sbs, dtype=np.float64)
    if not isinstance(probs, C.Array):
        probs = (_bffi.Problem * B)(*probs)
    _bffi.check(_bffi.lib().hjb_integrate(
        C.byref(desc), C.byref(tab), int(scheme), int(ham), int(order), int(restrict_sign), int(post_prev), _ptr(par_dev),
        sb.ctypes.data_as(_bffi._pd), probs, B, float(t0), float(tf), float(factorCFL), float(maxStep), float(stop_tol),
        _ptr(table), table.numel(), t.ctypes.data_as(_bffi._pd), steps.ctypes.data_as(_bffi._pi64),
        where.ctypes.data_as(_bffi._pi32), _stream(torch, device)))
    return t, steps, where


def step_bounds(g, tab, desc, ham, par_dev, B, torch, device):
    """hjb_step_bounds -> (B,) NumPy array."""
    keys = torch.empty((B, 4), dtype=torch.int64, device=device)
    sb = np.zeros(B, dtype=np.float64)
    _bffi.check(_bffi.lib().hjb_step_bounds(C.byref(desc), C.byref(tab), int(ham), _ptr(par_dev), B, _ptr(keys),
                                            sb.ctypes.data_as(_bffi._pd), None, _stream(torch, device)))
    return sb


def _nan_problems(torch, device, ptrs, active, n, dtype_id):
    """Indices of the problems whose state (ptrs[b], n elements) holds a NaN; `active` masks the ones to look at."""
    B = len(ptrs)
    ent = np.zeros(B, dtype=_bffi.ENTRY)
    ent["src"] = ptrs
    ent["active"] = active
    tab = upload_entries(ent, torch, device)
    flags = torch.empty((B,), dtype=torch.int32, device=device)
    _bffi.check(_bffi.lib().hjb_nan_flags(dtype_id, _ptr(tab), B, n, _ptr(flags), _stream(torch, device)))
    return [int(b) for b in np.nonzero(flags.cpu().numpy())[0]]


def _device_solve(setup, data0s, tau, compMethod, extraArgs, kinds, tensors, quiet):
    torch = require_gpu()
    g, ham, scheme = setup.grid, setup.ham, setup.scheme
    src = _unlazy(data0s)
    device = src.device if (is_tensor(src) and src.is_cuda) else torch.device("cuda", torch.cuda.current_device())
    keepLast = bool(_get(extraArgs, 'keepLast', False)) or bool(_get(extraArgs, 'lowMemory', False))
    with torch.cuda.device(device):
        desc, N = _descriptor(g, "float64")
        n = int(np.prod(N))
        B = len(setup.params)
        tab = tables(g, torch, device)
        y_init = _to_device(torch, src, device).reshape(B, n)          # only ever read
        par_dev = torch.from_numpy(np.ascontiguousarray(setup.params, dtype=np.float64)).to(device)
        sbs = step_bounds(g, tab, desc, ham, par_dev, B, torch, device)
        # post-step operators: one array operator from compMethod, one from the obstacles (hji_solver.py:566-599, 641-644)
        post_prev = _PREV.get(compMethod, _ffi.POST_NONE)
        arr_a = op_a = None
        if compMethod in _V0:
            op_a, arr_a = _V0[compMethod], y_init
        elif compMethod in _TARGET:
            if kinds['targetFunction'][0] == 'none':
                error('Need to define target function l(x)!')
            op_a = _TARGET[compMethod]
            arr_a = _to_device(torch, kinds['targetFunction'][1], device)
            arr_a = arr_a.reshape(B, n) if kinds['targetFunction'][0] == 'each' else arr_a.reshape(1, n).expand(B, n)
        arr_b = None
        if kinds['obstacleFunction'][0] != 'none':
            arr_b = _to_device(torch, kinds['obstacleFunction'][1], device)
            arr_b = arr_b.reshape(B, n) if kinds['obstacleFunction'][0] == 'each' else arr_b.reshape(1, n).expand(B, n)
        esz = 8
        row = lambda a, b: a.data_ptr() + b * a.stride(0) * esz        # noqa: E731  (a shared array has stride 0)
        # three state buffers and one stage buffer per problem: the state of problem b sits in slot[b] (-1: still data0s)
        S = torch.empty((3, B, n), dtype=torch.float64, device=device)
        W = torch.empty((B, n), dtype=torch.float64, device=device)
        slot = np.full(B, -1, dtype=np.int64)
        nt = len(tau)
        steps = np.zeros((B, nt - 1), dtype=np.int64)
        tNow = np.full(B, tau[0], dtype=np.float64)
        data = None
        if not keepLast:
            data = torch.empty((B, nt, n), dtype=torch.float64, device=device)
            data[:, 0] = y_init
        probs = (_bffi.Problem * B)()
        ar = torch.arange(B, device=device)
        path = "%s (no step taken)" % _bffi.kernel_name("float64", ham, scheme)

        def state_ptr(b):
            return row(y_init, b) if slot[b] < 0 else S[int(slot[b]), b].data_ptr()

        for i in range(1, nt):
            if not quiet:
                info('Computing %d value functions at time tau[%d]: %.4f' % (B, i, tau[i]))
            for b in range(B):
                free = [k for k in range(3) if k != slot[b]]
                p = probs[b]
                p.y_in, p.buf_a, p.buf_b = state_ptr(b), S[free[0], b].data_ptr(), S[free[1], b].data_ptr()
                p.work = W[b].data_ptr()
                p.post_a, p.op_a = (row(arr_a, b), op_a) if arr_a is not None else (None, 0)
                p.post_b, p.op_b = (row(arr_b, b), _bffi.ARR_MAX_NEG) if arr_b is not None else (None, 0)
            t, ns, where = integrate_batch(g, tab, desc, scheme, ham, par_dev, sbs, probs, tau[i - 1], tau[i], 3, post_prev,
                                           torch=torch, device=device)
            for b in range(B):
                if where[b]:
                    slot[b] = [k for k in range(3) if k != slot[b]][int(where[b]) - 1]
            if ns.max() > 0:
                path = _bffi.last_kernel()
            steps[:, i - 1] = ns
            tNow = t
            bad = _nan_problems(torch, device, [state_ptr(b) for b in range(B)], (ns > 0).astype(np.int32), n, _ffi.F64)
            if bad:
                error('Nans encountered in the integrated result of HJI PDE data in problems %s' % bad)   # hji_solver.py:544-545
            if data is not None:
                cur = torch.where(torch.as_tensor(slot < 0, device=device).reshape(B, 1), y_init,
                                  S[torch.as_tensor(np.maximum(slot, 0), device=device), ar])
                data[:, i] = cur
        if data is None:
            data = torch.where(torch.as_tensor(slot < 0, device=device).reshape(B, 1), y_init,
                               S[torch.as_tensor(np.maximum(slot, 0), device=device), ar])
            data = data.reshape((B,) + tuple(N))
        else:
            data = data.reshape((B, nt) + tuple(N))
        if not tensors:
            data = data.cpu().numpy()
    return data, steps, tNow, path


def HJIPDE_solve_batch(data0s, tau, schemeDatas, compMethod=None, extraArgs=None):
    global _last_path
    extraArgs = extraArgs if extraArgs is not None else Bundle({})
    quiet = bool(_get(extraArgs, 'quiet', False))
    tau = np.asarray(tau, dtype=np.float64).copy()
    if tau.ndim != 1 or len(tau) < 2:
        error('tau must be a vector of at least two times')
    if np.any(np.diff(tau) < 0):
        error('tau must be non-decreasing')
    if not (is_tensor(data0s) or isinstance(data0s, (HostView, DeviceArray))):
        data0s = np.asarray(data0s)
    B = int(data0s.shape[0])
    if B < 1:
        error('data0s must hold at least one problem')
    sds = _scheme_datas(schemeDatas, extraArgs, B)
    tensors = is_tensor(data0s) or isinstance(data0s, HostView)
    g = sds[0].grid if isfield(sds[0], 'grid') else None
    gdim = int(g.dim) if g is not None else int(np.ndim(_unlazy(data0s))) - 1
    kinds = {what: _per_problem(_get(extraArgs, what), gdim, B, what) for what in ('targetFunction', 'obstacleFunction')}
    setup, why = classify(data0s, sds, compMethod, extraArgs)
    if setup is not None and tuple(int(v) for v in data0s.shape[1:]) != tuple(int(v) for v in np.asarray(g.N).ravel()):
        error('data0s does not agree in array size with grid')
    extraOuts = Bundle({})
    if why is None:
        data, steps, tNow, _last_path = _device_solve(setup, data0s, tau, compMethod, extraArgs, kinds, tensors, quiet)
        extraOuts.steps, extraOuts.tNow = steps, tNow
    else:
        _last_path = "host loop: " + why
        info('HJIPDE_solve_batch: ' + _last_path)
        data, tau = _host_loop(data0s, tau, sds, compMethod, extraArgs, kinds, tensors)
        extraOuts.steps, extraOuts.tNow = None, None
    extraOuts.path = _last_path
    return data, tau, extraOuts
