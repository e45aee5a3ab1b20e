"""Hamilton-Jacobi problems on 5-D and 6-D grids: the front end of libhj_hidim.so (include/hj_hidim.h).

The solver of libhj_mi355x.so stops at four dimensions.  Every function of the package that meets a grid of 5 or 6
dimensions comes here instead: HJIPDE_solve (solve), termLaxFriedrichs / termRestrictUpdate (fused_term),
upwindFirstENO2 / ENO3 / WENO5 as shipped and computeGradients (upwind_one, upwind_all).  Grids of 7 or more dimensions
stay refused.

Two paths:
  fused   hamFunc / partialFunc are the methods of Plane5D or DubinsPair6D (dynamics.py, native_of's identity rule), or of a
          system registered with hidim_ham.register_hidim_hamiltonian (its kernel is compiled at run time around the
          user's expression and reads the system's own tables): every Runge-Kutta stage is ONE launch of hidim_substep_kernel, a whole tau interval one native call
          (hjh_integrate), the compMethod minimum / maximum and the obstacle mask applied by the last stage of a step.
          With set_hidim_trace(True) (trace_ham.py; off by default) foreign callbacks are traced into such a registration and, once
          checked against the callbacks on the caller's data, run the same way.
  split   any other callbacks: hjh_upwind writes derivL[d], derivR[d] of every axis from one gather per cell, the
          callbacks run on device tensors, and the dissipation sum, -(ham - diss) and the stage expressions follow as
          torch expressions in the reference's order.  This path holds 2 * dim derivative arrays of the grid's size
          (12 at 6-D) besides the state and the callbacks' own temporaries.
last_path() says which one the calling process's last call took.  The solve runs in fp64.
"""
import ctypes as C
import weakref

import numpy as np

from . import _ffi, _hffi
from .context import DeviceGrid, grid_bc, is_tensor, require_gpu, _raw_stream_getter, array_dtype_name
from .lazy import HostView, DeviceArray
from .utilities import Bundle, error, info, isfield, cputime, realmax

__all__ = ["solve", "fused_term", "upwind_one", "upwind_all", "step_bound", "hi_grid", "last_path", "is_hidim", "check_dim"]

SMALL = 1e-4            # HJIPDE_solve's `while tNow < tau[i] - small` (hji_solver.py:185)
FACTOR_CFL = 0.8        # its integratorOptions

_last_path = ""


def last_path():
    """What the calling process's last 5-D / 6-D call ran: the kernel's name, or 'split: <why>'."""
    return _last_path


def _set_path(p):
    global _last_path
    _last_path = p


def is_hidim(grid):
    return int(grid.dim) > 4


def check_dim(grid):
    if not 1 <= int(grid.dim) <= _hffi.MAX_DIM:
        error('grid.dim must be 1..%d (got %d): grids of more than %d dimensions have no device implementation'
              % (_hffi.MAX_DIM, int(grid.dim), _hffi.MAX_DIM))


class HiGrid(DeviceGrid):
    """What DeviceGrid is to libhj_mi355x.so, without an hj_ctx: the descriptor, the coordinate and trig tables, and the
    array marshalling (to_device, like, empty, ptr are DeviceGrid's own)."""

    def __init__(self, grid, dtype="float64", device=None):
        torch = require_gpu()
        check_dim(grid)
        self.torch = torch
        self.lib = _hffi.lib()
        self.dim = int(grid.dim)
        self.shape = tuple(int(n) for n in np.asarray(grid.N).ravel())
        self.numel = int(np.prod(self.shape))
        self.dtype_name = dtype
        self.tdtype = torch.float64 if dtype == "float64" else torch.float32
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.dx = [float(v) for v in np.asarray(grid.dx).ravel()]
        vs = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in grid.vs]
        bc, tz = grid_bc(grid)
        self.bc = bc
        self.desc = _hffi.grid_descriptor(self.dim, self.shape, [float(v[0]) for v in vs], [float(v[-1]) for v in vs],
                                          self.dx, bc, tz, dtype)
        # trig tables made by NumPy from g.vs, so that they are np.cos(grid.xs[2]) etc. bit for bit (rounded once for fp32)
        aux = [np.cos(vs[2]), np.sin(vs[2])]
        if self.dim == 6:
            aux += [np.cos(vs[5]), np.sin(vs[5])]
        self._keep = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.tdtype).to(self.device) for a in vs + aux]
        self.tab = _hffi.Tables()
        for d in range(self.dim):
            self.tab.coord[d] = self._keep[d].data_ptr()
        for s in range(len(aux)):
            self.tab.aux[s] = self._keep[self.dim + s].data_ptr()
        self._work = {}
        self._raw_stream = _raw_stream_getter(torch)
        self._keys = torch.zeros((4 * _hffi.MAX_DIM,), dtype=torch.int64, device=self.device)
        self._sb = {}
        self._user_tabs = weakref.WeakKeyDictionary()      # registered system -> (fingerprint, Tables, its tensors)

    def tables_of(self, system):
        """(Tables, fingerprint) for a launch of `system`: the grid's own for a built-in, and for a registered system (hidim_ham.py) the
        grid's coordinate tables with that system's aux tables -- kept on the device per system, away from the grid-wide cos / sin cache,
        and uploaded again when the system's tables change."""
        att = getattr(system, "_hj_native", None)
        if att is None or not hasattr(att, "tables"):
            return self.tab, ()
        fp = tuple(t.tobytes() for t in att.tables)
        hit = self._user_tabs.get(system)
        if hit is None or hit[0] != fp:
            torch = self.torch
            keep = [torch.from_numpy(np.array(t, dtype=np.float64)).to(self.tdtype).to(self.device) for t in att.tables]
            tab = _hffi.Tables()
            for d in range(self.dim):
                tab.coord[d] = self.tab.coord[d]
            for k, t in enumerate(keep):
                tab.aux[k] = t.data_ptr()
            hit = (fp, tab, keep)
            self._user_tabs[system] = hit
        return hit[1], fp

    def stream(self):
        return C.c_void_p(self._raw_stream(self.device.index))

    def bind_stream(self):
        pass

    def step_bound(self, ham, par, system=None):
        """stepBound of (grid, system): data independent, one hjh_step_bound call per parameter set (and, for a registered system, per
        content of its tables)."""
        tab, fp = self.tables_of(system)
        key = (ham, tuple(par), fp)
        sb = self._sb.get(key)
        if sb is None:
            v = C.c_double()
            _hffi.check(self.lib.hjh_step_bound(C.byref(self.desc), C.byref(tab), int(ham), _hffi.params(par),
                                                self.ptr(self._keys), C.byref(v), None, self.stream()))
            sb = self._sb[key] = float(v.value)
        return sb


def hi_grid(grid, dtype="float64"):
    """Cached HiGrid of a grid Bundle (kept on the Bundle itself, like context.device_grid)."""
    check_dim(grid)
    cache = grid.__dict__.get("_hj_hidim")
    if cache is None:
        cache = {}
        object.__setattr__(grid, "_hj_hidim", cache)
    torch = require_gpu()
    key = (dtype, torch.cuda.current_device())
    hg = cache.get(key)
    if hg is None:
        hg = cache[key] = HiGrid(grid, dtype)
    return hg


def step_bound(grid, ham, par, dtype="float64", system=None):
    """system: the registered system object whose tables the kernel reads (hidim_ham.py); not needed for the built-ins."""
    return hi_grid(grid, dtype).step_bound(ham, par, system)


def _check_scheme(sid):
    if sid == _ffi.SCHEME_IDS["WENO5"]:
        error('upwindFirstWENO5Intended (the intended WENO5, set_weno5_mode("weno5")) has no 5-D / 6-D kernel: its epsilon is a '
              'reduction over the whole grid; use upwindFirstWENO5 as shipped, upwindFirstENO3 or upwindFirstENO2')
    # the opt-in lean ENO arithmetic has no instantiation here: the exact one is what runs
    fast = {_ffi.SCHEME_IDS.get("ENO2_FAST"): _ffi.ENO2, _ffi.SCHEME_IDS.get("ENO3_FAST"): _ffi.ENO3}
    return fast.get(sid, sid)


# ------------------------------------------------------------------------------------------ derivatives
def upwind_all(sid, grid, data, dims=None):
    """derivL[d], derivR[d] (device tensors) for the axes of `dims` (default: all) with ONE launch of hidim_upwind_kernel and one host
    synchronisation for the reductions artificialDissipationGLF needs (tagged on the tensors, spatial.cached_minmax)."""
    sid = _check_scheme(sid)
    hg = hi_grid(grid, array_dtype_name(data))
    if tuple(data.shape) != hg.shape:
        error('data parameter does not agree in array size with grid')
    dims = list(range(hg.dim)) if dims is None else [int(d) for d in dims]
    phi = hg.to_device(data)
    dL, dR = [None] * hg.dim, [None] * hg.dim
    vp = C.c_void_p * _hffi.MAX_DIM
    pl, pr = vp(), vp()
    mask = 0
    for d in dims:
        dL[d], dR[d] = hg.empty(), hg.empty()
        pl[d], pr[d] = dL[d].data_ptr(), dR[d].data_ptr()
        mask |= 1 << d
    _hffi.check(hg.lib.hjh_upwind(C.byref(hg.desc), int(sid), hg.ptr(phi), mask, pl, pr, hg.ptr(hg._keys), hg.stream()))
    _set_path(_hffi.last_kernel())
    keys = hg._keys.cpu().numpy().view(np.uint64)
    for d in dims:
        mm = [_key_value(int(keys[4 * d + k])) for k in range(4)]            # { -min L, max L, -min R, max R }
        dL[d]._hj_minmax = (weakref.ref(dR[d]), dL[d]._version, dR[d]._version, min(-mm[0], -mm[2]), max(mm[1], mm[3]))
    return dL, dR


def _key_value(k):
    b = (k & 0x7fffffffffffffff) if (k & 0x8000000000000000) else (~k & 0xffffffffffffffff)
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def upwind_one(scheme_name, grid, data, dim):
    """upwindFirst*(grid, data, dim) on a 5-D / 6-D grid: NumPy in -> NumPy out, tensor in -> tensor out."""
    hg = hi_grid(grid, array_dtype_name(data))
    dL, dR = upwind_all(_ffi.SCHEME_IDS[scheme_name], grid, data, [dim])
    if is_tensor(data):
        return dL[dim], dR[dim]
    return hg.like(dL[dim], data), hg.like(dR[dim], data)


# ------------------------------------------------------------------------------------------ the term
def _substep(hg, sid, ham, par, stage, rs, src, y0, dst, dt=0.0, post_prev=0, op_a=0, post_a=None, op_b=0, post_b=None, tab=None):
    _hffi.check(hg.lib.hjh_substep(C.byref(hg.desc), C.byref(hg.tab if tab is None else tab), int(sid), int(ham), int(stage), int(rs), _hffi.params(par),
                                   hg.ptr(src), hg.ptr(y0), hg.ptr(dst), float(dt), int(post_prev), int(op_a), hg.ptr(post_a),
                                   int(op_b), hg.ptr(post_b), hg.stream()))


def fused_term(plan, t, y, restrict_sign):
    """termLaxFriedrichs (restrict_sign 0) / termRestrictUpdate over it (+-1) of a native 5-D / 6-D system: one launch of
    hidim_substep_kernel with HJ_STAGE_YDOT.  -> (ydot tensor of the grid's shape, stepBound, HiGrid), as term._fused_term."""
    grid, sid, ham, par = plan
    sid = _check_scheme(sid)
    hg = hi_grid(grid, array_dtype_name(y))
    if int(np.prod(y.shape)) != hg.numel:
        raise ValueError('y does not agree in size with grid')
    yd = hg.to_device(y)
    out = hg.empty()
    system = getattr(plan, "system", None)
    _substep(hg, sid, ham, par, _ffi.STAGE_YDOT, restrict_sign, yd, None, out, tab=hg.tables_of(system)[0])
    _set_path(_hffi.last_kernel())
    return out, hg.step_bound(ham, par, system), hg


# ------------------------------------------------------------------------------------------ HJIPDE_solve
_NONE = (None, 'none', 'set', 'zero', 'minWithZero')
_PREV = {'minVOverTime': _ffi.POST_MIN_PREV, 'maxVOverTime': _ffi.POST_MAX_PREV}
_V0 = {'minVWithV0': _hffi.ARR_MIN, 'maxVWithV0': _hffi.ARR_MAX}
_TARGET = {'minVWithL': _hffi.ARR_MIN, 'minVwithL': _hffi.ARR_MIN, 'minVWithTarget': _hffi.ARR_MIN,
           'maxVWithL': _hffi.ARR_MAX, 'maxVwithL': _hffi.ARR_MAX, 'maxVWithTarget': _hffi.ARR_MAX}
# extraArgs with no 5-D / 6-D implementation: named in the refusal
_REFUSED = ('stopInit', 'stopSetInclude', 'stopSetIntersect', 'stopLevel', 'discountFactor', 'discountMode', 'discountAnneal',
            'SDModFunc', 'SDModParams', 'computeTTR', 'ttrLevel', 'ttrCrossing', 'ttrInterpolate', 'ignoreBoundary')


def _get(b, name, default=None):
    return getattr(b, name) if (b is not None and isfield(b, name)) else default


def _unlazy(a):
    if isinstance(a, HostView):
        return a.device_tensor() if a.device_tensor() is not None else a.__array__()
    if isinstance(a, DeviceArray) and a.device_tensor() is not None:
        return a.device_tensor()
    return a


def _array_op(torch, op, y, other):
    # NaN propagating, as NumPy's minimum / maximum (torch.minimum / maximum do the same)
    if op == _hffi.ARR_MIN:
        return torch.minimum(y, other)
    if op == _hffi.ARR_MAX:
        return torch.maximum(y, other)
    return torch.maximum(y, -other)


def solve(data0, tau, schemeData, compMethod=None, extraArgs=None):
    """HJIPDE_solve on a grid of 5 or 6 dimensions (hji_solver.py hands over before it touches anything)."""
    from .dissipation import artificialDissipationGLF, artificialDissipationLLF, artificialDissipationLLLF
    from .dynamics import native_of
    from .integration import odeCFL3, odeCFLset
    from .spatial import upwindFirstWENO5, scheme_id_of
    from .term import termLaxFriedrichs, termRestrictUpdate

    extraArgs = extraArgs if extraArgs is not None else Bundle({})
    extraOuts = Bundle({})
    g = schemeData.grid
    check_dim(g)
    gDim = int(g.dim)
    quiet = bool(_get(extraArgs, 'quiet', False))
    keepLast = bool(_get(extraArgs, 'keepLast', False))
    lowMemory = bool(_get(extraArgs, 'lowMemory', False))
    flipOutput = bool(_get(extraArgs, 'flipOutput', False))
    tau = np.asarray(tau, dtype=np.float64).copy()
    if tau.ndim != 1 or len(tau) < 2:
        error('tau must be a vector of at least two times')
    if np.any(np.diff(tau) < 0):
        error('tau must be non-decreasing')
    # ---- what has no implementation at these dimensions: refused by name
    for name in _REFUSED:
        v = _get(extraArgs, name)
        if v is not None and v is not False:
            error('extraArgs.%s has no implementation on grids of 5 or 6 dimensions' % name)
    if isfield(extraArgs, 'addGaussianNoiseStandardDeviation'):
        error('extraArgs.addGaussianNoiseStandardDeviation has no implementation on grids of 5 or 6 dimensions')
    if isfield(schemeData, 'dissFunc') and schemeData.dissFunc in (artificialDissipationLLF, artificialDissipationLLLF):
        error('%s (a local Lax-Friedrichs dissipation) has no implementation on grids of 5 or 6 dimensions: '
              'artificialDissipationGLF only' % schemeData.dissFunc.__name__)
    if compMethod not in _NONE and compMethod not in _PREV and compMethod not in _V0 and compMethod not in _TARGET:
        error('Check which compMethod you are using')
    schemeData.dissFunc = artificialDissipationGLF
    if not isfield(schemeData, 'CoStateCalc') and not isfield(schemeData, 'derivFunc'):
        schemeData.derivFunc = upwindFirstWENO5
    calc = schemeData.CoStateCalc if isfield(schemeData, 'CoStateCalc') else schemeData.derivFunc
    sid = scheme_id_of(calc)
    if sid is not None:
        sid = _check_scheme(sid)

    targets = _get(extraArgs, 'targetFunction')
    obstacles = _get(extraArgs, 'obstacleFunction')
    for a, what in ((targets, 'target'), (obstacles, 'obstacle')):
        if a is not None and np.ndim(_unlazy(a)) not in (gDim, gDim + 1):
            error('Inconsistent %s dimensions!' % what)
    targ_tv = targets is not None and np.ndim(_unlazy(targets)) == gDim + 1
    obs_tv = obstacles is not None and np.ndim(_unlazy(obstacles)) == gDim + 1
    stopConverge = bool(_get(extraArgs, 'stopConverge', False))
    convergeThreshold = _get(extraArgs, 'convergeThreshold', 1e-5)

    torch = require_gpu()
    src = _unlazy(data0)
    tensors = is_tensor(src) or isinstance(data0, HostView)
    nd0 = src.dim() if is_tensor(src) else np.ndim(src)
    if nd0 != gDim:
        error('Inconsistent initial condition dimension!' if nd0 != gDim + 1 else
              'a time history in data0 has no implementation on grids of 5 or 6 dimensions')
    hg = hi_grid(g, "float64")
    if tuple(int(v) for v in src.shape) != hg.shape:
        error('data0 does not agree in array size with grid')
    startTime = cputime()
    n = hg.numel
    y_init = hg.to_device(src).reshape(n)          # only ever read (it may be the caller's own tensor)
    y = y_init
    store_all = not keepLast and not lowMemory
    if store_all:
        data = (torch.empty((len(tau), n), dtype=torch.float64, device=hg.device) if tensors
                else np.zeros((len(tau), n), dtype=np.float64))
        data[0] = y_init if tensors else y_init.cpu().numpy()

    restrict = compMethod in ('minWithZero', 'zero')
    rs = -1 if restrict else 0                   # termRestrictUpdate with positive = 0 (hji_solver.py)
    nat = native_of(schemeData.hamFunc, schemeData.partialFunc) if (isfield(schemeData, 'hamFunc') and isfield(schemeData, 'partialFunc')) else None
    why = not_traced = None
    if nat is None and sid is not None and isfield(schemeData, 'hamFunc') and isfield(schemeData, 'partialFunc'):
        from . import trace_ham
        if trace_ham.hidim_enabled():
            # foreign callbacks, traced (set_hidim_trace): a plan that has been checked against them on this data runs as a registered system does
            from .term import native_plan, explain_plan
            plan = native_plan(schemeData, y_init)
            if plan is not None and plan.traced:
                nat = (plan.system, plan[2], list(plan[3]))
            else:
                not_traced = explain_plan(schemeData).get('reason', 'no plan')
    if nat is None:
        why = 'hamFunc / partialFunc are not the methods of Plane5D / DubinsPair6D or of a system registered with register_hidim_hamiltonian'
        if not_traced is not None:
            why += ', and were not traced: %s' % not_traced
    elif _hffi.ham_dim(nat[1]) != gDim or nat[0].grid is not g:
        why = 'the system does not live on this grid'
    elif sid is None:
        why = 'the derivative function is not one of upwindFirstENO2 / ENO3 / WENO5'
    fused = why is None
    if fused:
        ham, par = nat[1], [float(v) for v in nat[2]]
        tab = hg.tables_of(nat[0])[0]
        sb = hg.step_bound(ham, par, nat[0])
        path = "%s (no step taken)" % _hffi.kernel_name("float64", ham, sid)
    else:
        path = "split: " + why
        if not quiet:
            info('HJIPDE_solve on a %d-D grid: %s' % (gDim, path))
        sd_run = Bundle(dict(innerFunc=termLaxFriedrichs, innerData=schemeData, positive=0)) if restrict else schemeData
        schemeFunc = termRestrictUpdate if restrict else termLaxFriedrichs
        options = odeCFLset(Bundle({'factorCFL': FACTOR_CFL, 'singleStep': 'on'}))
    post_prev = _PREV.get(compMethod, _ffi.POST_NONE)
    bufs = [hg.empty((n,)) for _ in range(3)] if fused else None     # the state rotates through them: y is never written by its own step
    work = hg.empty((n,)) if fused else None

    def prep(a):
        return hg.to_device(_unlazy(a)).reshape(n) if a is not None else None

    target_s = prep(targets) if (targets is not None and not targ_tv) else None
    obstacle_s = prep(obstacles) if (obstacles is not None and not obs_tv) else None
    stopped = None
    for i in range(1, len(tau)):
        if not quiet:
            info('Computing value function at time tau[%d]: %.4f' % (i, tau[i]))
        target_i = prep(targets[i]) if targ_tv else target_s
        obstacle_i = prep(obstacles[i]) if obs_tv else obstacle_s
        op_a, arr_a = 0, None
        if compMethod in _V0:
            op_a, arr_a = _V0[compMethod], y_init
        elif compMethod in _TARGET:
            if target_i is None:
                error('Need to define target function l(x)!')
            op_a, arr_a = _TARGET[compMethod], target_i
        op_b, arr_b = (_hffi.ARR_MAX_NEG, obstacle_i) if obstacle_i is not None else (0, None)
        y_start = y
        tNow = tau[i - 1]
        if fused:
            free = [b for b in bufs if b.data_ptr() != y.data_ptr()]
            tout, nsteps, where = C.c_double(), C.c_int64(), C.c_int32()
            _hffi.check(hg.lib.hjh_integrate(
                C.byref(hg.desc), C.byref(tab), int(sid), int(ham), 3, rs, int(post_prev), _hffi.params(par), float(sb),
                hg.ptr(y), hg.ptr(free[0]), hg.ptr(free[1]), hg.ptr(work), int(op_a), hg.ptr(arr_a), int(op_b), hg.ptr(arr_b),
                float(tNow), float(tau[i]), FACTOR_CFL, float(realmax), SMALL, C.byref(tout), C.byref(nsteps), C.byref(where),
                hg.stream()))
            if nsteps.value > 0:
                path = _hffi.last_kernel()
                y = free[where.value - 1]
            tNow = float(tout.value)
            if bool(torch.isnan(y).any()):
                error('Nans encountered in the integrated result of HJI PDE data')       # hji_solver.py:544-545
        else:
            ycol = y.reshape((n, 1) if not restrict else (n,))
            while tNow < tau[i] - SMALL:                                                  # hji_solver.py:536
                yLast = ycol
                if not quiet:
                    info('Cur Time %s bound: %s' % (tNow, tau[i] - SMALL))
                tNow, ycol, _ = odeCFL3(schemeFunc, [tNow, tau[i]], ycol, options, sd_run)
                if bool(torch.isnan(ycol).any()):
                    error('Nans encountered in the integrated result of HJI PDE data')
                if post_prev:
                    ycol = _array_op(torch, _hffi.ARR_MIN if post_prev == _ffi.POST_MIN_PREV else _hffi.ARR_MAX, ycol, yLast)
                if op_a:
                    ycol = _array_op(torch, op_a, ycol, arr_a.reshape(ycol.shape))
                if op_b:
                    ycol = _array_op(torch, op_b, ycol, arr_b.reshape(ycol.shape))
            y = ycol.reshape(n)
        if store_all:
            data[i] = y if tensors else y.cpu().numpy()
        if stopConverge:                                                                  # hji_solver.py:661-672, 706-722
            change = float((y - y_start).abs().max())
            if not quiet:
                info('Max change since last iteration: %s' % change)
            if change < convergeThreshold:
                extraOuts.stoptau = tau[i]
                stopped = i
                break
    if stopped is not None:
        tau = tau[:stopped + 1]
        if store_all:
            data = data[:stopped + 1]
    if store_all:
        data = data.reshape((len(tau),) + hg.shape)
        if flipOutput:
            data = data.flip(0) if tensors else np.flip(data, 0).copy()
    else:
        out = y.reshape(hg.shape)
        if y is y_init:
            out = out.clone()
        data = out if tensors else hg.like(out, src)
    _set_path(path)
    extraOuts.path = path
    if not quiet:
        info('Total execution time %s seconds' % (cputime() - startTime))
    return data, tau, extraOuts
