"""Diffusion and discount terms (reference ExplicitIntegration/Term/term_{trace_hess,disc}.py, Helper/Math/cell_mat_*.py):

    ydot, stepBound, schemeData = termTraceHessian(t, y, schemeData)   ydot = trace(L(x) D^2 phi R(x))
    ydot, stepBound, schemeData = termDiscount(t, y, schemeData)       ydot = -lambda(x) phi
    C = cellMatrixMultiply(A, B)                                      cell x cell, scalar x cell, numeric x numeric
    traceA = cellMatrixTrace(A)                                        sum of the diagonal of a square cell matrix

With termSum, termLaxFriedrichs and odeCFL1/2/3 they integrate phi_t + H(x, grad phi) = tr(sigma D^2 phi sigma^T) - lambda phi
on the device.  termTraceHessian with hessianFunc = hessianSecond is ONE native launch (hj_term_trace_hessian, the
HJ_CURV_TRACE mode of curv_kernel in csrc/hj_curv.h): the Hessian stencil of hessianSecond, the matrices L and R read per
node (array entries) or from the launch arguments (scalar entries), and max |trace(L D R)| for the step bound.  termDiscount
is a host-side array expression like termForcing.  `y` and the arrays in schemeData may be NumPy arrays or device tensors;
results come back as the kind of `y`.

Deviations from the shipped reference, neither of whose terms runs: termTraceHessian calls hessianSecond, which raises
(curvature.py), and multiplies with cellMatrixMultiply, which stores arrays into a float matrix (cell_mat_mult.py:19) and
forms A[i,0] * B[i,j] where B[0,j] is meant (:22); cellMatrixTrace treats its argument as a 3-D array (cell_mat_trace.py:13-17);
termDiscount accepts only a float lambda (term_disc.py:91, so the documented array form errors out) and reshapes y instead
of y[0] in the callable branch (:94).  Implemented here is what their docstrings and ToolboxLS describe.  Parity is
therefore UNPINNED; checked against the NumPy restatement in tests/trace_hess_ref.py and by behaviour (heat equation,
anisotropic covariance growth, discounted decay).
"""
import ctypes as C

import numpy as np

from . import _ffi
from .context import is_tensor
from .curvature import hessianSecond, _prep, _number
from .normal_reinit import _like
from .utilities import isfield, iscell, error

__all__ = ["termTraceHessian", "termDiscount", "cellMatrixMultiply", "cellMatrixTrace"]


def _numeric(a):
    return _number(a) or is_tensor(a) or (isinstance(a, np.ndarray) and a.dtype != object)


def _cell_size(A):
    """(rows, cols) of a cell matrix (a list of equally long lists); error otherwise."""
    if not A or not all(iscell(row) for row in A) or len({len(row) for row in A}) != 1:
        error('A and B must be cell arrays of dimension 2.')
    return len(A), len(A[0])


def cellMatrixMultiply(A, B):
    """Helper/Math/cell_mat_mult.py:7 as ToolboxLS's cellMatrixMultiply: a cell matrix is a list of lists whose entries are
    numbers, NumPy arrays or tensors.  cell x cell: C[i][j] = A[i][0] B[0][j] + A[i][1] B[1][j] + ... (ascending k);
    numeric x cell and cell x numeric: the numeric operand multiplies every entry; numeric x numeric: pointwise."""
    if iscell(A):
        if iscell(B):
            ra, ca = _cell_size(A)
            rb, cb = _cell_size(B)
            if ca != rb:
                error('Inner dimensions of A and B must match.')
            Cm = [[None] * cb for _ in range(ra)]
            for i in range(ra):
                for j in range(cb):
                    c = A[i][0] * B[0][j]
                    for k in range(1, ca):
                        c = c + A[i][k] * B[k][j]
                    Cm[i][j] = c
            return Cm
        if not _numeric(B):
            error('Input B must be a numeric array or a cell matrix')
        scalar, array = B, A
    elif _numeric(A):
        if _numeric(B):
            return A * B                          # pointwise (scalar x scalar included)
        if not iscell(B):
            error('Input B must be a numeric array or a cell matrix')
        scalar, array = A, B
    else:
        error('Input A must be a numeric array or a cell matrix')
    rows, cols = _cell_size(array)
    return [[scalar * array[i][j] for j in range(cols)] for i in range(rows)]


def cellMatrixTrace(A):
    """Helper/Math/cell_mat_trace.py:6 as ToolboxLS's cellMatrixTrace: A[0][0] + A[1][1] + ... of a square cell matrix
    (ascending i); the trace of a numeric matrix."""
    if iscell(A):
        rows, cols = _cell_size(A)
        if rows != cols:
            error('Cell matrix must be square')
        tr = A[0][0]
        for i in range(1, rows):
            tr = tr + A[i][i]
        return tr
    if isinstance(A, np.ndarray) and A.ndim == 2 and A.dtype != object:
        return np.trace(A)
    if is_tensor(A) and A.dim() == 2:
        return A.diagonal().sum()
    error('Input must be a cell matrix or a numeric matrix')


def _get_matrix(t, data, schemeData, inM, name, nd):
    """term_trace_hess.py:131 getMatrix: the three forms of L / R as an nd x nd cell matrix (list of lists) whose entries are
    numbers or arrays of the grid's size.  A callable is called with (t, data, schemeData)."""
    M = inM(t, data, schemeData) if callable(inM) else inM
    if isinstance(M, np.ndarray):
        if M.ndim == 0:
            M = M.item()
        elif M.dtype == object:
            M = M.tolist()                        # a cell matrix stored as an object array
        elif M.ndim == 2:
            M = [[float(v) for v in row] for row in M]
        else:
            error('%s must be a %d x %d matrix' % (name, nd, nd))
    if _number(M):
        if nd != 1:                               # a scalar is the 1 x 1 matrix (ToolboxLS)
            error('%s is a scalar: that is a 1 x 1 matrix, but grid.dim is %d' % (name, nd))
        M = [[M]]
    if not iscell(M) or not all(iscell(row) for row in M):
        error('Input matrix must be a matrix, cell matrix, or function handle.')
    if len(M) != nd or any(len(row) != nd for row in M):
        error('%s must be a %d x %d matrix' % (name, nd, nd))
    M = [[e.item() if isinstance(e, np.ndarray) and e.ndim == 0 else e for e in row] for row in M]
    for row in M:
        for e in row:
            if not (_number(e) or is_tensor(e) or (isinstance(e, np.ndarray) and e.dtype != object)):
                error('%s entries must be scalars or arrays the size of data' % name)
    return M


def _entry_on_device(dg, e, name):
    if int(np.prod(tuple(e.shape))) != int(np.prod(dg.shape)):
        error('%s entries must be scalars or arrays the size of data' % name)
    return dg.to_device(e).reshape(-1)


def _pack(dg, M, name, keep):
    """(array pointers, scalars) of a cell matrix for hj_term_trace_hessian; device copies of the arrays go into `keep`."""
    nn = dg.dim * dg.dim
    ptrs, scal = (C.c_void_p * nn)(), (C.c_double * nn)()
    for i in range(dg.dim):
        for j in range(dg.dim):
            e = M[i][j]
            if _number(e):
                scal[i * dg.dim + j] = float(e)
            else:
                a = _entry_on_device(dg, e, name)
                keep.append(a)
                ptrs[i * dg.dim + j] = a.data_ptr()
    return ptrs, scal


def _entries_like(M, proto, shape, name):
    """Array entries of a cell matrix as arrays of `proto`'s kind with `shape`; numbers stay numbers."""
    out = []
    for row in M:
        r = []
        for e in row:
            if _number(e):
                r.append(e)
                continue
            if int(np.prod(tuple(e.shape))) != int(np.prod(shape)):
                error('%s entries must be scalars or arrays the size of data' % name)
            r.append(_like(e.reshape(shape), proto, shape))
        out.append(r)
    return out


def _max_abs(a):
    if _number(a):
        return abs(float(a))
    if is_tensor(a):
        return float(a.abs().max())
    return float(np.max(np.abs(a)))


def termTraceHessian(t, y, schemeData):
    thisSchemeData = schemeData[0] if iscell(schemeData) else schemeData
    assert isfield(thisSchemeData, 'grid'), 'grid not in schemeData'
    assert isfield(thisSchemeData, 'hessianFunc'), 'hessianFunc not in schemeData'
    assert isfield(thisSchemeData, 'L'), 'L is not in schemeData'
    assert isfield(thisSchemeData, 'R'), 'R is not in schemeData'
    grid = thisSchemeData.grid
    y0 = y[0] if iscell(y) else y
    data = y0.reshape(grid.shape)
    nd = grid.dim
    L = _get_matrix(t, data, thisSchemeData, thisSchemeData.L, 'L', nd)        # term_trace_hess.py:103-104
    R = _get_matrix(t, data, thisSchemeData, thisSchemeData.R, 'R', nd)
    if thisSchemeData.hessianFunc is hessianSecond:
        # the whole term is ONE launch (hj_term_trace_hessian); NumPy data goes over PCIe and comes back as NumPy
        dg, phi = _prep(grid, data)
        keep = []
        Lp, Ls = _pack(dg, L, 'L', keep)
        Rp, Rs = _pack(dg, R, 'R', keep)
        out, sb = dg.empty(), C.c_double()
        _ffi.check(dg.lib.hj_term_trace_hessian(dg.ctx, dg.ptr(phi), Lp, Ls, Rp, Rs, dg.ptr(out), C.byref(sb)))
        return dg.like(out, y0, (-1, 1)), float(sb.value), schemeData
    # a foreign hessianFunc: its Hessian, then the cell helpers on whatever kind of array it returns
    P = thisSchemeData.hessianFunc(grid, data)                                   # :107
    if isinstance(P, tuple):                                                     # (second, first) as hessianSecond returns
        P = P[0]
    P = [list(row) for row in P]
    for i in range(nd):                                                          # :110-112  the upper right
        for j in range(i + 1, nd):
            P[i][j] = P[j][i]
    proto = P[0][0]
    shape = tuple(proto.shape)
    L = _entries_like(L, proto, shape, 'L')
    R = _entries_like(R, proto, shape, 'R')
    update = cellMatrixTrace(cellMatrixMultiply(cellMatrixMultiply(L, P), R))  # :115-116
    dx = [float(v) for v in np.asarray(grid.dx, dtype=np.float64).ravel()]
    D = [[1 / (dx[m] * dx[k]) for k in range(nd)] for m in range(nd)]           # :119
    maxT = _max_abs(cellMatrixTrace(cellMatrixMultiply(cellMatrixMultiply(L, D), R)))   # :120-122
    stepBound = float('inf') if maxT == 0 else 1 / (2 * maxT)
    return update.reshape(-1, 1), stepBound, schemeData                         # :127  no negation


def termDiscount(t, y, schemeData):
    thisSchemeData = schemeData[0] if iscell(schemeData) else schemeData
    assert isfield(thisSchemeData, 'grid'), 'grid not in schemeData'
    assert isfield(thisSchemeData, 'lambder'), 'lambder not in schemeData'
    grid = thisSchemeData.grid
    y0 = y[0] if iscell(y) else y
    data = y0.reshape(grid.shape)                                                # term_disc.py:85-88
    lambder = thisSchemeData.lambder
    if callable(lambder):
        lambder = lambder(t, data, thisSchemeData)                              # :93-95, on y[0]
    if not (_number(lambder) or is_tensor(lambder) or isinstance(lambder, np.ndarray)):
        error('schemeData.lambder must be a scalar, array or function handle')  # :96-97
    if isinstance(lambder, np.ndarray) and lambder.ndim == 0:
        lambder = float(lambder)
    if not _number(lambder):
        lambder = _like(lambder.reshape(data.shape), data, tuple(data.shape))
    delta = lambder * data                                                       # :101
    return (-delta).reshape(-1, 1), float('inf'), schemeData                    # :102-107  no derivative, no time step limit
