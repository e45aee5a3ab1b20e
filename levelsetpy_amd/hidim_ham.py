"""A user's hamFunc / partialFunc pair as a fused kernel on 5-D and 6-D grids (C ABI: hjh_ham_register, include/hj_hidim.h).

What user_ham.register_native_hamiltonian is to the solver of libhj_mi355x.so, for libhj_hidim.so: write H and alpha ONCE more, as a
device expression; hidim_substep_kernel and hidim_bound_kernel are compiled around it with hipRTC, and a schemeData that carries the system's
own bound methods runs as Plane5D and DubinsPair6D do -- one launch per Runge-Kutta stage, a whole tau interval in one native call, no
derivative arrays -- selected by callable identity (dynamics.native_of).

    Quad = register_hidim_hamiltonian("planar_quad", 6, '''
        const T k = (p[3] * aux[1] - p[1] * aux[0]) / par[0];        // aux[0] = sin(x4), aux[1] = cos(x4), looked up for this cell
        ...
        H = ...;  alpha[0] = fabs(x[1]); ... alpha[5] = ...;
    ''', nparams=8, aux_axes=(4, 4))
    sys_ = Quad(grid, params, tables=[np.sin(grid.vs[4]), np.cos(grid.vs[4])], hamiltonian=py_ham, dissipation=py_diss)
    Quad.attach(obj, params=..., tables=...)                         # or: an EXISTING object with .hamiltonian / .dissipation / .grid
    Quad.check("ENO3", "float64")                                    # compiles now, no GPU needed

In the expression: x[d] node coordinates, p[d] costates (the reference's derivC), par[k] parameters (at most HJH_PAR_SLOTS), aux[k] the value of
the caller's k-th table at this cell's index along axis aux_axes[k] (at most four tables), T the element type, device math functions; assign H
and every alpha[d].  The tables are 1-D NumPy arrays the caller makes from grid.vs: trigonometry done by NumPy on the host is then the same
number in the Python callbacks and in the kernel (device sin / cos in the expression are allowed as well, and differ from NumPy's in the last
bits).  With upwindFirstENO2 / ENO3 the expression is compiled with contraction off: written one operation per statement like the NumPy
callback, it rounds where NumPy rounds.

The expression has neither t, data nor the costate range: one that names dmin / dmax is refused (such a pair takes the split path).  No
column_src and no march: the kernel is one thread per cell.
"""
import ctypes as C
import os
import re

import numpy as np

from . import _ffi, _hffi
from .user_ham import ATTACH_EPOCH, HERE, RegisteredSystem, _Attached, _hiprtc_path

__all__ = ["register_hidim_hamiltonian", "HidimRegistration", "HidimSystem", "hidim_kernel_cache_stats"]

_NAMES = {}             # ham_id -> name, for the kernel's printed name


def name_of(ham_id):
    return _NAMES[int(ham_id)]


def _tables_of(reg, grid, tables):
    """The caller's tables as contiguous fp64 vectors, checked against the grid."""
    tables = [np.ascontiguousarray(np.asarray(t, dtype=np.float64)) for t in (tables if tables is not None else ())]
    if len(tables) != len(reg.aux_axes):
        raise ValueError("Hamiltonian '%s' reads %d tables, got %d" % (reg.name, len(reg.aux_axes), len(tables)))
    N = [int(n) for n in np.asarray(grid.N).ravel()]
    for k, (t, ax) in enumerate(zip(tables, reg.aux_axes)):
        if t.ndim != 1 or t.shape[0] != N[ax]:
            raise ValueError("Hamiltonian '%s': table %d runs along axis %d and must be a vector of N[%d] = %d values, got shape %s"
                             % (reg.name, k, ax, ax, N[ax], tuple(t.shape)))
    return tables


class _HiAttached(_Attached):
    """user_ham._Attached plus the system's tables (hidim.py keeps them on the device per grid, dtype, device and system)."""

    def __init__(self, reg, params, ham_func, diss_func, tables):
        _Attached.__init__(self, reg, params, ham_func, diss_func)
        self.tables = tables


class HidimSystem(RegisteredSystem):
    """A system object around a registration: the reference's callback protocol (.hamiltonian / .dissipation, from the Python callables given
    -- they serve the split path and parity checks) plus the native kernel and its tables."""

    def __init__(self, reg, grid, params, tables=(), hamiltonian=None, dissipation=None):
        RegisteredSystem.__init__(self, reg, grid, params, hamiltonian, dissipation)
        self.tables = _tables_of(reg, grid, tables)
        self._hj_native = _HiAttached(reg, lambda s: s.params, RegisteredSystem.hamiltonian, RegisteredSystem.dissipation, self.tables)
        self._hj_native.params(self)            # validates the count now


class HidimRegistration(object):
    def __init__(self, name, dim, device_src, nparams=0, aux_axes=()):
        self.name, self.dim, self.nparams, self.device_src = str(name), int(dim), int(nparams), str(device_src)
        self.aux_axes = tuple(int(a) for a in aux_axes)
        self.uses_range = False
        if self.dim not in (_hffi.MIN_DIM, _hffi.MAX_DIM):
            raise ValueError("register_hidim_hamiltonian: dim must be 5 or 6, got %d (2..4: register_native_hamiltonian)" % self.dim)
        if not 0 <= self.nparams <= _hffi.PAR_SLOTS:
            raise ValueError("Hamiltonian '%s': at most %d parameters (HJH_PAR_SLOTS), got %d" % (self.name, _hffi.PAR_SLOTS, self.nparams))
        if len(self.aux_axes) > 4:
            raise ValueError("Hamiltonian '%s': at most four tables (the aux slots of hjh_tables), got %d" % (self.name, len(self.aux_axes)))
        for k, ax in enumerate(self.aux_axes):
            if not 0 <= ax < self.dim:
                raise ValueError("Hamiltonian '%s': table %d runs along axis %d, outside the grid's 0..%d" % (self.name, k, ax, self.dim - 1))
        if '"' in self.name or "'" in self.name:
            raise ValueError("the name of a Hamiltonian must not contain quotes: %r" % self.name)
        if re.search(r"\bd(min|max)\b", self.device_src):
            raise ValueError("Hamiltonian '%s' reads the costate range (dmin / dmax): the 5-D / 6-D kernel has none -- its step bound is a "
                             "property of the grid.  Hand such a hamFunc / partialFunc over unregistered: they take the split path" % self.name)
        ham = C.c_int()
        rtc = _hiprtc_path()
        axes = (C.c_int32 * 4)(*(list(self.aux_axes) + [0] * (4 - len(self.aux_axes))))
        _hffi.check(_hffi.lib().hjh_ham_register(self.name.encode(), self.dim, self.nparams, self.device_src.encode(), len(self.aux_axes), axes,
                                                 os.path.join(HERE, "csrc").encode(), rtc.encode() if rtc else None, C.byref(ham)))
        self.ham_id = int(ham.value)
        _NAMES[self.ham_id] = self.name

    def check(self, scheme="WENO5_ASSHIPPED", dtype="float64"):
        """Compile the substep kernel of (scheme, dtype) and the bound kernel now (no GPU needed): raises ValueError with the compiler's
        message, which points into the expression as name:line, if it is wrong."""
        _hffi.check(_hffi.lib().hjh_ham_compile_check(self.ham_id, _ffi.SCHEME_IDS[scheme], _ffi.F64 if dtype == "float64" else _ffi.F32))
        return self

    def source(self):
        """The translation unit hipRTC is given (hjh_ham_source), for a look at it or an offline hipcc."""
        n = 2 * len(self.device_src.encode()) + 16384
        buf = C.create_string_buffer(n)
        _hffi.check(_hffi.lib().hjh_ham_source(self.ham_id, buf, n))
        return buf.value.decode()

    def __call__(self, grid, params=(), tables=(), hamiltonian=None, dissipation=None):
        return HidimSystem(self, grid, params, tables, hamiltonian, dissipation)

    def attach(self, obj, params=(), tables=()):
        """Mark an existing system object (it must have .grid and bound .hamiltonian / .dissipation methods): a schemeData whose hamFunc /
        partialFunc are THOSE methods then runs fused.  params: a list, or a callable of the object; tables: as in __call__."""
        cls = type(obj)
        if not hasattr(obj, "grid"):
            raise ValueError("the system object needs a .grid (the fused path checks that schemeData.grid is the same grid)")
        if int(obj.grid.dim) != self.dim:
            raise ValueError("Hamiltonian '%s' is %d-dimensional, the object's grid has dim %d" % (self.name, self.dim, obj.grid.dim))
        att = _HiAttached(self, params, getattr(cls, "hamiltonian", None), getattr(cls, "dissipation", None), _tables_of(self, obj.grid, tables))
        if att.ham_func is None or att.diss_func is None:
            raise ValueError("the system object's class needs hamiltonian() and dissipation() methods")
        att.params(obj)                      # validates the count now
        obj._hj_native = att
        ATTACH_EPOCH[0] += 1
        return obj


def hidim_kernel_cache_stats():
    """(5-D / 6-D kernels compiled with hipRTC, kernels loaded from the on-disk cache) in this process; the cache is
    user_ham.kernel_cache_stats's."""
    a, b = C.c_int(), C.c_int()
    _hffi.check(_hffi.lib().hjh_ham_cache_stats(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def register_hidim_hamiltonian(name, dim, device_src, nparams=0, aux_axes=()):
    """Register H / alpha of a 5-D or 6-D system as a device expression (module docstring); returns a HidimRegistration: call it to make a
    system object, or .attach() it to an existing one.  aux_axes: the axis each of the system's tables runs along."""
    return HidimRegistration(name, dim, device_src, nparams, aux_axes)
