"""CPU-only: systems registered at run time on 5-D / 6-D grids (levelsetpy_amd/hidim_ham.py, hjh_ham_* of include/hj_hidim.h), in the
manner of tests/test_hidim_host.py: every data pointer is a fake or null and every check comes before the first HIP call, and
hipRTC cross-compiles for gfx950 without a device.

  1. ids, identity of a registration, hjh_ham_info
  2. .check compiles substep and bound kernels for the three schemes and both types; a wrong symbol is reported as name:line
  3. every refusal at registration, each a ValueError by name
  4. hjh_substep with an unknown id, an id on the wrong dimension or a missing table: the error code and no launch
  5. native_of's identity rule for attached objects
  6. explain_plan
  7. the offline resource report of the three systems: no scratch
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, _hffi  # noqa: E402
from levelsetpy_amd.dynamics import native_of, native_plant_hi  # noqa: E402
import hidim_user_cases as UC  # noqa: E402
import hidim_user_resources as UR  # noqa: E402
from test_hidim_host import FAKE, EINVAL, grid, lgrid, tables  # noqa: E402

H = _hffi


def plane():
    return L.register_hidim_hamiltonian("plane5d_tables", 5, UC.PLANE_SRC, nparams=3, aux_axes=UC.PLANE_AXES)


def quad():
    return L.register_hidim_hamiltonian("planar_quad", 6, UC.QUAD_SRC, nparams=8, aux_axes=UC.QUAD_AXES)


def quad_grid():
    gmin, gmax, N, pd = UC.quad_limits()
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)


def info(ham):
    nd, npar, naux, built = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    axes = (C.c_int32 * 4)()
    rc = H.lib().hjh_ham_info(ham, C.byref(nd), C.byref(npar), C.byref(naux), axes, C.byref(built))
    return rc, (nd.value, npar.value, naux.value, tuple(axes), built.value)


# ------------------------------------------------------------------------------------------ 1. ids
def test_ids_identity_and_info():
    a, q = plane(), quad()
    assert a.ham_id >= H.HAM_USER_BASE and q.ham_id >= H.HAM_USER_BASE and a.ham_id != q.ham_id
    code = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hj_hidim.h")).read()
    assert "HJH_HAM_USER_BASE = %d" % H.HAM_USER_BASE in code
    # disjoint from the built-ins and from the range the solver's own registrations use
    assert H.HAM_USER_BASE > max(H.HAM_DIMS) and H.HAM_USER_BASE > _ffi.HAM_USER_BASE + 256
    assert plane().ham_id == a.ham_id and quad().ham_id == q.ham_id                       # the same text: the same id
    b = L.register_hidim_hamiltonian("plane5d_tables", 5, UC.PLANE_SRC + "\n", nparams=3, aux_axes=UC.PLANE_AXES)
    c = L.register_hidim_hamiltonian("plane5d_tables", 5, UC.PLANE_SRC, nparams=3, aux_axes=(2, 3))
    assert len({a.ham_id, b.ham_id, c.ham_id}) == 3                                       # changed text, changed axes: new ids
    assert info(a.ham_id)[0] == 0 and info(a.ham_id)[1][:4] == (5, 3, 2, (2, 2, -1, -1))
    assert info(q.ham_id)[0] == 0 and info(q.ham_id)[1][:4] == (6, 8, 2, (4, 4, -1, -1))
    assert info(c.ham_id)[1][4] == 0                                                      # never launched: no kernel built
    rc, _ = info(H.HAM_USER_BASE + 100000)
    assert rc == EINVAL and "unknown Hamiltonian id" in H.lib().hjh_last_error().decode()
    assert H.ham_dim(a.ham_id) == 5 and H.ham_dim(q.ham_id) == 6 and H.ham_dim(H.HAM_PLANE5D) == 5
    assert H.ham_dim(H.HAM_USER_BASE + 100000) is None and H.ham_dim(7) is None
    assert H.kernel_name("float64", q.ham_id, 1) == "hidim_substep_kernel<double, HamUser:planar_quad, 1>"
    assert (a.name, a.dim, a.nparams, a.aux_axes) == ("plane5d_tables", 5, 3, (2, 2))
    # register_native_hamiltonian keeps stopping at 4-D
    with pytest.raises(ValueError):
        L.register_native_hamiltonian("five", 5, "H = 0;", nparams=0)


# ------------------------------------------------------------------------------------------ 2. compile checks
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", ["ENO2", "ENO3", "WENO5_ASSHIPPED"])
def test_check_compiles_without_a_gpu(scheme, dtype):
    assert quad().check(scheme, dtype).ham_id == quad().ham_id


def test_the_generated_source_and_a_compile_error():
    q = quad()
    src = q.source()
    assert '#include "hj_hidim_dev.h"' in src and 'struct HamUser' in src and '#line 1 "planar_quad"' in src
    assert "c.aux[0] = P.aux[0][idx[4]];" in src and "c.aux[1] = P.aux[1][idx[4]];" in src
    assert src.count(UC.QUAD_SRC) == 2 and "#pragma clang fp contract(off)" in src        # the body under NP and without
    bad = L.register_hidim_hamiltonian("bad_quad", 6, "H = p[0];\nalpha[0] = T(1);\nalpha[1] = nosuch;\n", nparams=0)
    with pytest.raises(ValueError) as e:
        bad.check("ENO3", "float64")
    assert "bad_quad:3" in str(e.value) and "nosuch" in str(e.value) and "does not compile" in str(e.value)
    with pytest.raises(_ffi.Unsupported, match="scheme 2"):
        q.check("WENO5", "float64")
    # the library's own refusals
    lib, ham = H.lib(), C.c_int()
    inc = os.path.join(os.path.dirname(H.LIB_PATH)).encode()
    ax = (C.c_int32 * 4)(0, 0, 0, 9)
    for args, word in (((b"x", 4, 0, b"H = 0;", 0, ax, inc, None), "must be 5 or 6"), ((b"x", 5, 9, b"H = 0;", 0, ax, inc, None), "parameters"),
                       ((b"x", 5, 0, b"H = 0;", 5, ax, inc, None), "tables"), ((b"x", 5, 0, b"H = 0;", 4, ax, inc, None), "axis 9"),
                       ((b'x"y', 5, 0, b"H = 0;", 0, ax, inc, None), "quotes"), ((b"x", 5, 0, None, 0, ax, inc, None), "null argument")):
        rc = lib.hjh_ham_register(*(args + (C.byref(ham),)))
        assert rc != 0 and word in lib.hjh_last_error().decode(), (args, lib.hjh_last_error())
    assert lib.hjh_ham_source(q.ham_id, C.create_string_buffer(8), 8) == EINVAL and "buffer" in lib.hjh_last_error().decode()


# ------------------------------------------------------------------------------------------ 3. refusals at registration
def test_registration_refuses_by_name():
    ok = "H = p[0]; alpha[0] = alpha[1] = alpha[2] = alpha[3] = alpha[4] = T(1);"
    for dim in (4, 7, 3):
        with pytest.raises(ValueError, match="dim must be 5 or 6"):
            L.register_hidim_hamiltonian("x", dim, ok)
    with pytest.raises(ValueError, match="HJH_PAR_SLOTS"):
        L.register_hidim_hamiltonian("x", 5, ok, nparams=H.PAR_SLOTS + 1)
    with pytest.raises(ValueError, match="at most four tables"):
        L.register_hidim_hamiltonian("x", 5, ok, aux_axes=(0, 1, 2, 3, 4))
    for ax in (5, -1):
        with pytest.raises(ValueError, match="outside the grid"):
            L.register_hidim_hamiltonian("x", 5, ok, aux_axes=(2, ax))
    for name in ('a"b', "a'b"):
        with pytest.raises(ValueError, match="quotes"):
            L.register_hidim_hamiltonian(name, 5, ok)
    for word in ("dmin", "dmax"):
        with pytest.raises(ValueError, match="split path") as e:
            L.register_hidim_hamiltonian("x", 5, ok + " alpha[0] = %s[0];" % word)
        assert "costate range" in str(e.value)
    # a table whose length is not N[axis]: at __call__ and at attach
    g5 = lgrid("plane5d")
    reg = plane()
    good = UC.builtin_tables([np.asarray(v).ravel() for v in g5.vs])
    for tabs, word in (([good[0], good[1][:-1]], r"N\[2\] = 8"), ([good[0]], "reads 2 tables"), ([good[0], good[1].reshape(2, 4)], r"N\[2\] = 8")):
        with pytest.raises(ValueError, match=word):
            reg(g5, [0.8, 1.3, -1.0], tables=tabs)
        with pytest.raises(ValueError, match=word):
            reg.attach(L.Plane5D(g5), params=[0.8, 1.3, -1.0], tables=tabs)
    with pytest.raises(ValueError, match="takes 3 parameters"):
        reg(g5, [0.8, 1.3], tables=good)
    with pytest.raises(ValueError, match="5-dimensional"):
        reg(lgrid("pair6d"), [0.8, 1.3, -1.0], tables=good)


# ------------------------------------------------------------------------------------------ 4. the entry points refuse before any launch
def test_substep_with_a_user_id_refuses_before_any_launch():
    lib = H.lib()
    a, q = plane(), quad()
    par = H.params([1, 1, -1])
    before = lib.hjh_last_kernel()
    built = (info(a.ham_id)[1][4], info(q.ham_id)[1][4])

    def sub(g, tab, ham):
        return lib.hjh_substep(C.byref(g), C.byref(tab), _ffi.ENO2, ham, _ffi.STAGE_EULER, 0, par, FAKE, None, FAKE + 8, 0.01, 0, 0, None, 0, None, None)
    g5, g6 = grid(), grid((6, 5, 7, 5, 6, 8))
    sb = C.c_double()
    calls = [
        (lambda: sub(g5, tables(), H.HAM_USER_BASE + 100000), "unknown Hamiltonian id"),
        (lambda: sub(g6, tables(), a.ham_id), "lives on 5-D"),
        (lambda: sub(g5, tables(), q.ham_id), "lives on 6-D"),
        (lambda: sub(g5, tables(naux=1), a.ham_id), "aux table 1"),
        (lambda: sub(g6, tables(naux=0), q.ham_id), "aux table 0"),
        (lambda: sub(g5, tables(ncoord=4), a.ham_id), "coordinate table of axis 4"),
        (lambda: lib.hjh_step_bound(C.byref(g5), C.byref(tables(naux=1)), a.ham_id, par, FAKE, C.byref(sb), None, None), "aux table 1"),
        (lambda: lib.hjh_step_bound(C.byref(g5), C.byref(tables()), H.HAM_USER_BASE + 100000, par, FAKE, C.byref(sb), None, None), "unknown Hamiltonian id"),
        (lambda: lib.hjh_integrate(C.byref(g6), C.byref(tables(naux=1)), _ffi.ENO3, q.ham_id, 3, 0, 0, par, 0.1, FAKE, FAKE + 8, FAKE + 16, FAKE + 24,
                                   0, None, 0, None, 0.0, 1.0, 0.8, 1e300, 1e-4, None, None, None, None), "aux table 1"),
        (lambda: lib.hjh_integrate(C.byref(g5), C.byref(tables()), _ffi.ENO3, q.ham_id, 3, 0, 0, par, 0.1, FAKE, FAKE + 8, FAKE + 16, FAKE + 24,
                                   0, None, 0, None, 0.0, 1.0, 0.8, 1e300, 1e-4, None, None, None, None), "lives on 6-D"),
    ]
    for fn, word in calls:
        rc = fn()
        assert rc == EINVAL and word in lib.hjh_last_error().decode(), (rc, lib.hjh_last_error())
        assert lib.hjh_last_kernel() == before                      # nothing was launched: the record stays
    assert (info(a.ham_id)[1][4], info(q.ham_id)[1][4]) == built    # and nothing was built


# ------------------------------------------------------------------------------------------ 5. native_of
def test_native_of_recognises_attached_objects_by_identity():
    g5, g6 = lgrid("plane5d"), quad_grid()
    reg, q = plane(), quad()
    tabs = UC.builtin_tables([np.asarray(v).ravel() for v in g5.vs])
    s = reg(g5, [0.8, 1.3, -1.0], tables=tabs, hamiltonian=lambda self, t, d, p, sd=None: 0 * d)
    assert native_of(s.hamiltonian, s.dissipation) == (s, reg.ham_id, [0.8, 1.3, -1.0])
    s.params[0] = 0.9                                               # re-read at every call
    assert native_of(s.hamiltonian, s.dissipation)[2] == [0.9, 1.3, -1.0]
    assert all(np.array_equal(a, b) for a, b in zip(s._hj_native.tables, tabs))

    class Mine(object):
        def __init__(self, grid):
            self.grid, self.params = grid, list(UC.QUAD_PAR)

        def hamiltonian(self, t, data, p, sd=None):
            return UC.quad_ham(self, t, data, p, sd)

        def dissipation(self, t, data, lo, hi, sd, dim):
            return UC.quad_diss(self, t, data, lo, hi, sd, dim)

    class Overrides(Mine):
        def hamiltonian(self, t, data, p, sd=None):
            return 2 * Mine.hamiltonian(self, t, data, p, sd)

    class Renamed(Mine):
        pass

    qt = UC.quad_tables(g6.vs)
    m, o, r = (q.attach(k(g6), params=lambda v: v.params, tables=qt) for k in (Mine, Overrides, Renamed))
    assert native_of(m.hamiltonian, m.dissipation) == (m, q.ham_id, UC.QUAD_PAR)
    assert native_of(r.hamiltonian, r.dissipation)[1] == q.ham_id
    assert native_of(o.hamiltonian, o.dissipation)[1] == q.ham_id       # attached AS Overrides: its own methods are the registration's
    o2 = Overrides(g6)
    o2._hj_native = m._hj_native                                        # ... but a subclass riding on the parent's attachment is not native
    assert native_of(o2.hamiltonian, o2.dissipation) is None
    assert native_of(m.hamiltonian, r.dissipation) is None

    class Doubled(L.HidimSystem):                                       # a subclass of the registration's own system class that overrides a method
        def hamiltonian(self, t, data, p, sd=None):
            return 2 * L.HidimSystem.hamiltonian(self, t, data, p, sd)

    d = Doubled(q, g6, UC.QUAD_PAR, qt, UC.quad_ham, UC.quad_diss)
    assert native_of(d.hamiltonian, d.dissipation) is None
    assert native_of(lambda *a: 0, m.dissipation) is None
    # the rollout kernel has no plant for a registered system: computeOptTrajs keeps its host loop
    assert native_plant_hi(m) is None and native_plant_hi(s) is None
    with pytest.raises(ValueError, match="6-dimensional"):
        q.attach(Mine(g5), params=UC.QUAD_PAR, tables=qt)
    with pytest.raises(ValueError, match="grid"):
        q.attach(object.__new__(Overrides), params=UC.QUAD_PAR, tables=qt)


# ------------------------------------------------------------------------------------------ 6. explain_plan
def test_explain_plan_names_the_registration():
    g6 = quad_grid()
    q = quad()
    s = q(g6, UC.QUAD_PAR, tables=UC.quad_tables(g6.vs), hamiltonian=UC.quad_ham, dissipation=UC.quad_diss)
    sd = L.Bundle(dict(grid=g6, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
    assert L.explain_plan(sd) == dict(path='registered', ham_id=q.ham_id, params=UC.QUAD_PAR, library='libhj_hidim.so')
    # the two existing answers stay word for word
    b = L.DubinsPair6D(g6)
    sdb = L.Bundle(dict(grid=g6, hamFunc=b.hamiltonian, partialFunc=b.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
    assert L.explain_plan(sdb) == dict(path='built-in', ham_id=H.HAM_DUBINS_PAIR6D, params=[5.0, 5.0, 5.0, 5.0], library='libhj_hidim.so')
    plain = L.Bundle(dict(grid=g6, hamFunc=lambda *a: s.hamiltonian(*a), partialFunc=lambda *a: s.dissipation(*a),
                          dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
    e = L.explain_plan(plain)
    assert e == dict(path='split', reason='on a grid of 6 dimensions only Plane5D / DubinsPair6D with artificialDissipationGLF run fused; the '
                                          'tracer stops at 4-D', library='libhj_hidim.so')
    # a local dissipation, or a system on another grid, is not fused
    sdl = L.Bundle(dict(grid=g6, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationLLF, derivFunc=L.upwindFirstENO2))
    assert L.explain_plan(sdl)['path'] == 'split'
    sdo = L.Bundle(dict(grid=quad_grid(), hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
    assert L.explain_plan(sdo)['path'] == 'split'


# ------------------------------------------------------------------------------------------ 7. resources
_reports = {}


@pytest.mark.parametrize("which", [0, 1, 2], ids=["plane5d_tables", "pair6d_tables", "planar_quad"])
def test_no_scratch_in_the_registered_kernels(which):
    """The offline compile of hjh_ham_source (tools/hidim_user_resources.py): the substep kernels of both types and the three schemes and
    the two bound kernels of each system keep every per-cell value in registers -- no scratch, no LDS beyond the bound kernel's reduction."""
    reg = UR.test_registrations()[which]
    rows = UR.report(reg)
    assert len(rows) == 8
    for r in rows:
        print("%s %s: %d VGPRs, %d B/lane scratch, %d waves/SIMD" % (reg.name, r["kernel"], r["vgprs"], r["scratch"], r["occupancy"]))
    for r in rows:
        assert r["scratch"] == 0 and r["vgprs"] > 0, (reg.name, r)
