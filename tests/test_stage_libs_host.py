"""CPU-only: the refusals of the three libraries that integrate with one launch per RK stage -- libhj_batch.so, libhj_stoch.so and
libhj_hidim.so -- from ONE table, in the manner of tests/test_hidim_host.py.  Every data pointer is a fake or null and every check
comes before the first HIP call, so no device is touched.

  * every (library, entry point) a case applies to gives the return code and the WHOLE error text stated here, and leaves
    <prefix>_last_kernel() as it was.  The batch library is called with two problems, the second one the bad one: its
    per-problem refusals read "problem 1: ..."
  * an interval that needs no step: HJ_OK, t0, no step, the result in y_in -- per library and order
"""
import ctypes as C

import pytest

from levelsetpy_amd import _bffi, _ffi, _hffi, _qffi, _wffi

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
INF = float("inf")
SUBSTEP, INTEGRATE, BOUND, PLAN = "substep", "integrate", "step_bound", "plan"
LIBS = ("batch", "stoch", "hidim")
PREFIX = {"batch": "hjb", "stoch": "hjw", "hidim": "hjh"}
MODULE = {"batch": _bffi, "stoch": _wffi, "hidim": _hffi}
ENTRY_POINTS = {"batch": (SUBSTEP, INTEGRATE, BOUND, PLAN), "stoch": (SUBSTEP, INTEGRATE, BOUND, PLAN), "hidim": (SUBSTEP, INTEGRATE, BOUND)}
# the batch and stoch libraries run the relative Dubins system (3-D, aux tables 0 and 1), the 5-D / 6-D one the plane (aux 0 and 1)
HAM = {"batch": _ffi.HAM_DUBINS_REL, "stoch": _ffi.HAM_DUBINS_REL, "hidim": _hffi.HAM_PLANE5D}
SHAPE = {"batch": (7, 6, 8), "stoch": (7, 6, 8), "hidim": (7, 6, 8, 5, 9)}


def grid(lib, dtype=0, **put):
    """The library's descriptor; `put` overwrites (field, axis) entries: N=(2, 2) is N[2] = 2."""
    N = SHAPE[lib]
    nd = len(N)
    g = (_hffi if lib == "hidim" else _qffi).grid_descriptor(nd, list(N), [0.0] * nd, [0.1 * (n - 1) for n in N], [0.1] * nd, [0] * nd, [0] * nd,
                                                             "float64")
    g.dtype = dtype
    for field, (axis, value) in put.items():
        getattr(g, field)[axis] = value
    return g


def tables(lib, ncoord=6, naux=4):
    t = (_hffi if lib == "hidim" else _bffi).Tables()
    for d in range(min(ncoord, len(t.coord))):
        t.coord[d] = FAKE
    for s in range(naux):
        t.aux[s] = FAKE
    return t


def call(lib, entry, g="fake", tab="fake", scheme=_ffi.ENO2, stage=_ffi.STAGE_EULER, order=3, post_prev=0, op_a=0, post_a=None, op_b=0,
         post_b=None, y_in=FAKE, buf_a=FAKE + 8, buf_b=FAKE + 16, work=FAKE + 24, sb=0.05, sigma=None, form=_wffi.FORM_AUTO,
         t0=0.0, tf=1.0, out=None):
    """One call of `entry` of `lib`; what the keywords do not name is valid.  -> the return code."""
    L = MODULE[lib].lib()
    g = grid(lib) if g == "fake" else g
    tab = tables(lib) if tab == "fake" else tab
    pg, pt = (None if g is None else C.byref(g)), (None if tab is None else C.byref(tab))
    ham, nd = HAM[lib], len(SHAPE[lib])
    par = (C.c_double * 16)(*([1.0] * 16))
    sig = (C.c_double * (nd * nd))(*(sigma if sigma is not None else [0.1 if i % (nd + 1) == 0 else 0.0 for i in range(nd * nd)]))
    tout, nout, where = (C.c_double * 2)(-1, -1), (C.c_int64 * 2)(-1, -1), (C.c_int32 * 2)(-1, -1)
    if out is not None:
        out.extend([tout, nout, where])
    tail = (0.8, 1e300, 1e-4)                             # factor_cfl, max_step, stop_tol
    if lib == "batch":
        # two problems: the first one valid, the second one as the keywords say
        probs = (_bffi.Problem * 2)(_bffi.Problem(y_in=FAKE, buf_a=FAKE + 8, buf_b=FAKE + 16, work=FAKE + 24),
                                    _bffi.Problem(y_in=y_in, buf_a=buf_a, buf_b=buf_b, work=work, post_a=post_a, post_b=post_b, op_a=op_a, op_b=op_b))
        sbs = (C.c_double * 2)(0.05, sb)
        if entry == SUBSTEP:
            return L.hjb_substep(pg, pt, scheme, ham, stage, 0, C.addressof(par), FAKE, 2, None)
        if entry == BOUND:
            return L.hjb_step_bounds(pg, pt, ham, C.addressof(par), 2, None, sbs, None, None)
        if entry == PLAN:
            return L.hjb_plan(order, sbs, 2, t0, tf, *tail, tout, nout)
        return L.hjb_integrate(pg, pt, scheme, ham, order, 0, post_prev, C.addressof(par), sbs, probs, 2, t0, tf, *tail, None, 0, tout, nout, where, None)
    if lib == "stoch":
        if entry == SUBSTEP:
            e = _wffi.Entry(src=y_in, y0=None, dst=buf_a, post_a=post_a, post_b=post_b, dt=0.01, post_prev=post_prev, op_a=op_a, op_b=op_b)
            return L.hjw_substep(pg, pt, scheme, ham, stage, 0, par, sig, form, C.byref(e), None)
        if entry == BOUND:
            return L.hjw_step_bound(pg, pt, ham, par, sig, None, tout, None)
        if entry == PLAN:
            return L.hjw_plan(order, sb, t0, tf, *tail, tout, nout)
        p = _bffi.Problem(y_in=y_in, buf_a=buf_a, buf_b=buf_b, work=work, post_a=post_a, post_b=post_b, op_a=op_a, op_b=op_b)
        return L.hjw_integrate(pg, pt, scheme, ham, order, 0, post_prev, par, sig, form, sb, C.byref(p), t0, tf, *tail, tout, nout, where, None)
    if entry == SUBSTEP:
        return L.hjh_substep(pg, pt, scheme, ham, stage, 0, par, y_in, None, buf_a, 0.01, post_prev, op_a, post_a, op_b, post_b, None)
    if entry == BOUND:
        return L.hjh_step_bound(pg, pt, ham, par, None, tout, None, None)
    return L.hjh_integrate(pg, pt, scheme, ham, order, 0, post_prev, par, sb, y_in, buf_a, buf_b, work, op_a, post_a, op_b, post_b, t0, tf, *tail,
                           tout, nout, where, None)


# ------------------------------------------------------------------------------------------ the table
SETUP = (SUBSTEP, INTEGRATE, BOUND)                        # the entry points that take (grid, tables, system)
STAGED = (SUBSTEP, INTEGRATE)
NO_SCHEME = "scheme %d has no %s kernel (ENO2, ENO3, as-shipped WENO5 only)"
KIND = {"batch": "batched", "stoch": "stochastic", "hidim": "5-D / 6-D substep"}
# hjb_substep takes its stages' operators from a device table, which the host never reads
OPS = ((SUBSTEP, ("stoch", "hidim")), (INTEGRATE, LIBS))

# (id, keywords of call() -- a function of the library where the descriptor is one --, the entry points, the return code, the whole
# text: one string, or one per library; {p} is "problem 1: " where hjb_integrate speaks of a problem)
CASES = [
    ("null-grid", lambda lib: dict(g=None), SETUP, EINVAL,
     {"batch": "null grid descriptor or tables", "stoch": "null grid descriptor or tables", "hidim": "null grid descriptor"}),
    ("null-tables", lambda lib: dict(tab=None), SETUP, EINVAL,
     {"batch": "null grid descriptor or tables", "stoch": "null grid descriptor or tables", "hidim": "null tables"}),
    ("dtype7", lambda lib: dict(g=grid(lib, dtype=7)), SETUP, EINVAL, "unknown dtype 7"),
    ("small-N", lambda lib: dict(g=grid(lib, N=(2, 2))), SETUP, EINVAL, "N[2] = 2 out of range (need 3 .. 2^30)"),
    ("bc9", lambda lib: dict(g=grid(lib, bc=(1, 9))), SETUP, EINVAL, "unknown boundary kind 9 on axis 1"),
    ("dx0", lambda lib: dict(g=grid(lib, dx=(0, 0.0))), SETUP, EINVAL, "axis 0: dx must be positive and finite"),
    ("dx-negative", lambda lib: dict(g=grid(lib, dx=(2, -0.1))), SETUP, EINVAL, "axis 2: dx must be positive and finite"),
    ("null-coord", lambda lib: dict(tab=tables(lib, ncoord=2)), SETUP, EINVAL, "null coordinate table of axis 2"),
    ("null-aux", lambda lib: dict(tab=tables(lib, naux=1)), SETUP, EINVAL,
     {lib: "Hamiltonian %d reads aux table 1, which is null" % HAM[lib] for lib in LIBS}),
    ("scheme2", dict(scheme=2), STAGED, EUNSUPPORTED,
     {"batch": NO_SCHEME % (2, KIND["batch"]), "hidim": NO_SCHEME % (2, KIND["hidim"]),
      "stoch": "the intended WENO5 (HJ_WENO5) has no stochastic kernel: its epsilon is a reduction over the grid"}),
    ("scheme4", dict(scheme=4), STAGED, EUNSUPPORTED, {lib: NO_SCHEME % (4, KIND[lib]) for lib in LIBS}),
    ("stage5", dict(stage=5), (SUBSTEP,), EINVAL, "unknown stage 5"),
    ("order4", dict(order=4), (INTEGRATE, PLAN), EINVAL, "order must be 1, 2 or 3"),
    ("order0", dict(order=0), (INTEGRATE, PLAN), EINVAL, "order must be 1, 2 or 3"),
    ("post-prev3", dict(post_prev=3), OPS, EINVAL, "unknown post-step operator 3"),
    ("array-op4", dict(op_a=4, post_a=FAKE + 32), OPS, EINVAL, "{p}unknown array operator"),
    ("array-op-negative", dict(op_b=-1, post_b=FAKE + 32), OPS, EINVAL, "{p}unknown array operator"),
    ("op-without-array", dict(op_b=3), OPS, EINVAL, "{p}an array operator without its array"),
    ("null-buffer", dict(buf_b=None), (INTEGRATE,), EINVAL, "{p}null buffer"),
    ("null-y-in", dict(y_in=None), (INTEGRATE,), EINVAL, "{p}null buffer"),
    ("no-work-order2", dict(order=2, work=None), (INTEGRATE,), EINVAL, "{p}work buffer required for order >= 2"),
    ("equal-buffers", dict(buf_b=FAKE + 8), (INTEGRATE,), EINVAL, "{p}buffers must be distinct"),
    ("work-is-y-in", dict(work=FAKE), (INTEGRATE,), EINVAL, "{p}buffers must be distinct"),
    ("step-bound0", dict(sb=0.0), (INTEGRATE, PLAN), EINVAL,
     {"batch": "problem 1: the step bound must be positive (got 0)", "stoch": "problem 0: the step bound must be positive (got 0)",
      "hidim": "problem 0: the step bound must be positive (got 0)"}),
    # the substep's own arrays: each library words these its own way
    ("null-src", dict(y_in=None), ((SUBSTEP, ("stoch", "hidim")),), EINVAL, {"stoch": "null src or dst", "hidim": "null argument"}),
    ("dst-is-src", dict(buf_a=FAKE), ((SUBSTEP, ("stoch", "hidim")),), EINVAL,
     {"stoch": "dst must not alias an array the stage reads", "hidim": "dst must not alias src"}),
    ("y0-missing", dict(stage=_ffi.STAGE_RK3_FULL), ((SUBSTEP, ("stoch", "hidim")),), EINVAL, "stage 3 reads y0, which is null"),
    ("dst-is-post-array", dict(op_a=1, post_a=FAKE + 8), ((SUBSTEP, ("stoch",)),), EINVAL, "dst must not alias an array the stage reads"),
    ("buffer-is-post-array", dict(op_b=2, post_b=FAKE + 24), ((INTEGRATE, ("stoch",)),), EINVAL,
     "a buffer the interval writes aliases a post-step array"),
    # sigma
    ("sigma-inf", dict(sigma=[0.1, INF] + [0.0] * 7), ((SUBSTEP, ("stoch",)), (INTEGRATE, ("stoch",)), (BOUND, ("stoch",))), EINVAL,
     "sigma[0][1] is not finite"),
    ("sigma-nan", dict(sigma=[0.1] * 5 + [float("nan")] + [0.0] * 3), ((SUBSTEP, ("stoch",)), (INTEGRATE, ("stoch",)), (BOUND, ("stoch",))), EINVAL,
     "sigma[1][2] is not finite"),
    ("diagonal-form-off-diagonal", dict(sigma=[0.1, 0.0, 0.0, 0.2] + [0.0] * 5, form=_wffi.FORM_DIAGONAL),
     ((SUBSTEP, ("stoch",)), (INTEGRATE, ("stoch",))), EINVAL, "HJW_FORM_DIAGONAL with a sigma that has a non-zero off-diagonal entry"),
]


def expand():
    out = []
    for cid, kw, where, rc, text in CASES:
        for w in where:
            entry, libs = (w, LIBS) if isinstance(w, str) else w
            for lib in libs:
                if entry in ENTRY_POINTS[lib]:
                    t = text if isinstance(text, str) else text[lib]
                    out.append(pytest.param(lib, entry, kw, rc, t.replace("{p}", "problem 1: " if (lib, entry) == ("batch", INTEGRATE) else ""),
                                            id="%s-%s-%s" % (lib, entry, cid)))
    return out


@pytest.mark.parametrize("lib,entry,kw,rc,text", expand())
def test_refusal(lib, entry, kw, rc, text):
    L, pre = MODULE[lib].lib(), PREFIX[lib]
    last_kernel, last_error = getattr(L, pre + "_last_kernel"), getattr(L, pre + "_last_error")
    before = last_kernel()
    got = call(lib, entry, **(kw(lib) if callable(kw) else kw))
    assert (got, last_error().decode()) == (rc, text)
    assert last_kernel() == before                          # nothing was launched: the record stays


def test_the_table_covers_every_entry_point():
    seen = {(p.values[0], p.values[1]) for p in expand()}
    assert seen == {(lib, e) for lib in LIBS for e in ENTRY_POINTS[lib]}
    for lib in LIBS:
        for e in ENTRY_POINTS[lib]:
            name = "%s_%s" % (PREFIX[lib], "step_bounds" if (lib, e) == ("batch", BOUND) else e)
            assert name in MODULE[lib].SIGNATURES, name


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("lib", LIBS)
def test_an_interval_without_a_step(lib, order):
    """tf - t0 below stop_tol: HJ_OK, the time is t0, no step, and the result is where it was (result_in 0 = y_in)."""
    out = []
    rc = call(lib, INTEGRATE, order=order, t0=0.5, tf=0.5 + 5e-5, out=out)
    assert rc == OK, getattr(MODULE[lib].lib(), PREFIX[lib] + "_last_error")()
    tout, nout, where = out
    n = 2 if lib == "batch" else 1
    assert (list(tout)[:n], list(nout)[:n], list(where)[:n]) == ([0.5] * n, [0] * n, [0] * n)
