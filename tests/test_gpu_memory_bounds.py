"""Guarded-buffer tests over the C ABI: no kernel reads or writes outside the arrays it is given.

Every row calls an entry point of include/hj_mi355x.h through ctypes on arrays carved from tests/guarded_pool.py's pool
(the test owns every pointer) and follows guarded_pool.run_case: one reference run on fresh unguarded torch.zeros outputs, then
guarded runs at element offsets 0, 1, 2, 3 from a 512-byte boundary, each with input guards of NaN, +1e30 and -1e30.  Every
guarded run must pass GuardedPool.check (guards intact, inputs unchanged, every cell of the updated region written, nothing
outside it touched) and give arrays AND host scalars bit for bit equal to the reference run; where the entry point reports its
kernel (hj_last_kernel), the name must be the one the row claims.  Equality is exact: the per-cell arithmetic does not depend
on the data path and the reductions are max / min reductions.

Alignment.  Read from the code before the first run: every tiled kernel addresses memory through raw buffer descriptors whose
base is `array + plane offset` (hj_device.h make_srd) and per-lane BYTE offsets; the 8- and 16-byte buffer accesses of
hj_fusedv.h / hj_fused4v.h / hj_flat4v.h already start wherever a row starts (odd row lengths put rows on odd cells), which
gfx950 serves at element alignment; the direct, term, curvature and elementwise kernels use element-sized global accesses.
So element alignment is the library's contract, and the offset rows assert the same bits at offsets 1-3.  The only argument
with a stronger requirement is the 64-bit key array of hj_range_pass / hj_ctx_set_range_source (8 bytes: 64-bit atomics),
which is not an array of the ctx dtype; its rows run on the fp64 pool.

Kernel -> rows (the names are the kernels' as hj_last_kernel / a kernel trace report them)
  fused_substep_kernel      test_substep_rows[scalar-*], test_substep_rows_2d_4d[scalar2*-*, scalar4*-*, and flat4 / pair4 / pair4d
                            with ENO3 / WENO5], test_lf_term_rows[scalar-*], test_lf_term_rows_2d_4d, test_rk_step_rows[scalar-*],
                            test_rk_integrate_rows[*-scalar-*], test_term_rows[tiled-*], test_slab_mode_rows[scalar-*]
  fused_pair_kernel         test_substep_rows[pair_ring-*, pair_noring-*], test_substep_rows_2d_4d[pair2*-*, pair4d-*, pair4-1-*],
                            test_substep_rows_fast_eno, test_lf_term_rows[pair_ring-*, pair_noring-*], test_rk_step_rows[pair-*,
                            fuse12-* order 3], test_rk_integrate_rows[*-pair-*], test_large_grid_rows, test_slab_mode_rows[pair_ring-*],
                            test_deep_slab_step_rows, test_slab_rk_step_self_ring_rows (edge ranges [0, 3) + [n - 3, n) and interior)
  fused_pair_kernel (march along axis 1)   test_substep_rows[xp-*], test_lf_term_rows[xp-*]
  fused_pair4_kernel        test_substep_rows_2d_4d[pair4-0-*, pair4-2-*], test_lf_term_rows_2d_4d[pair4-*]
  fused_flat4_kernel        test_substep_rows_2d_4d[flat4-*], test_lf_term_rows_2d_4d[flat4-*]
  direct_substep_kernel     test_substep_rows[direct-*, direct_small-*], test_substep_rows_2d_4d[direct2-*, direct4*-*],
                            test_lf_term_rows[direct-*, direct_small-*], test_rk_step_rows[direct-*, coop-* order 1]
  coop_rk_kernel            test_rk_step_rows[coop-*] orders 2 and 3
  fused12_kernel / fused12_pair_kernel     test_stage12_rows, test_rk_step_rows[fuse12-*]
  max_d1sq_kernel, partials_to_values_kernel, keys_to_values_kernel, eps_seam_kernel   every WENO5 row above; test_max_d1sq_rows;
                            test_rk_step_rows[*-WENO5-*] with HJ_EPS_FUSE=1 (the epsilon producer and its seam kernel)
  bound_to_dt_kernel        left out: one thread, launched only by hj_rk_step with a range-reading Hamiltonian under the local
                            Lax-Friedrichs kinds; it reads and writes the context's own words and takes no caller array
  minmax_kernel             test_minmax_any_nan_rows, test_rk_step_rows (post arrays)
  any_nan_kernel            test_minmax_any_nan_rows
  ghost_kernel              test_ghost_rows
  upwind_kernel             test_upwind_rows
  upwind_all_kernel, lf_split_end_kernel   test_lf_split_rows
  rk_combine_kernel         test_rk_combine_rows
  term_kernel               test_term_rows[direct-*]
  curv_kernel               test_curvature_rows, test_trace_hessian_rows
  run-time (hipRTC) kernels "fused_pair_kernel (hipRTC)" (the 4-D one-cell-per-lane shape is left out), the range pass and
  alpha_bound_kernel        test_runtime_hamiltonian_rows (a Hamiltonian registered by hand; hj_static_step_bound; hj_range_pass with
                            its key array guarded, hj_bound_pass); test_python_level_views (a traced callback pair)
Left out, with the reason: the multi-rank forms of the slab steppers (one pool per rank; their kernels are those of the one-rank
rows: test_slab_rk_step_self_ring_rows drives hj_halo_exchange and hj_slab_rk_step as a one-rank RCCL ring, test_deep_slab_step_rows
the deep stepper as one rank of an external two-rank world).  1-D arrays reach the curvature rows only: every other entry point
refuses a 1-D context (include/hj_mi355x.h, hj_ctx_create).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi  # noqa: E402
from levelsetpy_amd.context import DeviceGrid  # noqa: E402

from guarded_pool import GuardedPool, run_case  # noqa: E402

XP_NAME = "fused_pair_kernel (march along axis 1)"
KNOBS = ("HJ_XP", "HJ_XP_TRIALS", "HJ_PAIR", "HJ_PAIR_RING", "HJ_FORCE_DIRECT", "HJ_MIN_CHUNK", "HJ_PAIR4", "HJ_FLAT4", "HJ_EPS_FUSE",
         "HJ_EPS_FUSE_MIN_CELLS", "HJ_FUSE12", "HJ_F12_PAIR", "HJ_COOP", "HJ_TERM_TILED_FROM", "HJ_FULL_ROWS", "HJ_KEEP_BOUNDS", "HJ_NT", "HJ_R")
TD = {"float64": torch.float64, "float32": torch.float32}
POOL_ELEMS = 44 * 1000 * 1000           # 201^3 = 8.1 M cells: four arrays of a step and their guards
_POOLS = {}


def pool(dtype):
    """One allocation per dtype for the whole module."""
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", POOL_ELEMS)
    return _POOLS[dtype]


# ------------------------------------------------------------------------------ grids, data, contexts
def grid(shape, periodic=(), tz=()):
    nd = len(shape)
    if nd == 3:
        lo, hi = [-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / shape[2])]
    elif nd == 4:
        lo = [-np.pi, -8., -np.pi, -8.]
        hi = [np.pi * (1 - 2 / shape[0]), 8 * (1 - 2 / shape[1]), np.pi * (1 - 2 / shape[2]), 8 * (1 - 2 / shape[3])]
    else:
        lo, hi = [-1.0 - 0.1 * d for d in range(nd)], [1.0 + 0.05 * d for d in range(nd)]
    g = L.createGrid(np.array(lo).reshape(-1, 1), np.array(hi).reshape(-1, 1), np.array(shape, dtype=np.int64).reshape(-1, 1),
                     list(periodic) if periodic else None, low_mem=bool(np.prod(shape) > 1e6))
    if tz:
        g.bdryData = [L.Bundle(dict(towardZero=True)) if d in tz else None for d in range(nd)]
    return g


def field(g, dtype, seed=0, noise=0.02):
    """A distance-like function bent by a wave plus noise, so that no two stencil values tie; built on the device."""
    vs = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
    nd = len(vs)
    xs = [v.reshape([-1 if k == d else 1 for k in range(nd)]) for d, v in enumerate(vs)]
    r2 = sum((xs[d] - 0.1) ** 2 for d in range(min(2, nd)))
    out = r2.sqrt() - 0.5 + 0.1 * torch.sin(3 * xs[-1] + 0.3) * torch.cos(2 * xs[0])
    out = out.expand([v.numel() for v in vs]).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = out + noise * torch.randn(out.shape, generator=gen, device="cuda", dtype=torch.float64)
    return out.to(TD[dtype]).contiguous()


def ctx(g, monkeypatch, dtype="float64", slab=None, pad=0, **env):
    """A fresh context: the knobs are read in hj_ctx_create."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HJ_DIRECT_BELOW", "0")
    monkeypatch.setenv("HJ_XP", "0")
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    dg = DeviceGrid(g, dtype, None, slab, pad) if slab is not None else DeviceGrid(g, dtype)
    dg.bind_stream()
    return dg


def kernel_name(dg):
    return (dg.lib.hj_last_kernel(dg.ctx) or b"").decode()


def ham_for(nd):
    return {2: (_ffi.HAM_DOUBLE_INTEGRATOR, [1., 0., 0., 0.]), 3: (_ffi.HAM_DUBINS_REL, [1., 1., 1., 2.]),
            4: (_ffi.HAM_DOUBLE_PENDULUM, [1., 0., 0., 0.])}[nd]


def run(op, dtype, what, depth=1):
    return run_case(op, pool(dtype), depth=depth, what=what)


def null_or(a):
    return a.ptr if a is not None else None


# ------------------------------------------------------------------------------ hj_rk_substep / hj_lf_term
KERNELS3 = {
    "scalar": (dict(HJ_PAIR="0"), ("fused_substep_kernel",)),
    "pair_ring": (dict(HJ_PAIR="2", HJ_PAIR_RING="1"), ("fused_pair_kernel",)),
    "pair_noring": (dict(HJ_PAIR="2", HJ_PAIR_RING="0"), ("fused_pair_kernel",)),
    "direct": (dict(HJ_FORCE_DIRECT="1"), ("direct_substep_kernel",)),
    "direct_small": (dict(HJ_DIRECT_BELOW=None), ("direct_substep_kernel",)),
    "xp": (dict(HJ_XP="2", HJ_PAIR="2", HJ_MIN_CHUNK="4"), (XP_NAME,)),
}
# (shape, periodic axes, towardZero axes): odd extents, partial tiles on every side; periodic and extrapolated variants
GRIDS3 = [((23, 14, 12), (2,), ()), ((24, 31, 40), (0, 2), ()), ((12, 50, 40), (), (1,)),
          ((23, 14, 12), (), (0, 2)), ((24, 31, 40), (), (1,)), ((12, 50, 40), (0, 1, 2), ())]
GRIDS2 = [((37, 41), (), (0,)), ((37, 41), (0, 1), ())]
STAGES = [("YDOT", _ffi.STAGE_YDOT, False), ("EULER", _ffi.STAGE_EULER, False), ("RK3_HALF", _ffi.STAGE_RK3_HALF, True),
          ("RK3_FULL", _ffi.STAGE_RK3_FULL, True), ("RK2_FULL", _ffi.STAGE_RK2_FULL, True)]
SCHEMES = ["ENO2", "ENO3", "WENO5_ASSHIPPED", "WENO5"]


def substep_op(dg, sid, stage, need_y0, data, data0, p0, p1, rs=0, eps_source=False, names=None, ring=None):
    ham, par = ham_for(dg.dim)
    par = _ffi.darr(par)
    lib = dg.lib

    def op(A):
        y = A.inp("y", data)
        y0 = A.inp("y0", data0) if need_y0 else None          # null for the YDOT and EULER stages
        out = A.out("out", data.shape, written=(p0, p1))
        eps = A.out("eps", (dg.dim,)) if eps_source else None
        A.arm()
        if eps_source:      # the intended WENO5 as the slab steppers run it: epsilon from a caller-reduced vector
            _ffi.check(lib.hj_max_d1sq(dg.ctx, y.ptr, eps.ptr))
            _ffi.check(lib.hj_ctx_set_weno_eps_source(dg.ctx, eps.ptr))
        try:
            _ffi.check(lib.hj_rk_substep(dg.ctx, sid, ham, par, 0.25, stage, 2e-3, rs, y.ptr, null_or(y0), out.ptr, 5, p0, p1))
            sb, am = C.c_double(), (C.c_double * 4)()
            _ffi.check(lib.hj_read_step_bound(dg.ctx, 5, C.byref(sb), am))
        finally:
            _ffi.check(lib.hj_ctx_set_weno_eps_source(dg.ctx, None))
        name = kernel_name(dg)
        if names is not None:
            assert name in names, (name, names)
        res = {"step_bound": sb.value, "alpha_max": tuple(am[:dg.dim]), "kernel": name}
        if ring is not None:
            nbuf, ahead = C.c_int(), C.c_int()
            _ffi.check(lib.hj_last_launch(dg.ctx, C.byref(nbuf), C.byref(ahead)))
            assert (ahead.value > 0) == ring, (nbuf.value, ahead.value)
        return res
    return op


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("gi", range(len(GRIDS3)))
@pytest.mark.parametrize("kernel", sorted(KERNELS3))
def test_substep_rows(kernel, gi, scheme, dtype, monkeypatch):
    """hj_rk_substep on the 3-D kernels: every stage kind over the whole grid (y0 null for YDOT / EULER), a proper sub-range
    [p0, p1) for EULER and RK3_FULL, and the clamp of termRestrictUpdate once per row."""
    shape, periodic, tz = GRIDS3[gi]
    env, names = KERNELS3[kernel]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype, **env)
    data, data0 = field(g, dtype, 1), field(g, dtype, 2)
    sid = _ffi.SCHEME_IDS[scheme]
    n0 = shape[0]
    xp = kernel == "xp"
    eps_source = xp and scheme == "WENO5"          # the transposed march takes the intended WENO5 with a caller-reduced epsilon
    ring = {"pair_ring": True, "pair_noring": False}.get(kernel)
    for sname, stage, need_y0 in STAGES:
        run(substep_op(dg, sid, stage, need_y0, data, data0, 0, n0, eps_source=eps_source, names=names, ring=ring), dtype,
            "hj_rk_substep %s %s %s %s %s whole" % (kernel, shape, scheme, dtype, sname))
        if sname in ("EULER", "RK3_FULL"):
            # (a window under HJ_XP=2 takes the transposed form where the call has one, else the axis-0 pair kernel)
            run(substep_op(dg, sid, stage, need_y0, data, data0, 4, n0 - 5, rs=(1 if sname == "EULER" else -1), eps_source=eps_source,
                           names=names + ("fused_pair_kernel",) if xp else names), dtype,
                "hj_rk_substep %s %s %s %s %s planes [4, %d) clamp" % (kernel, shape, scheme, dtype, sname, n0 - 5))


KERNELS24 = {
    # 2-D (double integrator)
    "scalar2": (2, "float64", dict(HJ_PAIR="0"), ("fused_substep_kernel",)),
    "pair2": (2, "float64", dict(HJ_PAIR="2"), ("fused_pair_kernel",)),
    "direct2": (2, "float64", dict(HJ_FORCE_DIRECT="1"), ("direct_substep_kernel",)),
    "scalar2f": (2, "float32", dict(HJ_PAIR="0"), ("fused_substep_kernel",)),
    "pair2f": (2, "float32", dict(HJ_PAIR="2"), ("fused_pair_kernel",)),
    # 4-D (double pendulum): fp32 light stencils have three tiled kernels of their own
    "flat4": (4, "float32", dict(HJ_PAIR="2", HJ_PAIR4="0", HJ_FLAT4="2"), ("fused_flat4_kernel",)),
    "pair4": (4, "float32", dict(HJ_PAIR="2", HJ_PAIR4="1", HJ_FLAT4="0"), None),     # names per grid below
    "pair4d": (4, "float32", dict(HJ_PAIR="2", HJ_PAIR4="0", HJ_FLAT4="0"), ("fused_pair_kernel",)),
    "scalar4": (4, "float32", dict(HJ_PAIR="0"), ("fused_substep_kernel",)),
    "direct4": (4, "float32", dict(HJ_FORCE_DIRECT="1"), ("direct_substep_kernel",)),
    "scalar4d": (4, "float64", dict(HJ_PAIR="2"), ("fused_substep_kernel",)),       # fp64 4-D has no pair kernel
    "direct4d": (4, "float64", dict(HJ_FORCE_DIRECT="1"), ("direct_substep_kernel",)),
}
GRIDS4 = [((8, 7, 9, 41), (0, 1, 2, 3), ()), ((7, 11, 6, 37), (0, 2), ()), ((6, 12, 8, 129), (1, 3), (0,))]
# the compile-time tiles of hj_fused4v.h need 34 or 66 cells of the contiguous axis placed so that no tile begins or ends 1 or 3
# cells from a row end (hj_inst.hip tile4_fits): 37 = 34 + 3 does not fit and runs the generic pair kernel
PAIR4_NAMES = {0: ("fused_pair4_kernel",), 1: ("fused_pair_kernel",), 2: ("fused_pair4_kernel",)}


ROWS24 = [(k, gi) for k in sorted(KERNELS24) for gi in range(len(GRIDS2) if KERNELS24[k][0] == 2 else len(GRIDS4))]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kernel,gi", ROWS24)
def test_substep_rows_2d_4d(kernel, gi, scheme, monkeypatch):
    nd, dtype, env, names = KERNELS24[kernel]
    shape, periodic, tz = (GRIDS2 if nd == 2 else GRIDS4)[gi]
    light = scheme in ("ENO2", "WENO5_ASSHIPPED")
    if kernel in ("flat4", "pair4", "pair4d") and not light:
        names = ("fused_substep_kernel",)       # ENO3 / WENO5 in 4-D: the one-cell-per-lane kernel whatever the knobs (hj_inst.hip launch_cfg, pair_dim)
    elif kernel == "pair4":
        names = PAIR4_NAMES[gi]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype, **env)
    data, data0 = field(g, dtype, 3), field(g, dtype, 4)
    sid = _ffi.SCHEME_IDS[scheme]
    n0 = shape[0]
    for sname, stage, need_y0 in STAGES:
        run(substep_op(dg, sid, stage, need_y0, data, data0, 0, n0, names=names), dtype,
            "hj_rk_substep %s %s %s %s whole" % (kernel, shape, scheme, sname))
    run(substep_op(dg, sid, _ffi.STAGE_RK3_FULL, True, data, data0, 2, n0 - 2, rs=-1, names=names), dtype,
        "hj_rk_substep %s %s %s planes [2, %d) clamp" % (kernel, shape, scheme, n0 - 2))


@pytest.mark.parametrize("sid", [4, 5], ids=["ENO2_FAST", "ENO3_FAST"])
def test_substep_rows_fast_eno(sid, monkeypatch):
    shape, periodic, tz = GRIDS3[1]
    g = grid(shape, periodic, tz)
    for env, names in (KERNELS3["pair_ring"], KERNELS3["scalar"], KERNELS3["direct"]):
        dg = ctx(g, monkeypatch, "float64", **env)
        data, data0 = field(g, "float64", 5), field(g, "float64", 6)
        run(substep_op(dg, sid, _ffi.STAGE_RK3_HALF, True, data, data0, 0, shape[0], names=names), "float64", "fast ENO %d %s" % (sid, names))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("gi", range(len(GRIDS3)))
@pytest.mark.parametrize("kernel", sorted(KERNELS3))
def test_lf_term_rows(kernel, gi, dtype, monkeypatch):
    """hj_lf_term (ydot and the host stepBound), every scheme, restrict_sign 0 / +1 / -1."""
    shape, periodic, tz = GRIDS3[gi]
    env, names = KERNELS3[kernel]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype, **env)
    data = field(g, dtype, 7)
    ham, par = ham_for(3)
    for k, scheme in enumerate(SCHEMES):
        rs = (0, 1, -1, 0)[(k + gi) % 4]

        def op(A, scheme=scheme, rs=rs):
            y = A.inp("y", data)
            out = A.out("ydot", data.shape)
            A.arm()
            sb = C.c_double()
            _ffi.check(dg.lib.hj_lf_term(dg.ctx, _ffi.SCHEME_IDS[scheme], ham, _ffi.darr(par), 0.1, rs, y.ptr, out.ptr, C.byref(sb)))
            # (hj_lf_term with the intended WENO5 reduces its own epsilon: that call has no transposed form, hj_instx.hip launch_xp)
            ok = names + ("fused_pair_kernel",) if (kernel == "xp" and scheme == "WENO5") else names
            assert kernel_name(dg) in ok, (kernel_name(dg), ok)
            return {"step_bound": sb.value}
        run(op, dtype, "hj_lf_term %s %s %s %s rs=%d" % (kernel, shape, scheme, dtype, rs))


@pytest.mark.parametrize("kernel,gi", ROWS24)
def test_lf_term_rows_2d_4d(kernel, gi, monkeypatch):
    """hj_lf_term on the 2-D and 4-D kernels (the light schemes, which select the 4-D fp32 kernels, and ENO3)."""
    nd, dtype, env, names = KERNELS24[kernel]
    shape, periodic, tz = (GRIDS2 if nd == 2 else GRIDS4)[gi]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype, **env)
    data = field(g, dtype, 7)
    ham, par = ham_for(nd)
    for scheme, rs in (("WENO5_ASSHIPPED", 0), ("ENO2", 1), ("ENO3", -1)):
        want = names
        if kernel in ("flat4", "pair4", "pair4d") and scheme == "ENO3":
            want = ("fused_substep_kernel",)
        elif kernel == "pair4":
            want = PAIR4_NAMES[gi]

        def op(A):
            y = A.inp("y", data)
            out = A.out("ydot", data.shape)
            A.arm()
            sb = C.c_double()
            _ffi.check(dg.lib.hj_lf_term(dg.ctx, _ffi.SCHEME_IDS[scheme], ham, _ffi.darr(par), 0.1, rs, y.ptr, out.ptr, C.byref(sb)))
            assert kernel_name(dg) in want, (kernel_name(dg), want)
            return {"step_bound": sb.value}
        run(op, dtype, "hj_lf_term %s %s %s rs=%d" % (kernel, shape, scheme, rs))


def test_large_grid_rows(monkeypatch):
    """201^3: the shapes only large grids select by default (the pair kernel with its parked ring from 6.5 M cells)."""
    g = grid((201, 201, 201), (2,), ())
    dg = ctx(g, monkeypatch, "float64")
    data, data0 = field(g, "float64", 8), field(g, "float64", 9)
    sid = _ffi.SCHEME_IDS["WENO5_ASSHIPPED"]
    run(substep_op(dg, sid, _ffi.STAGE_EULER, False, data, data0, 0, 201, names=("fused_pair_kernel",), ring=True), "float64", "201^3 EULER")
    run(substep_op(dg, sid, _ffi.STAGE_RK3_FULL, True, data, data0, 7, 190, names=("fused_pair_kernel",)), "float64", "201^3 RK3_FULL planes [7, 190)")


# ------------------------------------------------------------------------------ slab mode
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", ["ENO3", "WENO5"])
@pytest.mark.parametrize("periodic0", [False, True])
@pytest.mark.parametrize("kernel", ["scalar", "pair_ring"])
def test_slab_mode_rows(kernel, periodic0, scheme, dtype, monkeypatch):
    """hj_rk_substep on a slab context: `y` carries 3 pad planes on the sides with a neighbour (read), `out` carries them too and
    they must still hold only the sentinel; the guards lie BEYOND the pads."""
    n = (23, 14, 12)
    g = grid(n, (0, 2) if periodic0 else (2,), ())
    full = field(g, dtype, 10)
    env, names = KERNELS3[kernel]
    sid = _ffi.SCHEME_IDS[scheme]
    ham, par = ham_for(3)
    eps_full = None
    if scheme == "WENO5":
        dgf = ctx(g, monkeypatch, dtype, **env)
        eps_full = torch.zeros(3, dtype=TD[dtype], device="cuda")
        _ffi.check(dgf.lib.hj_max_d1sq(dgf.ctx, dgf.ptr(full), dgf.ptr(eps_full)))
        dgf.sync()
    for (b, e) in ((0, 10), (10, 23)):
        lo, hi = (b > 0) or periodic0, (e < n[0]) or periodic0
        dg = ctx(g, monkeypatch, dtype, slab=(b, e, int(lo), int(hi)), **env)
        body = full[b:e]
        lead = full[[(b - 3 + k) % n[0] for k in range(3)]] if lo else 3        # no neighbour: 3 planes nobody may touch
        trail = full[[(e + k) % n[0] for k in range(3)]] if hi else 3

        def op(A):
            y = A.inp("y", body, lead, trail)
            out = A.out("out", body.shape, lead=3, trail=3)
            eps = A.inp("eps", eps_full) if eps_full is not None else None
            A.arm()
            if eps is not None:
                _ffi.check(dg.lib.hj_ctx_set_weno_eps_source(dg.ctx, eps.ptr))
            try:
                _ffi.check(dg.lib.hj_rk_substep(dg.ctx, sid, ham, _ffi.darr(par), 0., _ffi.STAGE_EULER, 2e-3, 0, y.ptr, None, out.ptr, 0, 0, e - b))
                dg.sync()
            finally:
                _ffi.check(dg.lib.hj_ctx_set_weno_eps_source(dg.ctx, None))
            assert kernel_name(dg) in names, kernel_name(dg)
            return {}
        run(op, dtype, "slab [%d, %d) of %s %s %s %s" % (b, e, n, kernel, scheme, dtype))


@pytest.mark.parametrize("order", [1, 2, 3])
def test_deep_slab_step_rows(order, monkeypatch):
    """hj_slab_rk_step_deep as rank 0 of an external two-rank world (hj_comm_init_external: no communicator, the caller moves
    pads): `cur` with D = 3 * order pad planes is preserved, the slab planes of y_out are written; its pads and the two work
    arrays may hold the planes the stages recompute beyond the slab.  Guards are 3 * order + 1 planes."""
    n = (40, 14, 12)
    D = 3 * order
    g = grid(n, (2,), ())
    full = field(g, "float64", 11)
    b, e = 0, 22
    dg = ctx(g, monkeypatch, "float64", slab=(b, e, 0, 1), pad=D, HJ_PAIR="2")
    _ffi.check(dg.lib.hj_comm_init_external(dg.ctx, 0, 2, -1, 1))
    ham, par = ham_for(3)
    shape = (e - b,) + n[1:]

    def op(A):
        cur = A.inp("cur", full[b:e], D, full[e:e + D])
        out = A.out("y_out", shape, D, D, free=[(-D, 0), (e - b, e - b + D)])
        w0, w1 = A.scratch("work0", shape, D, D), A.scratch("work1", shape, D, D)
        A.arm()
        _ffi.check(dg.lib.hj_slab_rk_step_deep(dg.ctx, order, _ffi.SCHEME_IDS["WENO5_ASSHIPPED"], ham, _ffi.darr(par), 2e-3, 0,
                                               cur.ptr, out.ptr, w0.ptr, w1.ptr))
        _ffi.check(dg.lib.hj_slab_join(dg.ctx))
        dg.sync()
        torch.cuda.synchronize()
        return {"kernel": kernel_name(dg)}
    run(op, "float64", "hj_slab_rk_step_deep order %d" % order, depth=order)


@pytest.mark.parametrize("sched", [None, "overlap", "serial"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_slab_rk_step_self_ring_rows(order, sched, monkeypatch):
    """hj_halo_exchange and hj_slab_rk_step as a ONE-rank ring (the form tests/test_gpu_round4.py drives): a periodic axis 0 closed
    through a self send / receive inside the C library.  Per substep the edge plane ranges [0, 3) + [n - 3, n) run as a launch
    of their own (on the edge stream under the "overlap" schedule) next to the interior range [3, n - 3), and the exchange
    copies the fresh edge planes into the pads of the stage's destination.  Per argument: `cur` (body and pads) is preserved
    by the step; the pads of the state are written by hj_halo_exchange, its body is not; the body of y_out must be written
    everywhere and its pads may be (halo copies); work0 / work1 are scratch, pads included."""
    import torch.distributed as dist
    from levelsetpy_amd.dist import SlabDecomposition, NativeSlabStepper
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29597")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    nat = None
    try:
        n = (40, 18, 16)
        g = grid(n, (0, 2), ())
        full = field(g, "float64", 70)
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("HJ_XP", "0")
        monkeypatch.setenv("HJ_PAIR", "2")
        if sched is None:
            monkeypatch.delenv("HJ_SLAB_SCHEDULE", raising=False)
        else:
            monkeypatch.setenv("HJ_SLAB_SCHEDULE", sched)
        slab = SlabDecomposition(n[0], 1, 0, True, self_exchange=True)
        # (the stepper object supplies the slab context and its communicator; its own buffers are not used)
        nat = NativeSlabStepper(g, slab, _ffi.ENO3, _ffi.HAM_DUBINS_REL, [1., 1., 1., 2.], [float(v) for v in np.asarray(g.dx).ravel()],
                                order=order, deep=False)
        dg = nat.dg
        lib = dg.lib
        ham, par = ham_for(3)
        pads = [(-3, 0), (n[0], n[0] + 3)]
        for scheme in ("WENO5_ASSHIPPED", "WENO5", "ENO3"):
            def op(A):
                dg.bind_stream()
                cur = A.inout("cur", full, 3, 3, written=(), free=pads)
                out = A.out("y_out", n, 3, 3, free=pads)
                w0, w1 = A.scratch("work0", n, 3, 3), A.scratch("work1", n, 3, 3)
                A.arm()
                _ffi.check(lib.hj_halo_exchange(dg.ctx, cur.ptr))
                _ffi.check(lib.hj_slab_join(dg.ctx))
                dg.sync()
                torch.cuda.synchronize()
                filled = cur.full.clone()
                assert torch.equal(filled[:3], full[-3:]) and torch.equal(filled[-3:], full[:3])       # the ring's wrap
                _ffi.check(lib.hj_slab_rk_step(dg.ctx, order, _ffi.SCHEME_IDS[scheme], ham, _ffi.darr(par), 2e-3, 0, cur.ptr, out.ptr, w0.ptr, w1.ptr))
                _ffi.check(lib.hj_slab_join(dg.ctx))
                dg.sync()
                torch.cuda.synchronize()
                assert torch.equal(cur.full, filled), "hj_slab_rk_step wrote its input"
                assert kernel_name(dg) == "fused_pair_kernel", kernel_name(dg)
                # the pads of the result hold the ring's wrap of the result itself
                assert torch.equal(out.full[:3], out.view[-3:]) and torch.equal(out.full[-3:], out.view[:3])
                return {"state_with_pads": filled, "kernel": kernel_name(dg)}
            run(op, "float64", "hj_slab_rk_step self ring order %d %s schedule %s" % (order, scheme, sched))
    finally:
        if nat is not None:
            nat.close()
        if created:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------ hj_rk_step / hj_rk_integrate / hj_rk_stage12
STEP_KERNELS = {
    "scalar": (dict(HJ_PAIR="0"), ("fused_substep_kernel",)),
    "pair": (dict(HJ_PAIR="2"), ("fused_pair_kernel",)),
    "direct": (dict(HJ_FORCE_DIRECT="1"), ("direct_substep_kernel",)),
    "coop": (dict(HJ_DIRECT_BELOW=None, HJ_COOP="1"), ("coop_rk_kernel",)),       # (order 1 is one launch of the direct kernel: step_names)
    "fuse12": (dict(HJ_PAIR="2", HJ_FUSE12="1"), ("fused_pair_kernel",)),          # (the last launch; order 2 ends in the fused pair of stages)
}


F12_NAMES = ("fused12_pair_kernel", "fused12_kernel")


def step_names(kernel, order, rs, post, names):
    """The kernel of the LAST launch of one hj_rk_step, from the rules in hj_api.hip (coop_applies, use_stage12)."""
    if kernel == "coop":
        return ("direct_substep_kernel",) if order == 1 else ("coop_rk_kernel",)
    if kernel == "fuse12" and order == 2 and rs == 0 and post == 0:
        return F12_NAMES
    return names


def step_op(dg, order, sid, data, names, post=0, post_arr=None, rs=0, plan=None):
    ham, par = ham_for(dg.dim)
    lib = dg.lib

    def op(A):
        y = A.inp("y_in", data)
        out = A.out("y_out", data.shape)
        w0, w1 = A.scratch("work0", data.shape), A.scratch("work1", data.shape)
        other = A.inp("post_a", post_arr) if post_arr is not None else None
        A.arm()
        _ffi.check(lib.hj_ctx_set_post_step(dg.ctx, post))
        _ffi.check(lib.hj_ctx_set_post_arrays(dg.ctx, 1 if other is not None else 0, null_or(other), 0, None))
        t, dt = C.c_double(), C.c_double()
        try:
            _ffi.check(lib.hj_rk_step(dg.ctx, order, sid, ham, _ffi.darr(par), 0.5, 10.0, 0.8, 1e30, rs, y.ptr, out.ptr, w0.ptr, w1.ptr,
                                      C.byref(t), C.byref(dt)))
            dg.sync()
        finally:
            _ffi.check(lib.hj_ctx_set_post_step(dg.ctx, 0))
            _ffi.check(lib.hj_ctx_set_post_arrays(dg.ctx, 0, None, 0, None))
        assert kernel_name(dg) in names, (kernel_name(dg), names)
        if plan is not None:        # (launches, stages 1 + 2 fused) as hj_rk_plan reports them for this very context
            nl, fz = C.c_int(), C.c_int()
            _ffi.check(lib.hj_rk_plan(dg.ctx, order, sid, ham, _ffi.darr(par), rs, C.byref(nl), C.byref(fz)))
            assert (nl.value, fz.value) == plan, (nl.value, fz.value, plan)
        return {"t_out": t.value, "dt_out": dt.value, "kernel": kernel_name(dg)}
    return op


# (the cooperative launch and the fused stage pair have no form for the intended WENO5: include/hj_mi355x.h)
STEP_ROWS = [(k, s) for k in sorted(STEP_KERNELS) for s in SCHEMES if not (s == "WENO5" and k in ("coop", "fuse12"))]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kernel,scheme", STEP_ROWS)
def test_rk_step_rows(kernel, scheme, dtype, monkeypatch):
    """hj_rk_step, orders 1-3: y_in unchanged, y_out written everywhere, work0 / work1 guards intact; plain, with the fused
    post-step minimum and a post array, and with the clamp.  WENO5 runs with the epsilon producer (HJ_EPS_FUSE=1, no size floor)."""
    env, names = STEP_KERNELS[kernel]
    env = dict(env, HJ_EPS_FUSE="1", HJ_EPS_FUSE_MIN_CELLS="0")
    for shape, periodic, tz in (GRIDS3[1], GRIDS3[2]):
        g = grid(shape, periodic, tz)
        dg = ctx(g, monkeypatch, dtype, **env)
        data = field(g, dtype, 12)
        floor = field(g, dtype, 13) - 0.05
        for order in (1, 2, 3):
            # no quiet fallback: one launch under HJ_COOP from order 2 up; stages 1 + 2 fused under HJ_FUSE12 (order - 1 launches)
            plan = {"coop": (1, 0) if order >= 2 else (1, 0), "fuse12": (order - 1, 1) if order >= 2 else (1, 0)}.get(kernel)
            run(step_op(dg, order, _ffi.SCHEME_IDS[scheme], data, step_names(kernel, order, 0, 0, names), plan=plan), dtype,
                "hj_rk_step %s %s %s order %d" % (kernel, shape, scheme, order))
        # (the clamp keeps the stages apart under HJ_FUSE12: use_stage12 refuses restrict_sign != 0; the cooperative launch takes both)
        plan = {"coop": (1, 0), "fuse12": (3, 0)}.get(kernel)
        run(step_op(dg, 3, _ffi.SCHEME_IDS[scheme], data, step_names(kernel, 3, -1, 1, names), post=_ffi.POST_MIN_PREV, post_arr=floor, rs=-1,
                    plan=plan), dtype, "hj_rk_step %s %s %s order 3 post-step min, post array, clamp" % (kernel, shape, scheme))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kernel", ["scalar", "pair"])
@pytest.mark.parametrize("order,scheme", [(3, "WENO5_ASSHIPPED"), (2, "ENO3"), (1, "ENO2"), (3, "WENO5")])
def test_rk_integrate_rows(order, scheme, kernel, dtype, monkeypatch):
    """hj_rk_integrate, three steps: y_in is never written; buf_a / buf_b / work keep their guards; the result buffer and
    t_out / steps_out / result_in equal the reference run's."""
    env, names = STEP_KERNELS[kernel]
    shape, periodic, tz = GRIDS3[0]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype, **env)
    data = field(g, dtype, 14)
    ham, par = ham_for(3)

    def op(A):
        y = A.inp("y_in", data)
        a, b, w = A.scratch("buf_a", shape), A.scratch("buf_b", shape), A.scratch("work", shape)
        A.arm()
        _ffi.check(dg.lib.hj_ctx_set_post_step(dg.ctx, _ffi.POST_MAX_PREV))
        t, ns, which = C.c_double(), C.c_int64(), C.c_int()
        try:
            _ffi.check(dg.lib.hj_rk_integrate(dg.ctx, order, _ffi.SCHEME_IDS[scheme], ham, _ffi.darr(par), 0.0, 10.0, 0.8, 1e30, 0,
                                              y.ptr, a.ptr, b.ptr, w.ptr, 3, -1.0, C.byref(t), C.byref(ns), C.byref(which)))
            dg.sync()
        finally:
            _ffi.check(dg.lib.hj_ctx_set_post_step(dg.ctx, 0))
        assert ns.value == 3 and which.value in (1, 2) and kernel_name(dg) in names
        return {"t_out": t.value, "steps": ns.value, "result_in": which.value, "state": (a, b)[which.value - 1].view.clone()}
    run(op, dtype, "hj_rk_integrate %s %s order %d %s" % (kernel, scheme, order, dtype))


@pytest.mark.parametrize("f12_pair", ["0", "2"])
@pytest.mark.parametrize("shape_i", [0, 1, 2])
def test_stage12_rows(shape_i, f12_pair, monkeypatch):
    """hj_rk_stage12 (two stages in one launch; the buffer descriptor spans the whole array): 2-D and 3-D."""
    shape, periodic, tz = (GRIDS3[1], GRIDS3[2], GRIDS2[0])[shape_i]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, "float64", HJ_FUSE12="1", HJ_F12_PAIR=f12_pair, HJ_PAIR="2")
    data = field(g, "float64", 15)
    ham, par = ham_for(len(shape))
    for scheme in ("ENO2", "ENO3", "WENO5_ASSHIPPED"):
        # a grid without a two-cells-per-lane tiling answers HJ_EUNSUPPORTED under HJ_F12_PAIR=2: the row then asserts that
        # answer, and that the refused call touched nothing
        probe = torch.zeros_like(data)
        refused = dg.lib.hj_rk_stage12(dg.ctx, _ffi.SCHEME_IDS[scheme], ham, _ffi.darr(par), 2e-3, 0.75, 0.25, dg.ptr(data), dg.ptr(probe), 6) != 0
        dg.sync()
        assert not (refused and f12_pair == "0"), dg.lib.hj_last_error()

        def op(A, scheme=scheme, refused=refused):
            y = A.inp("y", data)
            out = A.out("out", shape, written=() if refused else None)
            A.arm()
            rc = dg.lib.hj_rk_stage12(dg.ctx, _ffi.SCHEME_IDS[scheme], ham, _ffi.darr(par), 2e-3, 0.75, 0.25, y.ptr, out.ptr, 6)
            if refused:
                assert rc == -3 and b"pair" in dg.lib.hj_last_error(), (rc, dg.lib.hj_last_error())
                dg.sync()
                return {"refused": rc}
            _ffi.check(rc)
            sb, am = C.c_double(), (C.c_double * 4)()
            _ffi.check(dg.lib.hj_read_step_bound(dg.ctx, 6, C.byref(sb), am))
            name = kernel_name(dg)
            # HJ_F12_PAIR=2: the two-cells-per-lane kernel or an error (hj_inst.hip launch_stage12), never the other kernel quietly
            assert name == ("fused12_kernel" if f12_pair == "0" else "fused12_pair_kernel"), name
            return {"step_bound": sb.value, "kernel": name}
        run(op, "float64", "hj_rk_stage12 %s %s pair=%s" % (shape, scheme, f12_pair))


# ------------------------------------------------------------------------------ array-level entry points
ALL_GRIDS = GRIDS2 + [GRIDS3[0], GRIDS3[2], GRIDS3[1], GRIDS3[4], GRIDS4[1]]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("gi", range(len(ALL_GRIDS)))
def test_ghost_rows(gi, dtype, monkeypatch):
    """hj_ghost: `out` is larger than `in`; every dim, widths 1-3."""
    shape, periodic, tz = ALL_GRIDS[gi]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype)
    data = field(g, dtype, 16)
    for dim in range(len(shape)):
        for w in (1, 2, 3):
            oshape = tuple(s + (2 * w if d == dim else 0) for d, s in enumerate(shape))

            def op(A):
                x = A.inp("in", data)
                out = A.out("out", oshape)
                A.arm()
                _ffi.check(dg.lib.hj_ghost(dg.ctx, dim, w, x.ptr, out.ptr))
                dg.sync()
                return {}
            run(op, dtype, "hj_ghost %s dim %d width %d %s" % (shape, dim, w, dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("gi", range(len(ALL_GRIDS)))
def test_upwind_rows(gi, scheme, dtype, monkeypatch):
    shape, periodic, tz = ALL_GRIDS[gi]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype)
    data = field(g, dtype, 17)
    for dim in range(len(shape)):
        def op(A):
            x = A.inp("phi", data)
            dl, dr = A.out("derivL", shape), A.out("derivR", shape)
            A.arm()
            mm = (C.c_double * 4)()
            _ffi.check(dg.lib.hj_upwind(dg.ctx, _ffi.SCHEME_IDS[scheme], dim, x.ptr, dl.ptr, dr.ptr, mm))
            return {"minmax4": tuple(mm)}
        run(op, dtype, "hj_upwind %s %s dim %d %s" % (shape, scheme, dim, dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("gi", range(len(ALL_GRIDS)))
def test_lf_split_rows(gi, scheme, dtype, monkeypatch):
    """hj_lf_split_begin (all derivatives in one launch, 4 * ndim reductions) and hj_lf_split_end (array and scalar alphas)."""
    shape, periodic, tz = ALL_GRIDS[gi]
    nd = len(shape)
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype)
    data = field(g, dtype, 18)
    keep = {}

    def begin(A):
        x = A.inp("y", data)
        dl = [A.out("derivL%d" % d, shape) for d in range(nd)]
        dr = [A.out("derivR%d" % d, shape) for d in range(nd)]
        A.arm()
        mm = (C.c_double * (4 * nd))()
        _ffi.check(dg.lib.hj_lf_split_begin(dg.ctx, _ffi.SCHEME_IDS[scheme], x.ptr, (C.c_void_p * nd)(*[a.view.data_ptr() for a in dl]),
                                            (C.c_void_p * nd)(*[a.view.data_ptr() for a in dr]), mm))
        keep["dl"], keep["dr"] = [a.view.clone() for a in dl], [a.view.clone() for a in dr]
        return {"minmax4n": tuple(mm)}
    run(begin, dtype, "hj_lf_split_begin %s %s %s" % (shape, scheme, dtype))
    alpha0 = (field(g, dtype, 19).abs() + 0.1).contiguous()
    hamv = field(g, dtype, 20)
    for with_ham in (True, False):
        def end(A):
            dl = [A.inp("derivL%d" % d, keep["dl"][d]) for d in range(nd)]
            dr = [A.inp("derivR%d" % d, keep["dr"][d]) for d in range(nd)]
            al = A.inp("alpha0", alpha0)
            hm = A.inp("ham", hamv) if with_ham else None
            out = A.out("out", shape)
            A.arm()
            sb, am = C.c_double(), (C.c_double * 4)()
            alphas = (C.c_void_p * nd)(*([al.view.data_ptr()] + [None] * (nd - 1)))        # dim 0 an array, the others scalars
            _ffi.check(dg.lib.hj_lf_split_end(dg.ctx, (C.c_void_p * nd)(*[a.view.data_ptr() for a in dl]),
                                              (C.c_void_p * nd)(*[a.view.data_ptr() for a in dr]), alphas, _ffi.darr([0.0, 0.7, 0.3, 1.1][:nd]),
                                              null_or(hm), out.ptr, C.byref(sb), am))
            return {"step_bound": sb.value, "alpha_max": tuple(am[:nd])}
        run(end, dtype, "hj_lf_split_end %s %s %s ham=%s" % (shape, scheme, dtype, with_ham))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_rk_combine_rows(mode, dtype, monkeypatch):
    g = grid((23, 14, 12), (2,), ())
    dg = ctx(g, monkeypatch, dtype)
    xs = [field(g, dtype, 21 + k) for k in range(3)]
    for n in (23 * 14 * 12, 1, 255, 257, 1001):          # none a multiple of 256
        assert n % 256
        def op(A):
            x0 = A.inp("x0", xs[0].reshape(-1)[:n]) if mode >= 2 else None
            y, z = A.inp("y", xs[1].reshape(-1)[:n]), A.inp("z", xs[2].reshape(-1)[:n])
            out = A.out("out", (n,))
            A.arm()
            _ffi.check(dg.lib.hj_rk_combine(dg.ctx, mode, 2e-3, null_or(x0), y.ptr, z.ptr, out.ptr, n))
            dg.sync()
            return {}
        run(op, dtype, "hj_rk_combine mode %d n %d %s" % (mode, n, dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_minmax_any_nan_rows(dtype, monkeypatch):
    g = grid((23, 14, 12), (2,), ())
    dg = ctx(g, monkeypatch, dtype)
    a, b = field(g, dtype, 24).reshape(-1), field(g, dtype, 25).reshape(-1)
    for n in (23 * 14 * 12, 1, 257, 1001):
        for opn in (_ffi.OP_MIN, _ffi.OP_MAX, _ffi.OP_MAX_NEG):
            def op(A):
                y = A.inout("y", a[:n])
                other = A.inp("other", b[:n])
                A.arm()
                _ffi.check(dg.lib.hj_minmax_with(dg.ctx, opn, y.ptr, other.ptr, n))
                dg.sync()
                return {}
            run(op, dtype, "hj_minmax_with op %d n %d %s" % (opn, n, dtype))
        for poison in (None, 0, n - 1):
            src = a[:n].clone()
            if poison is not None:
                src[poison] = float("nan")

            def op(A):
                y = A.inp("y", src)
                A.arm()
                has = C.c_int(-1)
                _ffi.check(dg.lib.hj_any_nan(dg.ctx, y.ptr, n, C.byref(has)))
                assert has.value == (0 if poison is None else 1)
                return {"has_nan": has.value}
            run(op, dtype, "hj_any_nan n %d poison %s %s" % (n, poison, dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("gi", range(len(ALL_GRIDS)))
def test_max_d1sq_rows(gi, dtype, monkeypatch):
    shape, periodic, tz = ALL_GRIDS[gi]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype)
    data = field(g, dtype, 26)

    def op(A):
        y = A.inp("y", data)
        out = A.out("max_d1sq", (len(shape),))
        A.arm()
        _ffi.check(dg.lib.hj_max_d1sq(dg.ctx, y.ptr, out.ptr))
        dg.sync()
        return {}
    run(op, dtype, "hj_max_d1sq %s %s" % (shape, dtype))


# ------------------------------------------------------------------------------ term kernels
# (only fp64 2-D / 3-D grids have a tiled term kernel: include/hj_mi355x.h)
TERM_ROWS = [(p, gi, d) for p in ("tiled", "direct") for gi in range(len(ALL_GRIDS)) for d in ("float64", "float32")
             if p == "direct" or (d == "float64" and len(ALL_GRIDS[gi][0]) in (2, 3))]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("path,gi,dtype", TERM_ROWS)
def test_term_rows(path, gi, dtype, scheme, monkeypatch):
    """hj_term_normal / _reinit / _convection, tiled (fp64 2-D / 3-D: the substep kernel with the term in the Hamiltonian's
    place) and direct (term_kernel), with array and scalar speed / velocity."""
    shape, periodic, tz = ALL_GRIDS[gi]
    nd = len(shape)
    tiled = path == "tiled"
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, dtype, HJ_TERM_TILED_FROM="0" if tiled else "-1", HJ_PAIR="0")
    want = "fused_substep_kernel" if tiled else "term_kernel"
    data, speed, init = field(g, dtype, 27), field(g, dtype, 28) + 0.3, field(g, dtype, 29)
    vel = [field(g, dtype, 30 + d) for d in range(nd)]
    sid = _ffi.SCHEME_IDS[scheme]
    lib = dg.lib

    def finish(sb):
        assert kernel_name(dg) == want, kernel_name(dg)
        return {"step_bound": sb.value}

    for arr in (True, False):
        def normal(A):
            y = A.inp("y", data)
            sp = A.inp("speed", speed) if arr else None
            out = A.out("ydot", shape)
            A.arm()
            sb = C.c_double()
            _ffi.check(lib.hj_term_normal(dg.ctx, sid, y.ptr, null_or(sp), -0.8, out.ptr, C.byref(sb)))
            return finish(sb)
        run(normal, dtype, "hj_term_normal %s %s %s %s array=%s" % (path, shape, scheme, dtype, arr))

        def convection(A):
            y = A.inp("y", data)
            vs = [A.inp("v%d" % d, vel[d]) if (arr and d != 1) else None for d in range(nd)]      # mixed: axis 1 a scalar
            out = A.out("ydot", shape)
            A.arm()
            sb = C.c_double()
            ptrs = (C.c_void_p * nd)(*[v.view.data_ptr() if v is not None else None for v in vs])
            _ffi.check(lib.hj_term_convection(dg.ctx, sid, y.ptr, ptrs, _ffi.darr([0.5, -0.25, 0.75, 1.0][:nd]), out.ptr, C.byref(sb)))
            return finish(sb)
        run(convection, dtype, "hj_term_convection %s %s %s %s arrays=%s" % (path, shape, scheme, dtype, arr))
    for sub in (0, 1):
        def reinit(A):
            y = A.inp("y", data)
            i0 = A.inp("initial", init)
            out = A.out("ydot", shape)
            A.arm()
            sb = C.c_double()
            _ffi.check(lib.hj_term_reinit(dg.ctx, sid, y.ptr, i0.ptr, sub, out.ptr, C.byref(sb)))
            return finish(sb)
        run(reinit, dtype, "hj_term_reinit %s %s %s %s subcell %d" % (path, shape, scheme, dtype, sub))


# ------------------------------------------------------------------------------ curvature and trace-Hessian kernel
from test_gpu_curvature import CASES as CURV_CASES, _grids as curv_grids  # noqa: E402


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N,periodic,tz", CURV_CASES)
def test_curvature_rows(N, periodic, tz, dtype, monkeypatch):
    """hj_term_curvature (array and scalar b), hj_curvature_second, hj_hessian_second (all ND + ND (ND + 1) / 2 outputs
    guarded), hj_laplacian_second, hj_centered_first_second for every dim; 1-D to 4-D."""
    g, _ = curv_grids(N, periodic, tz)
    nd = len(N)
    dg = ctx(g, monkeypatch, dtype)
    lib = dg.lib
    data, barr = field(g, dtype, 40), field(g, dtype, 41).abs() + 0.1

    def named(res=None):
        assert kernel_name(dg) == "curv_kernel", kernel_name(dg)
        dg.sync()
        return res or {}

    for arr in (True, False):
        def term(A):
            y = A.inp("y", data)
            b = A.inp("b", barr) if arr else None
            out = A.out("ydot", N)
            A.arm()
            sb = C.c_double()
            _ffi.check(lib.hj_term_curvature(dg.ctx, y.ptr, null_or(b), 0.6, out.ptr, C.byref(sb)))
            return named({"step_bound": sb.value})
        run(term, dtype, "hj_term_curvature %s %s %s %s array b=%s" % (N, periodic, tz, dtype, arr))

    def curvature(A):
        y = A.inp("y", data)
        k, m = A.out("curvature", N), A.out("grad_mag", N)
        A.arm()
        _ffi.check(lib.hj_curvature_second(dg.ctx, y.ptr, k.ptr, m.ptr))
        return named()
    run(curvature, dtype, "hj_curvature_second %s %s" % (N, dtype))

    def hessian(A):
        y = A.inp("y", data)
        first = [A.out("first%d" % d, N) for d in range(nd)]
        second = [[A.out("second%d%d" % (i, j), N) if j <= i else None for j in range(nd)] for i in range(nd)]
        A.arm()
        sp = (C.c_void_p * (nd * nd))(*[second[i][j].view.data_ptr() if j <= i else None for i in range(nd) for j in range(nd)])
        fp = (C.c_void_p * nd)(*[a.view.data_ptr() for a in first])
        _ffi.check(lib.hj_hessian_second(dg.ctx, y.ptr, sp, fp))
        return named()
    run(hessian, dtype, "hj_hessian_second %s %s" % (N, dtype))

    def laplacian(A):
        y = A.inp("y", data)
        out = A.out("laplacian", N)
        A.arm()
        _ffi.check(lib.hj_laplacian_second(dg.ctx, y.ptr, out.ptr))
        return named()
    run(laplacian, dtype, "hj_laplacian_second %s %s" % (N, dtype))
    for dim in range(nd):
        def centered(A):
            y = A.inp("y", data)
            out = A.out("centered", N)
            A.arm()
            _ffi.check(lib.hj_centered_first_second(dg.ctx, dim, y.ptr, out.ptr))
            return named()
        run(centered, dtype, "hj_centered_first_second %s dim %d %s" % (N, dim, dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N,periodic,tz", CURV_CASES)
def test_trace_hessian_rows(N, periodic, tz, dtype, monkeypatch):
    """hj_term_trace_hessian with mixed array / scalar entries of L and R, and with every entry a scalar."""
    g, _ = curv_grids(N, periodic, tz)
    nd = len(N)
    nn = nd * nd
    dg = ctx(g, monkeypatch, dtype)
    data = field(g, dtype, 42)
    cells = [field(g, dtype, 43 + e) * 0.5 for e in range(2)]
    lscal = [0.5 + 0.1 * e for e in range(nn)]
    rscal = [1.0 if e % (nd + 1) == 0 else 0.2 for e in range(nn)]
    for mixed in (True, False):
        def op(A):
            y = A.inp("y", data)
            la = A.inp("L0", cells[0]) if mixed else None               # entry 0 of L and the last entry of R are arrays
            ra = A.inp("Rlast", cells[1]) if mixed else None
            out = A.out("ydot", N)
            A.arm()
            lp = (C.c_void_p * nn)(*([la.view.data_ptr()] + [None] * (nn - 1))) if mixed else None
            rp = (C.c_void_p * nn)(*([None] * (nn - 1) + [ra.view.data_ptr()])) if mixed else None
            sb = C.c_double()
            _ffi.check(dg.lib.hj_term_trace_hessian(dg.ctx, y.ptr, lp, _ffi.darr(lscal), rp, _ffi.darr(rscal), out.ptr, C.byref(sb)))
            assert kernel_name(dg) == "curv_kernel", kernel_name(dg)
            dg.sync()
            return {"step_bound": sb.value}
        run(op, dtype, "hj_term_trace_hessian %s %s %s %s mixed=%s" % (N, periodic, tz, dtype, mixed))


# ------------------------------------------------------------------------------ run-time kernels
DRIFT_SRC = "H = p[0] * x[1] + par[0] * fabs(p[1]) - 0.3 * p[2]; alpha[0] = fabs(x[1]); alpha[1] = fabs(par[0]); alpha[2] = 0.3;"


def _burgers_src(dim):
    s = "H = par[0] * x[0] * p[1];\n"
    for d in range(dim):
        s += "H += 0.5 * p[%d] * p[%d];  alpha[%d] = fmax(fabs(dmin[%d]), fabs(dmax[%d]));\n" % (d, d, d, d, d)
    return s + "alpha[1] += fabs(par[0] * x[0]);\n"


@pytest.mark.parametrize("pair", ["0", "2"])
def test_runtime_hamiltonian_rows(pair, monkeypatch):
    """A Hamiltonian registered by hand (hipRTC kernels): substeps over the whole grid and a sub-range; a range-reading one
    through hj_range_pass (the 64-bit key array guarded too, on the fp64 pool: keys need 8-byte alignment), hj_bound_pass and
    the substep that reads the range."""
    shape, periodic, tz = GRIDS3[1]
    g = grid(shape, periodic, tz)
    dg = ctx(g, monkeypatch, "float64", HJ_PAIR=pair)
    data, data0 = field(g, "float64", 50), field(g, "float64", 51)
    reg = L.register_native_hamiltonian("bounds_drift_3d", 3, DRIFT_SRC, nparams=1)
    rng_reg = L.register_native_hamiltonian("bounds_burgers_3d", 3, _burgers_src(3), nparams=1)      # reads dmin / dmax: HJ_HAM_RANGE
    assert rng_reg.uses_range and not reg.uses_range
    par = _ffi.darr([0.7])
    want = "fused_pair_kernel (hipRTC)"      # 2-D / 3-D run-time kernels are pair kernels whatever HJ_PAIR says (hj_rtc.hip, shape_of); one cell per lane is 4-D only
    n0 = shape[0]
    for scheme in ("ENO2", "WENO5_ASSHIPPED", "WENO5"):
        sid = _ffi.SCHEME_IDS[scheme]
        for ham_id in (reg.ham_id, rng_reg.ham_id):
            for stage, need_y0, p0, p1 in ((_ffi.STAGE_EULER, False, 0, n0), (_ffi.STAGE_RK3_FULL, True, 3, n0 - 6)):
                def op(A):
                    y = A.inp("y", data)
                    y0 = A.inp("y0", data0) if need_y0 else None
                    out = A.out("out", shape, written=(p0, p1))
                    A.arm()
                    _ffi.check(dg.lib.hj_rk_substep(dg.ctx, sid, ham_id, par, 0., stage, 2e-3, 0, y.ptr, null_or(y0), out.ptr, 7, p0, p1))
                    sb, am = C.c_double(), (C.c_double * 4)()
                    _ffi.check(dg.lib.hj_read_step_bound(dg.ctx, 7, C.byref(sb), am))
                    assert kernel_name(dg) == want, kernel_name(dg)
                    res = {"step_bound": sb.value, "alpha_max": tuple(am[:3])}
                    if ham_id == reg.ham_id:        # alpha does not read the data: the cached bound of alpha_bound_kernel
                        ssb, sam = C.c_double(), (C.c_double * 4)()
                        _ffi.check(dg.lib.hj_static_step_bound(dg.ctx, ham_id, par, C.byref(ssb), sam))
                        res["static_step_bound"], res["static_alpha_max"] = ssb.value, tuple(sam[:3])
                    return res
                run(op, "float64", "run-time Hamiltonian %d %s pair=%s planes [%d, %d)" % (ham_id, scheme, pair, p0, p1))

        def range_pass(A):
            y = A.inp("y", data)
            keys = A.inout("keys", torch.zeros(8, dtype=torch.float64, device="cuda"))
            A.arm()
            assert keys.view.data_ptr() % 8 == 0
            _ffi.check(dg.lib.hj_range_pass(dg.ctx, sid, rng_reg.ham_id, par, y.ptr, keys.ptr))
            dg.sync()
            return {"range_keys": tuple(int(v) for v in keys.view.view(torch.int64).cpu())}
        run(range_pass, "float64", "hj_range_pass %s pair=%s" % (scheme, pair))

        def bound_pass(A):
            y = A.inp("y", data)
            A.arm()
            sb = C.c_double()
            _ffi.check(dg.lib.hj_ctx_set_dissipation(dg.ctx, _ffi.DISS_LLF))
            try:
                _ffi.check(dg.lib.hj_bound_pass(dg.ctx, sid, rng_reg.ham_id, par, y.ptr, C.byref(sb)))
            finally:
                _ffi.check(dg.lib.hj_ctx_set_dissipation(dg.ctx, _ffi.DISS_GLF))
            return {"step_bound": sb.value}
        run(bound_pass, "float64", "hj_bound_pass %s pair=%s" % (scheme, pair))


# ------------------------------------------------------------------------------ Python level: views of a caller's pool
def _views(flat, shape, k):
    """The same values as a view with storage offset k, as a strided slice, and as a transposed view reshaped back; each
    inside a pool whose other elements must not change.  -> [(what, pool, view of the grid's shape)]"""
    n = int(np.prod(shape))
    dt, dev = flat.dtype, flat.device
    out = []
    p = torch.full((n + 64,), 1e30, dtype=dt, device=dev)
    p[k:k + n] = flat
    v = p[k:k + n].view(shape)
    assert v.storage_offset() == k and v.is_contiguous()
    out.append(("offset %d" % k, p, v))
    p = torch.full((2 * n + 8,), -1e30, dtype=dt, device=dev)
    p[k:k + 2 * n:2] = flat
    v = p[k:k + 2 * n:2].view(shape)
    assert not v.is_contiguous()
    out.append(("strided slice", p, v))
    p = torch.full((n + 8,), 1e30, dtype=dt, device=dev)
    t = flat.view(shape).transpose(0, -1).contiguous()
    p[k:k + n] = t.reshape(-1)
    v = p[k:k + n].view(t.shape).transpose(0, -1)
    assert not v.is_contiguous() and tuple(v.shape) == tuple(shape)
    out.append(("transposed view", p, v))
    return out


class _Drift(object):
    """A hamFunc / partialFunc pair of the user's own (NumPy or torch arrays alike): traced into a run-time kernel on first use."""

    def __init__(self, grid):
        self.grid = grid

    def hamiltonian(self, t, data, p, sd=None):
        return 0.5 * p[0] + 0.25 * abs(p[1]) - 0.3 * p[2]

    def dissipation(self, t, data, dmin, dmax, sd, dim):
        return [0.5, 0.25, 0.3][dim]


def _ibits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k", [1, 3])
def test_python_level_views(k, dtype, monkeypatch):
    """termLaxFriedrichs (built-in and traced callbacks), odeCFL3 (one step), termCurvature, termTraceHessian, hessianSecond and
    curvatureSecond with the state given as a view with a nonzero storage offset and as non-contiguous views: the same bits as for a
    fresh contiguous copy, and the caller's tensor and the pool around it unchanged."""
    from guarded_pool import same_bits
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    shape, periodic, tz = GRIDS3[0]
    nd = 3
    g = grid(shape, periodic, tz)
    base = field(g, dtype, 60)
    sys_ = L.DubinsVehicleRel(g, 1, 1)
    sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstWENO5))
    drift = _Drift(g)
    sd_traced = L.Bundle(dict(grid=g, hamFunc=drift.hamiltonian, partialFunc=drift.dissipation, dissFunc=L.artificialDissipationGLF,
                              CoStateCalc=L.upwindFirstENO3))
    opts = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on')))
    ident = [[1.0 if i == j else 0.0 for j in range(nd)] for i in range(nd)]
    sd_curv = L.Bundle(dict(grid=g, b=0.4, curvatureFunc=L.curvatureSecond))
    sd_trace = L.Bundle(dict(grid=g, hessianFunc=L.hessianSecond, L=ident, R=[[0.3 if i == j else 0.05 for j in range(nd)] for i in range(nd)]))

    def ops(y3):
        col = y3.reshape(-1, 1)         # a view where the strides allow one (offset, strided slice), else the caller's own copy
        res = {}
        res["lf"], res["lf_sb"], _ = L.termLaxFriedrichs(0.0, col, sd)
        res["lf_traced"], res["lf_traced_sb"], _ = L.termLaxFriedrichs(0.0, col, sd_traced)
        res["ode_t"], res["ode_y"], _ = L.odeCFL3(L.termLaxFriedrichs, [0.0, 10.0], col, opts, sd)
        res["curv"], res["curv_sb"], _ = L.termCurvature(0.0, col, sd_curv)
        res["trace"], res["trace_sb"], _ = L.termTraceHessian(0.0, col, sd_trace)
        second, first = L.hessianSecond(g, y3)
        for i in range(nd):
            res["first%d" % i] = first[i]
            for j in range(i + 1):
                res["second%d%d" % (i, j)] = second[i][j]
        res["curvature"], res["grad_mag"] = L.curvatureSecond(g, y3)
        return dict((kk, v.clone() if torch.is_tensor(v) else float(v)) for kk, v in res.items())

    ref = ops(base.clone())
    assert ref["lf"].dtype == base.dtype
    for what, p, v in _views(base.reshape(-1), shape, k):
        before = p.clone()
        assert torch.equal(v, base), what
        got = ops(v)
        torch.cuda.synchronize()
        assert torch.equal(_ibits(p), _ibits(before)), "%s: the caller's pool changed" % what
        same_bits(got, ref, "python level %s %s" % (what, dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k", [1, 3])
def test_python_level_solve_on_a_view(k, dtype, monkeypatch):
    """HJIPDE_solve over a short span from a state that is a view (storage offset, strided, transposed) of a larger tensor."""
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    shape, periodic, tz = GRIDS3[0]
    g = grid(shape, periodic, tz)
    base = field(g, dtype, 61)
    sys_ = L.DubinsVehicleRel(g, 1, 1)
    tau = np.array([0.0, 0.02, 0.04])

    def solve(state):
        sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, derivFunc=L.upwindFirstENO3, uMode='min', dMode='max'))
        data, tau_o, _ = L.HJIPDE_solve(state, tau, sd, "minVOverTime", L.Bundle(dict(keepLast=True, quiet=True)))
        return torch.as_tensor(np.asarray(data.detach().cpu().numpy() if torch.is_tensor(data) else data))
    ref = solve(base.clone())
    for what, p, v in _views(base.reshape(-1), shape, k):
        before = p.clone()
        got = solve(v)
        torch.cuda.synchronize()
        assert torch.equal(_ibits(p), _ibits(before)), "%s: the caller's pool changed" % what
        assert got.shape == ref.shape and torch.equal(_ibits(got), _ibits(ref)), what
