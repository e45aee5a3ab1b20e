"""GPU: every kernel instantiation the library ships, launched through the C ABI by its recipe (tests/instantiation_recipes.py) and
compared with a reference.  A row switches the context's launch record on, runs the recipe's call, asserts that the instantiation it
claims is in the record (no row can pass on a fallback), and compares every output of the launch: ydot or the stage result (the
reference stage is formed from the oracle's ydot with odeCFLn's combination), the step bound, the termRestrictUpdate clamp.

References and tolerances are the suite's own:
  fp64 built-in systems against oracle.term_lax_friedrichs -- ENO2 / ENO3 on the Dubins car and the double integrator bit for bit, the two
    WENO5 arithmetics 1e-11 of max(1, |ref|), the 4-D pendulum's ENO and the lean ENO ids 4 / 5 by the masked rules of tests/fuzz_parity.py
    and test_fast_eno_mode_masked_parity_with_the_reference_golden;
  fp32: direct_substep_kernel<float> against the oracle's FLOAT32 mode on the same data -- ENO2 / ENO3 on the Dubins car and the double
    integrator bit for bit, step bound == (tests/test_gpu_fp32_exact.py holds the other stages, data sets and libraries to it) -- and,
    beside it, against the fp64 oracle on the same fp32-rounded data (test_gpu_fp32._fp32_close and that file's state rule); every other
    fp32 substep instantiation against that direct kernel on the same data, bit for bit (the same per-cell arithmetic: what the suite
    asserts between the fp64 families);
  term_kernel against oracle.term_normal / term_reinit / term_convection (tests/fuzz_terms.py; fp32 by the rule of
    test_fp32_split_path_terms_and_gradients), the tiled TermOp launches also bit for bit against term_kernel;
  curv_kernel against tests/curvature_ref.py and tests/trace_hess_ref.py with the tolerances of their GPU tests;
  the fused launches (coop_rk_kernel, fused12_kernel, fused12_pair_kernel) bit for bit against the stage launches they replace;
  the helper kernels against the oracle functions and NumPy expressions their existing tests use.
A failing row prints its recipe: symbol, knobs and grid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantiation_recipes as IR  # noqa: E402
import curvature_ref as CR  # noqa: E402
import trace_hess_ref as TR  # noqa: E402
import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi  # noqa: E402
from levelsetpy_amd.context import DeviceGrid, device_grid  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402

RECIPES = IR.recipes() if os.path.exists(_ffi.LIB_PATH) else []
REPORT = os.environ.get("HJ_INSTANTIATION_REPORT")      # a file: one line per instantiation compared (tools/kernel_coverage.py reads it)

PAR = {0: [1., 1., 1., 2.], 1: [1.25, 0., 0., 0.], 2: [1.0, 0., 0., 0.]}
BOX = {0: ([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi]), 1: ([-1., -1.5], [1., 1.5]), 2: ([-np.pi, -8., -np.pi, -8.], [np.pi, 8., np.pi, 8.])}
HAM_OF_DIM = {2: 1, 3: 0, 4: 2}
ORACLE_SCHEME = {0: "ENO2", 1: "ENO3", 2: "WENO5", 3: "WENO5_ASSHIPPED", 4: "ENO2", 5: "ENO3"}
TDT = {"float64": torch.float64, "float32": torch.float32}


class Problem(object):
    """One grid, its system and its data -- made once and shared, never written."""
    cache = {}

    def __init__(self, ham, N, periodic):
        lo, hi = (list(v) for v in BOX[ham])
        hi = [hi[d] - (hi[d] - lo[d]) / N[d] if d in periodic else hi[d] for d in range(len(N))]
        self.ham, self.N, self.periodic = ham, tuple(N), tuple(periodic)
        self.g = L.createGrid(np.asarray(lo).reshape(-1, 1), np.asarray(hi).reshape(-1, 1), np.asarray(N, dtype=np.int64).reshape(-1, 1),
                              list(periodic) if periodic else None)
        self.og = og = O.Grid(lo, hi, [int(n) for n in N], list(periodic))
        self.og32 = og32 = O.Grid(lo, hi, [int(n) for n in N], list(periodic), dtype=np.float32)
        self.osys32 = {0: lambda: O.DubinsRel(og32, 1, 1), 1: lambda: O.DoubleIntegrator(og32, 1.25), 2: lambda: O.DoublePendulum4D(og32, 1.0)}[ham]()
        self.osys = {0: lambda: O.DubinsRel(og, 1, 1), 1: lambda: O.DoubleIntegrator(og, 1.25), 2: lambda: O.DoublePendulum4D(og, 1.0)}[ham]()
        rng = np.random.default_rng(1000 * len(N) + int(np.sum(N)))
        base = {0: lambda: O.shape_cylinder(og, 2, None, .5), 1: lambda: O.shape_sphere(og, None, .45), 2: lambda: O.shape_sphere(og, None, 1.5)}[ham]()
        self.data = base + 0.05 * np.sin(3 * og.xs[0]) * np.cos(2 * og.xs[len(N) - 1]) + 0.02 * rng.standard_normal(N)
        self.start = self.data + 0.03 * np.cos(2 * og.xs[0]) + 0.01 * rng.standard_normal(N)      # y0 of the stages that combine with it
        self.refs = {}

    @classmethod
    def get(cls, ham, N, periodic):
        key = (ham, tuple(N), tuple(periodic))
        if key not in cls.cache:
            cls.cache[key] = cls(ham, N, periodic)
        return cls.cache[key]

    def arr(self, what, dtype):
        """The data as the kernels of `dtype` see it, in fp64."""
        a = getattr(self, what)
        return a.astype(np.float32).astype(np.float64) if dtype == "float32" else a

    def oracle(self, scheme, dtype):
        """(ydot, stepBound) of termLaxFriedrichs on this problem's data (fp32 rows: on the fp32-rounded data, in fp64)."""
        key = ("lf", ORACLE_SCHEME[scheme], dtype)
        if key not in self.refs:
            yd, sb = O.term_lax_friedrichs(self.og, self.osys, ORACLE_SCHEME[scheme], 0., self.arr("data", dtype).reshape(-1, 1))
            self.refs[key] = (np.asarray(yd).reshape(self.N), float(sb))
        return self.refs[key]

    def oracle32(self, scheme):
        """(ydot, stepBound) of the oracle's float32 mode on the data as the float kernels see it."""
        key = ("lf32", ORACLE_SCHEME[scheme])
        if key not in self.refs:
            yd, sb = O.term_lax_friedrichs(self.og32, self.osys32, ORACLE_SCHEME[scheme], 0., self.data.astype(np.float32).reshape(-1, 1))
            self.refs[key] = (yd.reshape(self.N), sb)
        return self.refs[key]

    def taint(self, scheme, dtype):
        """Cells whose ENO stencil selectors have a margin below 1e-12 in some dimension."""
        key = ("taint", ORACLE_SCHEME[scheme], dtype)
        if key not in self.refs:
            data = self.arr("data", dtype)
            t = np.zeros(self.N, dtype=bool)
            for d in range(len(self.N)):
                t |= O.eno_selector_margin(self.og, data, d, ORACLE_SCHEME[scheme]) < 1e-12
            self.refs[key] = t
        return self.refs[key]


def stage_of(stage, yd, y, y0, dt):
    """The stage result odeCFLn forms from ydot (ode_cfl_3.py:151-193)."""
    if stage == _ffi.STAGE_YDOT:
        return yd
    y1 = y + dt * yd
    if stage == _ffi.STAGE_EULER:
        return y1
    if stage == _ffi.STAGE_RK3_HALF:
        return 0.25 * (3 * y0 + y1)
    if stage == _ffi.STAGE_RK2_FULL:
        return 0.5 * (y0 + y1)
    return (1 / 3) * (y0 + 2 * y1)


def ctx_for(r, g, record=True):
    with IR.environment(r.env):
        dg = DeviceGrid(g, r.dtype)
    dg.bind_stream()
    if record:
        _ffi.check(dg.lib.hj_launch_record(dg.ctx, 1))
    return dg


def launched(dg, r):
    rec = IR.read_record(dg.lib, dg.ctx)
    assert r.symbol in rec, "the claimed instantiation was not launched; the record holds %s\n%s" % (sorted(rec), r.describe())
    return rec


def substep(dg, r, stage, dt, restrict, y, y0, out, slot):
    _ffi.check(dg.lib.hj_rk_substep(dg.ctx, r.scheme, r.ham, _ffi.darr(PAR[r.ham]), 0., stage, dt, restrict, dg.ptr(y),
                                    dg.ptr(y0) if stage >= _ffi.STAGE_RK3_HALF else None, dg.ptr(out), slot, 0, r.N[0]))


def bound(dg, slot):
    sb = C.c_double()
    _ffi.check(dg.lib.hj_read_step_bound(dg.ctx, slot, C.byref(sb), None))
    return sb.value


def tens(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(TDT[dtype]).contiguous()


def fp32_close(got, ref, scheme_name, what=""):
    from test_gpu_fp32 import _fp32_close
    _fp32_close(got, ref, scheme_name, what)


def compare_fp64(r, P, got, ref, what):
    """A fp64 substep output against the oracle, by the rule of the system and scheme."""
    diff = np.abs(got - ref)
    scale = max(1.0, float(np.abs(ref).max()))
    name = IR.SCHEME_NAMES[r.scheme]
    if r.ham == 2 and name.startswith("ENO"):
        # the build-defined 4-D system evaluates its drift in another order than the oracle's NumPy expression: selections flip at ties (fuzz_parity.py)
        assert float((diff > 1e-11 * scale).mean()) <= 2e-3 and float(diff.max()) <= 1e-3 * scale, (what, float(diff.max()), r.describe())
    elif name in ("ENO2", "ENO3"):
        assert np.array_equal(got, ref), (what, float(diff.max()), float((diff > 0).mean()), r.describe())
    elif name.endswith("_FAST"):
        taint = P.taint(r.scheme, r.dtype)
        assert float(taint.mean()) <= 1e-4, (float(taint.mean()), r.describe())
        assert float(diff[~taint].max()) <= 1e-11, (what, float(diff[~taint].max()), r.describe())
    else:
        assert float(diff.max()) <= 1e-11 * scale, (what, float(diff.max()), r.describe())


def compare_bound(r, sb, ref, exact_family=True):
    if r.dtype == "float32":
        assert abs(sb - ref) <= 1e-5 * ref, (sb, ref, r.describe())
    elif exact_family and r.ham in (0, 1) and IR.SCHEME_NAMES[r.scheme] in ("ENO2", "ENO3"):
        assert sb == ref, (sb, ref, r.describe())
    else:
        assert abs(sb - ref) <= 1e-13 * ref, (sb, ref, r.describe())


def ragged_tiles(dg, r):
    """The last tiled launch cut the grid into at least two chunks along axis 0 and two tiles along every other axis, none dividing its axis."""
    e = (C.c_int * 4)()
    _ffi.check(dg.lib.hj_last_tile(dg.ctx, e))
    for d in range(len(r.N)):
        assert 0 < e[d] < r.N[d] and r.N[d] % e[d] != 0, "axis %d: %d cells in pieces of %d\n%s" % (d, r.N[d], e[d], r.describe())


def done(r):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(r.symbol + "\n")


def rows(call):
    rs = [r for r in RECIPES if r.call == call]
    return pytest.mark.parametrize("r", rs, ids=[r.id for r in rs])


# ------------------------------------------------------------------------------------------------ the substep kernels
DIRECT32 = {}


def direct32(P, r, stage, dt, restrict=0):
    """direct_substep_kernel<float> on the same data: the fp32 instantiation that carries the oracle comparison (its own rows)."""
    key = (P.ham, P.N, P.periodic, r.scheme, stage, restrict)
    if key not in DIRECT32:
        with IR.environment(IR.knobs(HJ_FORCE_DIRECT=1)):
            dg = DeviceGrid(P.g, "float32")
        dg.bind_stream()
        y, y0 = tens(P.data, "float32"), tens(P.start, "float32")
        out = torch.empty_like(y)
        substep(dg, r, stage, dt, restrict, y, y0, out, 5)
        sb = bound(dg, 5)
        assert dg.lib.hj_last_kernel(dg.ctx) == b"direct_substep_kernel"
        DIRECT32[key] = (out, sb)
    return DIRECT32[key]


@rows("substep")
def test_substep_instantiation_against_its_reference(r):
    P = Problem.get(r.ham, r.N, r.periodic)
    ref_yd, ref_sb = P.oracle(r.scheme, r.dtype)
    dt = 0.5 * ref_sb
    dg = ctx_for(r, P.g)
    y, y0 = tens(P.data, r.dtype), tens(P.start, r.dtype)
    yn, y0n = P.arr("data", r.dtype), P.arr("start", r.dtype)
    name = IR.SCHEME_NAMES[r.scheme]
    is_direct = r.family == "direct_substep_kernel"
    stages = [r.stage] + ([_ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF] if is_direct else [])      # (the direct kernel takes its stage at run time)
    for k, stage in enumerate(stages):
        out = torch.empty_like(y)
        substep(dg, r, stage, dt, 0, y, y0, out, 1 + k)
        launched(dg, r)
        sb = bound(dg, 1 + k)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), r.describe()
        if r.tiled:
            # the launch really had several tiles and chunks (extents in the kernel's axis order: the marched axis, then the others)
            e = (C.c_int * 4)()
            _ffi.check(dg.lib.hj_last_tile(dg.ctx, e))
            marched = r.extra.get("marched_axis", 0)
            axes = [marched] + [d for d in range(len(r.N)) if d != marched]
            for kk, d in enumerate(axes):
                assert 0 < e[kk] < r.N[d] or d not in (marched,) + tuple(r.tiled_axes), (list(e), r.describe())
        ref = stage_of(stage, ref_yd, yn, y0n, dt)
        if r.dtype == "float64":
            compare_fp64(r, P, out.cpu().numpy(), ref, "stage %d" % stage)
            compare_bound(r, sb, ref_sb)
        elif is_direct:
            if r.ham in (0, 1) and name in ("ENO2", "ENO3"):
                # the float32 oracle, bit for bit (dt as the kernel converts it); the looser fp64 comparison stays beside it
                yd32, sb32 = P.oracle32(r.scheme)
                ref32 = stage_of(stage, yd32, P.data.astype(np.float32), P.start.astype(np.float32), np.float32(dt))
                got32 = out.cpu().numpy()
                assert ref32.dtype == np.float32 and np.array_equal(got32, ref32), (stage, int((got32 != ref32).sum()), r.describe())
                assert sb == sb32, (sb, sb32, r.describe())
            if stage == _ffi.STAGE_YDOT:
                fp32_close(out.cpu().numpy(), ref, name, "ydot")
            else:       # the state rule of test_fp32_builtin_systems_every_scheme_and_size_class
                diff = np.abs(out.cpu().numpy().astype(np.float64) - ref)
                scale = max(1.0, float(np.abs(ref).max()))
                if name.startswith("WENO"):
                    assert float(diff.max()) <= 2e-6 * scale, (stage, float(diff.max()), r.describe())
                else:
                    assert float(np.mean(diff > 2e-6 * scale)) <= 3e-3 and float(diff.max()) <= 1e-3 * scale, (stage, float(diff.max()), r.describe())
            compare_bound(r, sb, ref_sb)
        else:
            want, sbw = direct32(P, r, stage, dt)
            assert torch.equal(out, want), (float((out - want).abs().max()), float((out != want).float().mean()), r.describe())
            assert sb == sbw, (sb, sbw, r.describe())
        if stage == _ffi.STAGE_YDOT:
            # termRestrictUpdate's clamp rides in the same (flag-carrying) instantiation
            clamped, sbc = torch.empty_like(y), C.c_double()
            _ffi.check(dg.lib.hj_lf_term(dg.ctx, r.scheme, r.ham, _ffi.darr(PAR[r.ham]), 0., 1, dg.ptr(y), dg.ptr(clamped), C.byref(sbc)))
            launched(dg, r)
            torch.cuda.synchronize()
            assert torch.equal(clamped, torch.clamp(out, min=0.)) and sbc.value == sb, r.describe()
            assert bool((out < 0).any()) and bool((out > 0).any())          # the clamp selects on both sides
    if r.scheme == 2 and r.mode in (1, 2) and r.tiled and "marched_axis" not in r.extra:
        weno5_producer_step(r, P)
    done(r)


def oracle_rk3(P, dtype):
    """(t, y) after one odeCFL3 step of the intended WENO5 on the problem's data."""
    key = ("rk3", dtype)
    if key not in P.refs:
        P.refs[key] = O.ode_cfl_3(lambda tt, v: O.term_lax_friedrichs(P.og, P.osys, "WENO5", tt, v), [0., 1e9], P.arr("data", dtype).reshape(-1, 1), 0.8,
                                  single_step=True)
    return P.refs[key]


def compare_rk3(r, P, got):
    to, yo = oracle_rk3(P, r.dtype)
    diff = np.abs(got[0].cpu().numpy().astype(np.float64).reshape(-1, 1) - yo)
    scale = max(1.0, float(np.abs(yo).max()))
    if r.dtype == "float64":
        assert float(diff.max()) <= 1e-11 * scale and abs(got[1] - to) <= 1e-13 * to, (float(diff.max()), got[1], to, r.describe())
    else:
        assert float(diff.max()) <= 2e-6 * scale and abs(got[1] - to) <= 1e-5 * to, (float(diff.max()), got[1], to, r.describe())


def weno5_producer_step(r, P):
    """The epsilon rows of the intended WENO5.  Inside hj_rk_step a plain stage of this instantiation reduces max(D1^2) of its own output
    (FusedArgs::eps_part; eps_seam_kernel adds the seams) and the next stage folds those rows instead of running a pre-pass: one RK3
    step under the recipe's knobs (stage 1 is the MODE 1 instantiation, stages 2 and 3 the MODE 2 one) -- bit for bit the step whose
    epsilons come from the two-launch pre-pass (HJ_EPS_FUSE=0), and the oracle's step."""
    y = tens(P.data, r.dtype)
    with IR.environment(dict(r.env, HJ_EPS_FUSE_MIN_CELLS="0")):
        dg = DeviceGrid(P.g, r.dtype)
    dg.bind_stream()
    _ffi.check(dg.lib.hj_launch_record(dg.ctx, 1))
    got = rk_step(dg, r, 3, y)
    rec = launched(dg, r)
    assert any("eps_seam_kernel" in s for s in rec), (sorted(rec), r.describe())
    with IR.environment(dict(r.env, HJ_EPS_FUSE="0")):
        d2 = DeviceGrid(P.g, r.dtype)
    d2.bind_stream()
    _ffi.check(d2.lib.hj_launch_record(d2.ctx, 1))
    want = rk_step(d2, r, 3, y)
    rec2 = IR.read_record(d2.lib, d2.ctx)
    assert not any("eps_seam_kernel" in s for s in rec2), sorted(rec2)
    assert got[1:] == want[1:] and torch.equal(got[0], want[0]), (got[1:], want[1:], float((got[0] - want[0]).abs().max()), r.describe())
    compare_rk3(r, P, got)


# ------------------------------------------------------------------------------------------------ termNormal / termReinit / termConvection
def term_inputs(P, dtype):
    """speed, velocity components (an array along axis 0, scalars elsewhere) as the kernels of `dtype` see them."""
    nd = len(P.N)
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == "float32" else (lambda a: a)
    speed = rnd(0.5 + 0.3 * np.cos(P.og.xs[0]) * np.ones(P.N))
    vels = [rnd(np.sin(2 * P.og.xs[1]) * np.ones(P.N) + 0.2)] + [[0.3, -0.2, 0.5][d - 1] for d in range(1, nd)]
    return speed, vels


def term_oracle(P, kind, scheme, dtype):
    key = ("term", kind, scheme, dtype)
    if key not in P.refs:
        phi = P.arr("data", dtype)
        speed, vels = term_inputs(P, dtype)
        col = phi.reshape(-1, 1)
        if kind == 0:
            P.refs[key] = O.term_normal(P.og, speed, scheme, 0., col)
        elif kind == 1:
            P.refs[key] = O.term_reinit(P.og, phi, scheme, 0., col, 1)
        else:
            P.refs[key] = O.term_convection(P.og, vels, scheme, 0., col)
    return P.refs[key]


def term_call(dg, P, kind, sid, dtype):
    nd = len(P.N)
    speed, vels = term_inputs(P, dtype)
    y = tens(P.data, dtype)
    out, sb = torch.empty_like(y), C.c_double()
    if kind == 0:
        sp = tens(speed, dtype)
        _ffi.check(dg.lib.hj_term_normal(dg.ctx, sid, dg.ptr(y), dg.ptr(sp), 0.0, dg.ptr(out), C.byref(sb)))
    elif kind == 1:
        init = y.clone()
        _ffi.check(dg.lib.hj_term_reinit(dg.ctx, sid, dg.ptr(y), dg.ptr(init), 1, dg.ptr(out), C.byref(sb)))
    else:
        v0 = tens(vels[0], dtype)
        arrs = (C.c_void_p * nd)(*([v0.data_ptr()] + [None] * (nd - 1)))
        _ffi.check(dg.lib.hj_term_convection(dg.ctx, sid, dg.ptr(y), arrs, _ffi.darr([0.0] + vels[1:]), dg.ptr(out), C.byref(sb)))
    torch.cuda.synchronize()
    return out, sb.value


@rows("term")
def test_term_instantiation_against_the_oracle(r):
    nd = len(r.N)
    P = Problem.get(HAM_OF_DIM[nd], r.N, r.periodic)
    kind, scheme = r.extra["kind"], IR.SCHEME_NAMES[r.scheme]
    dg = ctx_for(r, P.g)
    out, sb = term_call(dg, P, kind, r.scheme, r.dtype)
    launched(dg, r)
    yo, sbo = term_oracle(P, kind, scheme, r.dtype)
    got = out.cpu().numpy().astype(np.float64).reshape(-1, 1)
    scale = max(1.0, float(np.abs(yo).max()))
    ra = np.abs(got - yo)
    if r.dtype == "float64":
        assert float(ra.max()) <= (1e-10 if kind == 1 else 1e-11) * scale, (float(ra.max()), r.describe())
        if kind == 1:
            phi = P.data
            from fuzz_terms import reinit_bound_without_noise_cells          # (imported for this helper only)
            sb_hi = reinit_bound_without_noise_cells(P.og, phi, phi, scheme, 1)
            assert sbo * (1 - 1e-12) <= sb <= sb_hi * (1 + 1e-12), (sb, sbo, sb_hi, r.describe())
        else:
            assert abs(sb - sbo) <= 1e-12 * abs(sbo), (sb, sbo, r.describe())
    else:
        # (termReinit's sign function and Godunov switches are discontinuous in the data: isolated cells may take the other branch in fp32)
        sc = float(np.abs(yo).max())
        assert abs(sb - sbo) <= 1e-4 * sbo, (sb, sbo, r.describe())
        assert np.mean(ra > 5e-4 * sc) <= (5e-3 if kind == 1 else 1e-4) and (kind == 1 or ra.max() <= 5e-4 * sc), (float(ra.max()), sc, r.describe())
    if r.family == "fused_substep_kernel":
        ragged_tiles(dg, r)
        # the tiled term launch: the same cell arithmetic as term_kernel, bit for bit
        with IR.environment(IR.knobs(HJ_TERM_TILED_FROM=-1)):
            d2 = DeviceGrid(P.g, r.dtype)
        d2.bind_stream()
        want, sbw = term_call(d2, P, kind, r.scheme, r.dtype)
        assert d2.lib.hj_last_kernel(d2.ctx) == b"term_kernel"
        assert torch.equal(out, want) and sb == sbw, (float((out - want).abs().max()), sb, sbw, r.describe())
    done(r)


# ------------------------------------------------------------------------------------------------ the second-order kernels
@rows("curv")
def test_curv_instantiation_against_the_restatement(r):
    from test_gpu_curvature import _grids, _phi, _close64, _close32, _dx_sum, _np, EPS32
    from test_gpu_trace_hessian import _forms, _round32, _abs_scale, _sd
    kind, nd, f32 = r.extra["kind"], len(r.N), r.dtype == "float32"
    g, og = _grids(r.N, r.periodic, ())
    phi = _phi(og)
    if f32:
        phi = phi.astype(np.float32).astype(np.float64)
    with IR.environment(r.env):
        dg = device_grid(g, r.dtype)
    _ffi.check(dg.lib.hj_launch_record(dg.ctx, 1))
    data = torch.as_tensor(phi, device="cuda", dtype=TDT[r.dtype])
    col = data.reshape(-1, 1)
    if kind == "curvature":
        k, m = L.curvatureSecond(g, data)
        k_ref, m_ref = CR.curvature_second(og, phi)
        if not f32:
            _close64(k, k_ref)
            _close64(m, m_ref)
        else:
            band = m_ref >= 0.5
            _close32(m, m_ref, phi, og, 1)
            d = np.abs(_np(k).astype(np.float64) - k_ref)[band]
            tol = 1e-5 * float(np.abs(k_ref[band]).max()) + 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, 2) / 0.5
            assert float(d.max()) <= tol, (float(d.max()), tol, r.describe())
    elif kind == "hessian":
        s, f = L.hessianSecond(g, data)
        s_ref, f_ref = CR.hessian_second(og, phi)
        for i in range(nd):
            (_close32(f[i], f_ref[i], phi, og, 1) if f32 else _close64(f[i], f_ref[i]))
            for j in range(i + 1):
                (_close32(s[i][j], s_ref[i][j], phi, og, 2) if f32 else _close64(s[i][j], s_ref[i][j]))
    elif kind == "laplacian":
        lap, ref = L.laplacianSecond(g, data), CR.laplacian_second(og, phi)
        (_close32(lap, ref, phi, og, 2) if f32 else _close64(lap, ref))
    elif kind == "centered":
        for d in range(nd):
            a, ref = L.centeredFirstSecond(g, data, d)[0], CR.centered_first_second(og, phi, d)
            (_close32(a, ref, phi, og, 1) if f32 else _close64(a, ref))
    elif kind == "term":
        b = 0.75 if f32 else 0.5 + 0.25 * np.cos(og.xs[0])
        ydot, sb, _ = L.termCurvature(0.0, col, L.Bundle(dict(grid=g, b=b if f32 else torch.as_tensor(b, device="cuda"), curvatureFunc=L.curvatureSecond)))
        want, sb_want = CR.term_curvature(og, phi, b)
        if not f32:
            _close64(ydot, want)
        else:
            _, m_ref = CR.curvature_second(og, phi)
            band = (m_ref >= 0.5).reshape(-1, 1)
            d = np.abs(_np(ydot).astype(np.float64) - want)[band]
            tol = 1e-5 * float(np.abs(want[band]).max()) + 0.75 * float(m_ref.max()) * 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, 2) / 0.5
            assert float(d.max()) <= tol, (float(d.max()), tol, r.describe())
        assert abs(sb - sb_want) <= 1e-13 * sb_want, (sb, sb_want, r.describe())
    else:
        name, Lg, Rg, Lw, Rw, all_scalar = _forms(og)[0 if kind == "trace_scalar" else 1]
        if f32:
            Lw, Rw = _round32(Lw, not all_scalar), _round32(Rw, not all_scalar)
        want, sb_want = TR.term_trace_hessian(og, phi, Lw, Rw)
        ydot, sb, _ = L.termTraceHessian(0.0, col, _sd(g, Lg, Rg))
        if not f32:
            _close64(ydot, want)
        else:
            tol = 1e-5 * float(np.abs(want).max()) + 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, 2) * _abs_scale(Lw, Rw)
            err = float(np.abs(_np(ydot).astype(np.float64) - want).max())
            assert err <= tol, (err, tol, r.describe())
        assert abs(sb - sb_want) <= 1e-12 * sb_want, (sb, sb_want, r.describe())
    launched(dg, r)
    done(r)


# ------------------------------------------------------------------------------------------------ the fused launches
def rk_step(dg, r, order, y, restrict=0):
    nxt, w1 = torch.empty_like(y), torch.empty_like(y)
    tout, dtout = C.c_double(), C.c_double()
    _ffi.check(dg.lib.hj_rk_step(dg.ctx, order, r.scheme, r.ham, _ffi.darr(PAR[r.ham]), 0., 1e9, 0.8, 1e300, restrict, dg.ptr(y), dg.ptr(nxt),
                                 dg.ptr(nxt) if order == 3 else dg.ptr(w1), dg.ptr(w1), C.byref(tout), C.byref(dtout)))
    torch.cuda.synchronize()
    return nxt, tout.value, dtout.value


@rows("coop")
def test_coop_instantiation_equals_the_stage_launches(r):
    """One cooperative launch per odeCFL2 / odeCFL3 step against the stage launches of the direct kernel it replaces: the same bits, times
    and step sizes -- plain, with termRestrictUpdate's clamp, and with the post-step minimum folded into the last stage.  (The grid needs
    far fewer workgroups than the device keeps resident: a launch that waits for every workgroup to be resident is not run at capacity
    beside other work on the same device.)"""
    P = Problem.get(r.ham, r.N, r.periodic)
    y = tens(P.data, r.dtype)
    cases = [(3, 0, 0), (2, 0, 0), (3, -1, 0), (2, 1, 0), (3, 0, 1), (2, 0, 1)]          # (order, clamp, post-step operator: 1 = min with the step's start)
    res = {}
    for coop in ("1", "0"):
        with IR.environment(dict(r.env, HJ_COOP=coop)):
            dg = DeviceGrid(P.g, r.dtype)
        dg.bind_stream()
        _ffi.check(dg.lib.hj_launch_record(dg.ctx, 1))
        for case in cases:
            _ffi.check(dg.lib.hj_ctx_set_post_step(dg.ctx, case[2]))
            res[(coop, case)] = rk_step(dg, r, case[0], y, case[1])
            rec = IR.read_record(dg.lib, dg.ctx)
            if coop == "1":
                # (besides it only the static step bound's kernel on the first step: no stage launch)
                assert r.symbol in rec and not any("substep_kernel" in s or "fused" in s for s in rec), (case, sorted(rec), r.describe())
            else:
                assert not any("coop_rk_kernel" in s for s in rec) and dg.lib.hj_last_kernel(dg.ctx) == b"direct_substep_kernel", sorted(rec)
        _ffi.check(dg.lib.hj_ctx_set_post_step(dg.ctx, 0))
    for case in cases:
        got, want = res[("1", case)], res[("0", case)]
        assert got[1:] == want[1:], (case, got[1:], want[1:], r.describe())
        assert torch.equal(got[0], want[0]), (case, float((got[0] - want[0]).abs().max()), r.describe())
        assert bool(torch.isfinite(want[0]).all()) and float((want[0] - y).abs().max()) > 1e-6
    plain, clamped, post = res[("0", (3, 0, 0))][0], res[("0", (3, -1, 0))][0], res[("0", (3, 0, 1))][0]
    assert not torch.equal(plain, clamped) and torch.equal(post, torch.minimum(plain, y)) and not torch.equal(post, plain)      # the flags did something
    done(r)


@rows("stage12")
def test_stage_fused_instantiation_equals_two_stage_launches(r):
    P = Problem.get(r.ham, r.N, r.periodic)
    dt = 0.5 * P.oracle(3, "float64")[1]          # (a step size only: the as-shipped WENO5's bound, computed once per grid)
    dg = ctx_for(r, P.g)
    with IR.environment(IR.knobs()):
        d2 = DeviceGrid(P.g, r.dtype)
    d2.bind_stream()
    y = tens(P.data, r.dtype)
    for ca, cb, stage2 in ((0.75, 0.25, _ffi.STAGE_RK3_HALF), (0.5, 0.5, _ffi.STAGE_RK2_FULL)):
        out, a, b = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        _ffi.check(dg.lib.hj_rk_stage12(dg.ctx, r.scheme, r.ham, _ffi.darr(PAR[r.ham]), dt, ca, cb, dg.ptr(y), dg.ptr(out), 2))
        launched(dg, r)
        ragged_tiles(dg, r)
        sb = bound(dg, 2)
        substep(d2, r, _ffi.STAGE_EULER, dt, 0, y, None, a, 3)
        substep(d2, r, stage2, dt, 0, a, y, b, 4)
        sbw = bound(d2, 3)
        torch.cuda.synchronize()
        assert torch.equal(out, b), (ca, float((out - b).abs().max()), float((out != b).float().mean()), r.describe())
        assert sb == sbw, (sb, sbw, r.describe())
        assert bool(torch.isfinite(out).all()) and float((out - y).abs().max()) > 1e-6
    done(r)


# ------------------------------------------------------------------------------------------------ the helper kernels
def close(a, ref, tol=1e-11, what=""):
    from test_gpu_parity import close as _close
    _close(a, ref, tol, what)


def h_upwind(r, P, dg):
    """hj_upwind (one dimension per launch) / hj_lf_split_begin (all dimensions in one): derivL, derivR and their four extrema per dimension."""
    nd, name = len(r.N), IR.SCHEME_NAMES[r.scheme]
    phi = P.arr("data", r.dtype)
    y = tens(P.data, r.dtype)
    dL, dR = [torch.empty_like(y) for _ in range(nd)], [torch.empty_like(y) for _ in range(nd)]
    mm = (C.c_double * (4 * nd))()
    if r.extra["entry"] == "hj_upwind":
        for d in range(nd):
            m4 = (C.c_double * 4)()
            _ffi.check(dg.lib.hj_upwind(dg.ctx, r.scheme, d, dg.ptr(y), dg.ptr(dL[d]), dg.ptr(dR[d]), m4))
            mm[4 * d:4 * d + 4] = list(m4)
    else:
        pl, pr = (C.c_void_p * nd)(*[t.data_ptr() for t in dL]), (C.c_void_p * nd)(*[t.data_ptr() for t in dR])
        _ffi.check(dg.lib.hj_lf_split_begin(dg.ctx, r.scheme, dg.ptr(y), pl, pr, mm))
    torch.cuda.synchronize()
    for d in range(nd):
        oL, oR = O.SCHEMES[name](P.og, phi, d)
        for got, ref, w in ((dL[d], oL, "L"), (dR[d], oR, "R")):
            if r.dtype == "float64":
                close(got.cpu().numpy(), ref, what="%s d%d" % (w, d))
            else:
                fp32_close(got.cpu().numpy(), ref, name, "%s d%d" % (w, d))
        ref4 = [oL.min(), oL.max(), oR.min(), oR.max()]
        got4 = [float(dL[d].min()), float(dL[d].max()), float(dR[d].min()), float(dR[d].max())]
        for k in range(4):
            # the reduction against the oracle (fp64) and, exactly, against the arrays the kernel itself wrote
            assert mm[4 * d + k] == got4[k], (d, k, mm[4 * d + k], got4[k], r.describe())
            if r.dtype == "float64":
                assert abs(mm[4 * d + k] - ref4[k]) <= 1e-11 * max(1, abs(ref4[k])), (d, k, r.describe())


def h_max_d1sq(r, P, dg):
    nd = len(r.N)
    y = tens(P.data, r.dtype)
    out = torch.zeros(4, device="cuda", dtype=TDT[r.dtype])
    _ffi.check(dg.lib.hj_max_d1sq(dg.ctx, dg.ptr(y), dg.ptr(out)))
    torch.cuda.synchronize()
    phi = P.arr("data", r.dtype)
    for d in range(nd):
        ref = float(O.max_d1_squared(P.og, phi, d))
        assert abs(float(out[d]) - ref) <= (1e-5 if r.dtype == "float32" else 1e-13) * ref, (d, float(out[d]), ref, r.describe())


def h_rk_step_weno5(r, P, dg):
    """One RK3 step of the intended WENO5 through hj_rk_step: the epsilon of every stage comes from the one-launch pre-pass
    (max_d1sq_kernel<.., 1024>: rows the consumer folds) or is reduced inside the producing launch (eps_seam_kernel) -- against the oracle's
    step, and bit for bit against the two-launch pre-pass (HJ_EPS_FUSE=0)."""
    y = tens(P.data, r.dtype)
    got = rk_step(dg, r, 3, y)
    rec = launched(dg, r)
    assert any("max_d1sq_kernel" in s for s in rec) or not r.symbol.count("max_d1sq"), sorted(rec)
    with IR.environment(dict(r.env, HJ_EPS_FUSE="0")):
        d2 = DeviceGrid(P.g, r.dtype)
    d2.bind_stream()
    want = rk_step(d2, r, 3, y)
    assert got[1:] == want[1:] and torch.equal(got[0], want[0]), (got[1:], want[1:], float((got[0] - want[0]).abs().max()), r.describe())
    compare_rk3(r, P, got)
    return "checked"


def h_static_bound(r, P, dg):
    sb = C.c_double()
    _ffi.check(dg.lib.hj_static_step_bound(dg.ctx, r.ham, _ffi.darr(PAR[r.ham]), C.byref(sb), None))
    ref = P.oracle(3, r.dtype)[1]          # alpha of the built-in systems does not read the data: termLaxFriedrichs' bound is the static one
    assert abs(sb.value - ref) <= (1e-5 if r.dtype == "float32" else 1e-13) * ref, (sb.value, ref, r.describe())


def h_elementwise(r, P, dg):
    """hj_rk_combine, hj_minmax_with, hj_any_nan, hj_ghost, hj_lf_split_end: NumPy on the same values (test_fp32_helper_kernels_through_the_c_abi)."""
    entry, tdt = r.extra["entry"], TDT[r.dtype]
    ndt = np.float32 if r.dtype == "float32" else np.float64
    rng = np.random.default_rng(9)
    if entry == "hj_rk_combine":
        x0, yy, zz = (rng.standard_normal(4097).astype(ndt) for _ in range(3))
        tx, ty, tz = (torch.as_tensor(v, device="cuda") for v in (x0, yy, zz))
        dt = ndt(0.0123)
        refs = {1: yy + dt * zz, 2: ndt(0.25) * (ndt(3) * x0 + (yy + dt * zz)), 3: ndt(1 / 3) * (x0 + ndt(2) * (yy + dt * zz)), 4: ndt(0.5) * (x0 + (yy + dt * zz))}
        for mode, ref in refs.items():
            out = torch.empty_like(tx)
            _ffi.check(dg.lib.hj_rk_combine(dg.ctx, mode, float(dt), dg.ptr(tx), dg.ptr(ty), dg.ptr(tz), dg.ptr(out), out.numel()))
            # (fp64: the kernel may contract y + dt*z where NumPy rounds twice -- an ulp or two of values below 8)
            assert float(np.abs(out.cpu().numpy() - ref).max()) <= (1e-6 if r.dtype == "float32" else 1e-14), (mode, r.describe())
    elif entry == "hj_minmax_with":
        a, b = tens(P.data, r.dtype), tens(P.start, r.dtype)
        for op, ref in ((_ffi.OP_MIN, torch.minimum(a, b)), (_ffi.OP_MAX, torch.maximum(a, b)), (_ffi.OP_MAX_NEG, torch.maximum(a, -b))):
            w = a.clone()
            _ffi.check(dg.lib.hj_minmax_with(dg.ctx, op, dg.ptr(w), dg.ptr(b), w.numel()))
            assert torch.equal(w, ref), (op, r.describe())
    elif entry == "hj_any_nan":
        a, has = tens(P.data, r.dtype), C.c_int(-1)
        _ffi.check(dg.lib.hj_any_nan(dg.ctx, dg.ptr(a), a.numel(), C.byref(has)))
        assert has.value == 0
        a.view(-1)[a.numel() - 3] = float("nan")
        _ffi.check(dg.lib.hj_any_nan(dg.ctx, dg.ptr(a), a.numel(), C.byref(has)))
        assert has.value == 1
    elif entry == "hj_ghost":
        x = P.arr("data", r.dtype)
        for d in range(len(r.N)):
            for w in (1, 3):
                shape = list(r.N)
                shape[d] += 2 * w
                out = torch.empty(shape, device="cuda", dtype=tdt)
                _ffi.check(dg.lib.hj_ghost(dg.ctx, d, w, dg.ptr(tens(x, r.dtype)), dg.ptr(out)))
                ref = O.add_ghost_periodic(x, d, w) if d in r.periodic else O.add_ghost_extrapolate(x, d, w)
                got = out.cpu().numpy().astype(np.float64)
                if r.dtype == "float64":
                    assert np.array_equal(got, ref), (d, w, r.describe())
                else:       # x0 + k (x0 - x1) in fp32 for k <= 3: a handful of roundings of eps32 = 1.2e-7 each
                    assert float(np.abs(got - ref).max()) <= 1e-6 * max(1.0, float(np.abs(ref).max())), (d, w, r.describe())
    else:       # hj_lf_split_end: out = -(ham - sum_d 0.5 (R_d - L_d) alpha_d); the bound from the array-valued alphas
        nd = len(r.N)
        arrs = [rng.standard_normal(r.N).astype(ndt) for _ in range(2 * nd + 2)]
        dL, dR, ham, al0 = arrs[:nd], arrs[nd:2 * nd], arrs[2 * nd], np.abs(arrs[2 * nd + 1]) + ndt(0.1)
        tl, tr_ = [torch.as_tensor(v, device="cuda") for v in dL], [torch.as_tensor(v, device="cuda") for v in dR]
        th, ta = torch.as_tensor(ham, device="cuda"), torch.as_tensor(al0, device="cuda")
        scal = [0.0] + [0.5 + 0.25 * d for d in range(1, nd)]
        out, sb = torch.empty_like(th), C.c_double()
        pl, pr = (C.c_void_p * nd)(*[t.data_ptr() for t in tl]), (C.c_void_p * nd)(*[t.data_ptr() for t in tr_])
        pa = (C.c_void_p * nd)(*([ta.data_ptr()] + [None] * (nd - 1)))
        _ffi.check(dg.lib.hj_lf_split_end(dg.ctx, pl, pr, pa, _ffi.darr(scal), dg.ptr(th), dg.ptr(out), C.byref(sb), None))
        torch.cuda.synchronize()
        diss = sum((ndt(0.5) * (dR[d] - dL[d])) * (al0 if d == 0 else ndt(scal[d])) for d in range(nd))
        ref = -(ham - diss)
        err = float(np.abs(out.cpu().numpy() - ref).max())
        assert err <= (1e-5 if r.dtype == "float32" else 1e-14) * max(1.0, float(np.abs(ref).max())), (err, r.describe())
        dx = np.asarray(P.og.dx, dtype=np.float64).ravel()
        sbw = 1.0 / (float(al0.max()) / dx[0] + sum(scal[d] / dx[d] for d in range(1, nd)))
        assert abs(sb.value - sbw) <= 1e-13 * sbw, (sb.value, sbw, r.describe())


def h_range_step(r, P, dg0):
    """bound_to_dt_kernel: deltaT formed on the device from the bound pass of a local Lax-Friedrichs step with a Hamiltonian whose alpha reads
    the costate range (tests/fuzz_parity.py, case_range): two odeCFL3 steps against the oracle."""
    from test_gpu_round5 import BurgersDriftLocal, _burgers_src
    dim, par0 = 2, 0.7
    N, pd = [41, 37], [1]
    lo, hi = [-1.0] * dim, [1.0, 1.0 - 2.0 / N[1]]
    g = L.createGrid(np.asarray(lo).reshape(-1, 1), np.asarray(hi).reshape(-1, 1), np.asarray(N, dtype=np.int64).reshape(-1, 1), pd)
    og = O.Grid(lo, hi, N, pd)
    d0 = O.shape_sphere(og, None, 0.5) + 0.1 * np.sin(3 * og.xs[0]) * np.cos(2 * og.xs[1]) + 0.02 * np.random.default_rng(2).standard_normal(N)
    reg = L.register_native_hamiltonian("burgers_drift_2d_instantiations", dim, _burgers_src(dim), nparams=1)
    sys_ = reg(g, [par0], hamiltonian=lambda s, t, data, p, sd: BurgersDriftLocal(g, par0).hamiltonian(t, data, p, sd),
               dissipation=lambda s, t, data, dmin, dmax, sd, dm: BurgersDriftLocal(g, par0).dissipation(t, data, dmin, dmax, sd, dm))
    sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationLLF, CoStateCalc=L.upwindFirstWENO5))
    op = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on')))
    with IR.environment(r.env):
        dg = device_grid(g, "float64")
    _ffi.check(dg.lib.hj_launch_record(dg.ctx, 1))
    y = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    yo, t, to = d0.reshape(-1, 1), 0., 0.
    for _ in range(2):
        t, y, _ = L.odeCFL3(L.termLaxFriedrichs, [t, 10.], y, op, sd)
        to, yo = O.ode_cfl_3(lambda tt, yy: O.term_lax_friedrichs(og, BurgersDriftLocal(og, par0), "WENO5_ASSHIPPED", tt, yy, diss="llf"), [to, 10.], yo, 0.8,
                             single_step=True)
    err = float(np.abs(y.cpu().numpy() - yo).max()) / max(1.0, float(np.abs(yo).max()))
    assert err <= 1e-11 and abs(t - to) <= 1e-12 * to, (err, t, to, r.describe())
    return dg


HELPERS = {"hj_upwind": h_upwind, "hj_lf_split_begin": h_upwind, "hj_max_d1sq": h_max_d1sq, "rk_step_weno5_rows": h_rk_step_weno5,
           "rk_step_weno5_fused": h_rk_step_weno5, "hj_static_step_bound": h_static_bound, "hj_rk_step_range": h_range_step}


@rows("helper")
def test_helper_instantiation_against_its_reference(r):
    P = Problem.get(r.ham, r.N, r.periodic)
    dg = ctx_for(r, P.g)
    other = HELPERS.get(r.extra["entry"], h_elementwise)(r, P, dg)          # (None: this ctx; a ctx: that one; "checked": the helper read the record)
    if other != "checked":
        launched(other or dg, r)
    done(r)
