"""GPU: the float instantiations against the oracle's float32 mode (oracle/hj_oracle.py, "WORKING PRECISION"), through the C ABI
and the Python front end, on the two data sets of tests/fp32_cases.py: sphere + noise, and the symmetric sphere on which 20-60 % of
the ENO3 cells sit on selector ties (tests/test_oracle_fp32.py asserts that share).

ENO2 / ENO3 -- array_equal, ties and NaN patterns included; step bounds ==:
  direct_substep_kernel<float> (hj_rk_substep, HJ_FORCE_DIRECT) for the Dubins car and the double integrator, every stage id;
  termLaxFriedrichs and one odeCFL1/2/3 single step through the front end (state array_equal, t ==);
  hidim_substep_kernel<float> (hjh_substep, hjh_step_bound) for Plane5D and DubinsPair6D, every stage; hidim_upwind_kernel<float>;
  batch_substep_kernel<float> (hjb_substep), three Dubins problems with different parameters;
  eval_costate == eval_u over the derivative arrays (2-D to 4-D: computeGradients' own; 5-D: the ORACLE's float32 arrays).
Not bitwise, with the reason (profiles/fp32_parity.txt lists them):
  the 4-D double pendulum -- a build-defined Hamiltonian evaluated in factored form (HamDoublePendulum::row, csrc/hj_device.h): its
    costates ARE the oracle's bits (same exact ENO code), so every cell, ties included, is held to a derived bound on the rounding of
    the Hamiltonian alone (pendulum_bound below);
  upwind_all_kernel / upwind_kernel (computeGradients, upwindFirstENO2|ENO3 at 2-D to 4-D) -- they form the selected candidate through
    upwind<>, where the compiler contracts D1 + dx D2 (+ c D3) into FMAs (documented in include/hj_mi355x.h); the tables and the
    selectors are uncontracted, so the SAME candidate is chosen: held on every cell to the contraction bound against the float32
    oracle (fma_bound below) and, margin-masked, to the derived C bound of tests/fp32_cases.py against the fp64 oracle.
As-shipped and intended WENO5 keep contracted / refactored forms: e_ker = max|kernel - oracle64| <= R * e_ref + tiny with
e_ref = max|oracle32 - oracle64|, R fixed from the ratios measured on the MI355X (profiles/fp32_parity.txt)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, _hffi, hidim, eval_u, eval_costate  # noqa: E402
from levelsetpy_amd.context import DeviceGrid, device_grid  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402
import fp32_cases as F  # noqa: E402
import hidim_cases as HC  # noqa: E402
import instantiation_recipes as IR  # noqa: E402
import query_ref as Q  # noqa: E402

SID = {"ENO2": _ffi.ENO2, "ENO3": _ffi.ENO3, "WENO5_ASSHIPPED": _ffi.WENO5_ASSHIPPED, "WENO5": _ffi.SCHEME_IDS["WENO5"]}
DERIV = {"ENO2": L.upwindFirstENO2, "ENO3": L.upwindFirstENO3, "WENO5_ASSHIPPED": L.upwindFirstWENO5, "WENO5": L.upwindFirstWENO5Intended}
STAGES = {"YDOT": _ffi.STAGE_YDOT, "EULER": _ffi.STAGE_EULER, "RK3_HALF": _ffi.STAGE_RK3_HALF, "RK3_FULL": _ffi.STAGE_RK3_FULL,
          "RK2_FULL": _ffi.STAGE_RK2_FULL}
ENO = ["ENO2", "ENO3"]
WENO = ["WENO5_ASSHIPPED", "WENO5"]
# R of the module docstring: twice the largest e_ker / e_ref measured on the MI355X over every WENO case of this file, rounded up to a
# power of two (profiles/fp32_parity.txt holds the table)
R_WENO = 8.0
SYSTEM_OF_DIM = {2: (lambda g, par: L.DoubleIntegrator(g, *par), (1.25,)), 3: (lambda g, par: L.DubinsVehicleRel(g, *par), (1, 1)),
                 4: (lambda g, par: L.DoublePendulum4D(g, *par), (1.0,))}


def product_grid(c):
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col(c.lo, np.float64), col(c.hi, np.float64), col(c.N, np.int64), c.pd if c.pd else None)


def dev32(a):
    assert a.dtype == np.float32
    return torch.as_tensor(np.array(a), device="cuda")


def stage_ref(stage, y, y0, dt, ydot):
    """odeCFLn's stage expressions (ode_cfl_3.py:151-241, ode_cfl_2.py:201) in the arrays' own precision; dt as the kernel converts it."""
    e = y + y.dtype.type(dt) * ydot
    if stage == "YDOT":
        return ydot
    if stage == "EULER":
        return e
    if stage == "RK3_HALF":
        return 0.25 * (3 * y0 + e)
    if stage == "RK3_FULL":
        return (1 / 3) * (y0 + 2 * e)
    return 0.5 * (y0 + e)


def equal(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = np.asarray(ref).reshape(got.shape)
    assert got.dtype == np.float32 and ref.dtype == np.float32, (what, got.dtype, ref.dtype)
    bad = int(np.sum(~((got == ref) | (np.isnan(got) & np.isnan(ref)))))
    assert bad == 0, "%s: %d of %d cells differ, max |diff| %.3g" % (what, bad, got.size, float(np.nanmax(np.abs(got.astype(np.float64) - ref))))


def weno_parity(what, got, ref32, ref64):
    """e_ker <= R e_ref + tiny (module docstring); tiny: one float32 ulp of the largest reference value (guards e_ref == 0)."""
    got = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64).reshape(-1)
    ref64 = np.asarray(ref64, dtype=np.float64).reshape(-1)
    e_ref = float(np.abs(np.asarray(ref32, dtype=np.float64).reshape(-1) - ref64).max())
    e_ker = float(np.abs(got - ref64).max())
    tiny = F.EPS32 * float(np.abs(ref64).max())
    print("fp32-parity %-58s e_ref %.3e  e_ker %.3e  ratio %.3f" % (what, e_ref, e_ker, e_ker / e_ref if e_ref else float("inf")))
    assert e_ker <= R_WENO * e_ref + tiny, (what, e_ker, e_ref)


def direct_ctx(g):
    with IR.environment(IR.knobs(HJ_FORCE_DIRECT=1)):
        dg = DeviceGrid(g, "float32")
    dg.bind_stream()
    return dg


def rk_substep(dg, sid, ham, par, stage, dt, y, y0, slot=1):
    out, sb = torch.full_like(y, float("nan")), C.c_double()
    _ffi.check(dg.lib.hj_rk_substep(dg.ctx, sid, ham, _ffi.darr(par), 0., stage, dt, 0, dg.ptr(y), dg.ptr(y0) if stage >= _ffi.STAGE_RK3_HALF else None,
                                    dg.ptr(out), slot, 0, dg.shape[0]))
    _ffi.check(dg.lib.hj_read_step_bound(dg.ctx, slot, C.byref(sb), None))
    torch.cuda.synchronize()
    assert dg.lib.hj_last_kernel(dg.ctx) == b"direct_substep_kernel"
    return out, sb.value


# ------------------------------------------------------------------------------------------ hj_rk_substep: the direct kernel
def pendulum_bound(c, what, scheme):
    """|ydot_kernel - ydot_oracle32| per cell for the 4-D pendulum, whose costates p_i (centred) and half jumps h_i are the SAME bits in
    both (exact ENO): ydot = -(sum p_i f_i + u(|p_1| + |p_3|) - sum h_i alpha_i), alpha_i = |f_i| + u [i in 1, 3].  Only f_1, f_3 and the
    sums differ.  F = w1^2 + w2^2 + 3 g bounds the sum of the moduli of f's terms (den = 2 - cos^2 >= 1).  Each evaluation of f carries at
    most: sin / cos of the angle difference to 8 u absolute either way (float32 sin of a difference rounded at up to 2 pi, or
    s2 c1 - c2 s1 from tables with u each) times coefficients <= F, twice (s and c); the denominator's relative 16 u; ten roundings of
    products / sums: (16 + 16 + 10) u F = 42 u F; two evaluations 84 u F <= 50 eps32 F.  The products and the two sums over four axes add
    at most 12 roundings of terms <= (|p_i| + |h_i|)(|f_i| + u) each in either evaluation: 24 u = 12 eps32.  With |f_i| + u <= F + u:
        bound = 62 eps32 (F_max + u) sum_i max_cells(|p_i| + |h_i|)."""
    d = c.deriv(what, scheme, 32)
    w = float(max(abs(c.lo[1]), abs(c.hi[1]))), float(max(abs(c.lo[3]), abs(c.hi[3])))
    Fmax = w[0] ** 2 + w[1] ** 2 + 3 * O.DoublePendulum4D.G
    s = sum(float(np.max(np.abs(0.5 * (a.astype(np.float64) + b)) + np.abs(0.5 * (b.astype(np.float64) - a)))) for a, b in d)
    return 62 * F.EPS32 * (Fmax + 1.0) * s


@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", ENO)
@pytest.mark.parametrize("nd,per", [(3, True), (2, False), (4, False)], ids=["dubins", "integrator", "pendulum"])
def test_direct_kernel_float_every_stage_is_the_float32_oracle(nd, per, scheme, what):
    c = F.Case.get(nd, per)
    g = product_grid(c)
    ham, par = SYSTEM_OF_DIM[nd][0](g, SYSTEM_OF_DIM[nd][1]).native()
    yd32, sb32 = c.term(what, scheme, 32)
    y, y0 = c.values(what, 32), c.values(what, 32, start=True)
    dt = 0.8 * sb32
    dg = direct_ctx(g)
    for k, (stage, sid) in enumerate(STAGES.items()):
        out, sb = rk_substep(dg, SID[scheme], ham, par, sid, dt, dev32(y), dev32(y0), 1 + k % 4)
        ref = stage_ref(stage, y, y0, dt, yd32)
        if nd != 4:
            equal(out, ref, "%s %s %s" % (what, scheme, stage))
            assert sb == sb32, (sb, sb32)
        else:
            b = pendulum_bound(c, what, scheme)
            if stage != "YDOT":             # the stage expressions are the same operations: dt * (the ydot bound) and a few ulps of the operands
                b = dt * b + 8 * F.EPS32 * (3 * float(np.abs(y0).max()) + float(np.abs(y).max()) + dt * float(np.abs(yd32).max()))
            err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
            print("pendulum %s %s %s: error / bound %.3g" % (what, scheme, stage, err / b))
            assert err <= b, (stage, err, b)
            assert abs(sb - sb32) <= 50 * F.EPS32 * sb32, (sb, sb32)          # max|f_i| to 50 eps32 F (pendulum_bound)


@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", ENO)
@pytest.mark.parametrize("nd,per", [(3, True), (2, False)], ids=["dubins", "integrator"])
def test_front_end_term_and_one_step_of_every_order(nd, per, scheme, what, monkeypatch):
    """termLaxFriedrichs' ydot and stepBound, then odeCFL1/2/3 single steps on float32 tensors (the product's default direct-kernel
    threshold: the suite runs with HJ_DIRECT_BELOW=0)."""
    monkeypatch.setenv("HJ_DIRECT_BELOW", "140000")
    c = F.Case.get(nd, per)
    g = product_grid(c)
    sys_ = SYSTEM_OF_DIM[nd][0](g, SYSTEM_OF_DIM[nd][1])
    sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationGLF, CoStateCalc=DERIV[scheme]))
    y = c.values(what, 32).reshape(-1, 1)
    yd32, sb32 = c.term(what, scheme, 32)
    f, sb, _ = L.termLaxFriedrichs(0., dev32(y), sd)
    dgc = device_grid(g, "float32")
    assert dgc.lib.hj_last_kernel(dgc.ctx) == b"direct_substep_kernel"
    equal(f, yd32.reshape(-1, 1), "termLaxFriedrichs")
    assert sb == sb32, (sb, sb32)
    op = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on')))
    term32 = lambda tt, v: O.term_lax_friedrichs(c.og32, c.system(32), scheme, tt, v)       # noqa: E731
    for ode, oode in ((L.odeCFL1, O.ode_cfl_1), (L.odeCFL2, O.ode_cfl_2), (L.odeCFL3, O.ode_cfl_3)):
        t, y1, _ = ode(L.termLaxFriedrichs, [0., 10.], dev32(y), op, sd)
        tr, yr = oode(term32, [0., 10.], y, 0.8, single_step=True, dtype=np.float32)
        equal(y1, yr, oode.__name__)
        assert float(t) == float(tr), (oode.__name__, t, tr)


# ------------------------------------------------------------------------------------------ 5-D / 6-D
class HiCase(object):
    cache = {}

    def __init__(self, name):
        gmin, gmax, N, pd = HC.limits(name)
        col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
        self.name = name
        self.g = L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)
        self.og = {64: O.Grid(gmin, gmax, N, pd), 32: O.Grid(gmin, gmax, N, pd, dtype=np.float32)}
        self.shape = self.og[64].shape
        self.sys = (L.Plane5D if self.g.dim == 5 else L.DubinsPair6D)(self.g, **HC.PARAMS[name])
        self.osys = {p: HC.oracle_system(name, self.og[p], **HC.PARAMS[name]) for p in (32, 64)}
        self.ham, self.par = self.sys.native()
        mid = [0.5 * (a + b) for a, b in zip(gmin, gmax)]
        sphere = O.shape_sphere(self.og[64], mid, 1.0)
        rng = np.random.default_rng(1)
        self.data = {"noisy": (sphere + 0.05 * rng.standard_normal(self.shape)).astype(np.float32), "symmetric": sphere.astype(np.float32)}
        self.start = {k: (v.astype(np.float64) + 0.03 * np.cos(2 * self.og[64].xs[0])).astype(np.float32) for k, v in self.data.items()}
        self._refs = {}

    @classmethod
    def get(cls, name):
        if name not in cls.cache:
            cls.cache[name] = cls(name)
        return cls.cache[name]

    def values(self, what, prec):
        return self.data[what] if prec == 32 else self.data[what].astype(np.float64)

    def term(self, what, scheme, prec):
        key = ("term", what, scheme, prec)
        if key not in self._refs:
            yd, sb = O.term_lax_friedrichs(self.og[prec], self.osys[prec], scheme, 0.0, self.values(what, prec).reshape(-1))
            self._refs[key] = (yd.reshape(self.shape), sb)
        return self._refs[key]

    def deriv(self, what, scheme, prec):
        key = ("deriv", what, scheme, prec)
        if key not in self._refs:
            self._refs[key] = [F.OFN[scheme](self.og[prec], self.values(what, prec), d) for d in range(self.g.dim)]
        return self._refs[key]


@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", ENO + ["WENO5_ASSHIPPED"])
@pytest.mark.parametrize("name", ["plane5d", "pair6d"])
def test_hidim_substep_float_every_stage_and_the_step_bound(name, scheme, what):
    c = HiCase.get(name)
    yd32, sb32 = c.term(what, scheme, 32)
    hg = hidim.hi_grid(c.g, "float32")
    sb = hg.step_bound(c.ham, c.par)
    assert sb == sb32, (sb, sb32)
    dt = 0.8 * sb32
    y, y0 = c.data[what], c.start[what]
    src, y0d = dev32(y), dev32(y0)
    for stage, sid in STAGES.items():
        out = torch.full(c.shape, float("nan"), dtype=torch.float32, device="cuda")
        hidim._substep(hg, SID[scheme], c.ham, c.par, sid, 0, src, y0d if sid >= _ffi.STAGE_RK3_HALF else None, out, dt)
        assert _hffi.last_kernel() == _hffi.kernel_name("float32", c.ham, SID[scheme])
        if scheme in ENO:
            equal(out, stage_ref(stage, y, y0, dt, yd32), "%s %s %s %s" % (name, what, scheme, stage))
        elif stage == "YDOT":
            weno_parity("hidim_substep %s %s %s" % (name, what, scheme), out, yd32, c.term(what, scheme, 64)[0])


@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", ENO + ["WENO5_ASSHIPPED"])
@pytest.mark.parametrize("name", ["plane5d", "pair6d"])
def test_hidim_derivative_kernel_float(name, scheme, what):
    c = HiCase.get(name)
    ref32, ref64 = c.deriv(what, scheme, 32), c.deriv(what, scheme, 64)
    derivC, derivL, derivR = L.computeGradients(c.g, dev32(c.data[what]), derivFunc=DERIV[scheme])
    assert hidim.last_path() == "hidim_upwind_kernel<float, %d, %d>" % (c.g.dim, SID[scheme])
    for d in range(c.g.dim):
        if scheme in ENO:
            equal(derivL[d], ref32[d][0], "derivL[%d]" % d)
            equal(derivR[d], ref32[d][1], "derivR[%d]" % d)
            equal(derivC[d], 0.5 * (ref32[d][0] + ref32[d][1]), "derivC[%d]" % d)
        else:
            weno_parity("hidim_upwind %s %s derivL[%d]" % (name, what, d), derivL[d], ref32[d][0], ref64[d][0])
            weno_parity("hidim_upwind %s %s derivR[%d]" % (name, what, d), derivR[d], ref32[d][1], ref64[d][1])
    if scheme in ENO and name == "plane5d":
        # eval_costate at query_ref.state_set's states: eval_u over the ORACLE's float32 derivC arrays, bit for bit
        xs = torch.as_tensor(Q.state_set(c.g, 200), device="cuda")
        got = eval_costate(c.g, dev32(c.data[what]), xs, DERIV[scheme])
        exp = torch.stack([eval_u(c.g, dev32(0.5 * (ref32[d][0] + ref32[d][1])), xs) for d in range(c.g.dim)], dim=-1)
        assert got.dtype == torch.float32 and bool(torch.isnan(got).any()) and bool(torch.isfinite(got).any())
        equal(got, exp.cpu().numpy(), "eval_costate 5-D")


# ------------------------------------------------------------------------------------------ the batch library
@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", ENO)
def test_batch_substep_float_three_dubins_problems(scheme, what):
    import test_gpu_batch as TB
    c = F.Case.get(3, True)
    g = product_grid(c)
    pars = [(1, 1), (1.45, 1.3), (1.9, 0.7)]
    bc = types.SimpleNamespace(g=g, systems=[L.DubinsVehicleRel(g, u, w) for u, w in pars])
    B = len(pars)
    y = np.stack([c.values(what, 32), c.values(what, 32, start=True), (c.values(what, 32) * np.float32(1.25))])
    y0 = y[::-1].copy()
    refs = [O.term_lax_friedrichs(c.og32, c.system(32, p), scheme, 0.0, y[b].reshape(-1, 1)) for b, p in enumerate(pars)]
    dts = [0.8 * sb for _, sb in refs]
    assert len(set(dts)) == B
    yt, y0t = dev32(y), dev32(y0)
    for stage in ("YDOT", "EULER", "RK3_HALF", "RK3_FULL", "RK2_FULL"):
        out = torch.full_like(yt, float("nan"))
        TB.substep(bc, "float32", scheme, STAGES[stage], TB.entries(B, src=list(yt), y0=list(y0t), dst=list(out), dt=dts))
        for b in range(B):
            equal(out[b], stage_ref(stage, y[b], y0[b], dts[b], refs[b][0].reshape(c.og32.shape)), "problem %d %s" % (b, stage))


# ------------------------------------------------------------------------------------------ the derivative kernels at 2-D to 4-D
def fma_bound(c, what, scheme, dim):
    """upwind<> against the float32 oracle on EVERY cell: the same tables and selectors (uncontracted), the selected candidate formed with
    FMAs instead of a rounded product and a rounded sum per term.  With |D1| <= 2A, |dx D2| <= 2A, |c D3| <= (8/3)A (tests/fp32_cases.py;
    A = G/dx): a contracted term drops one rounding of it, u (2 + 8/3) A, and the partial and final sums (<= 4A, <= (20/3)A) round from
    inputs that differ: one more u each side, 2u (4 + 20/3) A: together <= 28 u A = 14 eps32 A."""
    return 14.0 * F.GHOST_FACTOR[c.og64.bc[dim]] * F.EPS32 * float(np.abs(c.values(what, 64)).max()) / c.og64.dx.item(dim)


@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", ENO + ["WENO5_ASSHIPPED"])
@pytest.mark.parametrize("nd,per", F.GRIDS, ids=["%dd-%s" % (nd, "periodic" if per else "extrapolated") for nd, per in F.GRIDS])
def test_derivative_kernels_float_2d_to_4d(nd, per, scheme, what):
    """computeGradients (one launch for every axis) and upwindFirst* per axis: contracted candidates (module docstring)."""
    c = F.Case.get(nd, per)
    g = product_grid(c)
    ref32, ref64 = c.deriv(what, scheme, 32), c.deriv(what, scheme, 64)
    data = dev32(c.values(what, 32))
    derivC, derivL, derivR = L.computeGradients(g, data, derivFunc=DERIV[scheme])
    for d in range(nd):
        dl, dr = DERIV[scheme](g, data, d)
        assert dl.dtype == torch.float32 and torch.equal(dl, derivL[d]) and torch.equal(dr, derivR[d])       # one kernel body, the same bits
        for side, got in enumerate((dl, dr)):
            tag = "upwind %d-D %s %s %s deriv%s[%d]" % (nd, "periodic" if per else "extrapolated", what, scheme, "LR"[side], d)
            if scheme in ENO:
                err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref32[d][side]).max())
                assert err <= fma_bound(c, what, scheme, d), (tag, err, fma_bound(c, what, scheme, d))
                if what == "noisy":         # (the symmetric sphere leaves out far more than 1 %: tests/test_oracle_fp32.py)
                    ratio, left_out = F.within_bound(c, what, scheme, got.cpu().numpy(), side, d, masked=True)
                    assert left_out <= F.MAX_LEFT_OUT and ratio <= 1.0, (tag, ratio, left_out)
            else:
                weno_parity(tag, got, ref32[d][side], ref64[d][side])
    if scheme in ENO and nd == 3:
        xs = torch.as_tensor(Q.state_set(g, 200), device="cuda")
        got = eval_costate(g, data, xs, DERIV[scheme])
        exp = torch.stack([eval_u(g, derivC[d], xs) for d in range(nd)], dim=-1)
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).any())
        equal(got, exp.cpu().numpy(), "eval_costate")


# ------------------------------------------------------------------------------------------ WENO5 through the direct kernel
@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("scheme", WENO)
@pytest.mark.parametrize("nd,per", [(3, True), (2, False), (4, False)], ids=["dubins", "integrator", "pendulum"])
def test_direct_kernel_float_weno5_within_r_of_the_float32_oracle(nd, per, scheme, what):
    c = F.Case.get(nd, per)
    g = product_grid(c)
    ham, par = SYSTEM_OF_DIM[nd][0](g, SYSTEM_OF_DIM[nd][1]).native()
    (yd32, sb32), (yd64, sb64) = c.term(what, scheme, 32), c.term(what, scheme, 64)
    dg = direct_ctx(g)
    out, sb = rk_substep(dg, SID[scheme], ham, par, _ffi.STAGE_YDOT, 0.0, dev32(c.values(what, 32)), None)
    weno_parity("direct_substep %d-D %s %s" % (nd, what, scheme), out, yd32, yd64)
    if nd != 4:
        # these stencils hand over costates scaled by sc = 1/(60 dx) or 1/(12 dx) (scheme_scale): the published maximum is
        # fl(sc * alpha) / sc, one rounding (u) away from alpha, and so is the bound
        assert abs(sb - sb32) <= 2 * F.EPS32 * sb32, (sb, sb32)
    else:
        assert abs(sb - sb32) <= 50 * F.EPS32 * sb32, (sb, sb32)
