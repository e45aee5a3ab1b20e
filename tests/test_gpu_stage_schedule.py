"""GPU: an interval of libhj_batch.so, libhj_stoch.so and libhj_hidim.so is the same library's substeps chained by hand, bit for bit.

One schedule (rk_schedule, csrc/hj_stage_host.h) serves the three *_integrate entry points.  Per library and order 1, 2, 3: an interval
of two steps and one of three -- the last step cut short by the end of the span, the result once in buf_b and once in buf_a -- with
post_prev and both array operators set, against *_substep calls in the order and on the buffers the C ABI documents.  The smallest
grids that still have every axis: the double integrator on 7 x 6 (two problems for the batch), the plane on a 5-D grid of 3 .. 6 nodes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _bffi, _ffi, _hffi, _marshal, batch, hidim  # noqa: E402
from levelsetpy_amd.stochastic import _Call  # noqa: E402

pytestmark = pytest.mark.gpu

STAGES = {1: [_ffi.STAGE_EULER], 2: [_ffi.STAGE_EULER, _ffi.STAGE_RK2_FULL], 3: [_ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF, _ffi.STAGE_RK3_FULL]}
POST, OP_A, OP_B = _ffi.POST_MIN_PREV, _bffi.ARR_MAX, _bffi.ARR_MAX_NEG
CFL = 0.8


def make_grid(N):
    nd = len(N)
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col([-1.0] * nd, np.float64), col([1.0] * nd, np.float64), col(N, np.int64))


def fields(shape, n):
    rng = np.random.default_rng(11)
    return [torch.as_tensor(rng.standard_normal(shape), device="cuda") for _ in range(n)]


def stages_of(order, cur, nxt, work):
    """(stage, src, y0, dst) of one step, as include/hj_batch.h, hj_stoch.h and hj_hidim.h describe an interval's launches."""
    if order == 1:
        return [(cur, None, nxt)]
    if order == 2:
        return [(cur, None, work), (work, cur, nxt)]
    return [(cur, None, nxt), (nxt, cur, work), (work, cur, nxt)]


def chain(order, dts, y, substep):
    """The interval by hand on buffers of its own: substep(stage, src, y0, dst, dt, last) per launch.  -> the final state."""
    a, b, w = (torch.full_like(y, float("nan")) for _ in range(3))
    cur = y
    for k, dt in enumerate(dts):
        nxt = (a, b)[k & 1]
        for j, (src, y0, dst) in enumerate(stages_of(order, cur, nxt, w)):
            substep(STAGES[order][j], src, y0, dst, dt, j == order - 1)
        cur = nxt
    return cur


def spans(sb):
    """tf of an interval of two steps and of three from t0 = 0.1, the last step half a full one."""
    return [(n, 0.1 + (n - 0.5) * CFL * sb) for n in (2, 3)]


@pytest.mark.parametrize("order", [1, 2, 3])
def test_stoch_interval_is_its_substeps(order):
    g = make_grid((7, 6))
    dev = torch.device("cuda", torch.cuda.current_device())
    ham, par = L.DoubleIntegrator(g, 1.5).native()
    call = _Call(g, ham, _ffi.ENO3, par, np.array([[0.2, 0.05], [-0.1, 0.3]]), torch, dev)
    sb = call.step_bound()[0]
    y, pa, pb = fields(g.shape, 3)
    for n, tf in spans(sb):
        dts = batch.plan_interval(sb, 0.1, tf, CFL, 1e300, 1e-4, order)[0]
        assert len(dts) == n and dts[-1] < dts[0]
        a, b, w = (torch.full_like(y, float("nan")) for _ in range(3))
        t, steps, where = call.integrate(sb, y, a, b, w, 0.1, tf, order, -1, POST, OP_A, pa, OP_B, pb, CFL, 1e300, 1e-4)
        assert (steps, where) == (n, 2 - (n & 1))
        ref = chain(order, dts, y, lambda stage, src, y0, dst, dt, last: call.substep(
            stage, src, dst, y0, dt, -1, *((POST, OP_A, pa, OP_B, pb) if last else ())))
        torch.cuda.synchronize()
        assert torch.equal((a, b)[where - 1], ref) and not bool(torch.isnan(ref).any())


@pytest.mark.parametrize("order", [1, 2, 3])
def test_hidim_interval_is_its_substeps(order):
    g = make_grid((3, 6, 4, 5, 3))
    hg = hidim.hi_grid(g, "float64")
    ham, par = L.Plane5D(g, 0.8, 1.3, 'max').native()
    sb = hg.step_bound(ham, par)
    y, pa, pb = fields(g.shape, 3)
    for n, tf in spans(sb):
        dts = batch.plan_interval(sb, 0.1, tf, CFL, 1e300, 1e-4, order)[0]
        assert len(dts) == n and dts[-1] < dts[0]
        a, b, w = (torch.full_like(y, float("nan")) for _ in range(3))
        tout, steps, where = C.c_double(), C.c_int64(), C.c_int32()
        _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(hg.tab), _ffi.ENO3, ham, order, 1, POST, _hffi.params(par), sb,
                                         hg.ptr(y), hg.ptr(a), hg.ptr(b), hg.ptr(w), OP_A, hg.ptr(pa), OP_B, hg.ptr(pb), 0.1, tf, CFL,
                                         1e300, 1e-4, C.byref(tout), C.byref(steps), C.byref(where), hg.stream()))
        assert (steps.value, where.value) == (n, 2 - (n & 1))
        ref = chain(order, dts, y, lambda stage, src, y0, dst, dt, last: hidim._substep(
            hg, _ffi.ENO3, ham, par, stage, 1, src, y0, dst, dt, *((POST, OP_A, pa, OP_B, pb) if last else ())))
        torch.cuda.synchronize()
        assert torch.equal((a, b)[where.value - 1], ref) and not bool(torch.isnan(ref).any())


@pytest.mark.parametrize("order", [1, 2, 3])
def test_batch_interval_is_its_substeps(order):
    """Two problems whose bounds differ: over one span the first takes two or three steps, the second its own count, and sits the
    launches past its last step out."""
    g = make_grid((7, 6))
    dev = torch.device("cuda", torch.cuda.current_device())
    B = 2
    natives = [L.DoubleIntegrator(g, u).native() for u in (1.5, 0.3)]
    ham = natives[0][0]
    par = torch.as_tensor(np.asarray([list(p) + [0.0] * (_bffi.PAR_SLOTS - len(p)) for _, p in natives], dtype=np.float64), device="cuda")
    desc, _ = _marshal.descriptor(g, "float64")
    tab = batch.tables(g, torch, dev)
    sbs = batch.step_bounds(g, tab, desc, ham, par, B, torch, dev)
    y, pa, pb = fields((B,) + tuple(g.shape), 3)
    for n, tf in spans(float(sbs[0])):
        plans = [batch.plan_interval(float(sb), 0.1, tf, CFL, 1e300, 1e-4, order)[0] for sb in sbs]
        assert len(plans[0]) == n and 1 <= len(plans[1]) < n
        bufs = torch.full((3,) + tuple(y.shape), float("nan"), dtype=y.dtype, device="cuda")
        probs = [_bffi.Problem(y_in=y[p].data_ptr(), buf_a=bufs[0, p].data_ptr(), buf_b=bufs[1, p].data_ptr(), work=bufs[2, p].data_ptr(),
                               post_a=pa[p].data_ptr(), post_b=pb[p].data_ptr(), op_a=OP_A, op_b=OP_B) for p in range(B)]
        t, steps, where = batch.integrate_batch(g, tab, desc, _ffi.ENO3, ham, par, sbs, probs, 0.1, tf, order, POST, -1, CFL, 1e300, 1e-4,
                                                torch, dev)
        assert list(steps) == [len(p) for p in plans] and list(where) == [2 - (len(p) & 1) for p in plans]
        # by hand: one hjb_substep per launch for both problems, a finished problem inactive
        hand = torch.full_like(bufs, float("nan"))
        cur = [y[p] for p in range(B)]
        for k in range(n):
            live = [k < len(plans[p]) for p in range(B)]
            nxt = [hand[k & 1, p] for p in range(B)]
            per = [stages_of(order, cur[p], nxt[p], hand[2, p]) for p in range(B)]
            for j in range(order):
                ent = np.zeros(B, dtype=_bffi.ENTRY)
                for p in range(B):
                    if live[p]:
                        src, y0, dst = per[p][j]
                        ent[p]["src"], ent[p]["y0"], ent[p]["dst"] = src.data_ptr(), (0 if y0 is None else y0.data_ptr()), dst.data_ptr()
                        ent[p]["dt"], ent[p]["active"] = plans[p][k], 1
                        if j == order - 1:
                            ent[p]["post_prev"], ent[p]["op_a"], ent[p]["op_b"] = POST, OP_A, OP_B
                            ent[p]["post_a"], ent[p]["post_b"] = pa[p].data_ptr(), pb[p].data_ptr()
                e = batch.upload_entries(ent, torch, dev)
                _bffi.check(_bffi.lib().hjb_substep(C.byref(desc), C.byref(tab), _ffi.ENO3, ham, STAGES[order][j], -1, par.data_ptr(),
                                                    e.data_ptr(), B, _marshal.stream(torch, dev)))
                torch.cuda.synchronize()
            cur = [nxt[p] if live[p] else cur[p] for p in range(B)]
        for p in range(B):
            assert torch.equal(bufs[where[p] - 1, p], cur[p]) and not bool(torch.isnan(cur[p]).any()), (order, n, p)
