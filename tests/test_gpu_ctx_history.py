"""GPU: the result of a call does not depend on what its context did before (the contract at the top of tests/ctx_history_cases.py).

Every comparison is torch.equal on tensors and == on scalars: the reference is the same library on a context WITHOUT a history
(the rest of the suite holds that to the oracle), carrying the sticky settings the model says are in force and the same input arrays.
Beside it every hj_lf_term of a built-in fp64 ENO2 / ENO3 system under the settings the oracle knows is compared with
oracle.term_lax_friedrichs bit for bit, so that a sequence cannot pass with both sides wrong in the same way.

  1  random sequences of 60 ops, per grid, knob set and seed, a fresh context per op
  2  two live contexts on different grids and dtypes taking turns, on one stream and on two
  3  the bound ring across its wrap at four alignments, all 64 slots live
  4  the range-key ring and the pending stage bounds against a companion context that never reaches a wrap
  5  the tile-shape tuner's rotation and the launch-form trial of a thin grid: 40 identical steps each
  6  the context the Python layer caches on a grid Bundle, shared by every caller"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_history_cases as H  # noqa: E402
import instantiation_recipes as IR  # noqa: E402
import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi  # noqa: E402
from levelsetpy_amd.context import device_grid  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402

ORACLE_SCHEMES = {_ffi.ENO2: "ENO2", _ffi.ENO3: "ENO3"}


def same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and a == b


def first_difference(got, want):
    """Index and a description of the first output that differs (None: none does)."""
    if len(got) != len(want):
        return "%d outputs against %d" % (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        if not same(a, b):
            if torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape:
                bad = (a != b)
                return "output %d: %d of %d entries differ, first at flat index %d (%r against %r)" % (
                    k, int(bad.sum()), a.numel(), int(bad.reshape(-1).nonzero()[0]), a.reshape(-1)[bad.reshape(-1)][0].item(), b.reshape(-1)[bad.reshape(-1)][0].item())
            return "output %d: %r against %r" % (k, a, b)
    return None


def oracle_lf_term(P, scheme, pset, restrict):
    """(ydot, stepBound) of the oracle's termLaxFriedrichs (+ termRestrictUpdate's clamp) on the problem's y: computed once, shared."""
    key = (scheme, pset)
    if key not in P.oracle_refs:
        par = H.PSETS[P.case.ham][pset]
        osys = O.DubinsRel(P.og, par[0], par[2]) if P.case.ham == 0 else O.DoubleIntegrator(P.og, par[0])
        yd, sb = O.term_lax_friedrichs(P.og, osys, ORACLE_SCHEMES[scheme], 0., P.arrays["y"].reshape(-1, 1))
        P.oracle_refs[key] = (np.asarray(yd).reshape(P.case.N), float(sb))
    yd, sb = P.oracle_refs[key]
    return (np.maximum(yd, 0.) if restrict > 0 else np.minimum(yd, 0.) if restrict < 0 else yd), sb


class History(object):
    """One long-lived context walking through a sequence; step(i) runs step i on it and on a fresh context, and compares."""

    def __init__(self, case_name, knobs, seed, n=H.DEFAULT_N, stream=None):
        self.case, self.knobs, self.seed = H.CASES[case_name], H.KNOBS[knobs], seed
        self.steps = H.sequence(seed, case_name, n)
        self.stream = stream
        self.oracle_checks = 0
        with self.on_stream():
            self.long = H.State(self.case, self.knobs.env)
            H.replay(self.long, H.INITIAL_SETTINGS)
        self.model = H.Model(self.case)

    def on_stream(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else torch.cuda.stream(torch.cuda.current_stream())

    def where(self, i):
        return "case %s knobs %s seed %d, op %d (%s %r)\n  ops so far: %s" % (
            self.case.name, self.knobs.name, self.seed, i, self.steps[i].op.name, self.steps[i].p, H.describe(self.steps, i + 1))

    def step(self, i):
        with self.on_stream():
            self._step(i)

    def _step(self, i):
        s, long, model = self.steps[i], self.long, self.model
        op = s.op
        assert model.satisfied(s.needs), self.where(i)
        before = H.clone_arrays(long.A)
        got = tuple(op.run(long, s.p))
        slot, slot_value = op.slot(s.p), None
        if op.refused:
            assert isinstance(got[0], int) and got[0] != 0, "a call that must be refused returned %r\n%s" % (got[0], self.where(i))
        if op.model_ref:
            want = model.slots[s.p["slot"]]
        else:
            fresh = H.State(self.case, self.knobs.env, arrays=before)
            try:
                H.replay(fresh, model.settings)
                want = tuple(op.run(fresh, s.p))
                if slot is not None:
                    slot_value = fresh.bound(slot)
            finally:
                fresh.close()
        diff = first_difference(got, want)
        assert diff is None, "the context's history shows: %s\n%s" % (diff, self.where(i))
        if op.name.startswith("lf_term"):
            self.check_oracle(i, s, got)
        model.apply(s)
        H.note_slots(model, s, slot_value)
        for k, v in sorted(model.slots.items()):
            assert long.bound(k) == v, "slot %d holds %r, written as %r\n%s" % (k, long.bound(k), v, self.where(i))

    def check_oracle(self, i, s, got):
        st, case = self.model.settings, self.case
        if not (case.dtype == "float64" and case.ham in (0, 1) and s.p["scheme"] in ORACLE_SCHEMES and st["coords"] == "base"
                and (st["aux"] == "numpy" or len(case.N) == 2) and st["diss"] == _ffi.DISS_GLF):
            return
        yd, sb = oracle_lf_term(self.long.P, s.p["scheme"], s.p["pset"], s.p["restrict"])
        assert np.array_equal(got[0].cpu().numpy(), yd) and got[1] == sb, "hj_lf_term against the oracle: %d cells differ, bound %r against %r\n%s" % (
            int((got[0].cpu().numpy() != yd).sum()), got[1], sb, self.where(i))
        self.oracle_checks += 1

    def finish(self):
        with self.on_stream():
            self.long.note_record()
            seen = self.long.seen
            self.long.close()
        assert any(f in sym for f in self.knobs.family for sym in seen), "knobs %s on %s never launched %s; the record holds %s" % (
            self.knobs.name, self.case.name, self.knobs.family, sorted(seen))


# ------------------------------------------------------------------------------------------------ 1: random sequences
SEQUENCES = [(c, k.name, seed) for k in H.KNOBS.values() for c in k.cases for seed in H.DEFAULT_SEEDS]


@pytest.mark.parametrize("case,knobs,seed", SEQUENCES, ids=["%s-%s-%d" % t for t in SEQUENCES])
def test_random_sequence_against_fresh_contexts(case, knobs, seed):
    h = History(case, knobs, seed)
    for i in range(len(h.steps)):
        h.step(i)
    h.finish()
    if case in ("dubins64", "dint64", "ring64"):
        assert h.oracle_checks >= 1          # (lf_term_base_settings asks for the settings the oracle knows)


def test_the_sequences_reach_the_oracle():
    """Over the default seeds the hj_lf_term ops the oracle can check are there: the sequences hold steps it applies to."""
    n = 0
    for case in ("dubins64", "dint64", "ring64"):
        for seed in H.DEFAULT_SEEDS:
            model = H.Model(H.CASES[case])
            for s in H.sequence(seed, case):
                st = model.settings
                n += (s.op.name.startswith("lf_term") and s.p["scheme"] in ORACLE_SCHEMES and st["coords"] == "base" and st["diss"] == 0
                      and (st["aux"] == "numpy" or case == "dint64"))
                model.apply(s)
    assert n >= 12, n            # (one per sequence at least: the op that asks for those settings)


# ------------------------------------------------------------------------------------------------ 2: two live contexts
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("pair,knobs", [(("dubins64", "pend32"), "tune"), (("dint64", "dubins32"), "direct"), (("ring64", "dubins32"), "fuse12")])
def test_two_live_contexts_take_turns(pair, knobs, streams):
    """State that is global to the library, not to a context, would show here: two contexts on different grids and dtypes alternate."""
    ss = [torch.cuda.Stream(), torch.cuda.Stream()] if streams == 2 else [None, None]
    hs = [History(pair[0], knobs, 11, stream=ss[0]), History(pair[1], knobs, 12, stream=ss[1])]
    for i in range(H.DEFAULT_N):
        for h in hs:
            h.step(i)
    for h in hs:
        h.finish()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3: the bound ring, every alignment
def static_bound(st, par):
    sb, am = C.c_double(), (C.c_double * 4)()
    _ffi.check(st.lib.hj_static_step_bound(st.ctx, st.case.ham, _ffi.darr(par), C.byref(sb), am))
    return (sb.value, tuple(am)[:len(st.case.N)])


@pytest.mark.parametrize("extra,knobs", [(0, "tune"), (1, "tune"), (2, "tune"), (3, "tune"), (1, "direct")])
def test_bound_ring_keeps_every_live_slot_at_every_alignment(extra, knobs):
    """2048 + 64 + 8 substeps after `extra` launches, each into a seeded slot with one of eight parameter sets: every live slot holds the
    static step bound of the set that wrote it, read every 61 launches and at the end -- across the ring's wrap, with all 64 slots live."""
    case, env = H.CASES["ring64"], H.KNOBS[knobs].env
    want = []
    for par in H.RING_PSETS:
        fresh = H.State(case, env)
        want.append(static_bound(fresh, par))
        fresh.close()
    assert len(set(w[0] for w in want)) == len(want), want            # pairwise different bounds: a slot's content names its set
    st = H.State(case, env)
    _ffi.check(st.lib.hj_launch_record(st.ctx, 1))
    rng = np.random.default_rng(100 + extra)
    y, out = st.A["y"], st.A["s1"]
    held, launches = {}, 0

    def launch(slot, k):
        _ffi.check(st.lib.hj_rk_substep(st.ctx, _ffi.ENO2, case.ham, _ffi.darr(H.RING_PSETS[k]), 0., _ffi.STAGE_EULER, H.DT, 0, H.ptr(y), None, H.ptr(out),
                                        slot, 0, case.N[0]))
        held[slot] = k

    def read_all(when):
        for slot, k in sorted(held.items()):
            got = st.bound(slot)
            assert got == want[k], "after %d launches (%s): slot %d holds %r, written with set %d: %r" % (launches, when, slot, got, k, want[k])

    for _ in range(extra):
        launch(0, 0)
        launches += 1
    slots = list(rng.permutation(_ffi.BOUND_SLOTS)) + [int(v) for v in rng.integers(_ffi.BOUND_SLOTS, size=2048 + 8)]
    assert len(slots) == 2048 + 64 + 8
    for n, slot in enumerate(slots):
        launch(int(slot), int(rng.integers(len(H.RING_PSETS))))
        launches += 1
        if (n + 1) % 61 == 0:
            read_all("every 61")
    read_all("the end")
    assert len(held) == _ffi.BOUND_SLOTS and launches >= 2048 + 64 and launches == extra + len(slots)
    seen = st.note_record()
    st.close()
    assert any(f in sym for f in H.KNOBS[knobs].family for sym in seen), "knobs %s never launched %s; the record holds %s" % (
        knobs, H.KNOBS[knobs].family, sorted(seen))


# ------------------------------------------------------------------------------------------------ 4: range ring and pending stage bounds
RECREATE_EVERY = 64


@pytest.mark.parametrize("drain_every", [1, 8])
@pytest.mark.parametrize("first_passes", [0, 1])
@pytest.mark.parametrize("diss", [_ffi.DISS_GLF, _ffi.DISS_LLF])
def test_range_ring_and_pending_bounds_in_lockstep(diss, first_passes, drain_every):
    """800 RK3 steps of the range-reading Hamiltonian on a long-lived context A; its companion B is destroyed and re-created every 64
    steps, so it never reaches a wrap of the range-key ring (1024 entries) or of the bound ring.  Fed the same state, both give the same
    t, deltaT, state and hj_rk_prev_bounds at every step, and the same hj_rk_last_bounds at every step where it is called.
    hj_rk_last_bounds drains the pending stage bounds, so a step that follows it has nothing to decode and hj_rk_prev_bounds nothing new:
      drain_every = 1   hj_rk_last_bounds after EVERY step: held equal at every step; hj_rk_prev_bounds always reports nothing
      drain_every = 8   after every eighth step: in between, the next hj_rk_step decodes the pending bounds itself and
                        hj_rk_prev_bounds reports them, seven steps in eight.
    B is re-created only right after a step that drained (64 is a multiple of both cadences): A, like the new B, then has nothing
    pending, which is what makes hj_rk_prev_bounds comparable at B's first step."""
    assert RECREATE_EVERY % drain_every == 0
    case, env = H.RANGE_CASE, IR.knobs()
    ham, sid, par = H.range_ham(3), _ffi.WENO5_ASSHIPPED, _ffi.darr([0.7])

    def make():
        st = H.State(case, env)
        _ffi.check(st.lib.hj_ctx_set_dissipation(st.ctx, diss))
        return st

    def one(st, cur, out):
        tout, dtout = C.c_double(), C.c_double()
        _ffi.check(st.lib.hj_rk_step(st.ctx, 3, sid, ham, par, 0., 1e9, 0.8, 1e300, 0, H.ptr(cur), H.ptr(out), H.ptr(st.A["w0"]), H.ptr(st.A["w1"]),
                                     C.byref(tout), C.byref(dtout)))
        sp, npv, dtp = (C.c_double * 4)(), C.c_int(), C.c_double()
        _ffi.check(st.lib.hj_rk_prev_bounds(st.ctx, sp, C.byref(npv), C.byref(dtp)))
        return (tout.value, dtout.value, npv.value) + tuple(sp)[:npv.value] + ((dtp.value,) if npv.value else ())

    def last(st):
        sb, nb = (C.c_double * 4)(), C.c_int()
        _ffi.check(st.lib.hj_rk_last_bounds(st.ctx, sb, C.byref(nb)))
        return (nb.value,) + tuple(sb)[:nb.value]

    a, b = make(), make()
    keys = torch.zeros(8, dtype=torch.int64, device="cuda")
    for _ in range(first_passes):          # the other alignment of the range ring
        _ffi.check(a.lib.hj_range_pass(a.ctx, sid, ham, par, H.ptr(a.A["y"]), H.ptr(keys)))
    cur, nxt, out_b = a.A["y"].clone(), torch.zeros_like(a.A["y"]), torch.zeros_like(a.A["y"])
    reported = 0
    for k in range(800):
        if k and k % RECREATE_EVERY == 0:
            assert (k - 1) % drain_every == drain_every - 1          # the step before drained
            b.close()
            b = make()
        ra, rb = one(a, cur, nxt), one(b, cur, out_b)
        assert ra == rb, (k, ra, rb)
        assert torch.equal(nxt, out_b), (k, int((nxt != out_b).sum()))
        reported += ra[2] > 0
        if k % drain_every == drain_every - 1:
            la, lb = last(a), last(b)
            assert la == lb and la[0] == 3 and all(0 < v < float('inf') for v in la[1:]), (k, la, lb)
        cur, nxt = nxt, cur
    assert bool(torch.isfinite(cur).all())
    if drain_every == 8:
        assert reported >= 600           # (the next step decoded the pending bounds seven times in eight: 699 of 800)
    else:
        assert reported == 0             # (every step's bounds went out through hj_rk_last_bounds)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5: tuner history
def test_tuner_rotation_never_shows_in_the_result():
    """HJ_AUTOTUNE_MIN_MCELLS=0: the first launches per (scheme, stage class) take turns through the candidate tile shapes.  40 identical
    hj_rk_step calls from the same y into rotating buffers give the first call's bits and deltaT while hj_last_tile shows the rotation.
    (The launch-form trial of thin grids has the next test.)"""
    case = H.TUNER_CASE
    st = H.State(case, H.KNOBS["tune"].env)
    y = st.A["y"]
    bufs = [torch.zeros_like(y) for _ in range(3)]
    shapes, first = set(), None
    for k in range(40):
        out = bufs[k % 3]
        tout, dtout = C.c_double(), C.c_double()
        _ffi.check(st.lib.hj_rk_step(st.ctx, 3, _ffi.WENO5_ASSHIPPED, case.ham, st.par(0), 0., 1e9, 0.8, 1e300, 0, H.ptr(y), H.ptr(out), H.ptr(st.A["w0"]),
                                     H.ptr(st.A["w1"]), C.byref(tout), C.byref(dtout)))
        e = (C.c_int * 4)()
        _ffi.check(st.lib.hj_last_tile(st.ctx, e))
        shapes.add((st.lib.hj_last_kernel(st.ctx), tuple(e)))
        if first is None:
            first = (out.clone(), tout.value, dtout.value)
        assert (tout.value, dtout.value) == first[1:] and torch.equal(out, first[0]), (k, sorted(shapes))
    st.close()
    assert all(name.startswith(b"fused_pair_kernel") for name, _ in shapes), shapes
    if len(shapes) < 2:
        pytest.skip("the tuner has one candidate tile shape on %r: nothing rotates" % (case.N,))


def test_launch_form_trial_never_shows_in_the_result():
    """The per-key trial of the transposed march (hj_ctx::xp_choice) runs on thin single-domain grids from 6.5 M cells only (a context with
    slab flags never tries: xp_wanted): (20, 640, 520), HJ_XP=1, HJ_XP_TRIALS=2.  The first calls take turns between the two launch forms
    in runs of six substeps; 40 identical hj_rk_step calls give the first call's bits and deltaT, and hj_last_kernel shows both forms."""
    from levelsetpy_amd.context import DeviceGrid
    from test_gpu_parity import mk
    n = (20, 640, 520)
    g, _ = mk([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / n[2])], n, 2)
    x0 = torch.as_tensor(np.asarray(g.vs[0]).ravel(), device="cuda").reshape(-1, 1, 1)
    x1 = torch.as_tensor(np.asarray(g.vs[1]).ravel(), device="cuda").reshape(1, -1, 1)
    x2 = torch.as_tensor(np.asarray(g.vs[2]).ravel(), device="cuda").reshape(1, 1, -1)
    gen = torch.Generator(device="cuda").manual_seed(4)
    y = ((x0 * x0 + x1 * x1).sqrt() - 0.5 + 0.05 * torch.sin(3 * x2) + 0.01 * torch.randn(n, generator=gen, device="cuda", dtype=torch.float64)).contiguous()
    with IR.environment(dict(IR.knobs(HJ_XP=1), HJ_XP_TRIALS="2", HJ_XP_MAX_PLANES=None)):
        dg = DeviceGrid(g, "float64")
    dg.bind_stream()
    bufs, w0, w1 = [torch.zeros_like(y) for _ in range(2)], torch.zeros_like(y), torch.zeros_like(y)
    forms, first = [], None
    # How long the trial can last (hj_inst.hip, the launch-form choice; hj_host.h, hj_ctx::XP_RUN): a form starts a run only while it has
    # fewer than HJ_XP_TRIALS + 2 read runs, so at most 2 * (TRIALS + 2) runs of XP_RUN = 6 launches are trial runs: 48 launches, 16 RK3
    # steps.  A finished run is read back at a later call without waiting, so the decision may fall a few calls after that; the steps
    # below leave 16 more for it before the last 8, which must all have taken the form that was kept.  (That count is about
    # reaching the END of the trial, so that both the sampling calls and the settled ones are compared; a longer trial needs more steps here.)
    trials, xp_run = 2, 6
    trial_steps = 2 * (trials + 2) * xp_run // 3
    nsteps = trial_steps + 16 + 8
    assert nsteps == 40
    for k in range(nsteps):
        out = bufs[k % 2]
        tout, dtout = C.c_double(), C.c_double()
        _ffi.check(dg.lib.hj_rk_step(dg.ctx, 3, _ffi.WENO5_ASSHIPPED, _ffi.HAM_DUBINS_REL, _ffi.darr(H.PSETS[0][0]), 0., 1e9, 0.8, 1e300, 0, H.ptr(y), H.ptr(out),
                                     H.ptr(w0), H.ptr(w1), C.byref(tout), C.byref(dtout)))
        forms.append(dg.lib.hj_last_kernel(dg.ctx))
        if first is None:
            first = (out.clone(), tout.value, dtout.value)
        assert (tout.value, dtout.value) == first[1:] and torch.equal(out, first[0]), (k, forms)
    dg._finalizer()
    assert set(forms) == {b"fused_pair_kernel", b"fused_pair_kernel (march along axis 1)"}, forms
    assert len(set(forms[-8:])) == 1, forms          # the trial ended: one form is kept


# ------------------------------------------------------------------------------------------------ 6: the shared Python context
def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


@pytest.mark.parametrize("device_inputs", [False, True], ids=["numpy", "tensors"])
def test_the_shared_python_context_has_no_memory(device_inputs):
    """One grid Bundle, two systems, and what a session does to the context cached on the Bundle: every result equals the same call on a
    freshly created equal grid whose cache is empty."""
    from test_gpu_parity import dubins, sdata

    def world():
        g, og = dubins([14, 12, 16])
        rng = np.random.default_rng(5)
        d0 = O.shape_cylinder(og, 2, None, .5) + 0.02 * rng.standard_normal(og.shape)
        obst = L.shapeSphere(g, np.array([[1.5], [0.], [0.]]), .3)
        return dict(g=g, d0=d0, obst=obst, s1=L.DubinsVehicleRel(g, 1, 1), s2=L.DubinsVehicleRel(g, 1.5, .75))

    def arr(a):
        return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if device_inputs else np.array(a)

    op1 = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on')))
    tau = np.array([0., .01, .02])

    def lf(w, sys_="s1", diss=None, scheme=L.upwindFirstENO3):
        sd = sdata(w["g"], w[sys_], scheme)
        if diss is not None:
            sd.dissFunc = diss
        yd, sb, _ = L.termLaxFriedrichs(0., arr(w["d0"].reshape(-1, 1)), sd)
        return _np(yd), float(sb)

    def solve(w, comp, **extra):
        sd = L.Bundle(dict(grid=w["g"], hamFunc=w["s1"].hamiltonian, partialFunc=w["s1"].dissipation, derivFunc=L.upwindFirstENO3))
        ex = dict(quiet=True)
        ex.update({k: arr(v) for k, v in extra.items()})
        data, t, _ = L.HJIPDE_solve(arr(w["d0"]), tau, sd, comp, L.Bundle(ex))
        return _np(data), _np(t)

    def nan_solve(w):
        bad = w["d0"].copy()
        bad[4, 4, 4] = np.nan
        sd = L.Bundle(dict(grid=w["g"], hamFunc=w["s1"].hamiltonian, partialFunc=w["s1"].dissipation, derivFunc=L.upwindFirstENO2))
        with pytest.raises(ValueError):
            L.HJIPDE_solve(arr(bad), np.array([0., .01]), sd, 'set', L.Bundle(dict(quiet=True, keepLast=True)))
        return ()

    def raising_step(w):
        def post(t, y, s):
            raise RuntimeError("postTimeStep gives up")
        opp = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on', postTimeStep=post)))
        with pytest.raises(RuntimeError, match="gives up"):
            L.odeCFL2(L.termLaxFriedrichs, [0., 10.], arr(w["d0"].reshape(-1, 1)), opp, sdata(w["g"], w["s1"], L.upwindFirstENO3))
        return ()

    def rk3(w):
        t, y, _ = L.odeCFL3(L.termLaxFriedrichs, [0., 10.], arr(w["d0"].reshape(-1, 1)), op1, sdata(w["g"], w["s1"], L.upwindFirstWENO5))
        return float(t), _np(y)

    def reinit_curv(w):
        col = arr(w["d0"].reshape(-1, 1))
        a, sa, _ = L.termReinit(0., col, L.Bundle(dict(grid=w["g"], derivFunc=L.upwindFirstENO2, initial=arr(w["d0"]))))
        b, sb, _ = L.termCurvature(0., col, L.Bundle(dict(grid=w["g"], b=0.5, curvatureFunc=L.curvatureSecond)))
        return _np(a), float(sa), _np(b), float(sb)

    def behind_pythons_back(w):
        dg = device_grid(w["g"])
        _ffi.check(dg.lib.hj_ctx_set_dissipation(dg.ctx, _ffi.DISS_LLF))
        return ()

    calls = [
        ("termLaxFriedrichs GLF", lf),
        ("HJIPDE_solve minVWithTarget + obstacle", lambda w: solve(w, 'minVWithTarget', targetFunction=w["d0"], obstacleFunction=w["obst"])),
        ("termLaxFriedrichs again", lf),
        ("termLaxFriedrichs LLF", lambda w: lf(w, diss=L.artificialDissipationLLF)),
        ("odeCFL3 single step", rk3),
        ("HJIPDE_solve with a NaN", nan_solve),
        ("termLaxFriedrichs after the NaN", lf),
        ("odeCFL2 whose postTimeStep raises", raising_step),
        ("termLaxFriedrichs after the raise", lf),
        ("termReinit, termCurvature", reinit_curv),
        ("HJIPDE_solve maxVOverTime", lambda w: solve(w, 'maxVOverTime')),
        ("the second system's termLaxFriedrichs", lambda w: lf(w, "s2")),
        ("the first system's again", lf),
        ("hj_ctx_set_dissipation(LLF) behind Python's back", behind_pythons_back),
        ("termLaxFriedrichs GLF with its step bound", lf),
    ]
    shared = world()
    glf_bound = None
    for k, (name, call) in enumerate(calls):
        got = call(shared)
        if call is behind_pythons_back:
            continue
        want = call(world())
        assert len(got) == len(want), (k, name)
        for j, (a, b) in enumerate(zip(got, want)):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), "call %d (%s), output %d: %d entries differ" % (k + 1, name, j, int((a != b).sum()))
            else:
                assert a == b, "call %d (%s), output %d: %r against %r" % (k + 1, name, j, a, b)
        if call is lf:
            glf_bound = got[1] if glf_bound is None else glf_bound
            assert got[1] == glf_bound, (k, name, got[1], glf_bound)
    # the local kind's bound differs from the global one on this grid: call 15 would have shown a stale LLF
    assert lf(world(), diss=L.artificialDissipationLLF)[1] != glf_bound
