"""Call sequences on one hj_ctx against contexts without a history (test infrastructure: a helper module, not collected by pytest;
importable without a device).

THE CONTRACT (include/hj_mi355x.h refers to it where the setters are documented)

  The outputs of a C-ABI call on a context are a function of three things: the call's arguments, the contents of the arrays it reads,
  and the context's STICKY SETTINGS -- what the hj_ctx_set_* setters last wrote: stream, coords, aux, slab flags, dissipation kind,
  post-step operator, post-step arrays, WENO eps source, range source, axis-0 pad, and the launch-record switch.  Everything else in
  hj_ctx is hidden (the key rings and the slot map, the static step-bound cache, the epsilon rows, the tile-shape tuner, the launch-form
  trials, the pending stage bounds, the tiling / occupancy / stage-fusion caches) and must never show.
  A bound slot holds its result until the same slot is written again, whatever else is launched in between.  (Slots 60..63 are also
  written by the library itself: hj_lf_term leaves its bound in 63, a step of a range-reading Hamiltonian its stage bounds in 60..62;
  a caller that wants a slot to survive those calls uses 0..59.)
  hj_ctx_set_coords replaces the trig tables by libm's values of the new coordinates (hj_ctx_set_aux afterwards overrides them).
  A refused call (non-zero return) changes neither sticky nor hidden state.

What is here

  OPS        the table of ops: a name, the C entry points it issues, the arrays it reads and writes, and run(st, p) -> outputs (device
             tensors and host scalars) -- one C-ABI call or a fixed short group.  p is drawn per step by draw(rng, case, model).
  Model      the sticky settings in force, the arrays written so far and, per bound slot, the bound it must hold.
  sequence() a seeded list of steps; the settings a step requires are put in force by explicit setter steps in front of it.
  replay()   puts exactly the model's settings on a fresh context.
  State      one context with its arrays (the long-lived one, or a fresh one made for a single step).

tests/test_ctx_history_host.py checks the table and the generator without a device; tests/test_gpu_ctx_history.py runs the sequences."""
import ctypes as C
import os
import re
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantiation_recipes as IR  # noqa: E402
from levelsetpy_amd import _ffi  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hj_mi355x.h")
USER_SLOTS = 60                  # the library writes 60..63 itself (the contract above)
SCHEMES = (_ffi.ENO2, _ffi.ENO3, _ffi.WENO5, _ffi.WENO5_ASSHIPPED)
STAGES = (_ffi.STAGE_YDOT, _ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF, _ffi.STAGE_RK3_FULL, _ffi.STAGE_RK2_FULL)
DT = 2e-3                        # a step size well inside every grid's CFL bound
BOX = {0: ([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi]), 1: ([-1., -1.5], [1., 1.5]), 2: ([-np.pi, -8., -np.pi, -8.], [np.pi, 8., np.pi, 8.])}
# at least two parameter sets per built-in system; the Dubins car's in the oracle's form (v_e = v_p, w_e = w_p = w)
PSETS = {0: ([1., 1., 1., 2.], [1.5, 1.5, .75, 1.5]), 1: ([1.25], [.6]), 2: ([1.0], [1.7])}
# eight Dubins parameter sets for the ring runs: their static step bounds differ pairwise (the test asserts it)
RING_PSETS = [[1. + .125 * k, 1. + .125 * k, 1. + .0625 * k, 2. + .125 * k] for k in range(8)]

Case = namedtuple("Case", "name N periodic dtype ham")
CASES = {
    "dubins64": Case("dubins64", (14, 12, 16), (2,), "float64", 0),
    "dubins32": Case("dubins32", (14, 12, 16), (2,), "float32", 0),
    "dint64": Case("dint64", (24, 19), (), "float64", 1),
    "pend32": Case("pend32", (9, 8, 10, 12), (0, 1, 2, 3), "float32", 2),
    "ring64": Case("ring64", (8, 8, 8), (2,), "float64", 0),
}
# beside them: the grid of the range-ring run, and one whose rows are longer than a tile (the tuner then has several shapes to visit)
RANGE_CASE = Case("range64", (10, 9, 8), (), "float64", 0)
TUNER_CASE = Case("tuner64", (24, 70, 150), (2,), "float64", 0)

# The knob sets that switch the history-carrying machinery ON at these sizes (read in hj_ctx_create), and the kernel family each one
# means to exercise: a sequence must have launched one of `family` (a substring of the launch record's symbols) at least once.
#   tune    tile-shape tuner from 0 cells, epsilon rows reduced inside the producing launch from 0 cells, the pair kernel at any size
#   tiled   the one-cell-per-lane tiled kernel, tuner on
#   fuse12  hj_rk_step fuses stages 1 + 2
#   xp      the transposed march for every launch that has one (the auto rule, HJ_XP=1, and its per-key trial need 6.5 M cells: they
#           have a test of their own on a thin grid)
#   direct / below   the one-thread-per-cell kernel by force and by the size rule
Knobs = namedtuple("Knobs", "name env family cases")
ALL = tuple(CASES)
KNOBS = {k.name: k for k in (
    Knobs("tune", IR.knobs(HJ_PAIR=2, HJ_AUTOTUNE=1, HJ_AUTOTUNE_MIN_MCELLS=0, HJ_EPS_FUSE_MIN_CELLS=0),
          ("fused_pair_kernel", "fused_flat4_kernel", "fused_pair4_kernel"), ALL),
    Knobs("tiled", IR.knobs(HJ_PAIR=0, HJ_AUTOTUNE=1, HJ_AUTOTUNE_MIN_MCELLS=0, HJ_EPS_FUSE_MIN_CELLS=0), ("fused_substep_kernel",), ALL),
    Knobs("fuse12", IR.knobs(HJ_PAIR=2, HJ_FUSE12=1), ("fused12",), ("dubins64", "dubins32", "dint64", "ring64")),
    Knobs("xp", IR.knobs(HJ_PAIR=2, HJ_XP=2, HJ_TILE_CELLS=96), ("HamDubinsRelX",), ("dubins64", "dubins32", "ring64")),
    Knobs("direct", IR.knobs(HJ_FORCE_DIRECT=1), ("direct_substep_kernel",), ALL),
    # (the size rule does not apply to 4-D grids)
    Knobs("below", IR.knobs(HJ_DIRECT_BELOW=2000000000), ("direct_substep_kernel",), ("dubins64", "dubins32", "dint64", "ring64")),
)}
DEFAULT_SEEDS = (0, 1, 2, 3)
DEFAULT_N = 60


# ------------------------------------------------------------------------------------------------ problems (grid, data)
class Problem(object):
    """One grid with its NumPy data and coordinate tables: made once and shared, never written."""
    cache = {}

    def __init__(self, case):
        import levelsetpy_amd as L
        from oracle import hj_oracle as O
        N, per, ham = case.N, case.periodic, case.ham
        lo, hi = (list(v) for v in BOX[ham])
        hi = [hi[d] - (hi[d] - lo[d]) / N[d] if d in per else hi[d] for d in range(len(N))]
        self.case = case
        self.g = L.createGrid(np.asarray(lo).reshape(-1, 1), np.asarray(hi).reshape(-1, 1), np.asarray(N, dtype=np.int64).reshape(-1, 1),
                              list(per) if per else None)
        self.og = og = O.Grid(lo, hi, [int(n) for n in N], list(per))
        rng = np.random.default_rng(77 + 1000 * len(N) + int(np.sum(N)))
        base = {0: lambda: O.shape_cylinder(og, 2, None, .5), 1: lambda: O.shape_sphere(og, None, .45), 2: lambda: O.shape_sphere(og, None, 1.5)}[ham]()
        last = len(N) - 1
        self.arrays = {
            "y": base + 0.05 * np.sin(3 * og.xs[0]) * np.cos(2 * og.xs[last]) + 0.02 * rng.standard_normal(N),
            "y0": base + 0.03 * np.cos(2 * og.xs[0]) + 0.01 * rng.standard_normal(N),
            "other": base - 0.04 + 0.05 * rng.standard_normal(N),
            "obst": 0.3 - np.abs(og.xs[0] * np.ones(N)) + 0.02 * rng.standard_normal(N),
        }
        self.vs = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in self.g.vs]
        self.oracle_refs = {}

    @classmethod
    def get(cls, case):
        if case.name not in cls.cache:
            cls.cache[case.name] = cls(case)
        return cls.cache[case.name]

    def coords(self, which):
        return [v if which == "base" else np.ascontiguousarray(v * 1.01) for v in self.vs]

    def aux(self, which):
        """The trig tables of the built-in systems from the BASE coordinates: NumPy's (what DeviceGrid uploads), or those scaled."""
        vs, nd = self.vs, len(self.vs)
        tabs = {3: lambda: [np.cos(vs[2]), np.sin(vs[2])], 4: lambda: [np.sin(vs[0]), np.cos(vs[0]), np.sin(vs[2]), np.cos(vs[2])]}.get(nd, lambda: [])()
        return [np.ascontiguousarray(t * (0.9 if which == "pert" else 1.0)) for t in tabs]


# ------------------------------------------------------------------------------------------------ the model
INITIAL_SETTINGS = {
    "stream": "main", "coords": "base", "aux": "numpy", "slab": (0, 0), "diss": _ffi.DISS_GLF, "post_step": _ffi.POST_NONE,
    "post_arrays": None,          # or (op_a, array name, op_b, array name or None)
    "eps_source": None, "range_source": None, "axis0_pad": 0, "record": 1,
}
INPUT_ARRAYS = ("y", "y0", "other", "obst")
STATE_ARRAYS = ("s1", "s2", "out")       # written by ops, read by later ones


class Model(object):
    """What a context's outputs may depend on besides a call's arguments and arrays: the sticky settings in force -- and what the test
    knows about the context: the arrays written so far and the bound every live slot must hold."""

    def __init__(self, case):
        self.case = case
        self.settings = dict(INITIAL_SETTINGS)
        self.written = set(INPUT_ARRAYS)
        self.slots = {}           # slot -> the step index that wrote it (sequence()) or the (stepBound, alpha maxima) it must hold (GPU run)

    def apply(self, step):
        self.settings.update(step.op.sets(step.p))
        self.written.update(step.op.writes)

    def satisfied(self, needs):
        return all(self.settings[k] == v for k, v in needs.items())


Step = namedtuple("Step", "op p needs")


class Op(object):
    """One row of the table.  calls: the C entry points it issues; reads / writes: named arrays; draw(rng, case, model) -> (p, needs) or None
    when the op does not apply here; run(st, p) -> outputs; sets(p) -> the settings it leaves changed; slot(p) -> the bound slot it
    writes (None: none); refused: every call of the op must return non-zero; model_ref: there is no fresh-context run (the op reads
    what earlier ops left: its reference is the model)."""

    def __init__(self, name, calls, run, draw=None, reads=("y",), writes=(), sets=None, slot=None, refused=False, model_ref=False,
                 applies=None):
        self.name, self.calls, self.run = name, tuple(calls), run
        self.draw = draw or (lambda rng, case, model: ({}, {}))
        self.reads, self.writes = tuple(reads), tuple(writes)
        self.sets = sets or (lambda p: {})
        self.slot = slot or (lambda p: p.get("slot"))
        self.refused, self.model_ref = refused, model_ref
        self.applies = applies or (lambda case: True)

    def __repr__(self):
        return "Op(%s)" % self.name


# ------------------------------------------------------------------------------------------------ a context with its arrays
class State(object):
    """An hj_ctx (through DeviceGrid) under a knob set, its named arrays, and the streams the ops use."""

    def __init__(self, case, env, arrays=None):
        import torch
        from levelsetpy_amd.context import DeviceGrid
        self.torch, self.case, self.P = torch, case, Problem.get(case)
        with IR.environment(env):
            self.dg = DeviceGrid(self.P.g, case.dtype)
        self.dg.bind_stream()
        self.lib, self.ctx = self.dg.lib, self.dg.ctx
        self.main = self.dg._raw_stream(self.dg.device.index)
        self.side = None
        self.seen = set()          # every kernel symbol the launch record has reported
        if arrays is None:
            arrays = {k: torch.as_tensor(np.ascontiguousarray(v), device="cuda").to(self.dg.tdtype).contiguous() for k, v in self.P.arrays.items()}
            for k in STATE_ARRAYS + ("w0", "w1"):
                arrays[k] = torch.zeros_like(arrays["y"])
        self.A = arrays

    def close(self):
        self.dg._finalizer()       # hj_ctx_destroy now

    def par(self, pset):
        return _ffi.darr(PSETS[self.case.ham][pset])

    def zeros(self, shape=None):
        return self.torch.zeros(self.case.N if shape is None else shape, dtype=self.dg.tdtype, device="cuda")

    def bound(self, slot):
        sb, am = C.c_double(), (C.c_double * 4)()
        _ffi.check(self.lib.hj_read_step_bound(self.ctx, slot, C.byref(sb), am))
        return (sb.value, tuple(am)[:len(self.case.N)])

    def note_record(self):
        rec = IR.read_record(self.lib, self.ctx)
        self.seen |= rec
        return rec


def clone_arrays(A):
    return {k: v.clone() for k, v in A.items()}


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def ok(rc):
    _ffi.check(rc)


# ------------------------------------------------------------------------------------------------ replay
def apply_setting(st, key, value):
    """Write one sticky setting through its setter."""
    lib, ctx, P = st.lib, st.ctx, st.P
    if key == "stream":
        if value == "side" and st.side is None:
            st.side = st.torch.cuda.Stream()
        ok(lib.hj_ctx_set_stream(ctx, C.c_void_p(st.main if value == "main" else st.side.cuda_stream)))
    elif key == "coords":
        for d, v in enumerate(P.coords(value)):
            ok(lib.hj_ctx_set_coords(ctx, d, v.ctypes.data_as(_ffi._pd)))
    elif key == "aux":
        if value != "libm":
            for slot, tab in enumerate(P.aux(value)):
                ok(lib.hj_ctx_set_aux(ctx, slot, tab.ctypes.data_as(_ffi._pd), tab.size))
    elif key == "slab":
        ok(lib.hj_ctx_set_slab(ctx, value[0], value[1]))
    elif key == "diss":
        ok(lib.hj_ctx_set_dissipation(ctx, value))
    elif key == "post_step":
        ok(lib.hj_ctx_set_post_step(ctx, value))
    elif key == "post_arrays":
        if value is None:
            ok(lib.hj_ctx_set_post_arrays(ctx, 0, None, 0, None))
        else:
            op_a, a, op_b, b = value
            ok(lib.hj_ctx_set_post_arrays(ctx, op_a, ptr(st.A[a]), op_b, ptr(st.A[b]) if b else None))
    elif key == "eps_source":
        ok(lib.hj_ctx_set_weno_eps_source(ctx, ptr(st.A[value]) if value else None))
    elif key == "range_source":
        ok(lib.hj_ctx_set_range_source(ctx, ptr(st.A[value]) if value else None))
    elif key == "axis0_pad":
        assert value == 0          # (only the deep-halo slab stepper reads the pad tables: EXCLUDED below)
    elif key == "record":
        ok(lib.hj_launch_record(ctx, value))
    else:
        raise KeyError(key)


REPLAY_ORDER = ("stream", "coords", "aux", "slab", "diss", "post_step", "post_arrays", "eps_source", "range_source", "axis0_pad", "record")


def replay(st, settings):
    """Put exactly `settings` on the (fresh) context of `st`: every setter once, coordinates before the tables they reset."""
    assert set(settings) == set(REPLAY_ORDER)
    for key in REPLAY_ORDER:
        apply_setting(st, key, settings[key])


# ------------------------------------------------------------------------------------------------ the ops
def _substep(st, scheme, pset, stage, restrict, y, y0, out, slot, p0, p1, dt=DT):
    return st.lib.hj_rk_substep(st.ctx, scheme, st.case.ham, st.par(pset), 0., stage, dt, restrict, ptr(y), ptr(y0), ptr(out), slot, p0, p1)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _free_slot(rng):
    return int(rng.integers(USER_SLOTS))


def d_lf_term(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2)), restrict=_pick(rng, (0, 1, -1))), {}


def d_lf_term_base(rng, case, model):
    """hj_lf_term under the settings the oracle knows: base coordinates, NumPy's tables, the global bound; ENO2 / ENO3."""
    needs = {"coords": "base", "diss": _ffi.DISS_GLF}
    if len(case.N) >= 3:
        needs["aux"] = "numpy"
    return dict(scheme=_pick(rng, (_ffi.ENO2, _ffi.ENO3)), pset=int(rng.integers(2)), restrict=_pick(rng, (0, 1, -1))), needs


def r_lf_term(st, p):
    ydot, sb = st.zeros(), C.c_double()
    ok(st.lib.hj_lf_term(st.ctx, p["scheme"], st.case.ham, st.par(p["pset"]), 0., p["restrict"], ptr(st.A["y"]), ptr(ydot), C.byref(sb)))
    return ydot, sb.value


def d_substep_first(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2)), stage=_pick(rng, STAGES[:2]), restrict=_pick(rng, (0, 0, 1, -1)),
                slot=_free_slot(rng), split=bool(rng.integers(2))), {}


def d_substep_later(rng, case, model):
    p, needs = d_substep_first(rng, case, model)
    p["stage"] = _pick(rng, STAGES[2:])
    return p, needs


def _ranges(case, split):
    n0 = case.N[0]
    return [(0, n0 // 2), (n0 // 2, n0)] if split else [(0, n0)]


def r_substep_first(st, p):
    """YDOT / EULER of y into s1, over the whole range or over two plane ranges (the slot then holds the second range's bound)."""
    for p0, p1 in _ranges(st.case, p["split"]):
        ok(_substep(st, p["scheme"], p["pset"], p["stage"], p["restrict"], st.A["y"], None, st.A["s1"], p["slot"], p0, p1))
    return (st.A["s1"],) + st.bound(p["slot"])


def r_substep_later(st, p):
    """A stage that combines with y0: stencil input s1, y0 = y, into s2."""
    for p0, p1 in _ranges(st.case, p["split"]):
        ok(_substep(st, p["scheme"], p["pset"], p["stage"], p["restrict"], st.A["s1"], st.A["y"], st.A["s2"], p["slot"], p0, p1))
    return (st.A["s2"],) + st.bound(p["slot"])


def d_read_bound(rng, case, model):
    live = sorted(model.slots)
    if not live:
        return None
    return dict(slot=_pick(rng, live)), {}


def r_read_bound(st, p):
    return st.bound(p["slot"])


def d_rk_step(post):
    def draw(rng, case, model):
        p = dict(order=_pick(rng, (1, 2, 3)), scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2)), restrict=_pick(rng, (0, 0, -1)))
        if post is None:
            return p, {}
        if post:
            return p, {"post_step": _pick(rng, (_ffi.POST_MIN_PREV, _ffi.POST_MAX_PREV)),
                       "post_arrays": _pick(rng, ((1, "other", 3, "obst"), (2, "other", 0, None)))}
        return p, {"post_step": _ffi.POST_NONE, "post_arrays": None}
    return draw


def r_rk_step(st, p):
    tout, dtout = C.c_double(), C.c_double()
    A = st.A
    ok(st.lib.hj_rk_step(st.ctx, p["order"], p["scheme"], st.case.ham, st.par(p["pset"]), 0.25, 1e9, 0.8, 1e300, p["restrict"], ptr(A["y"]), ptr(A["out"]),
                         ptr(A["w0"]), ptr(A["w1"]), C.byref(tout), C.byref(dtout)))
    return A["out"], tout.value, dtout.value


def d_stage12(rng, case, model):
    return dict(scheme=_pick(rng, (_ffi.ENO2, _ffi.ENO3, _ffi.WENO5_ASSHIPPED)), pset=int(rng.integers(2)), coef=_pick(rng, ((.75, .25), (.5, .5))),
                slot=_free_slot(rng)), {}


def r_stage12(st, p):
    ok(st.lib.hj_rk_stage12(st.ctx, p["scheme"], st.case.ham, st.par(p["pset"]), DT, p["coef"][0], p["coef"][1], ptr(st.A["y"]), ptr(st.A["s2"]), p["slot"]))
    return (st.A["s2"],) + st.bound(p["slot"])


def d_rk_plan(rng, case, model):
    return dict(order=_pick(rng, (1, 2, 3)), scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2))), {}


def r_rk_plan(st, p):
    nl, fused = C.c_int(-1), C.c_int(-1)
    ok(st.lib.hj_rk_plan(st.ctx, p["order"], p["scheme"], st.case.ham, st.par(p["pset"]), 0, C.byref(nl), C.byref(fused)))
    return nl.value, fused.value


def d_integrate(rng, case, model):
    return dict(order=_pick(rng, (1, 2, 3)), scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2))), {}


def r_integrate(st, p):
    a, b, w = st.zeros(), st.zeros(), st.zeros()
    tout, steps, where = C.c_double(), C.c_int64(), C.c_int()
    ok(st.lib.hj_rk_integrate(st.ctx, p["order"], p["scheme"], st.case.ham, st.par(p["pset"]), 0., 1e9, 0.8, 1e300, 0, ptr(st.A["y"]), ptr(a), ptr(b), ptr(w),
                              3, -1., C.byref(tout), C.byref(steps), C.byref(where)))
    assert steps.value == 3 and where.value in (1, 2)
    return (a if where.value == 1 else b), tout.value, steps.value, where.value


def _static(st, pset):
    sb, am = C.c_double(), (C.c_double * 4)()
    ok(st.lib.hj_static_step_bound(st.ctx, st.case.ham, st.par(pset), C.byref(sb), am))
    return (sb.value, tuple(am)[:len(st.case.N)])


def r_static_aba(st, p):
    a, b, a2 = _static(st, 0), _static(st, 1), _static(st, 0)
    assert a == a2 and a[0] != b[0], (a, b, a2)
    return a + b + a2


def r_max_d1sq(st, p):
    out = st.zeros((4,))
    ok(st.lib.hj_max_d1sq(st.ctx, ptr(st.A["y"]), ptr(out)))
    return (out,)


def d_eps_source(rng, case, model):
    return dict(pset=int(rng.integers(2)), slot=_free_slot(rng)), {}


def r_eps_source(st, p):
    """The intended WENO5 with a caller-reduced epsilon, as the slab steppers run it: set, one substep, cleared."""
    eps = st.zeros((4,))
    ok(st.lib.hj_max_d1sq(st.ctx, ptr(st.A["y"]), ptr(eps)))
    ok(st.lib.hj_ctx_set_weno_eps_source(st.ctx, ptr(eps)))
    try:
        ok(_substep(st, _ffi.WENO5, p["pset"], _ffi.STAGE_EULER, 0, st.A["y"], None, st.A["s1"], p["slot"], 0, st.case.N[0]))
    finally:
        ok(st.lib.hj_ctx_set_weno_eps_source(st.ctx, None))
    return (st.A["s1"], eps) + st.bound(p["slot"])


def d_minmax(rng, case, model):
    return dict(op=_pick(rng, (_ffi.OP_MIN, _ffi.OP_MAX, _ffi.OP_MAX_NEG))), {}


def r_minmax(st, p):
    w = st.A["y"].clone()
    ok(st.lib.hj_minmax_with(st.ctx, p["op"], ptr(w), ptr(st.A["other"]), w.numel()))
    return (w,)


def d_any_nan(rng, case, model):
    return dict(nan=bool(rng.integers(2))), {}


def r_any_nan(st, p):
    a, has = st.A["y"].clone(), C.c_int(-1)
    if p["nan"]:
        a.view(-1)[a.numel() - 3] = float("nan")
    ok(st.lib.hj_any_nan(st.ctx, ptr(a), a.numel(), C.byref(has)))
    assert has.value == int(p["nan"])
    return (has.value,)


def d_upwind(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), dim=int(rng.integers(len(case.N)))), {}


def r_upwind(st, p):
    dL, dR, mm = st.zeros(), st.zeros(), (C.c_double * 4)()
    ok(st.lib.hj_upwind(st.ctx, p["scheme"], p["dim"], ptr(st.A["y"]), ptr(dL), ptr(dR), mm))
    return (dL, dR) + tuple(mm)


def d_ghost(rng, case, model):
    return dict(dim=int(rng.integers(len(case.N))), width=_pick(rng, (1, 3))), {}


def r_ghost(st, p):
    shape = list(st.case.N)
    shape[p["dim"]] += 2 * p["width"]
    out = st.zeros(shape)
    ok(st.lib.hj_ghost(st.ctx, p["dim"], p["width"], ptr(st.A["y"]), ptr(out)))
    return (out,)


def d_split(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), with_ham=bool(rng.integers(2))), {}


def r_split(st, p):
    """hj_lf_split_begin / hj_lf_split_end around a caller's Hamiltonian, scalar alphas."""
    nd = len(st.case.N)
    dL, dR = [st.zeros() for _ in range(nd)], [st.zeros() for _ in range(nd)]
    mm = (C.c_double * (4 * nd))()
    ok(st.lib.hj_lf_split_begin(st.ctx, p["scheme"], ptr(st.A["y"]), ptrs(dL), ptrs(dR), mm))
    out, sb, am = st.zeros(), C.c_double(), (C.c_double * 4)()
    ok(st.lib.hj_lf_split_end(st.ctx, ptrs(dL), ptrs(dR), None, _ffi.darr([0.5 + 0.25 * d for d in range(nd)]),
                              ptr(st.A["other"]) if p["with_ham"] else None, ptr(out), C.byref(sb), am))
    return tuple(dL) + tuple(dR) + tuple(mm) + (out, sb.value) + tuple(am)[:nd]


def d_combine(rng, case, model):
    return dict(mode=_pick(rng, (1, 2, 3, 4))), {}


def r_combine(st, p):
    out = st.zeros()
    ok(st.lib.hj_rk_combine(st.ctx, p["mode"], DT, ptr(st.A["y0"]), ptr(st.A["y"]), ptr(st.A["other"]), ptr(out), out.numel()))
    return (out,)


def d_term(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), array=bool(rng.integers(2))), {}


def r_term_normal(st, p):
    out, sb = st.zeros(), C.c_double()
    ok(st.lib.hj_term_normal(st.ctx, p["scheme"], ptr(st.A["y"]), ptr(st.A["other"]) if p["array"] else None, 0.7, ptr(out), C.byref(sb)))
    return out, sb.value


def r_term_reinit(st, p):
    out, sb = st.zeros(), C.c_double()
    ok(st.lib.hj_term_reinit(st.ctx, p["scheme"], ptr(st.A["y"]), ptr(st.A["y0"]), int(p["array"]), ptr(out), C.byref(sb)))
    return out, sb.value


def r_term_convection(st, p):
    nd = len(st.case.N)
    out, sb = st.zeros(), C.c_double()
    vel = [st.A["other"] if p["array"] else None] + [None] * (nd - 1)
    ok(st.lib.hj_term_convection(st.ctx, p["scheme"], ptr(st.A["y"]), ptrs(vel), _ffi.darr([0.4, -0.2, 0.5, 0.3][:nd]), ptr(out), C.byref(sb)))
    return out, sb.value


def d_curv(rng, case, model):
    return dict(array=bool(rng.integers(2))), {}


def r_term_curvature(st, p):
    out, sb = st.zeros(), C.c_double()
    b = st.A["other"].abs() if p["array"] else None
    ok(st.lib.hj_term_curvature(st.ctx, ptr(st.A["y"]), ptr(b), 0.6, ptr(out), C.byref(sb)))
    return out, sb.value


def r_hessian(st, p):
    nd = len(st.case.N)
    second = [st.zeros() if j <= i else None for i in range(nd) for j in range(nd)]
    first = [st.zeros() for _ in range(nd)]
    ok(st.lib.hj_hessian_second(st.ctx, ptr(st.A["y"]), ptrs(second), ptrs(first)))
    return tuple(t for t in second if t is not None) + tuple(first)


def r_second_order(st, p):
    """hj_curvature_second, hj_laplacian_second, hj_centered_first_second: one launch each of the kernel of hj_hessian_second."""
    k, m, lap, cen = st.zeros(), st.zeros(), st.zeros(), st.zeros()
    ok(st.lib.hj_curvature_second(st.ctx, ptr(st.A["y"]), ptr(k), ptr(m)))
    ok(st.lib.hj_laplacian_second(st.ctx, ptr(st.A["y"]), ptr(lap)))
    ok(st.lib.hj_centered_first_second(st.ctx, len(st.case.N) - 1, ptr(st.A["y"]), ptr(cen)))
    return k, m, lap, cen


def r_trace_hessian(st, p):
    nd = len(st.case.N)
    out, sb = st.zeros(), C.c_double()
    Ls = [0.5 + 0.1 * e for e in range(nd * nd)]
    Rs = [1.0 if e % (nd + 1) == 0 else 0.2 for e in range(nd * nd)]
    La = [st.A["other"] if (p["array"] and e == 0) else None for e in range(nd * nd)]
    ok(st.lib.hj_term_trace_hessian(st.ctx, ptr(st.A["y"]), ptrs(La) if p["array"] else None, _ffi.darr(Ls), None, _ffi.darr(Rs), ptr(out), C.byref(sb)))
    return out, sb.value


def setter(key, values, call):
    """A setter op: puts one sticky setting to a drawn value."""
    def draw(rng, case, model):
        return dict(value=_pick(rng, values)), {}

    def run(st, p):
        apply_setting(st, key, p["value"])
        return ()

    def sets(p):
        # new coordinates replace the trig tables by libm's (default_aux): the model follows
        return {key: p["value"], "aux": "libm"} if key == "coords" else {key: p["value"]}
    return Op("set_" + key, call, run, draw, reads=(), sets=sets)


def d_slab(rng, case, model):
    n0 = case.N[0]
    return dict(scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2)), stage=_pick(rng, STAGES[:2]), slot=_free_slot(rng),
                planes=_pick(rng, ((0, n0), (0, 3), (3, n0 - 3), (n0 - 3, n0)))), {}


def r_slab(st, p):
    """hj_ctx_set_slab(1, 1), a plane-range substep on an array with pad planes, hj_ctx_set_slab(0, 0)."""
    y = st.A["y"]
    pad = st.torch.cat([st.A["y0"][-3:], y, st.A["y0"][:3]]).contiguous()
    out = st.zeros()
    ok(st.lib.hj_ctx_set_slab(st.ctx, 1, 1))
    try:
        ok(_substep(st, p["scheme"], p["pset"], p["stage"], 0, pad[3:], None, out, p["slot"], p["planes"][0], p["planes"][1]))
        res = (out,) + st.bound(p["slot"])
    finally:
        ok(st.lib.hj_ctx_set_slab(st.ctx, 0, 0))
    return res


def d_stream(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2)), slot=_free_slot(rng)), {}


def r_stream(st, p):
    """hj_ctx_set_stream to a side stream, one substep there, and back."""
    st.torch.cuda.synchronize()           # the arrays were made on the main stream
    apply_setting(st, "stream", "side")
    try:
        ok(_substep(st, p["scheme"], p["pset"], _ffi.STAGE_EULER, 0, st.A["y"], None, st.A["s1"], p["slot"], 0, st.case.N[0]))
        res = (st.A["s1"],) + st.bound(p["slot"])
        ok(st.lib.hj_sync(st.ctx))
    finally:
        apply_setting(st, "stream", "main")
    return res


def d_record(rng, case, model):
    return dict(scheme=_pick(rng, SCHEMES), pset=int(rng.integers(2))), {"record": 1}


def r_record(st, p):
    """hj_launch_record off (a launch leaves no trace), on, a launch, read: the record holds that launch's kernels and nothing older."""
    st.note_record()
    ok(st.lib.hj_launch_record(st.ctx, 0))
    out = st.zeros()
    ok(_substep(st, p["scheme"], p["pset"], _ffi.STAGE_EULER, 0, st.A["y"], None, out, USER_SLOTS - 1, 0, st.case.N[0]))
    assert IR.read_record(st.lib, st.ctx) == set()
    ok(st.lib.hj_launch_record(st.ctx, 1))
    ok(_substep(st, p["scheme"], p["pset"], _ffi.STAGE_YDOT, 0, st.A["y"], None, out, USER_SLOTS - 1, 0, st.case.N[0]))
    rec = st.note_record()
    # (WHICH instantiation ran is launch state -- the tuner's business --, so the symbols themselves are no output)
    return out, len(rec) > 0


def range_ham(ndim):
    """A run-time Hamiltonian whose alpha reads the costate range (the body of test_bound_ring_reset_keeps_the_live_slots, any dimension)."""
    import levelsetpy_amd as L
    body = "H = par[0] * x[0] * p[1] + 0.5 * (%s);\n" % " + ".join("p[%d] * p[%d]" % (d, d) for d in range(ndim))
    for d in range(ndim):
        body += "alpha[%d] = fmax(fabs(dmin[%d]), fabs(dmax[%d]))%s;\n" % (d, d, d, " + fabs(par[0] * x[0])" if d == 1 else "")
    return L.register_native_hamiltonian("ctx_history_range_%dd" % ndim, ndim, body, nparams=1).ham_id


def d_range(rng, case, model):
    return dict(order=_pick(rng, (1, 2, 3)), par=_pick(rng, (0.7, 0.4))), {"diss": _pick(rng, (_ffi.DISS_GLF, _ffi.DISS_LLF, _ffi.DISS_LLLF))}


def r_range(st, p):
    """hj_range_pass, hj_rk_step, hj_rk_last_bounds, hj_rk_prev_bounds with a range-reading Hamiltonian under the dissipation kind in force;
    then hj_range_alpha_max (and, for the local kinds, hj_bound_pass) for the range of that pass, handed over as the range source."""
    ham, sid, par = range_ham(len(st.case.N)), _ffi.WENO5_ASSHIPPED, _ffi.darr([p["par"]])
    A, lib, ctx = st.A, st.lib, st.ctx
    keys = st.torch.zeros(2 * 4, dtype=st.torch.int64, device="cuda")
    ok(lib.hj_range_pass(ctx, sid, ham, par, ptr(A["y"]), ptr(keys)))
    tout, dtout = C.c_double(), C.c_double()
    ok(lib.hj_rk_step(ctx, p["order"], sid, ham, par, 0., 1e9, 0.8, 1e300, 0, ptr(A["y"]), ptr(A["out"]), ptr(A["w0"]), ptr(A["w1"]), C.byref(tout), C.byref(dtout)))
    sb, nb = (C.c_double * 4)(), C.c_int()
    ok(lib.hj_rk_last_bounds(ctx, sb, C.byref(nb)))
    assert nb.value == p["order"]
    sp, npv, dtp = (C.c_double * 4)(), C.c_int(), C.c_double()
    ok(lib.hj_rk_prev_bounds(ctx, sp, C.byref(npv), C.byref(dtp)))
    res = (A["out"], tout.value, dtout.value, nb.value) + tuple(sb)[:nb.value] + (npv.value,) + tuple(sp)[:npv.value]
    am = (C.c_double * 4)()
    ok(lib.hj_ctx_set_range_source(ctx, ptr(keys)))
    try:
        ok(lib.hj_range_alpha_max(ctx, ham, par, am))
        res += (keys,) + tuple(am)[:len(st.case.N)]
        kind = C.c_double()
        if p["diss"] != _ffi.DISS_GLF:
            ok(lib.hj_bound_pass(ctx, sid, ham, par, ptr(A["y"]), C.byref(kind)))
            res += (kind.value,)
    finally:
        ok(lib.hj_ctx_set_range_source(ctx, None))
    return res


def d_range_p(rng, case, model):
    p, needs = d_range(rng, case, model)
    p["diss"] = needs["diss"]
    return p, needs


def d_refused_alias(rng, case, model):
    live = sorted(s for s in model.slots if s < USER_SLOTS)
    return dict(slot=_pick(rng, live) if live else _free_slot(rng)), {}


def r_refused_alias(st, p):
    return (_substep(st, _ffi.ENO2, 0, _ffi.STAGE_EULER, 0, st.A["y"], None, st.A["y"], p["slot"], 0, st.case.N[0]),)


def r_refused_scheme(st, p):
    ydot, sb = st.zeros(), C.c_double(-1.)
    return (st.lib.hj_lf_term(st.ctx, 17, st.case.ham, st.par(0), 0., 0, ptr(st.A["y"]), ptr(ydot), C.byref(sb)), ydot, sb.value)


def r_refused_stage12(st, p):
    out = st.zeros()
    return (st.lib.hj_rk_stage12(st.ctx, _ffi.WENO5, st.case.ham, st.par(0), DT, .75, .25, ptr(st.A["y"]), ptr(out), p["slot"]), out)


def _le3(case):
    return len(case.N) <= 3


def _ge3(case):
    return len(case.N) >= 3


OPS = [
    Op("lf_term", ["hj_lf_term"], r_lf_term, d_lf_term, slot=lambda p: None),
    Op("lf_term_base_settings", ["hj_lf_term"], r_lf_term, d_lf_term_base, slot=lambda p: None),
    Op("substep_first", ["hj_rk_substep", "hj_read_step_bound"], r_substep_first, d_substep_first, writes=("s1",)),
    Op("substep_later", ["hj_rk_substep", "hj_read_step_bound"], r_substep_later, d_substep_later, reads=("y", "s1"), writes=("s2",)),
    Op("read_step_bound", ["hj_read_step_bound"], r_read_bound, d_read_bound, reads=(), slot=lambda p: None, model_ref=True),
    Op("rk_step", ["hj_rk_step"], r_rk_step, d_rk_step(None), writes=("out",)),
    Op("rk_step_plain", ["hj_rk_step"], r_rk_step, d_rk_step(False), writes=("out",)),
    Op("rk_step_post", ["hj_rk_step"], r_rk_step, d_rk_step(True), reads=("y", "other", "obst"), writes=("out",)),
    Op("rk_stage12", ["hj_rk_stage12", "hj_read_step_bound"], r_stage12, d_stage12, writes=("s2",), applies=_le3),
    Op("rk_plan", ["hj_rk_plan"], r_rk_plan, d_rk_plan, reads=()),
    Op("rk_integrate", ["hj_rk_integrate"], r_integrate, d_integrate),
    Op("static_step_bound_aba", ["hj_static_step_bound"], r_static_aba, reads=()),
    Op("max_d1sq", ["hj_max_d1sq"], r_max_d1sq),
    Op("weno_eps_source", ["hj_max_d1sq", "hj_ctx_set_weno_eps_source", "hj_rk_substep"], r_eps_source, d_eps_source, writes=("s1",)),
    Op("minmax_with", ["hj_minmax_with"], r_minmax, d_minmax, reads=("y", "other")),
    Op("any_nan", ["hj_any_nan"], r_any_nan, d_any_nan),
    Op("upwind", ["hj_upwind"], r_upwind, d_upwind),
    Op("ghost", ["hj_ghost"], r_ghost, d_ghost),
    Op("lf_split", ["hj_lf_split_begin", "hj_lf_split_end"], r_split, d_split, reads=("y", "other")),
    Op("rk_combine", ["hj_rk_combine"], r_combine, d_combine, reads=("y", "y0", "other")),
    Op("term_normal", ["hj_term_normal"], r_term_normal, d_term, reads=("y", "other")),
    Op("term_reinit", ["hj_term_reinit"], r_term_reinit, d_term, reads=("y", "y0")),
    Op("term_convection", ["hj_term_convection"], r_term_convection, d_term, reads=("y", "other")),
    Op("term_curvature", ["hj_term_curvature"], r_term_curvature, d_curv, reads=("y", "other")),
    Op("hessian_second", ["hj_hessian_second"], r_hessian),
    Op("second_order", ["hj_curvature_second", "hj_laplacian_second", "hj_centered_first_second"], r_second_order),
    Op("term_trace_hessian", ["hj_term_trace_hessian"], r_trace_hessian, d_curv, reads=("y", "other")),
    setter("diss", (_ffi.DISS_GLF, _ffi.DISS_LLF, _ffi.DISS_LLLF), ["hj_ctx_set_dissipation"]),
    setter("coords", ("base", "pert"), ["hj_ctx_set_coords"]),
    setter("aux", ("numpy", "pert"), ["hj_ctx_set_aux"]),
    setter("post_step", (_ffi.POST_NONE, _ffi.POST_MIN_PREV, _ffi.POST_MAX_PREV), ["hj_ctx_set_post_step"]),
    setter("post_arrays", (None, (1, "other", 3, "obst"), (2, "other", 0, None), (3, "obst", 1, "other")), ["hj_ctx_set_post_arrays"]),
    Op("slab", ["hj_ctx_set_slab", "hj_rk_substep", "hj_read_step_bound"], r_slab, d_slab, reads=("y", "y0")),
    Op("stream", ["hj_ctx_set_stream", "hj_rk_substep", "hj_sync"], r_stream, d_stream, writes=("s1",)),
    Op("launch_record", ["hj_launch_record", "hj_launch_record_read", "hj_rk_substep"], r_record, d_record, slot=lambda p: USER_SLOTS - 1),
    Op("range_step", ["hj_range_pass", "hj_rk_step", "hj_rk_last_bounds", "hj_rk_prev_bounds", "hj_ctx_set_range_source", "hj_range_alpha_max",
                      "hj_bound_pass"], r_range, d_range_p, writes=("out",), slot=lambda p: None,
       # (its kernels are compiled at run time, a second or two each: on the two fp64 3-D grids only)
       applies=lambda case: case.name in ("dubins64", "ring64")),
    Op("refused_alias", ["hj_rk_substep"], r_refused_alias, d_refused_alias, slot=lambda p: None, refused=True),
    Op("refused_scheme", ["hj_lf_term"], r_refused_scheme, slot=lambda p: None, refused=True),
    Op("refused_stage12", ["hj_rk_stage12"], r_refused_stage12, lambda rng, case, model: (dict(slot=_free_slot(rng)), {}), slot=lambda p: None, refused=True),
]
OPS[[o.name for o in OPS].index("set_aux")].applies = _ge3          # (the 2-D system reads no table)
BY_NAME = {o.name: o for o in OPS}
SETTERS = {"diss": BY_NAME["set_diss"], "coords": BY_NAME["set_coords"], "aux": BY_NAME["set_aux"], "post_step": BY_NAME["set_post_step"],
           "post_arrays": BY_NAME["set_post_arrays"]}
# settings the group ops change and restore themselves: never left changed between two steps
GROUP_SETTINGS = ("stream", "slab", "eps_source", "range_source", "axis0_pad", "record")
# the slots the library writes itself (the contract): an op that issues these calls voids what the model knows about them
LIBRARY_SLOTS = {"lf_term": (63,), "lf_term_base_settings": (63,), "refused_scheme": (), "range_step": (60, 61, 62)}

# Entry points that take an hj_ctx* and are in no op, each with its reason.
EXCLUDED = {
    "hj_ctx_create": "the harness: every State makes one",
    "hj_ctx_destroy": "the harness: every fresh State ends in one",
    "hj_ctx_set_axis0_pad": "the pad tables are read by launches beyond planes [0, N0) only, which the deep-halo slab stepper alone issues: needs a communicator",
    "hj_comm_init": "needs a communicator", "hj_comm_destroy": "needs a communicator", "hj_comm_info": "needs a communicator",
    "hj_comm_init_external": "needs a communicator's neighbours", "hj_halo_exchange": "needs a communicator",
    "hj_halo_exchange_depth": "needs a communicator", "hj_slab_join": "needs a communicator", "hj_slab_rk_step": "needs a communicator",
    "hj_slab_rk_step_deep": "needs a communicator",
    "hj_last_kernel": "reports the hidden launch state by design (the tuner test reads it)",
    "hj_last_launch": "reports the hidden launch state by design", "hj_last_tile": "reports the hidden launch state by design (the tuner test reads it)",
    "hj_ctx_state_generation": "a counter of setter calls: a function of the history by design",
}


def header_ctx_entry_points(path=HEADER):
    """Every function of the header that takes an hj_ctx* (hj_ctx** for hj_ctx_create)."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(set(m.group(1) for m in re.finditer(r"\b(hj_\w+)\s*\(\s*hj_ctx\s*\*", text)))


# ------------------------------------------------------------------------------------------------ sequences
def applicable(case):
    return [o for o in OPS if o.applies(case)]


def sequence(seed, case_name, n=DEFAULT_N):
    """A seeded list of n Steps for the case: every applicable op once in a shuffled order, then drawn at random; the settings a step
    needs are put in force by setter steps in front of it, and a step is only taken when every array it reads has been written."""
    case = CASES[case_name]
    rng = np.random.default_rng([seed, sorted(CASES).index(case_name)])
    ops = applicable(case)
    order = [ops[i] for i in rng.permutation(len(ops))]
    model, steps, k = Model(case), [], 0
    while len(steps) < n:
        op = order[k] if k < len(order) else _pick(rng, ops)
        k += 1
        if not set(op.reads) <= model.written:
            if k <= len(order):
                order.append(op)          # later, once its inputs exist
            continue
        drawn = op.draw(rng, case, model)
        if drawn is None:
            if k <= len(order):
                order.append(op)
            continue
        p, needs = drawn
        todo, ahead = [], dict(model.settings)
        for key in REPLAY_ORDER:          # (coordinates before the tables they reset: each setter is applied to `ahead` before the next key is looked at)
            if key in needs and ahead[key] != needs[key]:
                assert key in SETTERS, "no setter op for %s" % key
                todo.append(Step(SETTERS[key], dict(value=needs[key]), {}))
                ahead.update(SETTERS[key].sets(todo[-1].p))
        assert all(ahead[key] == v for key, v in needs.items()), (op.name, needs, ahead)
        for s in todo + [Step(op, p, needs)]:
            steps.append(s)
            model.apply(s)
            note_slots(model, s, len(steps) - 1)
    return steps[:n]


def note_slots(model, step, value):
    """The model's slots after `step`: the slot it wrote holds `value`; what the library's own slots held is void."""
    for s in LIBRARY_SLOTS.get(step.op.name, ()):
        model.slots.pop(s, None)
    slot = step.op.slot(step.p)
    if slot is not None and not step.op.refused:
        model.slots[slot] = value


def describe(steps, upto=None):
    return ", ".join("%d:%s" % (i, s.op.name) for i, s in enumerate(steps[:upto]))
