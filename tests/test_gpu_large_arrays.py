"""GPU: the solver library on arrays past 2 GiB, 4 GiB and 2^31 cells -- the sizes at which it changes behaviour (hj_api.hip choose_chunks:
one buffer descriptor below 4 GiB; hj_split.h: 64-bit index decoding from 2^31 cells; hj_inst.hip / hj_instx.hip: kernels switched off there;
the refusals of hj_rk_stage12 and hj_ctx_create).  tests/test_large_plans.py pins what is PLANNED for these shapes without a device; here the
launches run, each test asserts the kernel and chunking it meant to run, and the results are compared with the NumPy oracle on boxes
(tests/box_ref.py): the corners of the grid, every chunk seam the launch reports, the cells at flat byte offsets 2^31, 2^32, 2^33 and at flat
element offset 2^31, and seeded random places.

Data: the system's usual cylinder / sphere plus 0.05 * U(-1, 1) noise (no two cells share a neighbourhood), written on the device in blocks of
at most 2^26 cells; box inputs and outputs are gathered from the device tensors.  No test holds more than 48 GiB; one that finds less than its
need + 8 GiB free skips and says so.  HJ_LARGE_ARRAYS_PROFILE=<file> makes the run write what it measured (profiles/large_arrays.txt).

Boxes: at most 24 a case.  In 4-D the 16 corners leave room for ONE box per chunk seam (alternately across a tile seam and elsewhere) and two
random ones; everywhere else every seam gets both and there are four random boxes.  A launch cut into more chunks than that leaves room for
(the 2-D grid at the default environment: 85) gets the first and the last seam and an even spread of the others.

The last section ("walk") is the 1-D to 6-D node walk of libhj_hishapes.so, libhj_resample.so and libhj_measure.so on a 6-D grid past 2^32
nodes, whose first two axes are head axes, and hjh_substep of libhj_hidim.so past 2^31 cells; its boxes are placed by walk_places."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi  # noqa: E402
from levelsetpy_amd.context import DeviceGrid  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402

import box_ref as B  # noqa: E402
from test_gpu_parity import close  # noqa: E402
from test_gpu_fp32 import _fp32_close  # noqa: E402
from test_large_plans import TABLE, XP_NAME, KNOBS, span_bytes  # noqa: E402

GiB = 1 << 30
BLOCK = 1 << 26
STAGES = [_ffi.STAGE_YDOT, _ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF, _ffi.STAGE_RK3_FULL]
STAGE_NAME = {0: "YDOT", 1: "EULER", 2: "RK3_HALF", 3: "RK3_FULL"}
TB1 = {"HJ_TARGET_BLOCKS": "1"}
# the schemes of case A: ENO2, ENO3 and the as-shipped WENO5 with the longest chunks the cap allows, and at the default environment, where the
# intended WENO5 runs too
ENV_SCHEMES = [(e, s) for e in ({}, TB1) for s in ("ENO2", "ENO3", "WENO5_ASSHIPPED", "WENO5") if not (e and s == "WENO5")]
ENV_SCHEME_IDS = ["%s-%s" % ("TB1" if e else "default", s) for e, s in ENV_SCHEMES]

SYSTEMS = {
    "dubins": dict(ham=_ffi.HAM_DUBINS_REL, par=[1., 1., 1., 2.], gmin=[-.75, -1.25, -np.pi], gmax=[3.25, 1.25, np.pi], pd=[2],
                   make=lambda g: O.DubinsRel(g, 1, 1), axes=(0, 1), radius=.5),
    "integrator": dict(ham=_ffi.HAM_DOUBLE_INTEGRATOR, par=[1.25, 0., 0., 0.], gmin=[-1., -1.5], gmax=[1., 1.5], pd=[],
                       make=lambda g: O.DoubleIntegrator(g, 1.25), axes=(0, 1), radius=.45),
    "pendulum": dict(ham=_ffi.HAM_DOUBLE_PENDULUM, par=[1., 0., 0., 0.], gmin=[-np.pi, -8., -np.pi, -8.], gmax=[np.pi, 8., np.pi, 8.],
                     pd=[0, 1, 2, 3], make=lambda g: O.DoublePendulum4D(g, 1.0), axes=(0, 1, 2, 3), radius=2.0),
}

REPORT = []          # lines of profiles/large_arrays.txt
HEADER = """Large arrays: the solver library and the stateless libraries past 2 GiB, 4 GiB, 2^31 cells and (the 6-D node walk) 2^32 nodes
Written by tests/test_gpu_large_arrays.py (HJ_LARGE_ARRAYS_PROFILE=<this file>) on one %s; everything below this header is measured.

Per case: label (A..H as in the test file; TB1 = HJ_TARGET_BLOCKS=1, the longest chunks the 4 GiB cap allows; "tuner" = the untouched default
environment with the launch-time tile tuner on), shape, dtype, bytes, scheme, the kernel hj_last_kernel named, planes per chunk and tile
extents from hj_last_tile, boxes and cells compared with the NumPy oracle (tests/box_ref.py), the largest |kernel - oracle| / max(1, |oracle|)
over all stages of the case (0.00e+00: bit for bit), and for fp32 the largest error relative to max|oracle| and the largest share of a box's
cells beyond 2e-4 (test_gpu_fp32._fp32_close allows ENO 3e-3 of a box).  "wall" lines: seconds per test, the first test of a shape fills
its arrays; a later one finds them and the boxes' oracle values there.  "launch": the slowest substep launch of the case, between two events
on the stream.

"""
SKIPPED = []


def _report(line):
    REPORT.append(line)
    print(line, flush=True)


# ------------------------------------------------------------------ grids, data, memory
class Case(object):
    """A grid of one of the built-in systems: the product's Bundle (low_mem: no meshgrid), the oracle's light twin, the system."""

    def __init__(self, system, shape, dtype):
        s = SYSTEMS[system]
        self.system, self.shape, self.dtype, self.s = system, tuple(shape), dtype, s
        nd = len(shape)
        gmax = [s["gmax"][d] - (s["gmax"][d] - s["gmin"][d]) / shape[d] if d in s["pd"] else s["gmax"][d] for d in range(nd)]
        self.g = L.createGrid(np.array(s["gmin"]).reshape(-1, 1), np.array(gmax).reshape(-1, 1),
                              np.array(shape, dtype=np.int64).reshape(-1, 1), s["pd"] if s["pd"] else None, low_mem=True)
        self.G = B.light_grid(s["gmin"], gmax, shape, s["pd"])
        for a, b in zip(self.g.vs, self.G.vs):                 # the device's coordinates are the oracle's, bit for bit
            assert np.array_equal(np.asarray(a).ravel(), b.ravel())
        self.tdtype = torch.float64 if dtype == "f64" else torch.float32
        self.esz = 8 if dtype == "f64" else 4
        self.cells = int(np.prod(shape, dtype=np.int64))
        self.bytes = self.cells * self.esz
        self.bc = [1 if d in s["pd"] else 0 for d in range(nd)]

    def sb_closed_form(self):
        """stepBound of artificial_dissipation_glf with the per-axis maxima of alpha taken from the grid's vs (they separate per axis)."""
        vs = [v.ravel() for v in self.G.vs]
        dx = self.G.dx.ravel()
        if self.system == "dubins":
            a = [np.max(np.abs(1 - 1 * np.cos(vs[2]))) + np.max(np.abs(1 * vs[1])), np.max(np.abs(1 * np.sin(vs[2]))) + np.max(np.abs(1 * vs[0])), 2.]
        elif self.system == "integrator":
            a = [np.max(np.abs(vs[1])), 1.25]
        else:
            raise NotImplementedError(self.system)
        inv = 0
        for d in range(len(a)):
            inv += a[d] / dx.item(d)
        return float(1 / inv)

    def dt(self):
        """A step well inside every case's CFL bound (the pendulum's |f| <= ~ 8^2 * 2 + 4 g)."""
        if self.system == "pendulum":
            dx = self.G.dx.ravel()
            return 0.4 / (8. / dx[0] + 170. / dx[1] + 8. / dx[2] + 170. / dx[3])
        return 0.4 * self.sb_closed_form()

    def fill(self, seed):
        """smooth + 0.05 * U(-1, 1), on the device, in blocks of at most 2^26 cells of the (N0 * N1, ...) view."""
        N = self.shape
        out = torch.empty(N, dtype=self.tdtype, device="cuda")
        nd = len(N)
        flat = out.view((N[0] * N[1],) + tuple(N[2:]))
        per_row = int(np.prod(N[2:], dtype=np.int64)) if nd > 2 else 1
        rows = max(1, BLOCK // per_row)
        assert rows * per_row <= BLOCK
        gen = torch.Generator(device="cuda").manual_seed(seed)
        vs = [torch.as_tensor(v.ravel(), device="cuda") for v in self.G.vs]
        tail = 0
        for d in range(2, nd):
            if d in self.s["axes"]:
                tail = tail + (vs[d] ** 2).reshape([-1 if j == d else 1 for j in range(1, nd)])
        for r0 in range(0, N[0] * N[1], rows):
            r = torch.arange(r0, min(r0 + rows, N[0] * N[1]), device="cuda")
            sq = (vs[0][r // N[1]] ** 2 + vs[1][r % N[1]] ** 2).reshape([-1] + [1] * (nd - 2)) + tail
            full = (len(r),) + tuple(N[2:])                 # (the smooth part may be constant along an axis: the noise never is)
            blk = (sq.sqrt() - self.s["radius"]).expand(full)
            blk = blk + 0.05 * (2 * torch.rand(full, generator=gen, device="cuda", dtype=torch.float64) - 1)
            flat[r0:r0 + len(r)] = blk.to(self.tdtype)
        return out


def _need(nbytes, what):
    """Skip (and say so in the record) only when less than the need + 8 GiB is free."""
    assert nbytes <= 48 * GiB, (what, nbytes)
    held = sum(t.numel() * t.element_size() for t in _BUF.values() if torch.is_tensor(t))
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free + held < nbytes + 8 * GiB:
        msg = "%s needs %.1f GiB + 8 GiB, %.1f GiB free" % (what, nbytes / GiB, (free + held) / GiB)
        SKIPPED.append(msg)
        pytest.skip(msg)


_BUF = {}


def _arrays(case, extra=1):
    """y, y0 (two independent data arrays) and `extra` output / work arrays of the case's shape, kept while consecutive tests use the same
    shape and dtype and released when another one comes."""
    key = (case.system, case.shape, case.dtype)
    if _BUF.get("key") != key:
        _BUF.clear()
        torch.cuda.empty_cache()
        _need((2 + extra) * case.bytes + 3 * BLOCK * 8, "x".join(map(str, case.shape)) + " " + case.dtype)
        _BUF["key"] = key
        _BUF["y"] = case.fill(1234)
        _BUF["y0"] = case.fill(4321)
        for name in ("y", "y0"):                               # noise in every cell: differences along EVERY axis
            eps = eps_by_torch(case, _BUF[name])
            assert all(e > 0 for e in eps), (name, eps)
            _BUF["eps_" + name] = eps
    else:
        _need((2 + extra) * case.bytes, "x".join(map(str, case.shape)) + " " + case.dtype)
    outs = []
    for k in range(extra):
        if "w%d" % k not in _BUF:
            _BUF["w%d" % k] = torch.empty(case.shape, dtype=case.tdtype, device="cuda")
        outs.append(_BUF["w%d" % k])
    return _BUF["y"], _BUF["y0"], outs


@pytest.fixture(scope="module", autouse=True)
def _release_and_record():
    t0 = time.time()
    yield
    _BUF.clear()
    torch.cuda.empty_cache()
    path = os.environ.get("HJ_LARGE_ARRAYS_PROFILE")
    if path:
        with open(path, "w") as f:
            f.write(HEADER % torch.cuda.get_device_name(0))
            f.write("\n".join(REPORT) + "\n")
            f.write("skipped: %s\n" % ("; ".join(SKIPPED) if SKIPPED else "nothing"))
            f.write("module wall time %.1f s\n" % (time.time() - t0))


_FAULT = []


@pytest.fixture(autouse=True)
def _timed(request):
    """Wall time of every test; and after a device error (a fault shows at the next synchronisation at the latest) nothing more of this
    module is started on the GPU."""
    if _FAULT:
        pytest.fail("a device error earlier in this module (%s): not started" % _FAULT[0])
    t0 = time.perf_counter()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _FAULT.append(request.node.name)
        raise e
    _report("  wall %-90s %.3f s" % (request.node.name, time.perf_counter() - t0))


def _ctx(case, monkeypatch, env, autotune=False):
    """A fresh context: the environment knobs are read at hj_ctx_create."""
    for k in KNOBS + ("HJ_FUSE12",):
        monkeypatch.delenv(k, raising=False)
    if not autotune:
        monkeypatch.setenv("HJ_AUTOTUNE", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dg = DeviceGrid(case.g, "float64" if case.dtype == "f64" else "float32")
    dg.bind_stream()
    return dg


def _launched(dg):
    tile = (C.c_int * 4)()
    dg.lib.hj_last_tile(dg.ctx, tile)
    return dg.lib.hj_last_kernel(dg.ctx).decode(), [int(v) for v in tile]


def _substep(dg, case, scheme, stage, dt, y, y0, out, slot=3):
    _ffi.check(dg.lib.hj_rk_substep(dg.ctx, _ffi.SCHEME_IDS[scheme], case.s["ham"], _ffi.darr(case.s["par"]), 0., stage, dt, 0,
                                    dg.ptr(y), dg.ptr(y0) if stage >= _ffi.STAGE_RK3_HALF else None, dg.ptr(out), slot, 0, case.shape[0]))


# ------------------------------------------------------------------ boxes
def _extent(nd):
    return {2: (8, 24), 3: (8, 8, 16), 4: (8, 3, 3, 8)}[nd]


def _around(N, ext, centre):
    """A box of extents `ext` that holds the cell `centre`, as centred on it as the grid allows."""
    lo = [int(min(max(c - e // 2, 0), n - e)) for c, e, n in zip(centre, ext, N)]
    return lo, [l + e for l, e in zip(lo, ext)]


def place_boxes(case, kernel, tile, seed=99, cap=24):
    """[(kind, lo, hi)]: corners, chunk seams, offsets, random -- see the module docstring."""
    N, nd = case.shape, len(case.shape)
    ext = [min(e, n) for e, n in zip(_extent(nd), N)]
    rng = np.random.default_rng(seed)
    rand = lambda: [int(rng.integers(0, n - e + 1)) for n, e in zip(N, ext)]  # noqa: E731
    boxes = []
    for corner in range(1 << nd):
        lo = [(N[d] - ext[d]) if corner >> d & 1 else 0 for d in range(nd)]
        boxes.append(("corner", lo, [l + e for l, e in zip(lo, ext)]))
    # flat offsets
    offs = sorted(set([(1 << b) // case.esz for b in (31, 32, 33)] + [1 << 31]))
    for e in offs:
        if e >= case.cells:
            continue
        idx = [int(v) for v in np.unravel_index(e, N)]
        lo, hi = _around(N, ext, idx)
        boxes.append(("offset", lo, hi))
        if idx[-1] == 0:                     # a row (or plane) start: the cell before it in memory ends the previous row -- a box there too
            lo, hi = _around(N, ext, [int(v) for v in np.unravel_index(e - 1, N)])
            boxes.append(("offset-", lo, hi))
    # chunk seams on the axis of the march: planes [k * chunk - 4, k * chunk + 4)
    march = 1 if kernel == XP_NAME else 0
    chunk = tile[0]
    if chunk > 0:
        seams = list(range(1, (N[march] + chunk - 1) // chunk))
        room = None if cap is None else (cap - len(boxes) - (2 if nd == 4 else 4)) // (1 if nd == 4 else 2)
        if room is not None and len(seams) > room:
            # (a launch cut into more chunks than 24 boxes can visit -- the 2-D grid at the default environment, 85 chunks: the first and the
            #  last seam and an even spread of the others)
            seams = sorted(set(seams[int(round(j * (len(seams) - 1) / max(room - 1, 1)))] for j in range(room)))
        for j, k in enumerate(seams):
            kinds = ("seam+tile", "seam") if nd < 4 else (("seam",) if j % 2 else ("seam+tile",))
            for kind in kinds:
                lo = rand()
                if kind == "seam+tile":
                    # across the first tile seam of every tiled axis (the reported extents are cells per tile on axes 1..; on a transposed launch
                    # the tile's first extent lies along axis 0)
                    for a, d in enumerate([dd for dd in range(nd) if dd != march]):
                        E = tile[1 + a] if a + 1 < len(tile) else 0
                        if 0 < E < N[d]:
                            lo[d] = int(min(max(E - ext[d] // 2, 0), N[d] - ext[d]))
                hi = [l + e for l, e in zip(lo, ext)]
                lo[march], hi[march] = max(0, k * chunk - 4), min(N[march], k * chunk + 4)
                boxes.append((kind, lo, hi))
    for _ in range(2 if nd == 4 else 4):
        lo = rand()
        boxes.append(("random", lo, [l + e for l, e in zip(lo, ext)]))
    for kind, lo, hi in boxes:
        assert all(0 <= l < h <= n for l, h, n in zip(lo, hi, N)), (kind, lo, hi)
        assert int(np.prod([h - l for l, h in zip(lo, hi)])) <= 8 * 24 * 24
    assert cap is None or len(boxes) <= cap, len(boxes)
    # the kinds the shape has are all there
    kinds = set(k for k, _, _ in boxes)
    assert "corner" in kinds and "random" in kinds
    if chunk > 0 and chunk < N[march]:
        assert "seam+tile" in kinds and ("seam" in kinds or (nd == 4 and len(seams) == 1)), kinds
    assert ("offset" in kinds) == (case.bytes > (1 << 31))
    for e in offs:
        if e < case.cells:
            idx = np.unravel_index(e, N)
            assert any(k.startswith("offset") and all(l <= i < h for l, i, h in zip(lo, idx, hi)) for k, lo, hi in boxes), e
    return boxes


class Boxes(object):
    """The boxes of one case with their gathered inputs and, per scheme, the oracle's ydot -- computed once and shared by the stages."""

    def __init__(self, case, boxes, y, y0, m):
        self.case, self.m = case, m
        self.items = []
        for kind, lo, hi in boxes:
            idx, cmp = B.box(case.G, lo, hi, m)
            self.items.append(dict(kind=kind, lo=lo, hi=hi, idx=idx, cmp=cmp, y=B.gather(y, idx), y0=B.gather(y0, idx), ydot={}))
        self.cells = sum(int(np.prod([h - l for l, h in zip(b["lo"], b["hi"])])) for b in self.items)

    def ydot(self, b, scheme, eps=None):
        if scheme not in b["ydot"]:
            b["ydot"][scheme] = B.ydot(self.case.G, self.case.s["make"], scheme, b["idx"], b["y"], eps)
        return b["ydot"][scheme]


_BOXES = {}


def _boxes_for(case, kernel, tile, y, y0, m=B.M_SUBSTEP):
    key = (case.system, case.shape, case.dtype, kernel, tuple(tile), m)
    if key not in _BOXES:
        if len(_BOXES) > 6:
            _BOXES.clear()
        _BOXES[key] = Boxes(case, place_boxes(case, kernel, tile), y, y0, m)
    return _BOXES[key]


def compare(case, scheme, got, ref, what, stats, derivative=False):
    """fp64 ENO: array_equal; fp64 WENO5: test_gpu_parity.close at 1e-11; fp32: test_gpu_fp32._fp32_close against the fp64 oracle on the
    fp32-rounded input.  derivative=True (hj_upwind, hj_lf_split_begin: the derivative kernels contract a*b+c into FMAs, which the substep
    kernels' ENO path does not): the standing rule for fp64 derivatives, close at 1e-11, for every scheme (tests/test_gpu_parity.py).
    The figures go into `stats` before anything is asserted."""
    err = np.abs(got - ref)
    scale = max(1.0, float(np.max(np.abs(ref))))
    stats["max"] = max(stats.get("max", 0.0), float(err.max()) / scale)
    if case.dtype == "f32":
        rel = err / max(float(np.abs(ref).max()), 1e-30)
        stats["rel"] = max(stats.get("rel", 0.0), float(rel.max()))
        stats["share"] = max(stats.get("share", 0.0), float(np.mean(rel > 2e-4)))
        _fp32_close(got, ref, scheme, what)
    elif scheme.startswith("ENO") and not derivative:
        assert np.array_equal(got, ref), "%s: %d cells differ, max %.3e, first at %s" % (
            what, int((got != ref).sum()), float(err.max()), np.argwhere(got != ref)[:1].tolist())
    else:
        close(got, ref, 1e-11, what)


def check_stages(case, dg, scheme, stages, y, y0, out, want=None, eps=None, label=""):
    """Run each stage over the whole grid, assert the launch, compare on the boxes."""
    dt = case.dt()
    bx = None
    stats = {}
    for st in stages:
        out.fill_(float("nan"))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        _substep(dg, case, scheme, st, dt, y, y0, out)
        ev[1].record()
        torch.cuda.synchronize()
        stats["ms"] = max(stats.get("ms", 0.0), ev[0].elapsed_time(ev[1]))
        kernel, tile = _launched(dg)
        if want is not None:
            kern, chunks, chunk, tl = want
            assert kernel == kern, (kernel, want)
            if kern.startswith("fused_"):
                march = case.shape[1] if kernel == XP_NAME else case.shape[0]
                assert tile[0] == chunk and (march + chunk - 1) // chunk == chunks, (tile, want)
                assert [v for v in tile[1:] if v > 0] == tl, (tile, want)
        if kernel.startswith("fused_"):
            plan = {"kernel": kernel, "chunk_planes": tile[0]}
            assert span_bytes(list(case.shape), case.dtype, plan) < (1 << 32), (kernel, tile)
        else:
            assert tile == [0, 0, 0, 0], tile
        if bx is None:
            bx = _boxes_for(case, kernel, tile, y, y0)
        for b in bx.items:
            ref = B.stage_expr(st, dt, b["y"], b["y0"], bx.ydot(b, scheme, eps))[b["cmp"]]
            lo, hi = b["lo"], b["hi"]
            got = B.gather(out, [np.arange(l, h) for l, h in zip(lo, hi)])
            compare(case, scheme, got, ref, "%s %s %s box %s %s..%s" % (label, scheme, STAGE_NAME[st], b["kind"], lo, hi), stats)
    _report("%-10s %-14s %s %.3f GiB  %-16s %-40s chunk %d tile %s  boxes %d cells %d  launch %.2f ms  max err/scale %.2e%s" % (
        label, "x".join(map(str, case.shape)), case.dtype, case.bytes / GiB, scheme, kernel, tile[0], [v for v in tile[1:] if v > 0],
        len(bx.items), bx.cells, stats["ms"], stats["max"],
        "  fp32 max rel %.2e share beyond 2e-4 %.2e" % (stats["rel"], stats["share"]) if case.dtype == "f32" else ""))
    return kernel, tile


def eps_by_torch(case, y):
    """max over the unstripped first-divided-difference table of D1^2 per dim (O.max_d1_squared's formula) by plain torch in fp64, in
    blocks.  The ghost-to-ghost differences of an extrapolated axis repeat the first interior one in size and the periodic ones are interior
    pairs or the wrap pair, so the maximum runs over the forward differences, plus the wrap pair on a periodic axis."""
    N, nd = case.shape, len(case.shape)
    dx = case.G.dx.ravel()
    plane = case.cells // N[0]
    step = max(1, BLOCK // plane)
    m = [0.0] * nd
    for p in range(0, N[0], step):
        t = y[p:min(p + step + 1, N[0])].double()
        own = min(step, N[0] - p)
        if t.shape[0] > 1:
            m[0] = max(m[0], float((((1 / dx.item(0)) * (t[1:] - t[:-1])) ** 2).max()))
        for d in range(1, nd):
            a = t[:own]
            m[d] = max(m[d], float((((1 / dx.item(d)) * (a.narrow(d, 1, N[d] - 1) - a.narrow(d, 0, N[d] - 1))) ** 2).max()))
            if case.bc[d]:
                m[d] = max(m[d], float((((1 / dx.item(d)) * (a.select(d, 0) - a.select(d, N[d] - 1))) ** 2).max()))
        del t
    if case.bc[0]:
        m[0] = max(m[0], float((((1 / dx.item(0)) * (y[0].double() - y[N[0] - 1].double())) ** 2).max()))
    return m


# Where the chunk count is free (the default environment) it follows from the workgroups a CU holds: the dry plan takes them from the kernel's
# launch bound, a live context asks the runtime, so the plan's chunk count is an estimate there (documented: dist.plan_substep, hj_plan_substep
# in include/hj_mi355x.h).  The two differ for the fp32 ENO3 instantiation of the pair kernel: 4 chunks of 2050 planes on the device where the
# plan says 3 of 2734 (either keeps the span below 4 GiB; with HJ_TARGET_BLOCKS=1 the cap alone decides and they agree).  Kernel, tile and the
# span invariant are asserted from the plan all the same.
LIVE = {((8200, 512, 512), "f32", "ENO3"): ("fused_pair_kernel", 4, 2050, [16, 32])}


def _want(shape, dtype, env, scheme):
    if not env and (tuple(shape), dtype, scheme) in LIVE:
        return LIVE[(tuple(shape), dtype, scheme)]
    for N, dt, _ham, _bc, e, want in TABLE:
        if tuple(N) == tuple(shape) and dt == dtype and e == env:
            return want["light" if scheme in ("ENO2", "WENO5_ASSHIPPED") else "heavy"]
    raise KeyError((shape, dtype, env))


def test_eps_by_torch_is_the_oracles_formula():
    case = Case("dubins", (19, 17, 12), "f64")
    y = case.fill(5)
    og = O.Grid(case.G.min, case.G.max, case.shape, [2])
    assert eps_by_torch(case, y) == [O.max_d1_squared(og, y.cpu().numpy(), d) for d in range(3)]
    case = Case("pendulum", (9, 8, 7, 11), "f64")
    y = case.fill(6)
    og = O.Grid(case.G.min, case.G.max, case.shape, [0, 1, 2, 3])
    assert eps_by_torch(case, y) == [O.max_d1_squared(og, y.cpu().numpy(), d) for d in range(4)]


def test_the_data_and_the_boxes_on_a_small_grid(monkeypatch):
    """The machinery of this file where the full-grid oracle can still check it: fill, boxes, gather, comparison -- ENO2 on a grid of a few
    chunks, every box kind that does not need 2 GiB."""
    case = Case("dubins", (70, 66, 40), "f64")
    y, y0 = case.fill(1), case.fill(2)
    assert not torch.equal(y, y0) and float((y - y0).abs().max()) <= 0.1
    og = O.Grid(case.G.min, case.G.max, case.shape, [2])
    noise = y.cpu().numpy() - O.shape_cylinder(og, 2, None, .5)
    assert float(np.abs(noise).max()) <= 0.05 + 1e-12
    for d in range(3):                                         # the noise is per cell: it varies along every axis, in every line
        assert float(np.abs(np.diff(noise, axis=d)).max(axis=d).min()) > 0, d
    assert len(np.unique(noise)) > 0.99 * noise.size and abs(float(noise.mean())) < 1e-3 and 0.027 < float(noise.std()) < 0.031
    assert all(e > 0 for e in eps_by_torch(case, y))
    dg = _ctx(case, monkeypatch, {})
    out = torch.empty_like(y)
    dt = case.dt()
    _substep(dg, case, "ENO2", _ffi.STAGE_RK3_FULL, dt, y, y0, out)
    torch.cuda.synchronize()
    kernel, tile = _launched(dg)
    ydot, _ = O.term_lax_friedrichs(og, O.DubinsRel(og, 1, 1), "ENO2", 0., y.cpu().numpy().reshape(-1))
    ref = B.stage_expr(_ffi.STAGE_RK3_FULL, dt, y.cpu().numpy(), y0.cpu().numpy(), ydot.reshape(case.shape))
    assert np.array_equal(out.cpu().numpy(), ref)
    bx = Boxes(case, place_boxes(case, kernel, tile, cap=None), y, y0, 3)     # (a small grid is cut into many chunks)
    for b in bx.items:
        sl = np.ix_(*[np.arange(l, h) for l, h in zip(b["lo"], b["hi"])])
        assert np.array_equal(B.stage_expr(_ffi.STAGE_RK3_FULL, dt, b["y"], b["y0"], bx.ydot(b, "ENO2"))[b["cmp"]], ref[sl])


# ------------------------------------------------------------------ A: one descriptor past 2^31 bytes
A_SHAPE = (1030, 512, 512)


@pytest.mark.parametrize("scheme", ["ENO2", "ENO3", "WENO5_ASSHIPPED"])
def test_A_one_descriptor_past_2GiB(scheme, monkeypatch):
    case = Case("dubins", A_SHAPE, "f64")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, TB1)
    kernel, tile = check_stages(case, dg, scheme, STAGES, y, y0, out, _want(A_SHAPE, "f64", TB1, scheme), label="A TB1")
    assert tile[0] == 1030 and (1030 + 6) * 512 * 512 * 8 > (1 << 31)


def test_A_intended_weno5_and_max_d1sq(monkeypatch):
    case = Case("dubins", A_SHAPE, "f64")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {})
    eps = eps_by_torch(case, y)
    got = torch.zeros(3, dtype=torch.float64, device="cuda")
    _ffi.check(dg.lib.hj_max_d1sq(dg.ctx, dg.ptr(y), dg.ptr(got)))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    _report("A hj_max_d1sq %s against torch %s" % (got.tolist(), eps))
    assert np.all(np.abs(got - np.array(eps)) <= 1e-13 * np.array(eps)), (got, eps)       # same expression, fp64: rounding order at most
    check_stages(case, dg, "WENO5", STAGES, y, y0, out, _want(A_SHAPE, "f64", {}, "WENO5"), eps=eps, label="A default")


def _tuner_case(system, shape, dtype, scheme, monkeypatch, label, kernels=("fused_pair_kernel",)):
    """The one case per shape at the untouched default environment: the launch-time tile tuner is on (HJ_AUTOTUNE unset), so the tile is the
    tuner's and only the kernel, the span invariant and the boxes (placed by the REPORTED chunk and tile) are asserted."""
    case = Case(system, shape, dtype)
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {}, autotune=True)
    kernel, _ = check_stages(case, dg, scheme, [_ffi.STAGE_EULER], y, y0, out, None, label=label)
    assert kernel in kernels, kernel


def test_A_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("dubins", A_SHAPE, "f64", "ENO2", monkeypatch, "A tuner")


# ------------------------------------------------------------------ B: the cap binds
B_SHAPE = (2056, 512, 512)


@pytest.mark.parametrize("env,scheme", ENV_SCHEMES, ids=ENV_SCHEME_IDS)
def test_B_the_cap_binds(env, scheme, monkeypatch):
    case = Case("dubins", B_SHAPE, "f64")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, env)
    eps = eps_by_torch(case, y) if scheme == "WENO5" else None
    kernel, tile = check_stages(case, dg, scheme, STAGES, y, y0, out, _want(B_SHAPE, "f64", env, scheme), eps=eps,
                                label="B " + ("TB1" if env else "default"))
    assert (tile[0] + 6) * 512 * 512 * 8 < (1 << 32) and tile[0] < 2056           # the invariant, and more than one chunk
    if env:
        assert (tile[0] + 7) * 512 * 512 * 8 >= (1 << 32)                          # one more plane would not fit: the cap binds


def test_B_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("dubins", B_SHAPE, "f64", "WENO5_ASSHIPPED", monkeypatch, "B tuner")


def test_B_stage12_refuses_and_fuse12_steps_unfused(monkeypatch):
    case = Case("dubins", B_SHAPE, "f64")
    y, y0, (out, w0, w1) = _arrays(case, 3)
    dg = _ctx(case, monkeypatch, {"HJ_FUSE12": "1"})
    sid, par = _ffi.ENO2, _ffi.darr(case.s["par"])
    rc = dg.lib.hj_rk_stage12(dg.ctx, sid, case.s["ham"], par, 1e-4, 0.75, 0.25, dg.ptr(y), dg.ptr(out), 5)
    assert rc == -3 and b"array of 4 GiB or more" in dg.lib.hj_last_error()
    with pytest.raises(_ffi.Unsupported):
        _ffi.check(rc)
    launches, fused = C.c_int(), C.c_int()
    _ffi.check(dg.lib.hj_rk_plan(dg.ctx, 3, sid, case.s["ham"], par, 0, C.byref(launches), C.byref(fused)))
    assert fused.value == 0 and launches.value == 3
    tf = 0.5 * 0.8 * case.sb_closed_form()
    tout, dtout = C.c_double(), C.c_double()
    out.fill_(float("nan"))
    _ffi.check(dg.lib.hj_rk_step(dg.ctx, 3, sid, case.s["ham"], par, 0., tf, 0.8, 1e300, 0, dg.ptr(y), dg.ptr(out), dg.ptr(w0), dg.ptr(w1),
                                 C.byref(tout), C.byref(dtout)))
    torch.cuda.synchronize()
    kernel, tile = _launched(dg)
    assert kernel == "fused_pair_kernel" and dtout.value == tf
    bx = Boxes(case, place_boxes(case, kernel, tile), y, y0, B.M_RK3)
    for b in bx.items:
        t_ref, ref = B.rk3_step(case.G, case.s["make"], "ENO2", b["idx"], b["y"], tf)
        assert tout.value == t_ref, (tout.value, t_ref)
        got = B.gather(out, [np.arange(l, h) for l, h in zip(b["lo"], b["hi"])])
        compare(case, "ENO2", got, ref[b["cmp"]], "B FUSE12=1 step box %s %s" % (b["kind"], b["lo"]), {})
    _report("B FUSE12=1  hj_rk_stage12 refused; hj_rk_step: 3 launches of %s, %d boxes bitwise" % (kernel, len(bx.items)))


# ------------------------------------------------------------------ C: 2^31 cells
C_SHAPE = (8200, 512, 512)


@pytest.mark.parametrize("env,scheme", ENV_SCHEMES, ids=ENV_SCHEME_IDS)
def test_C_2e31_cells(env, scheme, monkeypatch):
    case = Case("dubins", C_SHAPE, "f32")
    assert case.cells >= (1 << 31)
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, env)
    eps = eps_by_torch(case, y) if scheme == "WENO5" else None
    kernel, tile = check_stages(case, dg, scheme, STAGES, y, y0, out, _want(C_SHAPE, "f32", env, scheme), eps=eps,
                                label="C " + ("TB1" if env else "default"))
    assert (tile[0] + 6) * 512 * 512 * 4 < (1 << 32) and tile[0] < 8200


def test_C_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("dubins", C_SHAPE, "f32", "WENO5_ASSHIPPED", monkeypatch, "C tuner")


@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED"])
def test_C_direct_kernel_decodes_64_bit(scheme, monkeypatch):
    case = Case("dubins", C_SHAPE, "f32")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {"HJ_FORCE_DIRECT": "1"})
    check_stages(case, dg, scheme, STAGES, y, y0, out, ("direct_substep_kernel", 1, 0, []), label="C direct")


def test_C_rk3_step(monkeypatch):
    case = Case("dubins", C_SHAPE, "f32")
    y, y0, (out, w0, w1) = _arrays(case, 3)
    dg = _ctx(case, monkeypatch, {})
    tf = 0.5 * 0.8 * case.sb_closed_form()
    tout, dtout = C.c_double(), C.c_double()
    out.fill_(float("nan"))
    scheme = "WENO5_ASSHIPPED"
    _ffi.check(dg.lib.hj_rk_step(dg.ctx, 3, _ffi.SCHEME_IDS[scheme], case.s["ham"], _ffi.darr(case.s["par"]), 0., tf, 0.8, 1e300, 0,
                                 dg.ptr(y), dg.ptr(out), dg.ptr(w0), dg.ptr(w1), C.byref(tout), C.byref(dtout)))
    torch.cuda.synchronize()
    kernel, tile = _launched(dg)
    assert kernel == "fused_pair_kernel" and (tile[0], tile[1], tile[2]) == (2050, 32, 64), (kernel, tile)
    bx = Boxes(case, place_boxes(case, kernel, tile), y, y0, B.M_RK3)
    stats = {}
    for b in bx.items:
        t_ref, ref = B.rk3_step(case.G, case.s["make"], scheme, b["idx"], b["y"], tf)
        print("t_out %r oracle %r dt_out %r tf %r" % (tout.value, t_ref, dtout.value, tf))
        assert tout.value == t_ref and dtout.value == tf
        got = B.gather(out, [np.arange(l, h) for l, h in zip(b["lo"], b["hi"])])
        compare(case, scheme, got, ref[b["cmp"]], "C rk3 step box %s %s" % (b["kind"], b["lo"]), stats)
    _report("C rk_step   %s order 3, t_out == oracle t, %d boxes (margin 9), fp32 max rel %.2e share %.2e" % (
        scheme, len(bx.items), stats["rel"], stats["share"]))


def test_C_step_bound(monkeypatch):
    """hj_read_step_bound after a substep over 2^31 cells against the closed form (alpha's maxima per axis from g.vs, put into the formula of
    artificial_dissipation_glf), by the rule of test_gpu_parity's small-grid step-bound tests: |sb - ref| <= 1e-13 * ref."""
    case = Case("dubins", C_SHAPE, "f32")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {})
    _substep(dg, case, "ENO2", _ffi.STAGE_EULER, case.dt(), y, y0, out, slot=7)
    sb, am = C.c_double(), (C.c_double * 4)()
    _ffi.check(dg.lib.hj_read_step_bound(dg.ctx, 7, C.byref(sb), am))
    ref = case.sb_closed_form()
    _report("C stepBound %r closed form %r relative difference %.3e alpha max %s" % (sb.value, ref, abs(sb.value - ref) / ref, list(am)[:3]))
    assert abs(sb.value - ref) <= 1e-13 * ref, (sb.value, ref)


@pytest.mark.parametrize("dim", [0, 1, 2])
def test_C_upwind_64_bit_side(dim, monkeypatch):
    case = Case("dubins", C_SHAPE, "f32")
    y, y0, (dl, dr) = _arrays(case, 2)
    dg = _ctx(case, monkeypatch, {})
    boxes = place_boxes(case, "upwind_kernel", [0, 0, 0, 0])
    bx = Boxes(case, boxes, y, y0, 3)
    stats = {}
    for scheme, fn in (("ENO3", O.upwind_first_eno3), ("WENO5_ASSHIPPED", lambda g, d, i: O.upwind_first_weno5(g, d, i, 'asshipped'))):
        dl.fill_(float("nan"))
        dr.fill_(float("nan"))
        _ffi.check(dg.lib.hj_upwind(dg.ctx, _ffi.SCHEME_IDS[scheme], dim, dg.ptr(y), dg.ptr(dl), dg.ptr(dr), None))
        torch.cuda.synchronize()
        for b in bx.items:
            g = B.box_grid(case.G, b["idx"])
            refL, refR = fn(g, b["y"], dim)
            rng_ = [np.arange(l, h) for l, h in zip(b["lo"], b["hi"])]
            compare(case, scheme, B.gather(dl, rng_), refL[b["cmp"]], "upwind L dim %d %s %s" % (dim, scheme, b["lo"]), stats, derivative=True)
            compare(case, scheme, B.gather(dr, rng_), refR[b["cmp"]], "upwind R dim %d %s %s" % (dim, scheme, b["lo"]), stats, derivative=True)
    _report("C hj_upwind dim %d ENO3 + WENO5_ASSHIPPED, %d boxes, fp32 max rel %.2e share %.2e" % (dim, len(bx.items), stats["rel"], stats["share"]))


def test_C_any_nan_and_minmax(monkeypatch):
    case = Case("dubins", C_SHAPE, "f32")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {})
    has = C.c_int(-1)
    n = case.cells
    _ffi.check(dg.lib.hj_any_nan(dg.ctx, dg.ptr(y), n, C.byref(has)))
    assert has.value == 0
    flat = out.view(-1)
    for at in (n - 1, (1 << 31) + 5):
        out.copy_(y)
        flat[at] = float("nan")
        _ffi.check(dg.lib.hj_any_nan(dg.ctx, dg.ptr(out), n, C.byref(has)))
        assert has.value == 1, at
        _ffi.check(dg.lib.hj_any_nan(dg.ctx, dg.ptr(out), at, C.byref(has)))          # the NaN lies just past the range
        assert has.value == 0, at
    step = 1 << 28
    for op, ref in ((_ffi.OP_MIN, lambda a, b: torch.minimum(a, b)), (_ffi.OP_MAX, lambda a, b: torch.maximum(a, b)),
                    (_ffi.OP_MAX_NEG, lambda a, b: torch.maximum(a, -b))):
        out.copy_(y)
        _ffi.check(dg.lib.hj_minmax_with(dg.ctx, op, dg.ptr(out), dg.ptr(y0), n))
        torch.cuda.synchronize()
        yf, y0f = y.view(-1), y0.view(-1)
        for p in range(0, n, step):
            assert torch.equal(flat[p:p + step], ref(yf[p:p + step], y0f[p:p + step])), (op, p)
    _report("C hj_any_nan (clean, last element, element 2^31 + 5) and hj_minmax_with (3 ops, torch.equal over %d cells)" % n)


# ------------------------------------------------------------------ D: wide planes
D_SHAPE = (40, 7400, 7400)


@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED", "WENO5"])
def test_D_wide_planes(scheme, monkeypatch):
    case = Case("dubins", D_SHAPE, "f32")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {})
    eps = eps_by_torch(case, y) if scheme == "WENO5" else None
    kernel, tile = check_stages(case, dg, scheme, [_ffi.STAGE_EULER, _ffi.STAGE_RK3_FULL], y, y0, out, _want(D_SHAPE, "f32", {}, scheme),
                                eps=eps, label="D default")
    assert kernel == ("direct_substep_kernel" if scheme == "WENO5" else "fused_pair_kernel")


def test_D_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("dubins", D_SHAPE, "f32", "ENO2", monkeypatch, "D tuner")


# ------------------------------------------------------------------ E: 4-D
def _record(dg, on):
    _ffi.check(dg.lib.hj_launch_record(dg.ctx, on))


def _record_read(dg):
    n = dg.lib.hj_launch_record_read(dg.ctx, None, 0)
    buf = C.create_string_buffer(max(n, 1))
    assert dg.lib.hj_launch_record_read(dg.ctx, buf, n) == n
    return buf.value.decode()


@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED", "WENO5"])
def test_E_4d_past_2e31_cells_leaves_the_fixed_tile_kernels(scheme, monkeypatch):
    shape = (1001, 129, 129, 129)
    case = Case("pendulum", shape, "f32")
    assert case.cells >= (1 << 31)
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {})
    eps = eps_by_torch(case, y) if scheme == "WENO5" else None
    _record(dg, 1)
    check_stages(case, dg, scheme, [_ffi.STAGE_EULER, _ffi.STAGE_RK3_FULL], y, y0, out, _want(shape, "f32", {}, scheme), eps=eps, label="E 1001")
    names = _record_read(dg)
    _record(dg, 0)
    assert names and "fused_flat4_kernel" not in names and "fused_pair4_kernel" not in names, names
    assert ("fused_substep_kernel" if scheme == "WENO5" else "fused_pair_kernel") in names, names


def test_E_1001_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("pendulum", (1001, 129, 129, 129), "f32", "ENO2", monkeypatch, "E 1001 tuner")


@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED"])
def test_E_4d_flat4_past_4GiB(scheme, monkeypatch):
    shape = (520, 129, 129, 129)
    case = Case("pendulum", shape, "f32")
    assert case.cells < (1 << 31) and case.bytes > (1 << 32)
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, {})
    check_stages(case, dg, scheme, [_ffi.STAGE_EULER, _ffi.STAGE_RK3_FULL], y, y0, out, _want(shape, "f32", {}, scheme), label="E 520")


def test_E_520_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("pendulum", (520, 129, 129, 129), "f32", "WENO5_ASSHIPPED", monkeypatch, "E 520 tuner", ("fused_flat4_kernel",))


# ------------------------------------------------------------------ F: 2-D at the limit
F_SHAPE = (32768, 16400)


@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED"])
def test_F_2d_span_4095_bytes_under_the_limit(scheme, monkeypatch):
    case = Case("integrator", F_SHAPE, "f64")
    y, y0, (out,) = _arrays(case)
    dg = _ctx(case, monkeypatch, TB1)
    kernel, tile = check_stages(case, dg, scheme, [_ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF], y, y0, out, _want(F_SHAPE, "f64", TB1, scheme),
                                label="F TB1")
    assert (tile[0] + 6) * 16400 * 8 == (1 << 32) - 4096


def test_F_default_environment_with_the_tuner(monkeypatch):
    _tuner_case("integrator", F_SHAPE, "f64", "ENO2", monkeypatch, "F tuner")


def test_F_lf_split_begin(monkeypatch):
    """hj_lf_split_begin (upwind_all_kernel): five arrays of 4 GiB, the derivatives against the oracle's on boxes."""
    case = Case("integrator", F_SHAPE, "f64")
    y, y0, d = _arrays(case, 4)
    dg = _ctx(case, monkeypatch, {})
    bx = Boxes(case, place_boxes(case, "upwind_all_kernel", [0, 0, 0, 0]), y, y0, 3)
    P = C.c_void_p * 2
    for scheme, fn in (("ENO2", O.upwind_first_eno2), ("WENO5_ASSHIPPED", lambda g, a, i: O.upwind_first_weno5(g, a, i, 'asshipped'))):
        for t in d:
            t.fill_(float("nan"))
        _ffi.check(dg.lib.hj_lf_split_begin(dg.ctx, _ffi.SCHEME_IDS[scheme], dg.ptr(y), P(d[0].data_ptr(), d[1].data_ptr()),
                                            P(d[2].data_ptr(), d[3].data_ptr()), None))
        torch.cuda.synchronize()
        stats = {}
        for b in bx.items:
            g = B.box_grid(case.G, b["idx"])
            rng_ = [np.arange(l, h) for l, h in zip(b["lo"], b["hi"])]
            for dim in range(2):
                refL, refR = fn(g, b["y"], dim)
                compare(case, scheme, B.gather(d[dim], rng_), refL[b["cmp"]], "split L dim %d %s %s" % (dim, scheme, b["lo"]), stats, derivative=True)
                compare(case, scheme, B.gather(d[2 + dim], rng_), refR[b["cmp"]], "split R dim %d %s %s" % (dim, scheme, b["lo"]), stats, derivative=True)
        _report("F hj_lf_split_begin %s: 5 arrays of %.2f GiB, %d boxes, max err/scale %.2e" % (scheme, case.bytes / GiB, len(bx.items), stats["max"]))


# ------------------------------------------------------------------ G: transposed march
@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED"])
def test_G_transposed_march_past_2GiB(scheme, monkeypatch):
    shape = (24, 3400, 3400)
    case = Case("dubins", shape, "f64")
    y, y0, (out, out0) = _arrays(case, 2)
    xp2 = {"HJ_XP": "2"}
    stages = [_ffi.STAGE_EULER, _ffi.STAGE_RK3_FULL]
    dg = _ctx(case, monkeypatch, xp2)
    dg0 = _ctx(case, monkeypatch, {"HJ_XP": "0"})              # (a context keeps the knobs it was created with)
    for st in stages:
        kernel, _ = check_stages(case, dg, scheme, [st], y, y0, out, _want(shape, "f64", xp2, scheme), label="G XP=2 " + STAGE_NAME[st])
        assert kernel == XP_NAME
        # the same call marched along axis 0, bit for bit over the whole array
        out0.fill_(float("nan"))
        _substep(dg0, case, scheme, st, case.dt(), y, y0, out0)
        torch.cuda.synchronize()
        assert _launched(dg0)[0] == "fused_pair_kernel"
        assert torch.equal(out, out0), STAGE_NAME[st]


def test_G_3400_default_environment_with_the_tuner(monkeypatch):
    """(the default environment times the two marches against each other on a context's first calls: either may run)"""
    _tuner_case("dubins", (24, 3400, 3400), "f64", "ENO2", monkeypatch, "G 3400 tuner", ("fused_pair_kernel", XP_NAME))


G_REFUSED = [((24, 4800, 4800), "f64"), ((24, 9500, 9500), "f32")]


@pytest.mark.parametrize("shape,dtype", G_REFUSED, ids=["the-cap-refuses", "2e31-cells-refuse"])
def test_G_refused_default_environment_with_the_tuner(shape, dtype, monkeypatch):
    _tuner_case("dubins", shape, dtype, "ENO2", monkeypatch, "G refused tuner")


@pytest.mark.parametrize("shape,dtype", G_REFUSED, ids=["the-cap-refuses", "2e31-cells-refuse"])
def test_G_transposed_march_refused(shape, dtype, monkeypatch):
    case = Case("dubins", shape, dtype)
    y, y0, (out,) = _arrays(case)
    xp2 = {"HJ_XP": "2"}
    dg = _ctx(case, monkeypatch, xp2)
    for scheme in ("ENO2", "WENO5_ASSHIPPED"):
        kernel, _ = check_stages(case, dg, scheme, [_ffi.STAGE_EULER, _ffi.STAGE_RK3_FULL], y, y0, out, _want(shape, dtype, xp2, scheme),
                                 label="G refused")
        assert kernel == "fused_pair_kernel"


# ------------------------------------------------------------------ H: the context refusal
def test_H_a_plane_of_2e31_cells_is_refused_without_allocating():
    N = (2, 46341, 46341)
    assert N[1] * N[2] >= (1 << 31) > 46340 * 46340
    lib = _ffi.lib()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    ctx = C.c_void_p()
    rc = lib.hj_ctx_create(C.byref(ctx), 3, (C.c_int64 * 3)(*N), _ffi.darr([0, 0, 0]), _ffi.darr([1, 1, 1]), (C.c_int * 3)(0, 0, 1),
                           (C.c_int * 3)(0, 0, 0), _ffi.F32, torch.cuda.current_device())
    assert rc == -3 and not ctx.value and b"axis-0 plane exceeds 2^31 cells" in lib.hj_last_error()
    assert torch.cuda.mem_get_info()[0] >= free_before            # no context, no device memory taken for one
    _report("H hj_ctx_create N = %s refused: %s" % (N, lib.hj_last_error().decode()))


# ------------------------------------------------------------------ the stateless libraries past 2^31 elements
# One 8 to 9 GiB array each (the stored stack of eval_u: fp64, 16 GiB, for a bit-for-bit comparison), checked against the library's NumPy
# restatement on boxes / windows.  The eikonal and surface libraries are left out: a full-size eikonal solve takes seconds per pass, and a
# surface of that size needs a design of its own.
class _Shape(object):
    """What place_boxes reads of a Case."""

    def __init__(self, shape, esz):
        self.shape, self.esz = tuple(shape), esz
        self.cells = int(np.prod(shape, dtype=np.int64))
        self.bytes = self.cells * esz


def _tool_start(nbytes, what):
    _BUF.clear()
    _BOXES.clear()
    torch.cuda.empty_cache()
    _need(nbytes, what)


def _ranges(lo, hi):
    return [np.arange(l, h) for l, h in zip(lo, hi)]


def test_tools_evaluate_shape_past_2e31_nodes():
    import types
    import shapes_ref as R
    from levelsetpy_amd import shapes as S
    N = (1300, 1300, 1280)
    sh = _Shape(N, 4)
    assert sh.cells >= (1 << 31)
    _tool_start(sh.bytes, "evaluate_shape %s f32" % (N,))
    g = L.createGrid(np.array([[-1.], [-1.2], [-.9]]), np.array([[1.1], [1.], [1.]]), np.array(N, dtype=np.int64).reshape(-1, 1), None, low_mem=True)
    centre, radius, normal, point = [0.3, -0.2, 0.1], 0.7, [1., 2., -1.], [0.1, 0., 0.]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = S.evaluate_shape(g, S.union(S.sphere(centre, radius), S.hyperplane(normal, point)), 'float32')
    assert tuple(out.shape) == N and out.dtype == torch.float32
    boxes = place_boxes(sh, "shapes", [0, 0, 0, 0])
    assert sum(k.startswith("offset") for k, _, _ in boxes) >= 3
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
    for kind, lo, hi in boxes:
        gb = types.SimpleNamespace(dim=3, vs=[vs[d][lo[d]:hi[d]] for d in range(3)])
        ref = R.union(R.sphere(gb, centre, radius), R.hyperplane(gb, normal, point)).astype(np.float32)
        got = B.gather(out, _ranges(lo, hi)).astype(np.float32)
        assert np.array_equal(got, ref), (kind, lo)
    _report("tools evaluate_shape %s f32 %.2f GiB kernel %s: %d boxes bitwise" % (N, sh.bytes / GiB, S.last_info()["kernel"], len(boxes)))


@pytest.mark.parametrize("mode", ["intersection", "union"])
def test_tools_back_project_past_2e31_nodes(mode):
    import types
    import decomp_ref as R
    from levelsetpy_amd import decomp as D
    n = 216
    N = (n,) * 4
    sh = _Shape(N, 4)
    assert sh.cells >= (1 << 31)
    _tool_start(sh.bytes, "backProject %s f32" % (N,))
    dims = [[0, 2], [3, 1]]
    lo_hi = {0: (-1., 1.), 2: (-2., 0.5), 3: (0., 3.), 1: (-.5, .25)}
    mk = lambda axes: L.createGrid(np.array([[lo_hi[a][0]] for a in axes]), np.array([[lo_hi[a][1]] for a in axes]),  # noqa: E731
                                   np.array([[n]] * len(axes), dtype=np.int64), None, low_mem=(len(axes) > 2))
    gs = [mk(dims[0]), mk(dims[1])]
    g = mk([0, 1, 2, 3])
    gen = torch.Generator(device="cuda").manual_seed(8)
    datas = [torch.randn((n, n), generator=gen, device="cuda", dtype=torch.float32) for _ in range(2)]
    out = D.backProject(g, gs, datas, dims, mode=mode, method='nodes')
    assert tuple(out.shape) == N and out.dtype == torch.float32 and "backproject_nodes_kernel" in D.last_path()
    host = [d.cpu().numpy() for d in datas]
    boxes = place_boxes(sh, "decomp", [0, 0, 0, 0])
    for kind, lo, hi in boxes:
        sub, gb = [], []
        for s, axes in enumerate(dims):
            sub.append(host[s][lo[axes[0]]:hi[axes[0]], lo[axes[1]]:hi[axes[1]]])
            gb.append(types.SimpleNamespace(N=np.array(sub[-1].shape)))
        ref = R.back_project([h - l for l, h in zip(lo, hi)], gb, sub, dims, mode, np.float32)
        got = B.gather(out, _ranges(lo, hi)).astype(np.float32)
        assert np.array_equal(got, ref), (kind, lo)
    _report("tools backProject %s f32 %.2f GiB %s (%s): %d boxes bitwise" % (N, sh.bytes / GiB, D.last_path(), mode, len(boxes)))


def test_tools_back_project_refuses_a_subsystem_of_2e31_nodes():
    from levelsetpy_amd import decomp as D
    n = 46341
    assert n * n > 0x7fffffff
    _tool_start(2 * n * n * 4, "backProject refusal, a subsystem of %d^2 f32 nodes" % n)
    g = L.createGrid(np.array([[-1.], [-1.]]), np.array([[1.], [1.]]), np.array([[n], [n]], dtype=np.int64), None, low_mem=True)
    data = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    with pytest.raises(_ffi.Unsupported, match="at most 2\\^31 - 1 per field"):
        D.backProject(g, [g], [data], [[0, 1]], method='nodes')
    _report("tools backProject refuses a subsystem of %d^2 nodes" % n)


@pytest.mark.parametrize("interpolate", [False, True], ids=["stamp", "interpolate"])
@pytest.mark.parametrize("crossing", ["first", "last"])
def test_tools_td2ttr_stack_past_2e31_elements(crossing, interpolate):
    import ttr_ref as R
    from levelsetpy_amd import TD2TTR
    from levelsetpy_amd import _tffi
    T, n = 17, 1 << 27
    assert T * n == (1 << 31) + (1 << 27) and (T - 1) * n == (1 << 31)         # the last slice starts at element 2^31
    key = ("ttr", T, n)
    if _BUF.get("key") != key:
        _tool_start(T * n * 4 + n * 8, "TD2TTR stack of %d x 2^27 f32" % T)
        gen = torch.Generator(device="cuda").manual_seed(17)
        tau = np.linspace(0., 1., T)
        data = torch.empty((T, n), dtype=torch.float32, device="cuda")
        for b in range(0, n, BLOCK):
            psi = 1.4 * torch.rand(BLOCK, generator=gen, device="cuda", dtype=torch.float64) - 0.2
            for k in range(T):
                noise = 0.05 * (2 * torch.rand(BLOCK, generator=gen, device="cuda", dtype=torch.float64) - 1)
                data[k, b:b + BLOCK] = (psi - 0.8 * tau[k] + noise).float()
        _BUF.update(key=key, data=data, tau=tau)
    data, tau = _BUF["data"], _BUF["tau"]
    g = L.createGrid(np.array([[0.]]), np.array([[1.]]), np.array([[n]], dtype=np.int64), None, low_mem=True)
    out = TD2TTR(g, data, tau, 0.0, crossing, interpolate)
    assert _tffi.last_kernel() == "ttr_from_stack_kernel<float>" and out.dtype == torch.float64 and out.numel() == n
    out = out.reshape(-1)
    w = 4096
    rng = np.random.default_rng(3)
    windows = [0, n - w] + [int(v) for v in rng.integers(0, n - w, 4)]           # start (node 0's last slice sits AT offset 2^31), end, random
    reached = 0
    for a in windows:
        ref = R.TD2TTR(data[:, a:a + w].cpu().numpy(), tau, 0.0, crossing, interpolate)
        got = out[a:a + w].cpu().numpy()
        assert np.array_equal(got, ref), (a, int((got != ref).sum()))
        reached += int(np.isfinite(ref).sum())
    assert reached > len(windows) * w // 2
    _report("tools TD2TTR %d x 2^27 f32 (2^31 + 2^27 elements) crossing=%s interpolate=%s: %d windows of %d nodes bitwise" % (
        T, crossing, interpolate, len(windows), w))


def test_tools_eval_u_field_stride_past_2e31_elements():
    import query_ref as Q
    from levelsetpy_amd import eval_u
    n, T = 1024, 2049
    assert (T - 1) * n * n == (1 << 31)                                          # the last field starts at element 2^31
    _tool_start(T * n * n * 8, "eval_u stack of %d fields of %d^2 fp64" % (T, n))
    g, _og = Q.make_grids((n, n), (1,))
    gen = torch.Generator(device="cuda").manual_seed(5)
    data = torch.empty((T, n, n), dtype=torch.float64, device="cuda")
    for k in range(0, T, 64):
        data[k:k + 64] = torch.randn((min(64, T - k), n, n), generator=gen, device="cuda", dtype=torch.float64)
    xs = Q.state_set(g, 1000)
    got = eval_u(g, data, torch.as_tensor(xs, device="cuda"))
    assert tuple(got.shape) == (T, 1000)
    got = got.cpu().numpy()
    for k in (0, 1023, T - 2, T - 1):
        ref = Q.eval_u_ref(g, data[k].cpu().numpy(), xs)
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref)), k
        ok = ~np.isnan(ref)
        assert ok.sum() > 500 and np.array_equal(got[k][ok], ref[ok]), k
    _report("tools eval_u %d fields of %d^2 fp64 (field %d starts at element 2^31), 1000 states: fields 0, 1023, %d, %d bitwise" % (
        T, n, T - 1, T - 2, T - 1))


# ------------------------------------------------------------------ the 1-D to 6-D node walk past 2^32 nodes, hidim past 2^31 cells
# libhj_hishapes.so, libhj_resample.so and libhj_measure.so share one node walk (csrc/hj_index_dev.h).  tests/test_gpu_node_walk.py runs
# its head axes and its launches on small grids with the plan's limits lowered; here the limits are the constants and the grid is real:
# 4 305 300 000 nodes, 16.04 GiB per fp32 array, the tail (axes 2 .. 5, 717 550 000 nodes) times 3 past 2^31, so axes 0 and 1 are the head:
# six head indices, one of the two head extents no power of two.  Boxes: the grid's corners, both sides of each of the five head-index
# seams (the last tail node of head index h, the first of h + 1), the elements at flat offsets 2^31 and 2^32, four seeded random places.
WALK_N = (2, 3, 5, 127, 1000, 1130)
WALK_EXT = (2, 3, 2, 3, 4, 8)                                    # a box's extents: both head axes whole


def _walk_plan(binding, *args):
    """The published plan of WALK_N at the default limits: the form these cases mean to run."""
    assert "HJ_INDEX_TAIL_BELOW" not in os.environ and "HJ_INDEX_LAUNCH_BLOCKS" not in os.environ
    p = binding.plan(WALK_N, *args)
    assert p.total == 4305300000 >= (1 << 32) and p.first_tail == 2 and p.tail == 717550000 and p.head == 6
    assert p.tail * WALK_N[1] >= (1 << 31) > p.tail and p.chunks == (p.tail + 255) // 256
    # a launch has fewer than 2^32 threads (one launch of all 16 817 580 workgroups ran 10 333 184 threads of them and reported nothing:
    # profiles/node_walk_head.txt), so a grid past 2^32 nodes takes two launches at least: five head indices, then (1, 2) alone
    assert (p.launches, p.heads_per_launch, p.blocks_full, p.blocks_last) == (2, 5, 5 * p.chunks, p.chunks) and p.blocks_full * 256 < (1 << 32)
    return p


def walk_places(N, tail, head, seed=99):
    """[(kind, multi-index)]: corners, head-index seams, flat offsets 2^31 and 2^32 (where the grid has them), four random nodes."""
    nd, total = len(N), int(np.prod(N, dtype=np.int64))
    at = lambda flat: tuple(int(v) for v in np.unravel_index(flat, N))           # noqa: E731
    places = [("corner", tuple((N[d] - 1) if c >> d & 1 else 0 for d in range(nd))) for c in range(1 << nd)]
    for h in range(head - 1):
        places += [("seam-", at((h + 1) * tail - 1)), ("seam+", at((h + 1) * tail))]
    places += [("offset", at(e)) for e in (1 << 31, 1 << 32) if e < total]
    rng = np.random.default_rng(seed)
    places += [("random", tuple(int(rng.integers(0, n)) for n in N)) for _ in range(4)]
    return places


def walk_boxes(N, ext, places):
    """[(kinds, lo, hi)]: a box of extents `ext` (clipped to the grid) around every place; places that give the same box share it."""
    ext = [min(e, n) for e, n in zip(ext, N)]
    boxes = {}
    for kind, idx in places:
        lo, hi = _around(N, ext, idx)
        assert all(l <= i < h for l, i, h in zip(lo, idx, hi)) and all(0 <= l < h <= n for l, h, n in zip(lo, hi, N))
        boxes.setdefault((tuple(lo), tuple(hi)), []).append(kind)
    out = [("+".join(sorted(set(k))), list(lo), list(hi)) for (lo, hi), k in boxes.items()]
    kinds = set(k for ks, _, _ in out for k in ks.split("+"))
    assert {"corner", "random"} <= kinds and ("offset" in kinds) == (int(np.prod(N, dtype=np.int64)) > (1 << 31))
    return out


def _walk_setup(what, arrays):
    _tool_start(arrays * 4 * int(np.prod(WALK_N, dtype=np.int64)), "%s %s f32" % (what, WALK_N))


def test_walk_the_places_on_a_small_grid():
    """The placement, without a large array: a (2, 3, 4, 5, 6, 7) grid split like WALK_N."""
    N, tail = (2, 3, 4, 5, 6, 7), 4 * 5 * 6 * 7
    places = walk_places(N, tail, 6)
    assert [k for k, _ in places].count("corner") == 64 and [k for k, _ in places].count("random") == 4
    seams = [i for k, i in places if k.startswith("seam")]
    assert seams[:4] == [(0, 0, 3, 4, 5, 6), (0, 1, 0, 0, 0, 0), (0, 1, 3, 4, 5, 6), (0, 2, 0, 0, 0, 0)] and len(seams) == 10
    assert seams[4:6] == [(0, 2, 3, 4, 5, 6), (1, 0, 0, 0, 0, 0)]                 # the seam where the first head axis moves on
    boxes = walk_boxes(N, WALK_EXT, places)
    # (the head axes and the last axis are whole in every box: 8 corner boxes)
    assert 8 <= len(boxes) <= len(places) and any("seam" in k and "corner" in k for k, _, _ in boxes)
    big = walk_places(WALK_N, 717550000, 6)
    assert ("offset", tuple(int(v) for v in np.unravel_index(1 << 32, WALK_N))) in big and len(big) == 64 + 10 + 2 + 4


def test_walk_evaluate_shape_past_2e32_nodes():
    import hishapes_ref as H
    from levelsetpy_amd import _kffi, shapes as S
    _walk_plan(_kffi, 1)
    _walk_setup("evaluate_shape", 1)
    N = WALK_N
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)          # noqa: E731
    g = L.createGrid(col([-1., -1.2, -.9, -1.1, -1., -.8]), col([1.1, 1., 1., .9, 1.2, 1.]), col(N, np.int64), None, low_mem=True)
    rows = np.array([[1., .5, -.3, .2, .1, -.4], [-.2, 1., .4, -.1, .3, .2], [.3, -.1, .2, 1., -.5, .6]])
    node = S.union(S.sphere_of(rows, [.1, -.05, .2], .9), S.hyperplane([1., 2., -1., .5, -.7, .3], [.1, 0., 0., .2, -.1, 0.]),
                   S.rectangle_by_corners([-.5, -.6, -.4, -.7, -.3, -.2], [.6, .4, .5, .3, .8, .7]))
    comp = S.compile_program_hi(node, 6)
    t0 = time.perf_counter()
    out = S.evaluate_shape(g, node, 'float32')
    torch.cuda.synchronize()
    call = time.perf_counter() - t0
    assert tuple(out.shape) == N and out.dtype == torch.float32 and S.last_info()["kernel"] == _kffi.kernel_name("float32")
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
    boxes = walk_boxes(N, WALK_EXT, walk_places(N, 717550000, 6))
    nodes = 0
    for kind, lo, hi in boxes:
        ref = H.run_program(H.PlainGrid([vs[d][lo[d]:hi[d]] for d in range(6)]), comp)[0].astype(np.float32)
        got = B.gather(out, _ranges(lo, hi)).astype(np.float32)
        assert np.array_equal(got, ref), (kind, lo)
        nodes += ref.size
    from levelsetpy_amd import _gffi
    assert int(S.last_info()["flags"][0]) & (_gffi.NEG | _gffi.POS) == _gffi.NEG | _gffi.POS      # both signs on the grid
    _report("walk evaluate_shape %s f32 %.2f GiB kernel %s, first_tail 2, 6 head indices, 2 launches: %d boxes (%d nodes) bitwise; the call %.3f s" % (
        N, 4 * out.numel() / GiB, S.last_info()["kernel"], len(boxes), nodes, call))


def test_walk_migrate_grid_past_2e32_nodes():
    import hishapes_ref as H
    import query_ref as Q
    import resample_ref as R
    from levelsetpy_amd import _mffi, resample
    _walk_plan(_mffi)
    _walk_setup("migrateGrid", 1)
    N = WALK_N
    src, pd = (3, 4, 5, 9, 11, 12), (2,)
    smin, smax = Q.grid_bounds(src, pd)
    rO = R.RefGrid(smin, smax, src, pd)
    gO = L.createGrid(rO.min.reshape(-1, 1), rO.max.reshape(-1, 1), rO.N.reshape(-1, 1), list(pd))
    data = R.field(rO, 77).astype(np.float32)
    c, h = 0.5 * (smin + smax), 0.5 * (smax - smin)
    # the destination: from 0.9 half-widths below the source box's centre to 1.2 above it, so a part of every axis falls outside
    dst = H.PlainGrid([np.linspace(c[d] - 0.9 * h[d], c[d] + 1.2 * h[d], n) for d, n in enumerate(N)])
    # inside is separable per axis (the identity map): the nodes of axis d that locate finds inside, the other coordinates at the centre
    inside = []
    for d in range(6):
        y = np.tile(c, (N[d], 1))
        y[:, d] = dst.vs[d]
        inside.append(int((~Q.locate(rO, y)[2]).sum()))
    assert all(0 < k < n for k, n, d in zip(inside, N, range(6)) if d not in pd) and inside[2] == N[2], inside
    filled = int(np.prod(inside, dtype=np.int64))
    boxes = walk_boxes(N, WALK_EXT, walk_places(N, 717550000, 6))
    dt = torch.as_tensor(data, device="cuda")
    for fill in ('nan', -2.5):
        t0 = time.perf_counter()
        out = L.migrateGrid(gO, dt, dst, fill=fill)
        torch.cuda.synchronize()
        call = time.perf_counter() - t0
        assert tuple(out.shape) == N and out.dtype == torch.float32
        assert resample.last_path() == _mffi.kernel_names("float32", 6, 0, False)
        assert int(resample.last_info()["counts"]) == filled, (resample.last_info()["counts"], inside)
        some_in = some_out = 0
        for kind, lo, hi in boxes:
            ref, cnt = R.resample_ref(rO, data, H.PlainGrid([dst.vs[d][lo[d]:hi[d]] for d in range(6)]), None, None, None, fill, dtype=np.float32)
            got = B.gather(out, _ranges(lo, hi)).astype(np.float32)
            assert np.array_equal(got, ref, equal_nan=True), (kind, lo, fill)
            some_in += int(cnt)
            some_out += ref.size - int(cnt)
        assert some_in > 0 and some_out > 0
        del out
        _report("walk migrateGrid %s -> %s f32 %.2f GiB fill %s, %s: %d of %d nodes filled == the product of the per-axis counts %s; "
                "%d boxes (%d nodes inside, %d outside) bitwise; the call %.3f s" % (
                    src, N, 4 * int(np.prod(N, dtype=np.int64)) / GiB, fill, resample.last_path(), filled,
                    int(np.prod(N, dtype=np.int64)), inside, len(boxes), some_in, some_out, call))


def test_walk_set_volume_past_2e32_nodes():
    import measure_ref as MR
    from levelsetpy_amd import _kffi, _vffi, measure, shapes as S
    _walk_plan(_vffi, 1)
    _walk_plan(_kffi, 1)
    _walk_setup("setVolume (and the array leaf that builds its data)", 2)
    N = WALK_N
    total = int(np.prod(N, dtype=np.int64))
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)          # noqa: E731
    g = L.createGrid(col([0.] * 6), col([n - 1 for n in N]), col(N, np.int64), None, low_mem=True)     # unit spacing: node = coordinate
    assert all(np.array_equal(np.asarray(v).ravel(), np.arange(n)) for v, n in zip(g.vs, N))
    centres = sorted(set(i for _, i in walk_places(N, 717550000, 6)))
    # a ball of radius 0.6 around every place holds its centre alone; everything else is positive.  A program holds 64 instructions: 31 balls
    # a pass, a later pass takes the earlier result as an array leaf
    data = None
    t0 = time.perf_counter()
    for k in range(0, len(centres), 31):
        parts = ([S.array(data)] if data is not None else []) + [S.sphere(np.array(c, dtype=np.float64), 0.6) for c in centres[k:k + 31]]
        data = S.evaluate_shape(g, S.union(*parts), 'float32')
        assert S.last_info()["kernel"] == _kffi.kernel_name("float32")
    torch.cuda.synchronize()
    build = time.perf_counter() - t0
    # windows: a ball's bounding box plus one node, clipped; windows that meet are merged until none do
    wins = [([max(0, i - 2) for i in c], [min(n, i + 3) for i, n in zip(c, N)]) for c in centres]
    merged = True
    while merged:
        merged = False
        for a in range(len(wins)):
            for b in range(a + 1, len(wins)):
                if all(wins[a][0][d] < wins[b][1][d] and wins[b][0][d] < wins[a][1][d] for d in range(6)):
                    wins[a] = ([min(x, y) for x, y in zip(wins[a][0], wins[b][0])], [max(x, y) for x, y in zip(wins[a][1], wins[b][1])])
                    del wins[b]
                    merged = True
                    break
            if merged:
                break
    want = dict(cells=int(np.prod([n - 1 for n in N], dtype=np.int64)), full=0, cut=0, invalid=0, Q_cut=0, inside=0, nan=0, lo=list(N), hi=[-1] * 6)
    for lo, hi in wins:
        w = B.gather(data, _ranges(lo, hi)).astype(np.float32)
        r = MR.measure_ref(w, 0.0, ())
        for key in ("full", "cut", "invalid", "Q_cut", "inside", "nan"):
            want[key] += r[key]
        if r["inside"]:
            want["lo"] = [min(a, l + b) for a, l, b in zip(want["lo"], lo, r["lo"])]
            want["hi"] = [max(a, l + b) for a, l, b in zip(want["hi"], lo, r["hi"])]
    want["Q"] = want["full"] * 720 * MR.Q_ONE + want["Q_cut"]
    assert want["inside"] == len(centres) and want["cut"] > len(centres) and want["full"] == 0
    # the condition of the test: no inside node lies outside a window
    flat, below = data.view(-1), 0
    for a in range(0, total, 1 << 28):
        below += int((flat[a:a + (1 << 28)] <= 0).sum())
    assert below == want["inside"], (below, want["inside"])
    t0 = time.perf_counter()
    vol = L.setVolume(g, data)
    torch.cuda.synchronize()
    call = time.perf_counter() - t0
    got = measure.last_info()[0]
    assert measure.last_path() == _vffi.kernel_names("float32", None, 6)
    for key in ("cells", "full", "cut", "invalid", "Q_cut", "Q", "inside", "nan", "lo", "hi"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert vol == MR.volume_of(want["Q"], 6, 1.0)
    _report("walk setVolume %s f32 %.2f GiB %s: %d balls in %d disjoint windows, cut %d inside %d Q_cut %d lo %s hi %s, every integer ==; "
            "the data in %d passes of evaluate_shape %.3f s, the call %.3f s" % (
                N, 4 * total / GiB, measure.last_path(), len(centres), len(wins), want["cut"], want["inside"], want["Q_cut"], want["lo"],
                want["hi"], (len(centres) + 30) // 31, build, call))


def _box_grid32(G, idx):
    """box_ref.box_grid in the oracle's float32 mode: the fp64 nodes kept for the trig tables, the working coordinates rounded once."""
    g = O.Grid(G.min, G.max, [len(i) for i in idx], None, dtype=np.float32)
    g.bc = ['extrapolate'] * G.dim
    g.dx = G.dx.copy()
    vs64 = [np.asarray(G.vs[d]).reshape(-1, 1)[idx[d]].copy() for d in range(G.dim)]
    g.xs64 = np.meshgrid(*vs64, indexing='ij')
    g.vs = [v.astype(np.float32) for v in vs64]
    g.xs = [x.astype(np.float32) for x in g.xs64]
    return g


def test_walk_hidim_substep_past_2e31_cells():
    """hjh_substep of libhj_hidim.so, DubinsPair6D, ENO2, fp32, stage EULER on 36^6 = 2 176 782 336 cells: the 64-bit branch of decode at six
    axes and gather_stencils' 64-bit offsets, against the float32 oracle on boxes (margin 3), bit for bit as tests/test_gpu_fp32_exact.py
    holds ENO2."""
    import hidim_cases as HC
    from levelsetpy_amd import _hffi, hidim
    N = (36,) * 6
    sh = _Shape(N, 4)
    assert sh.cells == 2176782336 >= (1 << 31)
    _tool_start(2 * sh.bytes + (1 << 30), "hjh_substep %s f32" % (N,))
    pd = [2, 5]
    gmin, gmax = [-2.0, -2.2, 0.0, -2.1, -1.9, 0.0], [2.1, 2.0, 2 * np.pi * (1 - 1 / 36), 1.9, 2.2, 2 * np.pi * (1 - 1 / 36)]
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)          # noqa: E731
    g = L.createGrid(col(gmin), col(gmax), col(N, np.int64), pd, low_mem=True)
    G = B.light_grid(gmin, gmax, N, pd)
    for a, b in zip(g.vs, G.vs):
        assert np.array_equal(np.asarray(a).ravel(), b.ravel())
    system = L.DubinsPair6D(g, **HC.PARAMS["pair6d"])
    ham, par = system.native()
    # the data of tests/hidim_cases.py with noise per cell, written on the device one axis-0 slab at a time
    y = torch.empty(N, dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(36)
    x = [torch.as_tensor(v.ravel(), device="cuda") for v in G.vs]
    shape5 = lambda d: [-1 if j == d else 1 for j in range(1, 6)]                # noqa: E731
    for i in range(N[0]):
        base = ((x[0][i] - x[3].reshape(shape5(3))) ** 2 + (x[1].reshape(shape5(1)) - x[4].reshape(shape5(4))) ** 2 + 0.01).sqrt() - 1
        y[i] = (base.expand(N[1:]) + 0.05 * (2 * torch.rand(N[1:], generator=gen, device="cuda", dtype=torch.float64) - 1)).float()
    del base
    out = torch.empty(N, dtype=torch.float32, device="cuda")
    hg = hidim.hi_grid(g, "float32")
    dt = 0.004
    t0 = time.perf_counter()
    hidim._substep(hg, _ffi.ENO2, ham, par, _ffi.STAGE_EULER, 0, y, None, out, dt)
    torch.cuda.synchronize()
    call = time.perf_counter() - t0
    assert _hffi.last_kernel() == _hffi.kernel_name("float32", ham, _ffi.ENO2)
    ext = (2, 2, 2, 2, 2, 4)
    places = [(k, i) for k, i in walk_places(N, sh.cells, 1)]
    assert [k for k, _ in places].count("offset") == 1
    boxes = walk_boxes(N, ext, places)
    cells = 0
    for kind, lo, hi in boxes:
        idx, cmp = B.box(G, lo, hi, B.M_SUBSTEP)
        gb = _box_grid32(G, idx)
        yb = B.gather(y, idx).astype(np.float32)
        yd, _ = O.term_lax_friedrichs(gb, HC.DubinsPair6D(gb, **HC.PARAMS["pair6d"]), "ENO2", 0.0, yb.reshape(-1))
        assert yd.dtype == np.float32
        ref = (yb + np.float32(dt) * yd.reshape(yb.shape))[tuple(cmp)]
        got = B.gather(out, _ranges(lo, hi)).astype(np.float32)
        assert ref.dtype == np.float32 and np.array_equal(got, ref), (kind, lo, int((got != ref).sum()))
        assert not np.array_equal(got, yb[tuple(cmp)])                           # the step moved the data
        cells += ref.size
    _report("walk hjh_substep %s f32 %.2f GiB per array %s EULER: %d boxes (%d cells, margin %d) bitwise against the float32 oracle; the call %.3f s" % (
        N, sh.bytes / GiB, _hffi.last_kernel(), len(boxes), cells, B.M_SUBSTEP, call))
