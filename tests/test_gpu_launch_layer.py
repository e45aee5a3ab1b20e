"""The launch layer the tiled substep kernels share (levelsetpy_amd/csrc/hj_launch.h): the HJ_TIMING_DUMP path beside the enqueue, and the
process-wide table of dynamic-LDS grants.  fp64 Dubins on grids of a few tens of cells per axis, pair kernel at any size."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, dist  # noqa: E402
from levelsetpy_amd.context import DeviceGrid  # noqa: E402

from test_gpu_parity import _substep, dubins  # noqa: E402

PAR_DUBINS = [1., 1., 1., 2.]
SCHEME = "WENO5_ASSHIPPED"
KNOBS = dict(HJ_DIRECT_BELOW="0", HJ_PAIR="2", HJ_AUTOTUNE="0")
BC = (_ffi.BC_EXTRAPOLATE, _ffi.BC_EXTRAPOLATE, _ffi.BC_PERIODIC)       # dubins(): axis 2 periodic


def _case(n):
    g, _ = dubins(np.array(n))
    rng = np.random.default_rng(7)
    return g, L.shapeCylinder(g, 2, np.zeros((3, 1)), .5) + 0.01 * rng.standard_normal(n)


def _plan(n, stage):
    return dist.plan_substep(n, BC, "float64", _ffi.SCHEME_IDS[SCHEME], _ffi.HAM_DUBINS_REL, stage, 0, n[0])


def test_timing_dump_writes_one_row_per_workgroup_and_leaves_the_result_alone(tmp_path, monkeypatch):
    """HJ_TIMING_DUMP=file (read when the context is created): every tiled launch appends `# launch nblocks=K ...` and K rows of
    `index start end start2 end2 + 8 phase sums` (tools/block_timing.py, tools/stamp_summary.py).  One Euler substep: the file holds
    exactly that, K is the planner's workgroup count, and `out` is bitwise what a context without the dump computes."""
    n = (40, 36, 40)
    g, data = _case(n)
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)
    path = tmp_path / "timing.txt"
    outs = {}
    for dump in (False, True):
        if dump:
            monkeypatch.setenv("HJ_TIMING_DUMP", str(path))
        else:
            monkeypatch.delenv("HJ_TIMING_DUMP", raising=False)
        dg = DeviceGrid(g, "float64")
        dg.bind_stream()
        y, out = dg.to_device(data), dg.empty()
        _substep(dg, SCHEME, _ffi.HAM_DUBINS_REL, PAR_DUBINS, _ffi.STAGE_EULER, 2e-3, y, None, out)
        dg.sync()
        assert dg.lib.hj_last_kernel(dg.ctx) == b"fused_pair_kernel"
        outs[dump] = out
    assert torch.equal(outs[False], outs[True])
    assert float((outs[True] - torch.as_tensor(data, device="cuda")).abs().max()) > 0
    plan = _plan(n, _ffi.STAGE_EULER)
    assert plan["kernel"] == "fused_pair_kernel"
    lines = path.read_text().splitlines()
    headers = [ln for ln in lines if ln.startswith("#")]
    assert len(headers) == 1 and lines[0] == headers[0] and headers[0].startswith("# launch nblocks="), headers
    fields = dict(f.split("=") for f in headers[0][len("# launch "):].split())
    K = int(fields["nblocks"])
    print("timing dump: header %r, %d rows; planned workgroups %d" % (headers[0], len(lines) - 1, plan["workgroups"]))
    assert K == plan["workgroups"]
    assert (int(fields["ntiles"]), int(fields["chunk"]), int(fields["stage"])) == (plan["tiles"], plan["chunk_planes"], _ffi.STAGE_EULER)
    rows = [[int(v) for v in ln.split()] for ln in lines[1:]]
    assert len(rows) == K and all(len(r) == 13 for r in rows)
    assert [r[0] for r in rows] == list(range(K))
    assert all(r[2] >= r[1] > 0 for r in rows)        # every workgroup stamped its start and its end


def test_lds_grants_of_two_contexts_share_one_table(monkeypatch):
    """More than 64 KB of dynamic LDS is granted per (device, kernel function), raised and never lowered, in ONE table for the process.  Two
    contexts launch the same fused_pair_kernel instantiations with the halo ring parked in LDS (HJ_PAIR_RING=1): 40x36x40 first, then
    48x44x160, whose longer rows ask for more, then the first again -- every RK3 step bitwise the step with the double buffer (HJ_PAIR_RING=0,
    under 64 KB: no grant at all)."""
    small, big = (40, 36, 40), (48, 44, 160)
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)
    cases = {n: _case(n) for n in (small, big)}

    def step(dg, y):
        nxt, w0, w1 = dg.empty(), dg.empty(), dg.empty()
        tout, dtout = C.c_double(), C.c_double()
        _ffi.check(dg.lib.hj_rk_step(dg.ctx, 3, _ffi.SCHEME_IDS[SCHEME], _ffi.HAM_DUBINS_REL, _ffi.darr(PAR_DUBINS), 0., 1e9, 0.8, 1e300, 0,
                                     dg.ptr(y), dg.ptr(nxt), dg.ptr(w0), dg.ptr(w1), C.byref(tout), C.byref(dtout)))
        dg.sync()
        assert dg.lib.hj_last_kernel(dg.ctx) == b"fused_pair_kernel"
        return nxt

    res = {}
    for ring in ("1", "0"):
        monkeypatch.setenv("HJ_PAIR_RING", ring)
        lds = [max(_plan(n, st)["lds_bytes"] for st in (_ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF)) for n in (small, big)]
        print("HJ_PAIR_RING=%s: planned LDS bytes %s" % (ring, lds))
        if ring == "1":
            assert 64 * 1024 < lds[0] < lds[1]
        else:
            assert max(lds) <= 64 * 1024
        ctx = {n: DeviceGrid(cases[n][0], "float64") for n in (small, big)}         # both alive at once
        for dg in ctx.values():
            dg.bind_stream()
        y = {n: ctx[n].to_device(cases[n][1]) for n in (small, big)}
        a = step(ctx[small], y[small])
        b = step(ctx[big], y[big])
        a2 = step(ctx[small], a)
        nbuf, ahead = C.c_int(), C.c_int()
        _ffi.check(ctx[small].lib.hj_last_launch(ctx[small].ctx, C.byref(nbuf), C.byref(ahead)))
        assert (ahead.value > 0 and nbuf.value == 2 + ahead.value) if ring == "1" else (nbuf.value, ahead.value) == (2, 0)
        res[ring] = (a, b, a2)
    for r1, r0 in zip(res["1"], res["0"]):
        assert torch.equal(r1, r0)
    assert float((res["1"][2] - res["1"][0]).abs().max()) > 0
