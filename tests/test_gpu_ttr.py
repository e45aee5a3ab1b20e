"""Time-to-reach functions on the device (levelsetpy_amd/ttr.py, libhj_ttr.so) against the NumPy restatement tests/ttr_ref.py,
BIT FOR BIT: the three entry points on the closed-form stacks of tests/test_ttr_ref.py with special values sprinkled in, the
fold on the device, guarded-buffer runs, bad arguments, the front ends (postTimeStepTTR as an integrator hook, TD2TTR,
HJIPDE_solve's computeTTR) and a census of the library's kernels.

PINNED to the reference: test_init_branch_golden_on_the_device (tests/golden/ttr.npz).  Everything else is UNPINNED (the
reference's update branch raises) and is held to the restatement.

Sizes: n in {1, 7, 957, 1024, 1025} -- one node, less than a wavefront, the odd node count of the 33 x 29 grid, one and two
passes of a workgroup's 512 nodes with a tail of one -- and PAST = 2048 blocks x 256 threads x 2 nodes + 77, at which the
grid-stride loop takes a second pass.  T in {1, 2, 3, 5, 9, 17}: no update at all, and depths on both sides of the kernel's
unroll by four (remainder loop only, one unrolled group, groups plus remainder).  field_stride in {n, n + 1, n + 3}: slices of
alternating alignment.  64-bit indexing is run elsewhere: tests/test_gpu_large_arrays.py
(test_tools_td2ttr_stack_past_2e31_elements) folds a stack of 17 x 2^27 elements, whose last slice starts at element 2^31.

Kernel -> test that launches it (each test asserts the name through hjt_last_kernel; test_census_of_the_ttr_library checks
the table against `nm -D libhj_ttr.so`):
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import postTimeStepTTR, TD2TTR  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _ffi, _tffi  # noqa: E402
from levelsetpy_amd.lazy import HostView  # noqa: E402

import ttr_ref as R  # noqa: E402
from guarded_pool import GuardedPool, PlainAlloc, run_case  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ttr.npz")
TD = {"float64": torch.float64, "float32": torch.float32}
ND = {"float64": np.float64, "float32": np.float32}
CT = {"float64": "double", "float32": "float"}
DT = {"float64": _ffi.F64, "float32": _ffi.F32}
NS = (1, 7, 957, 1024, 1025)
PAST = 2048 * 256 * 2 + 77
MODES = (0, 1, 2, 3)
LEVELS = (0.0, 0.1)

# kernel (as hjt_last_kernel names it) -> the test that launches it and asserts that name
CENSUS = {
    "ttr_from_stack_kernel<double>": "test_from_stack_bitwise",
    "ttr_from_stack_kernel<float>": "test_from_stack_bitwise",
    "ttr_init_kernel<double>": "test_init_then_updates_bitwise_and_equal_to_from_stack",
    "ttr_init_kernel<float>": "test_init_then_updates_bitwise_and_equal_to_from_stack",
    "ttr_update_kernel<double>": "test_init_then_updates_bitwise_and_equal_to_from_stack",
    "ttr_update_kernel<float>": "test_init_then_updates_bitwise_and_equal_to_from_stack",
}
__doc__ += "\n".join("  %-34s %s" % kv for kv in sorted(CENSUS.items())) + "\n"


def launched(kernel, test):
    """The calling thread's last launch ran `kernel`, and the census credits it to `test`."""
    assert _tffi.last_kernel() == kernel, (_tffi.last_kernel(), kernel)
    assert CENSUS[kernel] == test


def same(a, b):
    """Bit for bit, NaN equal to NaN (whatever its payload)."""
    a, b = (np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------ shared cases and references
_CASES, _REFS = {}, {}


def case(T, n, level, dtype):
    """(stack of T slices x n nodes in `dtype`, tau): the expanding disc for T <= 9, the oscillating set for T = 17, widened past
    957 nodes by repeating the grid with a small shift, special values sprinkled in.  Computed once, never modified."""
    key = (T, n, level, dtype)
    if key not in _CASES:
        base, tau = (R.oscillating_set() if T == 17 else R.expanding_disc(T))[:2]
        flat = base.reshape(T, -1)
        reps = -(-n // flat.shape[1])
        wide = np.concatenate([flat + 0.003 * r for r in range(reps)], axis=1)[:, :n]
        data = R.sprinkle(wide, level, seed=T + n)[0].astype(ND[dtype])
        data.setflags(write=False)
        tau.setflags(write=False)
        _CASES[key] = (data, tau)
    return _CASES[key]


def reference(T, n, level, dtype, mode):
    key = (T, n, level, dtype, mode)
    if key not in _REFS:
        data, tau = case(T, n, level, dtype)
        out = R.fold(data, tau, level, mode)
        out.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def strided(data, stride, dtype, pad=-1e30):
    """The stack on the device with slices `stride` elements apart (the last one not padded); the gaps hold a value that would
    change the result if it were read as data."""
    T, n = data.shape
    buf = torch.full(((T - 1) * stride + n,), pad, dtype=TD[dtype], device="cuda")
    d = torch.as_tensor(np.array(data), device="cuda")
    for k in range(T):
        buf[k * stride:k * stride + n] = d[k]
    return buf


def from_stack(lib, dtype, buf, T, stride, n, tau_dev, level, mode):
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    _tffi.check(lib.hjt_ttr_from_stack(DT[dtype], p(buf), T, stride, n, p(tau_dev), level, mode, p(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_from_stack_bitwise(dtype):
    lib = _tffi.lib()
    for T in (1, 2, 3, 5, 9, 17):
        for n in NS:
            for level in LEVELS:
                data, tau = case(T, n, level, dtype)
                tau_dev = torch.as_tensor(np.array(tau), device="cuda")
                for stride in (n, n + 1, n + 3):
                    buf = strided(data, stride, dtype)
                    for mode in MODES:
                        out = from_stack(lib, dtype, buf, T, stride, n, tau_dev, level, mode)
                        assert same(out, reference(T, n, level, dtype, mode)), (T, n, level, stride, mode)
    launched("ttr_from_stack_kernel<%s>" % CT[dtype], "test_from_stack_bitwise")
    # the grid-stride tail: one n just past what a full grid covers in one pass
    data, tau = case(5, PAST, 0.0, dtype)
    tau_dev = torch.as_tensor(np.array(tau), device="cuda")
    buf = strided(data, PAST + 1, dtype)
    for mode in MODES:
        out = from_stack(lib, dtype, buf, 5, PAST + 1, PAST, tau_dev, 0.0, mode)
        assert same(out, reference(5, PAST, 0.0, dtype, mode)), mode


# ------------------------------------------------------------------------------------------ 2. the fold on the device
def device_fold(lib, dtype, data, tau, level, mode):
    """hjt_ttr_init on slice 0, hjt_ttr_update on the others; also checks last_y after every call."""
    n = data.shape[1]
    d = torch.as_tensor(np.array(data), device="cuda")
    ttr = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    last = torch.full((n,), 7.0, dtype=TD[dtype], device="cuda")
    _tffi.check(lib.hjt_ttr_init(DT[dtype], p(d[0]), n, float(tau[0]), level, p(ttr), p(last), _stream()))
    kernels = [_tffi.last_kernel()]
    assert same(last, data[0])
    for k in range(1, len(tau)):
        _tffi.check(lib.hjt_ttr_update(DT[dtype], p(d[k]), n, float(tau[k]), float(tau[k - 1]), level, mode, p(ttr), p(last), _stream()))
        kernels.append(_tffi.last_kernel())
        assert same(last, data[k])
    return ttr, kernels


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_init_then_updates_bitwise_and_equal_to_from_stack(dtype):
    lib = _tffi.lib()
    for T in (1, 2, 3, 5, 9, 17):
        for n in NS:
            for level in LEVELS:
                data, tau = case(T, n, level, dtype)
                tau_dev = torch.as_tensor(np.array(tau), device="cuda")
                buf = strided(data, n, dtype)
                for mode in MODES:
                    ttr, kernels = device_fold(lib, dtype, data, tau, level, mode)
                    assert kernels == ["ttr_init_kernel<%s>" % CT[dtype]] + ["ttr_update_kernel<%s>" % CT[dtype]] * (T - 1)
                    assert same(ttr, reference(T, n, level, dtype, mode)), (T, n, level, mode)
                    assert same(ttr, from_stack(lib, dtype, buf, T, n, n, tau_dev, level, mode))
    data, tau = case(5, PAST, 0.0, dtype)
    for mode in (0, 3):
        ttr, _ = device_fold(lib, dtype, data, tau, 0.0, mode)
        assert same(ttr, reference(5, PAST, 0.0, dtype, mode)), mode
    launched("ttr_update_kernel<%s>" % CT[dtype], "test_init_then_updates_bitwise_and_equal_to_from_stack")
    y = torch.as_tensor(np.array(data[0]), device="cuda")
    L.ttr.ttr_init(y, 0.0)
    launched("ttr_init_kernel<%s>" % CT[dtype], "test_init_then_updates_bitwise_and_equal_to_from_stack")


def test_init_branch_golden_on_the_device():
    """PINNED: the initialisation branch equals the reference's postTimeStepTTR on its recorded inputs."""
    z = np.load(GOLDEN)
    for name in ("vec", "col", "arr"):
        y, t = z[name + "_y"], float(z[name + "_t"])
        for y_in in (y, torch.as_tensor(y, device="cuda")):
            y_out, sd = postTimeStepTTR(t, y_in, L.Bundle({}))
            assert y_out is y_in
            assert same(np.asarray(sd.ttr) if not torch.is_tensor(y_in) else sd.ttr, z[name + "_ttr"])
            assert same(np.asarray(sd.ttrLastY) if not torch.is_tensor(y_in) else sd.ttrLastY, z[name + "_lastY"])
            assert sd.ttrLastT == float(z[name + "_lastT"])


# ------------------------------------------------------------------------------------------ 3. bounds
_POOLS = {}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", 400 * 1000)
    return _POOLS[dtype]


def run_guarded(dtype, op, what):
    """run_case for an operation with arrays of two dtypes: op(D, F, arm) carves the arrays of the data's dtype from D and the
    fp64 ones (ttr, tau) from F.  The fp64 pool drives run_case; for fp32 data a second pool (a second plain allocator in the
    reference run) is begun with the same fill and offset, checked after the call, and its results join the returned dict."""
    if dtype == "float64":
        return run_case(lambda a: op(a, a, a.arm), pool("float64"), what=what)[0]
    P32 = pool("float32")

    def both(a):
        if isinstance(a, GuardedPool):
            b = P32.begin(a.fill, a.offset_elems)
        else:
            b = PlainAlloc(torch.float32, "cuda")
        res = dict(op(b, a, lambda: (a.arm(), b.arm())))
        if isinstance(a, GuardedPool):
            b.check()
        else:
            torch.cuda.synchronize()
        res.update(("f32 " + k, v) for k, v in b.results().items())
        return res
    return run_case(both, pool("float64"), what=what)[0]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernels_stay_inside_their_arrays(dtype):
    """The three entry points on views carved from tests/guarded_pool.py's pools, at element offsets 0-3 and with guards of NaN
    and +-1e30, odd n and odd stride: guards intact, inputs (y, data, tau_dev) unchanged, every element of the outputs written,
    the same bits as on fresh arrays."""
    lib = _tffi.lib()
    T, n, stride, level = 9, 957, 959, 0.1
    data, tau = case(T, n, level, dtype)
    buf = strided(data, stride, dtype, pad=0.05)
    d = torch.as_tensor(np.array(data), device="cuda")
    tau_t = torch.as_tensor(np.array(tau), device="cuda")
    ttr0 = torch.as_tensor(R.fold(data[:4], tau[:4], level, 0), device="cuda")        # the state after three updates

    def init(D, F, arm):
        y = D.inp("y", d[0])
        ttr, last = F.out("ttr", (n,)), D.out("last_y", (n,))
        arm()
        _tffi.check(lib.hjt_ttr_init(DT[dtype], y.ptr, n, 0.25, level, ttr.ptr, last.ptr, _stream()))
        return {"kernel": _tffi.last_kernel()}

    def update(mode):
        def op(D, F, arm):
            y = D.inp("y", d[4])
            ttr, last = F.inout("ttr", ttr0), D.inout("last_y", d[3])
            arm()
            _tffi.check(lib.hjt_ttr_update(DT[dtype], y.ptr, n, float(tau[4]), float(tau[3]), level, mode, ttr.ptr, last.ptr, _stream()))
            return {"kernel": _tffi.last_kernel()}
        return op

    def stack(mode):
        def op(D, F, arm):
            a = D.inp("data", buf)
            tv = F.inp("tau", tau_t)
            ttr = F.out("ttr", (n,))
            arm()
            _tffi.check(lib.hjt_ttr_from_stack(DT[dtype], a.ptr, T, stride, n, tv.ptr, level, mode, ttr.ptr, _stream()))
            return {"kernel": _tffi.last_kernel()}
        return op

    assert run_guarded(dtype, init, "init")["kernel"] == "ttr_init_kernel<%s>" % CT[dtype]
    for mode in MODES:
        assert run_guarded(dtype, update(mode), "update %d" % mode)["kernel"] == "ttr_update_kernel<%s>" % CT[dtype]
        assert run_guarded(dtype, stack(mode), "stack %d" % mode)["kernel"] == "ttr_from_stack_kernel<%s>" % CT[dtype]


# ------------------------------------------------------------------------------------------ 4. bad arguments
def test_entry_points_refuse_bad_arguments():
    lib = _tffi.lib()
    n = 16
    y = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda")
    stack = torch.stack([y, y - 0.5])
    tau = torch.tensor([0.0, 1.0], dtype=torch.float64, device="cuda")
    ttr = torch.full((n,), 5.0, dtype=torch.float64, device="cuda")
    last = torch.full((n,), 6.0, dtype=torch.float64, device="cuda")
    F = _ffi.F64
    bad = [
        lambda: lib.hjt_ttr_init(F, None, n, 0.0, 0.0, p(ttr), p(last), None),
        lambda: lib.hjt_ttr_init(F, p(y), n, 0.0, 0.0, None, p(last), None),
        lambda: lib.hjt_ttr_init(F, p(y), n, 0.0, 0.0, p(ttr), None, None),
        lambda: lib.hjt_ttr_init(F, p(y), -1, 0.0, 0.0, p(ttr), p(last), None),
        lambda: lib.hjt_ttr_update(F, None, n, 1.0, 0.0, 0.0, 0, p(ttr), p(last), None),
        lambda: lib.hjt_ttr_update(F, p(y), n, 1.0, 0.0, 0.0, 0, None, p(last), None),
        lambda: lib.hjt_ttr_update(F, p(y), n, 1.0, 0.0, 0.0, 0, p(ttr), None, None),
        lambda: lib.hjt_ttr_update(F, p(y), n, 1.0, 0.0, 0.0, 0, p(ttr), p(y), None),             # y == last_y
        lambda: lib.hjt_ttr_update(F, p(y), n, 1.0, 0.0, 0.0, 4, p(ttr), p(last), None),          # unknown mode
        lambda: lib.hjt_ttr_from_stack(F, None, 2, n, n, p(tau), 0.0, 0, p(ttr), None),
        lambda: lib.hjt_ttr_from_stack(F, p(stack), 2, n, n, None, 0.0, 0, p(ttr), None),
        lambda: lib.hjt_ttr_from_stack(F, p(stack), 2, n, n, p(tau), 0.0, 0, None, None),
        lambda: lib.hjt_ttr_from_stack(F, p(stack), 0, n, n, p(tau), 0.0, 0, p(ttr), None),       # T = 0
        lambda: lib.hjt_ttr_from_stack(F, p(stack), 2, n - 1, n, p(tau), 0.0, 0, p(ttr), None),   # field_stride < n
        lambda: lib.hjt_ttr_from_stack(F, p(stack), 2, n, n, p(tau), 0.0, -1, p(ttr), None),      # unknown mode
    ]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert lib.hjt_last_error(), k
    for call in (lambda: lib.hjt_ttr_init(7, p(y), n, 0.0, 0.0, p(ttr), p(last), None),           # unknown dtype
                 lambda: lib.hjt_ttr_update(7, p(y), n, 1.0, 0.0, 0.0, 0, p(ttr), p(last), None),
                 lambda: lib.hjt_ttr_from_stack(-1, p(stack), 2, n, n, p(tau), 0.0, 0, p(ttr), None)):
        assert call() == -3
        assert b"dtype" in lib.hjt_last_error()
    with pytest.raises(_ffi.Unsupported):
        _tffi.check(lib.hjt_ttr_init(7, p(y), n, 0.0, 0.0, p(ttr), p(last), None))
    with pytest.raises(ValueError):
        _tffi.check(lib.hjt_ttr_from_stack(F, p(stack), 0, n, n, p(tau), 0.0, 0, p(ttr), None))
    torch.cuda.synchronize()
    assert bool((ttr == 5.0).all()) and bool((last == 6.0).all())                                 # nothing was launched
    # n = 0: fine, and launches nothing
    _tffi.check(lib.hjt_ttr_from_stack(F, p(stack), 2, n, n, p(tau), 0.0, 0, p(ttr), None))
    assert _tffi.last_kernel() == "ttr_from_stack_kernel<double>"
    assert lib.hjt_ttr_init(F, None, 0, 0.0, 0.0, None, None, None) == 0
    assert lib.hjt_ttr_update(F, None, 0, 1.0, 0.0, 0.0, 0, None, None, None) == 0
    assert _tffi.last_kernel() == "ttr_from_stack_kernel<double>"
    assert lib.hjt_ttr_from_stack(F, None, 2, 0, 0, p(tau), 0.0, 0, None, None) == 0
    g = L.createGrid(np.array([[-1.0, -1.0]]).T, np.array([[1.0, 1.0]]).T, np.array([[4, 4]]).T, None)
    with pytest.raises(ValueError):
        TD2TTR(g, stack.reshape(2, 4, 4), [0.0])                      # one time for two slices
    with pytest.raises(ValueError):
        TD2TTR(g, stack.reshape(2, 4, 4), [1.0, 0.0])                 # decreasing
    with pytest.raises(ValueError):
        TD2TTR(g, stack.reshape(2, 2, 8), [0.0, 1.0])                 # not the grid's shape
    with pytest.raises(ValueError):
        TD2TTR(g, stack.reshape(2, 4, 4), [0.0, 1.0], crossing='middle')
    with pytest.raises(AssertionError):
        postTimeStepTTR(1.0, y, L.Bundle(dict(ttr=ttr)))              # .ttr without the auxiliary fields


# ------------------------------------------------------------------------------------------ 5. front ends
def dubins(n):
    """The Dubins problem of smoke() on n^3 nodes."""
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
    d0 = L.shapeCylinder(g, 2, np.zeros((3, 1)), .5)
    s = L.DubinsVehicleRel(g, 1, 1)
    sd = L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation,
                       dissFunc=L.artificialDissipationGLF, CoStateCalc=L.upwindFirstWENO5))
    return g, d0, sd


@pytest.mark.parametrize("where", ["tensor", "numpy"])
def test_post_time_step_hook_in_the_integrator(where):
    g, d0, sd = dubins(24)
    opts = {} if where == "tensor" else dict(ttrCrossing='first', ttrLevel=0.05)
    for k, v in opts.items():
        setattr(sd, k, v)
    y0 = L.expand(d0.flatten(), 1)
    if where == "tensor":
        y0 = torch.as_tensor(y0, device="cuda")
    seen = []

    def record(t, y, s):
        seen.append((float(t), np.array(y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y))))
        return y, s
    y_back, sd = postTimeStepTTR(0.0, y0, sd)                          # the initial data, as the reference's docstring advises
    assert y_back is y0
    op = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='off', postTimeStep=[postTimeStepTTR, record])))
    t, y, sd = L.odeCFL3(L.termLaxFriedrichs, [0., 0.3], y0, op, sd)
    assert len(seen) >= 3 and seen[-1][0] == float(t)
    kind = torch.Tensor if where == "tensor" else HostView
    assert isinstance(sd.ttr, kind) and isinstance(sd.ttrLastY, kind) and sd.ttrLastT == float(t)
    assert tuple(sd.ttr.shape) == tuple(y0.shape)
    if where == "tensor":
        assert sd.ttr.is_cuda and sd.ttr.dtype == torch.float64
    taus = [0.0] + [s[0] for s in seen]
    stack = np.stack([np.asarray(d0, dtype=np.float64).reshape(-1, 1)] + [s[1] for s in seen])
    want = R.fold(stack, taus, opts.get('ttrLevel', 0.0), R.mode_bits(opts.get('ttrCrossing', 'last'), True))
    got = sd.ttr if where == "tensor" else np.asarray(sd.ttr)
    assert same(got, want)
    assert same(sd.ttrLastY if where == "tensor" else np.asarray(sd.ttrLastY), seen[-1][1])
    assert np.isfinite(want).sum() > (stack[0] <= opts.get('ttrLevel', 0.0)).sum()      # the set grew: crossings were recorded


def test_hjipde_solve_compute_ttr_equals_td2ttr_of_the_stored_solve():
    g, d0, sd = dubins(21)
    tau = np.linspace(0.0, 0.4, 5)
    full, tau_out, outs = L.HJIPDE_solve(d0, tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True)))
    assert not hasattr(outs, 'TTR') and len(tau_out) == 5 and full.shape == (5, 21, 21, 21)
    for extra in (dict(ttrCrossing='first'), dict(ttrCrossing='last'), dict(), dict(ttrInterpolate=True, ttrLevel=0.05)):
        kw = dict(crossing=extra.get('ttrCrossing', 'first'), interpolate=extra.get('ttrInterpolate', False),
                  level=extra.get('ttrLevel', 0.0))
        want = TD2TTR(g, full, tau, **kw)
        assert isinstance(want, np.ndarray) and want.shape == (21, 21, 21) and want.dtype == np.float64
        assert same(want, R.TD2TTR(full, tau, kw['level'], kw['crossing'], kw['interpolate']))
        for keep in ('keepLast', 'lowMemory'):
            last, _, outs = L.HJIPDE_solve(d0, tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, computeTTR=True, **{keep: True}, **extra)))
            assert same(last, full[-1])
            assert isinstance(outs.TTR, np.ndarray) and same(outs.TTR, want), (extra, keep)
        assert np.isfinite(want).sum() > (full[0] <= kw['level']).sum()
    # store-all mode with the option, a device tensor in, flipOutput: the same TTR, as a tensor
    d_t = torch.as_tensor(d0, device="cuda")
    flipped, _, outs = L.HJIPDE_solve(d_t, tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, computeTTR=True, flipOutput=True)))
    assert same(flipped.flip(0), full)
    assert torch.is_tensor(outs.TTR) and outs.TTR.is_cuda and same(outs.TTR, TD2TTR(g, full, tau))
    # a given history is folded first: continuing from the first three slices gives the TTR of the whole solve
    _, _, outs = L.HJIPDE_solve(full[:3], tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, computeTTR=True, keepLast=True)))
    assert same(outs.TTR, TD2TTR(g, full, tau))
    # tensor / HostView in -> tensor out
    assert torch.is_tensor(TD2TTR(g, torch.as_tensor(full, device="cuda"), tau))
    assert torch.is_tensor(TD2TTR(g, HostView(torch.as_tensor(full, device="cuda")), tau))


# ------------------------------------------------------------------------------------------ 6. census
def test_census_of_the_ttr_library():
    """Every __device_stub__ of `nm -D libhj_ttr.so` is in CENSUS, and every entry names a test of this file that asserts
    the launch through hjt_last_kernel (the `launched(kernel, test)` calls)."""
    out = subprocess.check_output(["nm", "-D", "-C", _tffi.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+<[^>]*>)\(", out))
    assert stubs, "no kernels found in %s" % _tffi.LIB_PATH
    assert stubs == set(CENSUS), (sorted(stubs - set(CENSUS)), sorted(set(CENSUS) - stubs))
    src = open(os.path.abspath(__file__)).read()
    for kernel, test in CENSUS.items():
        fn = globals().get(test)
        assert callable(fn), test
        body = src[src.index("def %s(" % test):]
        body = body[:body.index("\n\n\n")]
        assert 'launched(' in body and '"%s"' % test in body, test
