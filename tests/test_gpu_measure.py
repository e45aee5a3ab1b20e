"""GPU: levelsetpy_amd.measure (libhj_measure.so) against the NumPy / Python-integer restatement tests/measure_ref.py and against
the package itself.  Every integer of a record is compared with ==: the sums are integer sums and the per-simplex arithmetic is
one rounding per operation, so no tolerance is due.  The grids are measure_ref.GRIDS, the smallest at which the decode, the periodic
wrap, the ballot compaction and the rounds of the cut-cell list can go wrong; tests/test_measure_ref.py proves the restatement on
closed forms.
"""
import ctypes as C

import numpy as np
import pytest

import measure_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("cells", "full", "cut", "invalid", "Q_cut", "Q", "inside", "nan", "lo", "hi")
IDS = ["x".join(map(str, N)) for N, _ in R.GRIDS]


def _L():
    import levelsetpy_amd as L
    return L


def pkg_grid(N, periodic=(), low_mem=False):
    """The package's grid of measure_ref.grid_vectors: the same vs and dx bit for bit."""
    L = _L()
    vs, dx, mins, maxs = R.grid_vectors(N, periodic)
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    g = L.createGrid(col(mins), col(maxs), col(N, np.int64), list(periodic) if periodic else None, low_mem=low_mem)
    for d in range(len(N)):
        assert np.array_equal(np.asarray(g.vs[d]).ravel(), vs[d]) and float(np.asarray(g.dx).ravel()[d]) == dx[d]
        assert (g.bdry[d] is L.addGhostPeriodic) == (d in periodic)
    return g


_CASES = {}


def case(i):
    """(N, periodic, package grid, fp64 field, its record by the restatement) of GRIDS[i], made once."""
    if i not in _CASES:
        N, per = R.GRIDS[i]
        data = R.field(N, per)
        data.setflags(write=False)
        _CASES[i] = (N, per, pkg_grid(N, per), data, R.measure_ref(data, 0.0, per))
    return _CASES[i]


def same_record(got, want, what=""):
    for k in KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def cellvol(N, per):
    return R.cell_volume(R.grid_vectors(N, per)[1])


# ------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("i", range(len(R.GRIDS)), ids=IDS)
def test_every_integer_of_the_record_equals_the_restatement(i):
    from levelsetpy_amd import measure, _vffi
    L = _L()
    N, per, g, data, want = case(i)
    D = len(N)
    empty = want["cells"] - want["full"] - want["cut"] - want["invalid"]
    print("%s: cells %d full %d cut %d empty %d" % (N, want["cells"], want["full"], want["cut"], empty))
    if want["cells"] > 1:                                         # the condition the cases were chosen for
        assert want["full"] > 0 and want["cut"] > 0 and empty > 0 and want["invalid"] == 0, want
    vol, info = L.setVolume(g, data, return_info=True)
    same_record(measure.last_info()[0], want, N)
    assert isinstance(vol, float) and vol == R.volume_of(want["Q"], D, cellvol(N, per))
    assert measure.last_path() == info["kernel"] == _vffi.kernel_names("float64", None, D)
    assert (info["cells"], info["full"], info["cut"], info["invalid"], info["inside"], info["nan"], info["Q"]) == (
        want["cells"], want["full"], want["cut"], want["invalid"], want["inside"], want["nan"], want["Q"])
    for level in (0.31, -0.4):                                    # another level: one fp64 subtraction per node
        L.setVolume(g, data, level)
        same_record(measure.last_info()[0], R.measure_ref(data, level, per), (N, level))


@pytest.mark.parametrize("i", [1, 2, 5], ids=[IDS[k] for k in (1, 2, 5)])
def test_fp32_data_is_widened_then_measured(i):
    import torch
    from levelsetpy_amd import measure, _vffi
    L = _L()
    N, per, g, data, _ = case(i)
    d32 = data.astype(np.float32)
    want = R.measure_ref(d32, 0.03, per)
    assert want["cut"] > 0
    for arg in (d32, torch.as_tensor(d32, device="cuda")):
        vol = L.setVolume(g, arg, 0.03)
        same_record(measure.last_info()[0], want, N)
        assert vol == R.volume_of(want["Q"], len(N), cellvol(N, per)) and measure.last_path() == _vffi.kernel_names("float32", None, len(N))


@pytest.mark.parametrize("i", [2, 4], ids=[IDS[k] for k in (2, 4)])
def test_a_stack_of_three_fields(i):
    from levelsetpy_amd import measure
    L = _L()
    N, per, g, _, _ = case(i)
    stack = R.field(N, per, seed=5, stack=3)
    vols, info = L.setVolume(g, stack, return_info=True)
    assert vols.shape == (3,) and vols.dtype == np.float64 and info["cut"].dtype == np.int64
    for k in range(3):
        want = R.measure_ref(stack[k], 0.0, per)
        same_record(measure.last_info()[k], want, (N, k))
        assert vols[k] == R.volume_of(want["Q"], len(N), cellvol(N, per)) and info["cut"][k] == want["cut"] and info["Q"][k] == want["Q"]
    assert len(set(vols)) == 3


def test_more_fields_than_one_launch_holds():
    """65535 + 70 fields on (3, 2): the second launch's fields are measured as the first's, each against its own restatement."""
    L = _L()
    N, S = (3, 2), 65535 + 70
    g = pkg_grid(N)
    rng = np.random.default_rng(9)
    kinds = rng.uniform(-1, 1, (16,) + N)
    kinds[3] = -1.0
    kinds[7] = 1.0
    which = (np.arange(S) * 7) % 16
    vols, info = L.setVolume(g, kinds[which], return_info=True)
    want = [R.measure_ref(k) for k in kinds]
    assert len(set(w["Q"] for w in want)) >= 14 and which[65534] != which[65535] != which[65536]
    for key in ("full", "cut", "inside"):
        assert np.array_equal(info[key], np.array([w[key] for w in want])[which]), key
    assert info["Q"] == [want[k]["Q"] for k in which]
    assert np.array_equal(vols, np.array([R.volume_of(w["Q"], 2, cellvol(N, ())) for w in want])[which])


def test_nan_and_infinite_nodes():
    from levelsetpy_amd import measure
    L = _L()
    N, per, g, data, _ = case(2)
    d = data.copy()
    d[1, 2, 3] = np.nan
    d[4, 4, 6] = np.inf                                           # on the periodic axis' last node: its cells wrap
    d[7, 1, 0] = -np.inf
    d[8, 7, 2] = np.nan                                           # a corner node of the grid
    want = R.measure_ref(d, 0.0, per)
    assert want["invalid"] >= 20 and want["nan"] == 2 and want["cut"] > 0 and want["full"] > 0
    vol = L.setVolume(g, d)
    same_record(measure.last_info()[0], want)
    assert np.isfinite(vol)


def test_views_at_odd_element_offsets_a_hostview_and_a_low_mem_grid():
    import torch
    from levelsetpy_amd import measure
    from levelsetpy_amd.lazy import HostView
    L = _L()
    for i, dtype in ((1, torch.float64), (3, torch.float32), (5, torch.float64)):
        N, per, g, data, _ = case(i)
        d = data.astype(np.float32) if dtype == torch.float32 else data
        want = R.measure_ref(d, 0.0, per)
        n = d.size
        for off in (1, 2, 3):
            big = torch.full((n + 8,), 1e30, dtype=dtype, device="cuda")
            view = big[off:off + n].view(N)
            view.copy_(torch.as_tensor(np.array(d)))
            assert view.data_ptr() == big.data_ptr() + off * big.element_size()
            L.setVolume(g, view)
            same_record(measure.last_info()[0], want, (N, off))
        L.setVolume(g, HostView(torch.as_tensor(d, device="cuda")))
        same_record(measure.last_info()[0], want, (N, "HostView"))
    N, per, g, data, want = case(5)
    glow = pkg_grid(N, per, low_mem=True)
    assert np.size(glow.xs[0]) < data.size
    assert L.setVolume(glow, data) == L.setVolume(g, data)
    same_record(measure.last_info()[0], want, "low_mem")


# ------------------------------------------------------------------------------------------ compare
@pytest.mark.parametrize("i", [1, 3, 5], ids=[IDS[k] for k in (1, 3, 5)])
def test_compare_is_four_measurements_of_the_minimum_and_maximum_arrays(i):
    import torch
    from levelsetpy_amd import measure, _vffi
    L = _L()
    N, per, g, a, _ = case(i)
    D = len(N)
    b = R.field_b(N, per)
    level = 0.02
    for ta, tb in ((np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32)):
        A, B = torch.as_tensor(a.astype(ta), device="cuda"), torch.as_tensor(b.astype(tb), device="cuda")
        out = L.setCompare(g, A, B, level)
        got = measure.last_info()
        assert measure.last_path() == _vffi.kernel_names(np.dtype(ta).name, np.dtype(tb).name, D)
        wide = (A.double(), B.double())
        separate = {}
        for name, arr in (("A", A), ("B", B), ("union", torch.minimum(*wide)), ("intersection", torch.maximum(*wide))):
            L.setVolume(g, arr, level)
            separate[name] = measure.last_info()[0]
        want = R.compare_ref(a.astype(ta), b.astype(tb), level, per)
        for name in R.SETS:
            same_record(got[name][0], separate[name], (N, name, "separate"))
            same_record(got[name][0], want[name], (N, name, "restatement"))
        # neither set holds the other: the four volumes are four different numbers
        assert want["intersection"]["Q"] < min(want["A"]["Q"], want["B"]["Q"]) and max(want["A"]["Q"], want["B"]["Q"]) < want["union"]["Q"]
        assert want["intersection"]["cut"] > 0 and want["union"]["cut"] > 0
        vals = R.compare_values(want, D, cellvol(N, per))
        assert (out.volA, out.volB, out.union, out.intersection, out.symdiff, out.iou) == vals
    # a NaN in either input propagates into the union and the intersection
    a2 = a.copy()
    a2[(1,) * D] = np.nan
    L.setCompare(g, a2, b)
    want = R.compare_ref(a2, b, 0.0, per)
    for name in R.SETS:
        same_record(measure.last_info()[name][0], want[name], (N, name, "nan"))
    assert want["union"]["nan"] == 1 and want["B"]["nan"] == 0 and want["union"]["invalid"] > 0


def test_compare_stacks_and_broadcasts_b():
    from levelsetpy_amd import measure
    L = _L()
    N, per, g, _, _ = case(2)
    a = R.field(N, per, seed=5, stack=3)
    b = R.field(N, per, seed=6, stack=3) + 0.05
    for bb, pick in ((b, lambda k: b[k]), (b[1], lambda k: b[1]), (b[1:2], lambda k: b[1])):
        out = L.setCompare(g, a, bb)
        assert out.symdiff.shape == (3,)
        for k in range(3):
            want = R.compare_ref(a[k], pick(k), 0.0, per)
            for name in R.SETS:
                same_record(measure.last_info()[name][k], want[name], (name, k))
            assert (out.volA[k], out.volB[k], out.union[k], out.intersection[k], out.symdiff[k], out.iou[k]) == R.compare_values(
                want, 3, cellvol(N, per))
    empty = L.setCompare(g, np.ones(N), np.full(N, 2.0))
    assert empty.union == 0.0 and empty.symdiff == 0.0 and np.isnan(empty.iou)


# ------------------------------------------------------------------------------------------ bounds and the crop
@pytest.mark.parametrize("i", [0, 1, 4, 5], ids=[IDS[k] for k in (0, 1, 4, 5)])
def test_bounds_are_numpys_and_truncate_keeps_them(i):
    import torch
    L = _L()
    N, per, g, data, want = case(i)
    vs, dx, _, _ = R.grid_vectors(N, per)
    for pad in (0, 1, 2):
        b = L.setBounds(g, data, pad=pad)
        lo, hi, xmin, xmax = R.bounds_ref(N, vs, dx, per, want["lo"], want["hi"], pad)
        inside = np.argwhere(data <= 0)
        assert want["lo"] == list(inside.min(axis=0)) and want["hi"] == list(inside.max(axis=0))
        assert list(b.lo) == lo and list(b.hi) == hi and np.array_equal(b.xmin.ravel(), xmin) and np.array_equal(b.xmax.ravel(), xmax)
        assert b.xmin.shape == (len(N), 1)
        gH, dH = L.truncateGrid(g, data, b.xmin, b.xmax)
        keep, ref = R.truncate_ref(vs, data, xmin, xmax)
        assert [list(k) for k in keep] == [list(range(l, h + 1)) for l, h in zip(lo, hi)]
        assert isinstance(dH, np.ndarray) and np.array_equal(dH, ref)
        gT, dT = L.truncateGrid(g, torch.as_tensor(data, device="cuda"), b.xmin, b.xmax)
        assert dT.is_cuda and np.array_equal(dT.cpu().numpy(), ref)
        for d in range(len(N)):
            assert np.array_equal(np.asarray(gT.vs[d]).ravel(), vs[d][keep[d]])
            assert (gT.bdry[d] is L.addGhostPeriodic) == (d in per and len(keep[d]) == N[d])
    assert L.setBounds(g, np.ones(N)) is None
    stack = np.stack([data, data + 0.2])
    b2 = L.setBounds(g, stack, pad=0)                             # a stack: the box of all its fields
    assert list(b2.lo) == list(L.setBounds(g, data, pad=0).lo)
    gS, dS = L.truncateGrid(g, torch.as_tensor(stack, device="cuda"), b2.xmin, b2.xmax)
    assert np.array_equal(dS.cpu().numpy(), R.truncate_ref(vs, stack, b2.xmin.ravel(), b2.xmax.ravel(), lead=1)[1])


# ------------------------------------------------------------------------------------------ the C ABI on guarded buffers
@pytest.mark.parametrize("i", [1, 4, 5], ids=[IDS[k] for k in (1, 4, 5)])
def test_guarded_buffers(i):
    """hjv_measure on views of one guarded allocation, at element offsets 0 .. 3: no guard and no input changes, every word of
    every record is written, and the bits are those of the run on fresh arrays.  Two fields, measured and compared."""
    import torch
    import guarded_pool as GP
    from levelsetpy_amd import _vffi
    N, per, g, _, _ = case(i)
    D, total = len(N), int(np.prod(N))
    a = R.field(N, per, seed=31, stack=2)
    b = R.field(N, per, seed=32) - 0.04
    desc = _vffi.extents_descriptor(N, per)
    pool = GP.GuardedPool(torch.float64, "cuda", 1 << 20)
    for compare in (0, 1):
        sets = 4 if compare else 1

        def op(alloc):
            da = alloc.inp("a", torch.as_tensor(a, device="cuda").reshape(2, total))
            db = alloc.inp("b", torch.as_tensor(b, device="cuda").reshape(1, total))
            rec = alloc.out("records", (2 * sets, _vffi.RECORD_WORDS))          # int64 in an fp64 view: the bits are compared
            work = alloc.scratch("work", (int(_vffi.lib().hjv_workspace_size(C.byref(desc), 2, compare)) // 8,))
            alloc.arm()
            _vffi.check(_vffi.lib().hjv_measure(C.byref(desc), da.ptr, 2, total, db.ptr if compare else None, 0, 1, total, 0.01,
                                                rec.ptr, work.ptr, None))
            return {}
        ref, arrays = GP.run_case(op, pool, what="measure %d-D compare %d" % (D, compare))
        words = arrays["records"].view(torch.int64).cpu().numpy().reshape(2, sets, _vffi.RECORD_WORDS)
        from levelsetpy_amd.measure import _record
        for k in range(2):
            want = R.compare_ref(a[k], b, 0.01, per) if compare else {"A": R.measure_ref(a[k], 0.01, per)}
            for s, name in enumerate(R.SETS[:sets]):
                same_record(_record(words[k, s], D), want[name], (N, compare, k, name))


# ------------------------------------------------------------------------------------------ a solve continued on the cropped grid
def test_a_plane5d_solve_continues_on_the_grid_cropped_by_the_bounds():
    import torch
    L = _L()
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    N = (13, 12, 8, 5, 5)
    top = 2 * np.pi * (1 - 1.0 / N[2])
    g = L.createGrid(col([-2, -2, 0, 0.5, -1]), col([2, 2, top, 1.5, 1]), col(N, np.int64), [2])
    X = np.meshgrid(*[np.asarray(v).ravel() for v in g.vs], indexing="ij")
    data = np.sqrt((X[0] - 0.2) ** 2 + (X[1] + 0.1) ** 2) - 0.7
    b = L.setBounds(g, data, pad=2)
    assert list(b.lo) == [3, 2, 0, 0, 0] and list(b.hi) == [10, 9, 7, 4, 4]          # cropped in x and y, whole elsewhere
    gT, dT = L.truncateGrid(g, torch.as_tensor(data, device="cuda"), b.xmin, b.xmax)
    gH, dH = L.truncateGrid(g, data, b.xmin, b.xmax)
    assert tuple(dT.shape) == (8, 8, 8, 5, 5) and gT.bdry[2] is L.addGhostPeriodic and gT.bdry[0] is L.addGhostExtrapolate
    results = []
    for gg, dd in ((gT, dT), (gH, dH)):
        plane = L.Plane5D(gg, a_max=0.8, alpha_max=1.3, u_mode='min')
        sd = L.Bundle(dict(grid=gg, hamFunc=plane.hamiltonian, partialFunc=plane.dissipation, dissFunc=L.artificialDissipationGLF,
                           derivFunc=L.upwindFirstENO2))
        V = L.HJIPDE_solve(dd, np.array([0.0, 0.05]), sd, 'minVOverTime', L.Bundle(dict(quiet=True, keepLast=True)))[0]
        results.append(V.cpu().numpy() if hasattr(V, "cpu") else np.asarray(V))
    assert results[0].shape == (8, 8, 8, 5, 5) and np.array_equal(results[0], results[1])
    assert not np.array_equal(results[0], dH)                     # the solve moved the data
    assert L.setVolume(gT, results[0]) >= L.setVolume(gT, dH) > 0.0          # minVOverTime: the tube only grows
