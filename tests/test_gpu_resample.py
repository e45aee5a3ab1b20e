"""GPU: levelsetpy_amd.resample (libhj_resample.so) against the NumPy restatement tests/resample_ref.py and against the package
itself.  fp64 results are held to the restatement with array_equal: the operations and their order are the same, no tolerance
is due.  The grids are tests/resample_ref.py's PAIRS, the smallest at which the decode, the corner loop and the chunking can go
wrong; tests/test_resample_ref.py proves the restatement on closed forms and that these cases fill, and leave, a tenth of the
destination's nodes.
"""
import ctypes as C

import numpy as np
import pytest

import resample_ref as R

pytestmark = pytest.mark.gpu

FILLS = ('max', 'nan', 2.5)
REDUCES = (None, 'min', 'max')


def _L():
    import levelsetpy_amd as L
    return L


def pkg_grid(ref, low_mem=False):
    """The package's grid of a RefGrid: the same bounds and extents, hence the same vs and dx bit for bit."""
    L = _L()
    pd = [d for d in range(ref.dim) if ref.bc[d] == 'periodic']
    g = L.createGrid(ref.min.reshape(-1, 1), ref.max.reshape(-1, 1), ref.N.reshape(-1, 1), pd if pd else None, low_mem=low_mem)
    for d in range(ref.dim):
        assert np.array_equal(np.asarray(g.vs[d]).ravel(), ref.vs[d]) and float(np.asarray(g.dx).ravel()[d]) == ref.dx[d]
    return g


_PAIRS = {}


def pair(i):
    """(ref gOld, ref gNew, package gOld, package gNew, fp64 data) of PAIRS[i], made once."""
    if i not in _PAIRS:
        rO, rN = R.ref_pair(i)
        gO = pkg_grid(rO)
        _PAIRS[i] = (rO, rN, gO, gO if rN is rO else pkg_grid(rN), R.field(rO, i))
    return _PAIRS[i]


def same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=True), "%d of %d elements differ" % (
        int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), got.size)


# ------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("i", range(len(R.PAIRS)), ids=["x".join(map(str, p[0])) for p in R.PAIRS])
def test_fp64_equals_the_restatement_for_every_map_fold_and_fill(i):
    L = _L()
    rO, rN, gO, gN, data = pair(i)
    for name, (A, b) in R.maps_for(rO.dim, rO).items():
        members = R.members_ref(rO, data, rN, A, b)
        share = members[1].mean()
        assert i == len(R.PAIRS) - 1 or 0.1 <= share <= 0.9, (name, share)       # nodes on both sides (not the grid onto itself)
        for reduce in REDUCES:
            for fill in FILLS:
                want, counts = R.resample_ref(rO, data, rN, A, b, reduce, fill, members=members)
                got, info = L.transformData(gO, data, gN, A=A, b=b, reduce=reduce, fill=fill, return_info=True)
                assert isinstance(got, np.ndarray)
                same(got, want)
                assert np.array_equal(info["counts"], counts) and info["counts"].dtype == np.int64, (name, reduce, fill)
                from levelsetpy_amd import _mffi, resample
                assert resample.last_path() == info["kernel"] == _mffi.kernel_names("float64", rO.dim, REDUCES.index(reduce), fill == 'max')


@pytest.mark.parametrize("i", [1, 3])
def test_fp32_data_and_output_are_the_fp64_result_rounded_once(i):
    import torch
    L = _L()
    rO, rN, gO, gN, data = pair(i)
    d32 = data.astype(np.float32)
    A, b = R.maps_for(rO.dim, rO)['rotation']
    for reduce, fill in ((None, 'max'), ('min', 'nan'), ('max', 2.5)):
        want, counts = R.resample_ref(rO, d32, rN, A, b, reduce, fill, dtype=np.float32)
        got = L.transformData(gO, torch.as_tensor(d32, device="cuda"), gN, A=A, b=b, reduce=reduce, fill=fill)
        assert got.dtype == torch.float32 and got.is_cuda
        same(got, want)
        same(L.transformData(gO, d32, gN, A=A, b=b, reduce=reduce, fill=fill), want)                 # NumPy fp32 stays fp32
        wide, _ = R.resample_ref(rO, d32, rN, A, b, reduce, fill)
        same(L.transformData(gO, d32, gN, A=A, b=b, reduce=reduce, fill=fill, dtype='float64'), wide)
        narrow, _ = R.resample_ref(rO, data, rN, A, b, reduce, fill, dtype=np.float32)
        same(L.transformData(gO, data, gN, A=A, b=b, reduce=reduce, fill=fill, dtype='float32'), narrow)


# ------------------------------------------------------------------------------------------ batches
def poses(D, K, seed, gO):
    """K rotations in axes (0, 1) with shifts of up to a cell and a half."""
    rng = np.random.default_rng(seed)
    A = np.stack([R.rotation_map(D, t, 0, 1, 2 if D >= 3 else None)[0] for t in rng.uniform(-0.8, 0.8, K)])
    b = rng.uniform(-1.5, 1.5, (K, D)) * np.asarray(gO.dx).ravel()
    return A, b


def test_a_stack_of_three_maps_and_a_time_stack_of_three_fields():
    L = _L()
    rO, rN, gO, gN, _ = pair(1)
    data = R.field(rO, 11, stack=3)
    A, b = poses(3, 3, 1, rO)
    for fill in FILLS:
        want, counts = R.resample_ref(rO, data[0], rN, A, b, None, fill)
        got, info = L.transformData(gO, data[0], gN, A=A, b=b, fill=fill, return_info=True)
        assert want.shape == (3,) + rN.shape and np.array_equal(info["counts"], counts) and len(set(counts)) > 1
        same(got, want)
        want, counts = R.resample_ref(rO, data, rN, A[0], b[0], None, fill)                          # fields share one map
        got, info = L.transformData(gO, data, gN, A=A[0], b=b[0], fill=fill, return_info=True)
        assert want.shape == (3,) + rN.shape and np.array_equal(info["counts"], counts)
        same(got, want)
        for reduce in REDUCES:                                                                        # fields x K together
            want, counts = R.resample_ref(rO, data, rN, A, b, reduce, fill)
            got, info = L.transformData(gO, data, gN, A=A, b=b, reduce=reduce, fill=fill, return_info=True)
            assert want.shape == ((3, 3) if reduce is None else (3,)) + rN.shape and np.array_equal(info["counts"], counts)
            same(got, want)


@pytest.mark.parametrize("i", [0, 1])
def test_three_hundred_maps_folded(i):
    L = _L()
    rO, rN, gO, gN, data = pair(i)
    A, b = poses(rO.dim, 300, 2, rO)
    members = R.members_ref(rO, data, rN, A, b)
    assert (members[1].sum(axis=0) > 100).any() and not members[1].all(axis=0).all()
    for reduce in ('min', 'max'):
        want, counts = R.resample_ref(rO, data, rN, A, b, reduce, 'max', members=members)
        got, info = L.transformData(gO, data, gN, A=A, b=b, reduce=reduce, return_info=True)
        same(got, want)
        assert info["counts"] == counts and info["K"] == 300


def test_more_maps_than_one_launch_has_rows():
    """K = 65537 on a (3, 3) grid: gridDim.y ends at 65535, the last two members take a second launch.  The maps repeat with
    period 7 (the restatement is run on the 7 and on the last, which is its own), so a member that read another member's row
    shows."""
    L = _L()
    rO = R.RefGrid([-1.0, -1.0], [1.0, 1.0], [3, 3])
    gO = pkg_grid(rO)
    data = R.field(rO, 21)
    K = 65537
    uniq = np.array([[0.1 * j, -0.07 * j] for j in range(7)] + [[0.45, 0.3]])
    which = np.arange(K) % 7
    which[-1] = 7
    b = uniq[which]
    want_u, counts_u = R.resample_ref(rO, data, rO, None, uniq, None, 'max')
    got, info = L.transformData(gO, data, A=None, b=b, return_info=True)
    assert got.shape == (K, 3, 3)
    same(got, want_u[which])
    assert np.array_equal(info["counts"], counts_u[which])
    fold, count = R.resample_ref(rO, data, rO, None, uniq, 'min', 'nan')                              # min is idempotent: the fold of the 8
    got, info = L.transformData(gO, data, b=b, reduce='min', fill='nan', return_info=True)
    same(got, fold)
    assert info["counts"] == count
    from levelsetpy_amd import _mffi
    assert _mffi.plan((3, 3), 1, K).array_launches == 2


# ------------------------------------------------------------------------------------------ data and fill
def test_nan_and_inf_in_the_data():
    """A stored NaN is inside: it propagates through the fold, is counted as filled and is never the maximum; +-inf are values."""
    L = _L()
    rO, rN, gO, gN, data = pair(1)
    data = data.copy()
    data[3, 4, 2], data[7, 2, 5], data[10, 8, 1], data[5, 5, 5] = np.nan, np.inf, -np.inf, np.nan
    A, b = poses(3, 4, 3, rO)
    members = R.members_ref(rO, data, rN, A, b)
    assert np.isnan(members[0][:, 0, :][members[1]]).any()          # a stored NaN reaches nodes that are inside
    for reduce in REDUCES:
        for fill in FILLS:
            want, counts = R.resample_ref(rO, data, rN, A, b, reduce, fill, members=members)
            got, info = L.transformData(gO, data, gN, A=A, b=b, reduce=reduce, fill=fill, return_info=True)
            same(got, want)
            assert np.array_equal(info["counts"], counts)
    got = L.transformData(gO, data, gN, A=A, b=b, reduce='min', fill='max')
    assert np.isinf(got).any() or np.isnan(got).any()
    finite = data.copy()
    finite[7, 2, 5] = 0.0                                     # without +inf the maximum is finite although NaN nodes are inside
    want, _ = R.resample_ref(rO, finite, rN, fill='max')
    got = L.transformData(gO, finite, gN)
    same(got, want)
    outside = ~R.members_ref(rO, finite, rN)[1][0].reshape(rN.shape)
    assert np.isnan(got[~outside]).any() and np.isfinite(got[outside]).all() and len(set(got[outside])) == 1


def test_a_map_that_sends_every_node_outside():
    L = _L()
    rO, rN, gO, gN, data = pair(0)
    for reduce in REDUCES:
        got, info = L.transformData(gO, data, gN, b=np.array([100.0, 0.0]), reduce=reduce, fill='max', return_info=True)
        assert np.isnan(got).all() and info["counts"] == 0
        got, info = L.transformData(gO, data, gN, b=np.array([100.0, 0.0]), reduce=reduce, fill=-3.0, return_info=True)
        assert (got == -3.0).all() and info["counts"] == 0


# ------------------------------------------------------------------------------------------ views and memory
def test_views_a_host_view_and_a_low_mem_destination():
    import torch
    L = _L()
    from levelsetpy_amd.lazy import HostView
    rO, rN, gO, gN, data = pair(2)
    want, _ = R.resample_ref(rO, data, rN, fill='max')
    big = torch.zeros(data.size + 3, dtype=torch.float64, device="cuda")
    view = big[3:].view(data.shape)                          # 24 bytes off the allocation's alignment
    view.copy_(torch.as_tensor(data))
    got = L.migrateGrid(gO, view, gN)
    assert torch.is_tensor(got) and got.is_cuda
    same(got, want)
    got = L.migrateGrid(gO, HostView(torch.as_tensor(data, device="cuda")), gN)
    assert torch.is_tensor(got)
    same(got, want)
    low = pkg_grid(rN, low_mem=True)
    assert np.asarray(low.xs[0]).size < want.size           # no dense coordinates exist
    same(L.migrateGrid(gO, data, low), want)
    strided = torch.as_tensor(np.stack([data, data], axis=-1), device="cuda")[..., 0]               # not contiguous: copied, never read by stride
    same(L.migrateGrid(gO, strided, gN), want)


@pytest.mark.parametrize("i", [0, 2, 3])
def test_guarded_buffers(i):
    """hjm_resample on views of one guarded allocation, at element offsets 0 .. 3: no guard, no input changes, every output
    element is written, and the bits are those of the run on fresh arrays.  Both kernels run (FILL_MAX), unfolded and folded."""
    import torch
    import guarded_pool as GP
    from levelsetpy_amd import _hffi, _mffi
    from levelsetpy_amd._marshal import _descriptor
    rO, rN, gO, gN, data = pair(i)
    D, K = rO.dim, 3
    A, b = poses(D, K, 4, rO)
    table = np.concatenate([A.reshape(K, -1), b], axis=1)
    stack = R.field(rO, 31, stack=2)
    src, N = _descriptor(_hffi, gO, "float64")
    dst = _mffi.extents_descriptor(rN.shape)
    total = int(np.prod(rN.shape))
    pool = GP.GuardedPool(torch.float64, "cuda", 1 << 21)
    for reduce, arrays in ((_mffi.REDUCE_NONE, 2 * K), (_mffi.REDUCE_MIN, 2)):
        def op(alloc):
            d = alloc.inp("data", torch.as_tensor(stack, device="cuda"))
            m = alloc.inp("maps", torch.as_tensor(table, device="cuda"))
            cs = [alloc.inp("coord%d" % k, torch.as_tensor(rN.vs[k], device="cuda")) for k in range(D)]
            out = alloc.out("out", (arrays, total))
            counts = alloc.out("counts", (arrays,))           # int64 in an fp64 view: the bits are compared
            work = alloc.scratch("work", (int(_mffi.lib().hjm_workspace_size(arrays)) // 8,))
            alloc.arm()
            _mffi.check(_mffi.lib().hjm_resample(C.byref(src), C.byref(dst), C.byref(_mffi.coord_table([c.view.data_ptr() for c in cs])),
                                                 d.ptr, 2, data.size, m.ptr, K, reduce, _mffi.FILL_MAX, 0.0, out.ptr, 0, counts.ptr,
                                                 work.ptr, None))
            return {}
        ref, arrays_ref = GP.run_case(op, pool, what="resample %d-D reduce %d" % (D, reduce))
        want, counts = R.resample_ref(rO, stack, rN, A, b, {0: None, 1: 'min'}[reduce], 'max')
        same(arrays_ref["out"].reshape(want.shape), want)
        assert np.array_equal(arrays_ref["counts"].view(torch.int64).cpu().numpy().reshape(counts.shape), counts)


# ------------------------------------------------------------------------------------------ against the package itself
@pytest.mark.parametrize("i", [1, 2])
def test_migrate_shift_and_rotate_are_eval_u_at_the_same_coordinates(i):
    L = _L()
    rO, rN, gO, gN, data = pair(i)
    D = rO.dim
    dense = R.node_states(rN)
    same(L.migrateGrid(gO, data, gN, fill='nan'), L.eval_u(gO, data, dense).reshape(rN.shape))
    own = R.node_states(rO)
    shift = np.array([0.31, -0.17]) * rO.dx[:2]
    from levelsetpy_amd import resample
    A, b = resample.shiftMap(gO, shift, (0, 1))
    same(L.shiftData(gO, data, shift, (0, 1), fill='nan'), L.eval_u(gO, data, R.apply_map(own, A, b)).reshape(rO.shape))
    A, b = resample.rotateMap(gO, 0.4, (0, 1), 2)
    same(L.rotateData(gO, data, 0.4, (0, 1), 2, fill='nan'), L.eval_u(gO, data, R.apply_map(own, A, b)).reshape(rO.shape))


def test_the_fold_is_torch_minimum_over_the_stack_with_outside_members_masked():
    import torch
    L = _L()
    rO, rN, gO, gN, data = pair(1)
    t = torch.as_tensor(data, device="cuda")
    from levelsetpy_amd import resample
    thetas = np.array([0.3, -0.5, 1.1, 2.0])              # none is the identity: the box's corners leave it under every one
    stack = L.rotateData(gO, t, thetas, (0, 1), 2, fill='nan')
    assert stack.shape == (4,) + rO.shape
    inside = torch.as_tensor(np.stack([R.members_ref(rO, data, rO, *resample.rotateMap(gO, th, (0, 1), 2))[1][0] for th in thetas]),
                             device="cuda").reshape(stack.shape)
    masked = torch.where(inside, stack, torch.full_like(stack, float('inf')))
    want = masked[0]
    for k in range(1, 4):
        want = torch.minimum(want, masked[k])
    want = torch.where(inside.any(dim=0), want, torch.full_like(want, float('nan')))
    got = L.rotateData(gO, t, thetas, (0, 1), 2, fill='nan', reduce='min')
    assert torch.equal(torch.nan_to_num(got, nan=12345.0), torch.nan_to_num(want, nan=12345.0))
    assert 0.1 < float(inside.any(dim=0).double().mean()) < 1.0


# ------------------------------------------------------------------------------------------ end to end
def col(v, t=np.float64):
    return np.asarray(v, dtype=t).reshape(-1, 1)


def test_a_plane5d_solve_continues_from_migrated_data():
    """Coarse solve, migration onto a finer grid, continued solve: the same bits whether the migration ran on the device (tensor
    in, tensor out, no host pass) or in the restatement."""
    import torch
    L = _L()
    top = 2 * np.pi
    lo, hiC, hiF = [-1, -1, 0, -1, -1], [1, 1, top * (1 - 1.0 / 6), 1, 1], [1, 1, top * (1 - 1.0 / 8), 1, 1]
    gC = L.createGrid(col(lo), col(hiC), col([5, 5, 6, 5, 5], np.int64), [2], low_mem=True)
    gF = L.createGrid(col(lo), col(hiF), col([7, 6, 8, 6, 7], np.int64), [2], low_mem=True)
    rC = R.RefGrid(lo, hiC, [5, 5, 6, 5, 5], pd=(2,))
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in gC.vs], indexing='ij')
    data0 = np.sqrt(xs[0] ** 2 + xs[1] ** 2 + 0.3 * xs[3] ** 2) - 0.5
    args = L.Bundle(dict(quiet=True, keepLast=True))

    def solve(g, d, tau):
        sys5 = L.Plane5D(g, a_max=1.0, alpha_max=1.0)
        sd = L.Bundle(dict(grid=g, hamFunc=sys5.hamiltonian, partialFunc=sys5.dissipation, derivFunc=L.upwindFirstENO2))
        out = L.HJIPDE_solve(d, np.array(tau), sd, 'minVOverTime', args)[0]
        return out if torch.is_tensor(out) else torch.as_tensor(np.asarray(out), device="cuda")
    coarse = solve(gC, torch.as_tensor(data0, device="cuda"), [0.0, 0.05])
    fine = L.migrateGrid(gC, coarse, gF)
    assert torch.is_tensor(fine) and fine.is_cuda and fine.shape == (7, 6, 8, 6, 7)
    host, _ = R.resample_ref(rC, coarse.cpu().numpy(), gF, fill='max')
    same(fine, host)
    same(solve(gF, fine, [0.05, 0.1]), solve(gF, torch.as_tensor(host, device="cuda"), [0.05, 0.1]).cpu().numpy())


def test_a_3d_solve_with_a_placed_union_obstacle():
    import torch
    L = _L()
    n = 15
    g = L.createGrid(col([-2, -2, -np.pi]), col([2, 2, np.pi * (1 - 2.0 / n)]), col([n, n, n], np.int64), 2)
    rG = R.RefGrid([-2, -2, -np.pi], [2, 2, np.pi * (1 - 2.0 / n)], [n, n, n], pd=(2,))
    base = np.asarray(L.shapeCylinder(g, 2, np.array([[0.9, 0.0, 0.0]]).T, 0.35))
    thetas = np.array([0.0, 2.1, -2.1])
    from levelsetpy_amd import resample
    A, b = resample.rotateMap(g, thetas, (0, 1), 2)
    obstacle = L.transformData(g, torch.as_tensor(base, device="cuda"), A=A, b=b, reduce='min')
    host, _ = R.resample_ref(rG, base, rG, A, b, 'min', 'max')
    same(obstacle, host)
    assert (host < 0).sum() > (base < 0).sum()               # more than one placed copy
    data0 = torch.as_tensor(np.asarray(L.shapeCylinder(g, 2, np.zeros((3, 1)), 0.4)), device="cuda")
    car = L.DubinsVehicleRel(g, 1, 1)
    sd = L.Bundle(dict(grid=g, hamFunc=car.hamiltonian, partialFunc=car.dissipation, derivFunc=L.upwindFirstENO2))

    def solve(obs):
        out = L.HJIPDE_solve(data0, np.array([0.0, 0.2]), sd, 'minVOverTime', L.Bundle(dict(quiet=True, keepLast=True, obstacleFunction=obs)))[0]
        return np.asarray(out.cpu() if torch.is_tensor(out) else out)
    assert np.array_equal(solve(obstacle), solve(torch.as_tensor(host, device="cuda")))
