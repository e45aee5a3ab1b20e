"""libhj_eikonal.so on the GPU against the NumPy restatement tests/eikonal_ref.py.

Tolerance.  The device relaxes tile by tile in an order no two runs need share, the restatement in synchronous passes.
Both reach the fixed point of the same monotone map; the comparison allows  16 eps (sum_d N_d) max finite |u|:  the map
is non-expansive, an update adds a bounded number of roundings, and a value depends on a chain of at most sum_d N_d
updates.  The measured difference is printed per case (0 is expected).  NaN and inf patterns must be equal exactly.
Measured on an MI355X: 0 on every case but the periodic (19, 14, 22) one, 1.1e-16 there (one ulp of one value).  The cause is
the order of updates: a node keeps min(old, candidate), and a candidate recomputed from neighbours that have since decreased
can round one ulp above the value kept from before.  The checks the issue asks to be exact (two runs, solo against batched
members, banded against unbanded inside the band) are asserted with array_equal and measured 0.

  * shapes with partial tiles, exactly one tile and many tiles in 1 to 4 dimensions; anisotropic dx; colliding fronts;
    level != 0; fp32; periodic first and last axes; walls, max_passes; band; speed; members; views; marshalling;
  * independent of the restatement's iteration: repeatability, one application of rule 2, signs, the frozen values;
  * use with shapes, extract_level_set and HJIPDE_solve; guarded buffers through the C ABI.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _effi, _marshal, _qffi, eikonal  # noqa: E402
import eikonal_ref as R  # noqa: E402
from guarded_pool import GuardedPool, run_case  # noqa: E402

EPS = np.finfo(np.float64).eps
_GRIDS, _REFS = {}, {}


def grid(shape, pd=(), box=None):
    """[-1, 1]^D (or box[d] = (lo, hi)); a periodic axis leaves out its last node."""
    key = (tuple(shape), tuple(pd), None if box is None else tuple(box))
    if key not in _GRIDS:
        nd = len(shape)
        lo = np.array([(box[d][0] if box else -1.0) for d in range(nd)], dtype=np.float64).reshape(-1, 1)
        hi = np.array([(box[d][1] if box else 1.0) for d in range(nd)], dtype=np.float64).reshape(-1, 1)
        for d in pd:
            hi[d] = lo[d] + (hi[d] - lo[d]) * (1.0 - 1.0 / shape[d])
        _GRIDS[key] = L.createGrid(lo, hi, np.array(shape, dtype=np.int64).reshape(-1, 1), list(pd) if pd else None)
    return _GRIDS[key]


def coords(g):
    return np.meshgrid(*[np.ravel(v) for v in g.vs], indexing='ij')


def dx_of(g):
    return [float(v) for v in np.asarray(g.dx).ravel()]


def periodic_of(g):
    return [f is L.addGhostPeriodic for f in g.bdry]


def shape_of(g):
    return tuple(int(v) for v in np.asarray(g.N).ravel())


def sphere(g, centre=0.0, radius=0.5, distort=True):
    X = coords(g)
    c = np.broadcast_to(np.asarray(centre, dtype=np.float64), (len(X),))
    r = np.sqrt(sum((x - ci) ** 2 for x, ci in zip(X, c)))
    return (r - radius) * (1.0 + 0.5 * X[0]) if distort else r - radius


def ref(key, g, data, **kw):
    """The restatement's result, computed once per case and never changed."""
    if key not in _REFS:
        out = R.signed_distance(data, dx_of(g), periodic_of(g), **kw)
        out.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def tolerance(shape, want):
    finite = np.abs(want[np.isfinite(want)]).astype(np.float64)
    return 16 * EPS * sum(shape) * (finite.max() if finite.size else 0.0)


def close(got, want, shape, what=""):
    """NaN and inf in equal places, finite values within the tolerance; prints the measured difference."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), what
    fin = np.isfinite(want)
    diff = float(np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)).max()) if fin.any() else 0.0
    print("%s: max |device - restatement| = %.3g (tolerance %.3g)" % (what, diff, tolerance(shape, want)))
    assert diff <= tolerance(shape, want), (what, diff)
    return diff


# ------------------------------------------------------------------------------------------ against the restatement
SHAPES = [(5, 4), (37,), (16, 32), (19, 14, 22), (33, 27, 29), (7, 6, 5, 6), (9, 8, 70), (300,), (40, 70)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distorted_sphere(shape):
    g = grid(shape)
    data = sphere(g, 0.1)
    out = L.signedDistance(g, data)
    assert isinstance(out, np.ndarray)
    close(out, ref(("sphere", shape), g, data), shape, "sphere %r" % (shape,))
    assert eikonal.last_path() == "eikonal_init_kernel<double>;eikonal_tile_kernel<%d>;eikonal_finish_kernel<double>" % len(shape)


def test_one_dimensional_grid_shape():
    g = grid((37,))
    data = sphere(g, 0.1)
    out = L.signedDistance(g, data.reshape(g.shape))                 # g.shape of a 1-D grid is (N, 1)
    assert out.shape == tuple(g.shape)
    close(out.reshape(-1), ref(("sphere", (37,)), g, data), (37,), "1-D column")


def test_anisotropic_dx():
    shape = (23, 31, 9)
    g = grid(shape, box=[(-1, 1), (-2, 2), (-0.5, 0.5)])
    assert len(set(dx_of(g))) == 3
    data = sphere(g, 0.1, 0.4)
    close(L.signedDistance(g, data), ref("aniso", g, data), shape, "anisotropic")


def test_two_discs_whose_fronts_collide():
    shape = (41, 37)
    g = grid(shape)
    data = np.minimum(sphere(g, (-0.45, 0.0), 0.2, False), sphere(g, (0.5, 0.1), 0.25, False))
    close(L.signedDistance(g, data), ref("collide", g, data), shape, "two discs")


def test_level():
    shape = (33, 27, 29)
    g = grid(shape)
    data = sphere(g, 0.1) + 0.2
    want = ref(("sphere", shape), g, sphere(g, 0.1))
    out = L.signedDistance(g, data, level=0.2)
    # data - level differs from the sphere by the rounding of +0.2 - 0.2: hold it to the restatement of the same subtraction
    close(out, ref("level", g, data, level=0.2), shape, "level 0.2")
    assert np.abs(out - want).max() < 1e-12


@pytest.mark.parametrize("pd,shape", [((0,), (30, 26)), ((2,), (19, 14, 22)), ((1,), (40, 70)), ((0,), (37,))], ids=str)
def test_periodic_axes(pd, shape):
    g = grid(shape, pd)
    centre = [0.0] * len(shape)
    centre[pd[0]] = -0.9
    data = sphere(g, centre, 0.15, False)
    want = ref(("periodic", pd, shape), g, data)
    close(L.signedDistance(g, data), want, shape, "periodic %r %r" % (pd, shape))
    plain = R.signed_distance(data, dx_of(g))
    assert np.abs(plain - want).max() > 0.5                          # the wrap matters in this case


def wall_case():
    shape = (47, 70)
    g = grid(shape)
    data = sphere(g, (-0.5, 0.0), 0.2, False)
    walled = data.copy()
    walled[23, :] = np.nan
    walled[23, 2:5] = data[23, 2:5]
    walled[35, 8:] = np.nan                                          # a second wall, open at the other end: a turn
    return shape, g, data, walled


def test_walls_with_a_gap():
    shape, g, data, walled = wall_case()
    want = ref("walls", g, walled)
    out, info = L.signedDistance(g, walled, max_passes=4 * 47 * 70 // 16, return_info=True)
    close(out, want, shape, "walls")
    assert np.isnan(out[23, 10]) and out[40, 60] > ref("walls-free", g, data)[40, 60] + 0.5
    print("walls: %d passes" % info.passes)
    assert info.passes > 1


def test_too_few_passes_raise():
    shape, g, data, walled = wall_case()
    with pytest.raises(ValueError) as caught:
        L.signedDistance(g, walled, max_passes=1)
    assert "max_passes = 1" in str(caught.value)
    close(L.signedDistance(g, walled), ref("walls", g, walled), shape, "walls after a refusal")


def test_band():
    shape = (160, 200)                                               # 10 x 7 tiles, of which the band's ring meets a few
    g = grid(shape)
    data = sphere(g, 0.0, 0.3)
    band = 5 * max(dx_of(g))
    full, info_full = L.signedDistance(g, data, return_info=True)
    out, info = L.signedDistance(g, data, band=band, return_info=True)
    close(out, ref("band", g, data, band=band), shape, "band")
    clamped = np.abs(full) > band
    assert clamped.any() and np.array_equal(out[clamped], np.sign(full[clamped]) * band)
    print("band: max |banded - unbanded| inside the band = %.3g" % np.abs(out[~clamped] - full[~clamped]).max())
    assert np.array_equal(out[~clamped], full[~clamped])             # unchanged from the unbanded solve: no accepted value
                                                                     # ever depended on a neighbour above the band
    mp = _effi.default_max_passes(shape)
    work = lambda i: i.active_tile_launch_fraction * _effi.launched_passes(i.passes, mp)        # noqa: E731
    print("band: active tile launches %.1f of a pass against %.1f" % (work(info), work(info_full)))
    assert 0 < work(info) < work(info_full)
    ntiles = _effi.tile_count(shape)
    assert work(info) * ntiles < ntiles                              # fewer launches did work, all passes together, than there are
                                                                     # tiles: some tile beyond the band never ran


def test_speed():
    shape = (33, 40)
    g = grid(shape)
    data = sphere(g, (-0.4, 0.0), 0.2)
    close(L.signedDistance(g, data, speed=2.5), ref("speed-scalar", g, data, speed=2.5), shape, "speed 2.5")
    X = coords(g)
    speed = 1.0 + 0.5 * np.sin(3 * X[0]) * np.cos(2 * X[1])
    speed[20, 5:30] = 0.0                                            # a zero-speed wall
    speed[5, 5] = np.nan
    want = ref("speed-array", g, data, speed=speed)
    out = L.signedDistance(g, data, speed=speed)
    close(out, want, shape, "speed array")
    assert np.isnan(out[20, 5:30]).all() and np.isnan(out[5, 5]) and np.isnan(out).sum() == 26
    close(L.signedDistance(g, torch.as_tensor(data, device="cuda"), speed=torch.as_tensor(speed, device="cuda")), want, shape, "speed tensor")


def test_fp32_in_and_out():
    shape = (33, 27, 29)
    g = grid(shape)
    data = sphere(g, 0.1).astype(np.float32)
    out = L.signedDistance(g, data)
    assert out.dtype == np.float32
    wide = data.astype(np.float64)
    want64 = ref("fp32-wide", g, wide)
    dev64 = L.signedDistance(g, wide)
    exact = dev64 == want64
    print("fp32: %d of %d fp64 values equal the restatement's" % (exact.sum(), exact.size))
    want32 = want64.astype(np.float32)
    assert np.array_equal(out[exact], want32[exact])
    assert (np.abs(out[~exact] - want32[~exact]) <= np.spacing(np.abs(want32[~exact]))).all()
    assert np.array_equal(L.signedDistance(g, wide, dtype='float32'), dev64.astype(np.float32))
    assert np.array_equal(L.signedDistance(g, data, dtype='float64'), dev64)
    assert eikonal.last_path().endswith("<double>") and L.signedDistance(g, data).dtype == np.float32 and eikonal.last_path().endswith("<float>")


def test_members_that_need_different_pass_counts():
    shape = (70, 40)
    g = grid(shape)
    X = coords(g)
    members = [X[0] + 0.93,                                          # a front that crosses five tiles of axis 0
               np.sin(9 * X[0]) * np.cos(7 * X[1]) + 0.05,          # interfaces in every tile
               2.0 + X[0]]                                           # a single sign
    solo, passes = [], []
    for m in members:
        out, info = L.signedDistance(g, m, return_info=True)
        solo.append(out)
        passes.append(info.passes)
    print("solo passes:", passes)
    assert passes[2] == 1 and passes[1] < passes[0]                  # the condition of this test
    both, info = L.signedDistance(g, np.stack(members), return_info=True)
    assert info.passes > passes[2]                                   # the call goes on for its slowest member (the exact count
                                                                     # depends on the order in which tiles of one pass run)
    for k in range(3):
        assert np.array_equal(both[k], solo[k]), k
        close(both[k], ref(("members", k), g, members[k]), shape, "member %d" % k)
    last = eikonal.last_info()
    assert list(last["flags"]) == [3, 3, 2] and len(last["messages"]) == 1 and "single sign on grid" in last["messages"][0] \
        and "member 2" in last["messages"][0]
    assert np.array_equal(both[2], np.full(shape, np.inf))
    assert np.array_equal(L.signedDistance(g, -members[2], band=0.25), np.full(shape, -0.25))


def test_more_members_than_one_launch_holds():
    shape, K = (3, 3), 65537
    g = grid(shape)
    rng = np.random.default_rng(5)
    patterns = rng.uniform(-1.0, 1.0, (16,) + shape)
    data = patterns[np.arange(K) % 16]
    out = L.signedDistance(g, torch.as_tensor(data, device="cuda")).cpu().numpy()
    for p in range(16):
        want = ref(("many", p), g, patterns[p])
        mine = out[p::16]
        assert np.array_equal(mine, np.broadcast_to(mine[0], mine.shape))
        close(mine[0], want, shape, "pattern %d" % p)
    assert np.array_equal(out[65536], out[0]) and np.array_equal(out[65535], out[15])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_view_at_an_odd_element_offset(dtype):
    shape = (19, 14, 22)
    g = grid(shape)
    td = torch.float64 if dtype == "float64" else torch.float32
    data = torch.as_tensor(sphere(g, 0.1), device="cuda").to(td)
    base = torch.zeros(data.numel() + 3, dtype=td, device="cuda")
    view = base[1:1 + data.numel()].view(shape)
    view.copy_(data)
    assert view.data_ptr() % 16 == base.element_size() and view.is_contiguous()
    out = L.signedDistance(g, view)
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == td
    assert torch.equal(out, L.signedDistance(g, data)) and torch.equal(view, data)


def test_host_view_in_gives_a_tensor_out():
    from levelsetpy_amd.lazy import HostView
    shape = (16, 32)
    g = grid(shape)
    data = sphere(g, 0.1)
    t = torch.as_tensor(data, device="cuda")
    out = L.signedDistance(g, HostView(t))
    assert torch.is_tensor(out) and out.is_cuda and torch.equal(out, L.signedDistance(g, t))
    grown = L.addCRadius(g, HostView(t), 0.1)
    assert torch.is_tensor(grown) and torch.equal(grown, out - 0.1)
    close(out, ref(("sphere", shape), g, data), shape, "HostView")


def test_kinds_of_result():
    shape = (16, 32)
    g = grid(shape)
    data = sphere(g, 0.1)
    want = ref(("sphere", shape), g, data)
    a = L.signedDistance(g, data)
    t = L.signedDistance(g, torch.as_tensor(data, device="cuda"))
    c = L.signedDistance(g, torch.as_tensor(data))
    assert isinstance(a, np.ndarray) and torch.is_tensor(t) and t.is_cuda and torch.is_tensor(c) and not c.is_cuda
    assert np.array_equal(a, t.cpu().numpy()) and np.array_equal(a, c.numpy())
    close(a, want, shape, "kinds")
    out, info = L.signedDistance(g, data, return_info=True)
    assert info.passes >= 1 and 0 < info.active_tile_launch_fraction <= 1 and info.path == eikonal.last_path()
    launched = _effi.launched_passes(info.passes, _effi.default_max_passes(shape))
    assert launched == 8 and info.passes < 8                          # one tile: the share counts all 8 passes launched, and the tile
    assert info.active_tile_launch_fraction * launched == round(info.active_tile_launch_fraction * launched) >= 1       # ran a whole number of times


# ------------------------------------------------------------------------------------------ independent of the restatement's iteration
INDEPENDENT = [((33, 27, 29), ()), ((40, 70), (1,)), ((7, 6, 5, 6), ())]


@pytest.mark.parametrize("shape,pd", INDEPENDENT, ids=str)
def test_properties_of_the_result(shape, pd):
    g = grid(shape, pd)
    data = sphere(g, 0.1, 0.45)
    dx, per = dx_of(g), periodic_of(g)
    one = L.signedDistance(g, data)
    two = L.signedDistance(g, data)
    assert np.array_equal(one, two)                                  # two runs, one result
    assert np.array_equal(np.sign(one), np.sign(data))               # the interface did not move
    u0, near, wall, s, phi = R.init(data, 0.0, dx, per)
    assert near.any() and np.array_equal(np.abs(one)[near], u0[near])            # rule 1, exactly
    u = np.abs(one)
    again = R.sweep(u, near, wall, dx, per, s)                       # one application of rule 2 moves nothing
    moved = np.abs(again - u).max()
    print("rule 2 applied once to the device's result moves a node by at most %.3g" % moved)
    assert moved <= tolerance(shape, one)


# ------------------------------------------------------------------------------------------ use
def test_add_c_radius_of_a_rectangle():
    shape = (41, 37)
    g = grid(shape)
    rect = L.shapeRectangleByCorners(g, [-0.4, -0.3], [0.5, 0.2], output='tensor')
    grown = L.addCRadius(g, rect, 0.15)
    assert torch.is_tensor(grown) and torch.equal(grown, L.signedDistance(g, rect) - 0.15)
    a = L.addCRadius(g, rect.cpu().numpy(), 0.15)
    assert isinstance(a, np.ndarray) and np.array_equal(a, grown.cpu().numpy())
    X = coords(g)
    far = (X[0] > 0.5 + 0.15) & (np.abs(X[1] + 0.05) < 0.2)          # straight out of a face: the grown set ends 0.15 further
    assert (a[far] > 0).all() and (a[(X[0] > 0.5) & (X[0] < 0.6) & (np.abs(X[1] + 0.05) < 0.2)] < 0).all()


def test_level_set_of_the_redistanced_union_keeps_its_topology():
    shape = (33, 27, 29)
    g = grid(shape)
    union = L.shapeUnion([sphere(g, (-0.3, 0.0, 0.0), 0.35, False), sphere(g, (0.35, 0.1, 0.0), 0.3, False)])
    assert not (union == 0).any()
    a = L.extract_level_set(g, union)
    b = L.extract_level_set(g, L.signedDistance(g, union))
    assert a.verts.shape == b.verts.shape and a.verts.shape[0] > 100 and np.array_equal(a.faces, b.faces)
    assert np.abs(a.verts - b.verts).max() < 0.5 * max(dx_of(g))


def test_a_solve_fed_the_redistanced_array_runs():
    n = 21
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
    squashed = 3.0 * L.shapeCylinder(g, 2, np.zeros((3, 1)), .5) ** 3        # the same set, far from a distance function
    data0 = L.signedDistance(g, squashed)
    assert np.array_equal(np.sign(data0), np.sign(squashed))
    s = L.DubinsVehicleRel(g, 1, 1)
    sd = L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstENO2))
    V, tau, _ = L.HJIPDE_solve(data0, np.linspace(0, 0.2, 3), sd, 'minVOverTime', L.Bundle(dict(quiet=True, keepLast=True)))
    V = _marshal.unlazy(V)
    V = V.detach().cpu().numpy() if torch.is_tensor(V) else np.asarray(V)
    assert np.isfinite(V).all() and (V <= data0 + 1e-12).all() and (V < data0 - 1e-3).any()


# ------------------------------------------------------------------------------------------ guarded buffers
_POOLS = {}
GUARDED = {(21, 37): (1,), (9, 8, 19): (), (5, 4, 5, 9): (0,)}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(torch.float64 if dtype == "float64" else torch.float32, "cuda", 200 * 1000)
    return _POOLS[dtype]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", sorted(GUARDED), ids=lambda s: "x".join(map(str, s)))
def test_guarded_buffers(shape, dtype):
    """Through the C ABI: data, speed, the output and the workspace are views of one arena with guards around each; at
    element offsets 0 .. 3 and with NaN / +-1e30 guards, the guards and the inputs stay intact, every output element is
    written, and the results are those of a run on fresh unguarded arrays.  K = 2 members.  The fp32 runs take their workspace
    from a plain allocation: an odd fp32 element offset is not the 8-byte alignment the workspace must have, and the fp64
    runs guard the same code."""
    g = grid(shape, GUARDED[shape])
    K = 2
    td = torch.float64 if dtype == "float64" else torch.float32
    data = np.stack([sphere(g, 0.1, 0.4), sphere(g, -0.2, 0.3, False)])
    data[1][tuple(n // 2 for n in shape)] = np.nan
    speed = np.ones(shape)
    speed[tuple(n // 3 for n in shape)] = 0.0
    bc, tz = [int(p) for p in periodic_of(g)], [0] * len(shape)
    desc = _qffi.grid_descriptor(len(shape), list(shape), [0.0] * len(shape), [0.0] * len(shape), dx_of(g), bc, tz, dtype)
    need = C.c_int64(0)
    lib = _effi.lib()
    _effi.check(lib.hje_workspace_size(desc, K, C.byref(need)))
    total = int(np.prod(shape))
    data_t = torch.as_tensor(data, device="cuda").to(td)
    speed_t = torch.as_tensor(speed, device="cuda")

    def op(alloc):
        d = alloc.inp("data", data_t.reshape(K, total))
        if dtype == "float64":
            sp = alloc.inp("speed", speed_t.reshape(-1)).ptr
            ws = alloc.scratch("ws", (need.value // 8,)).ptr
            keep = None
        else:
            keep = (speed_t, torch.empty(need.value // 8, dtype=torch.int64, device="cuda"))
            sp, ws = C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr())
        out = alloc.out("out", (K, total))
        passes = C.c_int64(0)
        alloc.arm()
        _effi.check(lib.hje_signed_distance(desc, d.ptr, K, total, 0.0, float("inf"), sp, 1.0, out.ptr, ws, need.value, 1000,
                                            C.byref(passes), None))
        torch.cuda.synchronize()
        assert passes.value >= 1
        return {"kernel": _effi.last_kernel()}

    refd, arrays = run_case(op, pool(dtype), what="signed_distance %s %s" % (shape, dtype))
    assert refd["kernel"].startswith("eikonal_init_kernel<%s>;eikonal_tile_kernel<%d>" % ("double" if dtype == "float64" else "float", len(shape)))
    got = arrays["out"].cpu().numpy().reshape((K,) + shape)
    src = data_t.cpu().numpy()
    for k in range(K):
        want = R.signed_distance(src[k], dx_of(g), periodic_of(g), speed=speed)
        if dtype == "float64":
            close(got[k], want, shape, "guarded member %d" % k)
        else:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want))
            assert (np.abs(got[k] - want)[~np.isnan(want)] <= np.spacing(np.abs(want[~np.isnan(want)]))).all()
