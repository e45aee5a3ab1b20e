"""GPU: the head paths of the node walk (levelsetpy_amd/csrc/hj_index_dev.h) in the kernels of libhj_hishapes.so, libhj_resample.so
and libhj_measure.so.  On every grid the other GPU tests run, the plan is one launch with every axis in the tail: the add-with-carry
over the head axes, the 64-bit node0 + head' * tail + t and the walk over several launches run only on grids past 2^31 nodes.  The
plan's two limits, lowered through the environment (include/hj_hishapes.h, a test facility), bring all three to grids of at most
50 400 nodes; tests/test_node_index_host.py has decoded every node of these plans on the host first.

Every test sets the limits, reads the published plan, asserts the form it means to run (tests/node_walk_cases.py) and then holds the
result, bit for bit, to the library's NumPy restatement AND to the same call with the limits unset.  A wrong head decode faults
nothing: it stores the right values of the wrong node, which only these comparisons show.  The guarded-buffer tests of the three
libraries run once more under the several-launches form.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _kffi, _mffi, _vffi, measure, resample, shapes as S  # noqa: E402
import hishapes_ref as H  # noqa: E402
import measure_ref as MR  # noqa: E402
import node_walk_cases as W  # noqa: E402
import query_ref as Q  # noqa: E402
import resample_ref as RR  # noqa: E402
import shapes_ref as SR  # noqa: E402
import test_gpu_hishapes as TH  # noqa: E402
import test_gpu_measure as TM  # noqa: E402
import test_gpu_resample as TR  # noqa: E402

ids = lambda N: "x".join(map(str, N))  # noqa: E731
CASES = [(N, form) for N in W.GRIDS for form in W.forms_of(N)]
CASE_IDS = ["%s-%s" % (ids(N), form) for N, form in CASES]
MEASURED = [(N, form) for N, form in CASES if N != W.ONE_NODE_AXES]           # an axis of the measure library has two nodes or more
MEASURED_IDS = ["%s-%s" % (ids(N), form) for N, form in MEASURED]


def planned(binding, N, form, *args):
    """The library's published plan of grid N under the limits now set: the form asserted, and printed for the profile."""
    p = W.check_form(binding.plan(N, *args), N, form)
    print("%s %s: first_tail %d tail %d head %d chunks %d heads_per_launch %d launches %d first heads %s" % (
        ids(N), form, p.first_tail, p.tail, p.head, p.chunks, p.heads_per_launch, p.launches, W.first_heads(p, N)[:4]))
    return p


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ------------------------------------------------------------------------------------------ shapes: hi_scene_kernel<float|double>
_SCENES = {}


def scene3(shape):
    """TH.scene at K = 3 -- every leaf kind and operator, an array leaf shared and one per member --, its program and its
    restatement, once per grid."""
    if shape not in _SCENES:
        g, node = TH.grid(shape), TH.scene(shape, K=3)
        comp = S.compile_program_hi(node, len(shape))
        assert comp.K == 3 and set(o[0] for o in comp.ops) == set(range(1, 11)) and [p for _, p in comp.arrays] == [False, True]
        want = H.run_program(g, comp)
        want.setflags(write=False)
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2]) and np.any(want < 0) and np.any(want > 0)
        _SCENES[shape] = (g, node, want)
    return _SCENES[shape]


@pytest.mark.parametrize("dtype", TH.DTYPES)
@pytest.mark.parametrize("shape,form", CASES, ids=CASE_IDS)
def test_shapes_three_members_every_leaf_flags_and_a_series_member(shape, form, dtype, monkeypatch):
    g, node, want64 = scene3(shape)
    want = want64.astype(TH.NP[dtype])
    W.set_limits(monkeypatch)
    unset = S.evaluate_shape(g, node, dtype)
    unset_flags = list(S.last_info()["flags"])
    W.set_limits(monkeypatch, shape, form)
    planned(_kffi, shape, form, 3)
    got = S.evaluate_shape(g, node, dtype)
    info = S.last_info()
    print("kernel", info["kernel"])
    assert info["kernel"] == _kffi.kernel_name(dtype) and info["K"] == 3 and tuple(got.shape) == (3,) + shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(bits(got), bits(unset))
    assert list(info["flags"]) == unset_flags == [SR.flags(w) for w in want]
    series = S.series(g, node, dtype)
    for k in (2, 0):                                              # one member on demand: the launch's k0 and the per-member leaf's base
        one = series[k]
        assert S.last_info()["K"] == 1 and S.last_info()["kernel"] == _kffi.kernel_name(dtype)
        assert torch.equal(bits(one), bits(unset[k])) and np.array_equal(one.cpu().numpy(), want[k])


# ------------------------------------------------------------------------------------------ resample: every ND, both kernels
# the source of every destination of that dimension: small, one periodic axis (two at 6-D)
SOURCES = {2: ((9, 8), (1,)), 3: ((7, 6, 5), (2,)), 4: ((5, 4, 6, 4), (2,)), 5: ((4, 3, 5, 3, 4), (2,)), 6: ((4, 3, 3, 4, 3, 3), (2, 5))}
_RESAMPLED = {}


def resample_case(N):
    """(package source grid, destination, fp64 data, runs) once per destination N.  The destination is coordinate vectors alone
    (an axis of one node has no spacing): from 0.9 half-widths below the source box's centre to 1.2 above it, so the upper end of
    every axis with more than one node falls outside and the lower end, of an axis of two nodes too, inside.  A run is (label, the data, the
    arguments of transformData, the restatement's array and counts)."""
    if N not in _RESAMPLED:
        D = len(N)
        src, pd = SOURCES[D]
        smin, smax = Q.grid_bounds(src, pd)
        rO = RR.RefGrid(smin, smax, src, pd)
        c, h = 0.5 * (smin + smax), 0.5 * (smax - smin)
        dst = H.PlainGrid([np.linspace(c[d] - 0.9 * h[d], c[d] + 1.2 * h[d], n) if n > 1 else np.array([c[d] + 0.013])
                           for d, n in enumerate(N)])
        assert 'periodic' in rO.bc
        data = RR.field(rO, 50 + D)
        d32 = data.astype(np.float32)
        M = W.nodes_of(N)
        runs = []
        for name, (A, b) in RR.maps_for(D, rO).items():           # the identity, a shift, a rotation
            want, counts = RR.resample_ref(rO, data, dst, A, b, None, 'nan')
            assert 0 < int(counts) < M, (N, name, counts)         # nodes on both sides
            runs.append((name, data, dict(A=A, b=b, fill='nan'), want, counts))
        A, b = RR.maps_for(D, rO)['rotation']
        want, counts = RR.resample_ref(rO, d32, dst, A, b, None, 'max', dtype=np.float32)
        runs.append(("fp32 rotation", d32, dict(A=A, b=b, fill='max'), want, counts))
        A3, b3 = TR.poses(D, 3, 1, rO)
        members = RR.members_ref(rO, data, dst, A3, b3)
        for reduce, fill in ((None, 'max'), (None, 2.5), ('min', 'max'), ('min', 'nan'), ('max', 2.5)):
            want, counts = RR.resample_ref(rO, data, dst, A3, b3, reduce, fill, members=members)
            # (the three poses of the 2-D fold, one axis periodic, bring every node inside between them)
            assert (0 < counts).all() and ((counts < M).all() if reduce is None or D > 2 else True), (N, reduce, counts)
            assert reduce is not None or len(set(counts)) > 1, (N, counts)
            runs.append(("K = 3 reduce %s fill %s" % (reduce, fill), data, dict(A=A3, b=b3, reduce=reduce, fill=fill), want, counts))
        _RESAMPLED[N] = (TR.pkg_grid(rO), dst, runs)
    return _RESAMPLED[N]


@pytest.mark.parametrize("N,form", CASES, ids=CASE_IDS)
def test_resample_maps_folds_fills_counts_and_fp32(N, form, monkeypatch):
    gO, dst, runs = resample_case(N)
    D = len(N)
    W.set_limits(monkeypatch)
    unset = [L.transformData(gO, data, dst, return_info=True, **kw) for _, data, kw, _, _ in runs]
    W.set_limits(monkeypatch, N, form)
    planned(_mffi, N, form)
    seen = set()
    for (label, data, kw, want, counts), (plain, plain_info) in zip(runs, unset):
        got, info = L.transformData(gO, data, dst, return_info=True, **kw)
        reduce = TR.REDUCES.index(kw.get('reduce'))
        assert resample.last_path() == info["kernel"] == _mffi.kernel_names(str(data.dtype), D, reduce, kw['fill'] == 'max'), label
        seen.update(info["kernel"].split(";"))
        TR.same(got, want)
        TR.same(got, plain)
        assert np.array_equal(info["counts"], counts) and np.array_equal(plain_info["counts"], counts), label
        assert np.array_equal(resample.last_info()["counts"], counts), label
    print("kernels", sorted(seen))
    assert {"resample_fill_kernel<%d, 0>" % D, "resample_fill_kernel<%d, 1>" % D, "resample_kernel<float, %d, 0>" % D} <= seen
    assert {"resample_kernel<double, %d, %d>" % (D, r) for r in (0, 1, 2)} <= seen


# ------------------------------------------------------------------------------------------ measure: every ND, both compare modes
_MEASURED = {}


def periodic_of(N):
    """A head axis of every form, or two: the first axis; at 5-D and on the small 6-D grid the second, which the carry reaches
    (and whose restatement, a Python loop over the simplices of every cut cell, has fewer cut cells to walk)."""
    return (0,) if len(N) < 5 else ((1,) if W.nodes_of(N) < 5000 else (0, 1))


def measure_fields(N, per):
    """(a, b): the noisy planes of measure_ref on a small grid.  On the 50 400 nodes of (6, 5, 7, 5, 6, 8) two balls in node
    units, each around one node that is the LAST of both periodic axes: the few cells that hold it are cut, all of them across a
    head index, most of them across a wrap."""
    if W.nodes_of(N) < 5000:
        return MR.field(N, per), MR.field_b(N, per)
    I = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in N], indexing="ij")
    ball = lambda c, r: np.sqrt(sum((I[d] - c[d]) ** 2 for d in range(len(N)))) - r     # noqa: E731
    return ball((5, 4, 3, 0, 0, 7), 0.8125), ball((5, 4, 3, 0, 1, 7), 0.9375)


def cut_cells(f, per):
    stack = np.stack([c.reshape(-1) for c in MR.corner_values(f, per)])
    return int(((stack > 0).any(axis=0) & (stack < 0).any(axis=0)).sum())


def measure_case(N):
    """(periodic axes, package grid, what is measured and the restatement's records) once per grid: the field a, the stack
    (a, a + 0.11, b), a against b at level 0 (so the records of A and B are the stack's), and a in fp32 at level 0.03."""
    if N not in _MEASURED:
        per = periodic_of(N)
        a, b = measure_fields(N, per)
        a32 = a.astype(np.float32)
        stack = np.stack([a, a + 0.11, b])
        want = dict(stack=[MR.measure_ref(s, 0.0, per) for s in stack], fp32=MR.measure_ref(a32, 0.03, per))
        want["one"] = one = want["stack"][0]
        with np.errstate(invalid="ignore"):
            want["compare"] = {"A": one, "B": want["stack"][2], "union": MR.record_of_f(np.minimum(a, b) - 0.0, per),
                               "intersection": MR.record_of_f(np.maximum(a, b) - 0.0, per)}
        # the conditions of the case: cut cells, some of them across a periodic head axis' wrap (without the wrap there are fewer),
        # the set not the whole grid
        small = W.nodes_of(N) < 5000
        assert 0 < cut_cells(a, ()) < cut_cells(a, per) == one["cut"] and 0 < one["inside"] < W.nodes_of(N) and one["invalid"] == 0
        assert (one["full"] > 0) == small and len(set(w["Q"] for w in want["stack"])) == 3
        assert want["compare"]["union"]["cut"] > 0 and want["compare"]["union"]["Q"] > max(one["Q"], want["stack"][2]["Q"])
        _MEASURED[N] = (per, TM.pkg_grid(N, per), a, b, a32, stack, want)
    return _MEASURED[N]


def measure_all(N):
    """Every record, volume and bound the front end gives for the case, under the limits now set -> a dict of plain values."""
    per, g, a, b, a32, stack, _ = measure_case(N)
    out, kernels = {}, set()

    def records(key, info, count=1):
        out[key] = [dict((k, r[k]) for k in TM.KEYS) for r in info[:count]]
        kernels.add(measure.last_path())
    out["vol"] = L.setVolume(g, a)
    records("one", measure.last_info())
    L.setVolume(g, torch.as_tensor(a32, device="cuda"), 0.03)
    records("fp32", measure.last_info())
    out["vols"] = list(L.setVolume(g, stack))
    records("stack", measure.last_info(), 3)
    for key, aa in (("compare", a), ("mixed", a32)):              # fp64 against fp64; fp32 against fp64
        c = L.setCompare(g, aa, b)
        out[key + " values"] = (c.volA, c.volB, c.union, c.intersection, c.symdiff, c.iou)
        for name in MR.SETS:
            records(key + " " + name, measure.last_info()[name])
    bounds = L.setBounds(g, a, pad=1)
    out["bounds"] = (list(bounds.lo), list(bounds.hi), bounds.xmin.ravel().tolist(), bounds.xmax.ravel().tolist())
    return out, kernels


@pytest.mark.parametrize("N,form", MEASURED, ids=MEASURED_IDS)
def test_measure_records_compare_fp32_a_stack_and_bounds_with_periodic_head_axes(N, form, monkeypatch):
    per, g, a, b, a32, stack, want = measure_case(N)
    D = len(N)
    W.set_limits(monkeypatch)
    unset, _ = measure_all(N)
    W.set_limits(monkeypatch, N, form)
    p = planned(_vffi, N, form, 1, per)
    assert all(d < p.first_tail for d in per)                     # the periodic axes are head axes
    got, kernels = measure_all(N)
    print("kernels", sorted(kernels))
    assert kernels == {_vffi.kernel_names("float64", None, D), _vffi.kernel_names("float32", None, D),
                       _vffi.kernel_names("float64", "float64", D), _vffi.kernel_names("float32", "float64", D)}
    TM.same_record(got["one"][0], want["one"], (N, "one"))
    TM.same_record(got["fp32"][0], want["fp32"], (N, "fp32"))
    for k in range(3):
        TM.same_record(got["stack"][k], want["stack"][k], (N, "stack", k))
        assert got["vols"][k] == MR.volume_of(want["stack"][k]["Q"], D, TM.cellvol(N, per))
    for name in MR.SETS:
        TM.same_record(got["compare " + name][0], want["compare"][name], (N, "compare", name))
    assert got["compare values"] == MR.compare_values(want["compare"], D, TM.cellvol(N, per))
    # fp32 against fp64: held to the call with the limits unset (below), and its set B is the fp64 one's
    TM.same_record(got["mixed B"][0], want["compare"]["B"], (N, "mixed", "B"))
    assert got["vol"] == MR.volume_of(want["one"]["Q"], D, TM.cellvol(N, per))
    vs, dx, _, _ = MR.grid_vectors(N, per)
    lo, hi, xmin, xmax = MR.bounds_ref(N, vs, dx, per, want["one"]["lo"], want["one"]["hi"], 1)
    assert got["bounds"] == (lo, hi, xmin.tolist(), xmax.tolist())
    assert got == unset                                           # every integer, volume and bound of the call with the limits unset


# ------------------------------------------------------------------------------------------ guarded buffers, several launches
def several_launches(monkeypatch, binding, N, heads_per_launch, *args):
    monkeypatch.setenv(W.ENV_TAIL, "1")
    monkeypatch.setenv(W.ENV_BLOCKS, str(heads_per_launch))
    p = binding.plan(N, *args)
    assert p.first_tail == len(N) - 1 and p.chunks == 1 and p.heads_per_launch == heads_per_launch
    assert p.launches >= 3 and p.head % p.heads_per_launch != 0
    assert any(sum(1 for v in h if v) >= 2 for h in W.first_heads(p, N))
    return p


def test_guarded_buffers_shapes_over_several_launches(monkeypatch):
    shape = (3, 4, 3, 3, 2, 4)
    several_launches(monkeypatch, _kffi, shape, 50, 2)            # 216 head indices: 50, 50, 50, 50, 16
    TH.test_guarded_buffers(shape)


def test_guarded_buffers_resample_over_several_launches(monkeypatch):
    i = 3
    several_launches(monkeypatch, _mffi, RR.PAIRS[i][1], 900)     # (5, 6, 5, 4, 7, 6): 4200 head indices in launches of 900
    TR.test_guarded_buffers(i)


def test_guarded_buffers_measure_over_several_launches(monkeypatch):
    i = 5
    N, per = MR.GRIDS[i]
    several_launches(monkeypatch, _vffi, N, 61, 2, per)           # (5, 3, 3, 2, 3, 3): 270 head indices in launches of 61
    TM.test_guarded_buffers(i)


# ------------------------------------------------------------------------------------------ a limit that is no limit
@pytest.mark.parametrize("env,bad", [(W.ENV_TAIL, "0"), (W.ENV_BLOCKS, "-1"), (W.ENV_TAIL, str(2 ** 31 + 1)), (W.ENV_BLOCKS, str(2 ** 31))])
def test_the_launching_entry_points_refuse_a_wrong_limit_by_name(env, bad, monkeypatch):
    N = (5, 3, 4, 3, 3)
    g, node, _ = scene3(N)
    gO, dst, runs = resample_case(N)
    per, gm, a = measure_case(N)[:3]
    W.set_limits(monkeypatch)
    monkeypatch.setenv(env, bad)
    for call in (lambda: S.evaluate_shape(g, node), lambda: L.transformData(gO, runs[0][1], dst), lambda: L.setVolume(gm, a)):
        with pytest.raises(Exception, match=env):
            call()
