"""Level-set extraction on the device (levelsetpy_amd/surface.py, libhj_surface.so) against tests/surface_ref.py: verts BIT FOR
BIT, faces equal in order, each up to a cyclic rotation; fp64 and fp32 data; guarded-buffer runs; bad arguments; a census of
the library's kernels; the Python front end, implicit_mesh and the example.

UNPINNED: the reference's implicit_mesh is skimage's Lewiner marching cubes, which cannot be run here; the kernels are held
to the NumPy restatement, which tests/test_surface_ref.py proves on closed-form surfaces.

Grids are the smallest on which the kernels can go wrong: one cell (2x2x2, 2x2), flat and non-cubic ones (2x5x3, 64x3, 7x9),
9x11x13 (two scan tiles of 1024 nodes), and 33x21x70 / 130x67, whose node counts are ragged against the tile and the
workgroup and span 48 / 9 tiles.

Kernel -> test that launches it (each test asserts the names through hjs_last_kernel; test_census_of_the_surface_library checks
the table against `nm -D libhj_surface.so`):
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
from levelsetpy_amd import extract_level_set, level_set_measure, implicit_mesh  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _sffi  # noqa: E402
from levelsetpy_amd.lazy import HostView  # noqa: E402

import surface_ref as S  # noqa: E402
from guarded_pool import GuardedPool, PlainAlloc, BoundsError, same_bits, OFFSETS, FILLS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = {"float64": torch.float64, "float32": torch.float32}
ND = {"float64": np.float64, "float32": np.float32}
CT = {"float64": "double", "float32": "float"}
GRIDS3 = [(2, 2, 2), (2, 5, 3), (9, 11, 13), (33, 21, 70)]
GRIDS2 = [(2, 2), (7, 9), (64, 3), (130, 67)]

# kernel (as hjs_last_kernel names it) -> the test that launches it and asserts that name
CENSUS = {
    "classify_kernel<double, 2>": "test_grids_and_fields_bitwise",
    "classify_kernel<double, 3>": "test_grids_and_fields_bitwise",
    "classify_kernel<float, 2>": "test_grids_and_fields_bitwise",
    "classify_kernel<float, 3>": "test_grids_and_fields_bitwise",
    "scan_blocks_kernel": "test_grids_and_fields_bitwise",
    "emit_kernel<double, 2>": "test_grids_and_fields_bitwise",
    "emit_kernel<double, 3>": "test_grids_and_fields_bitwise",
    "emit_kernel<float, 2>": "test_grids_and_fields_bitwise",
    "emit_kernel<float, 3>": "test_grids_and_fields_bitwise",
}
__doc__ += "\n".join("  %-32s %s" % kv for kv in sorted(CENSUS.items())) + "\n"


def launched(kernels, test):
    """The calling thread's last call launched exactly `kernels`, in order, and the census credits them to `test`."""
    assert _sffi.last_kernels() == list(kernels), (_sffi.last_kernels(), kernels)
    for k in kernels:
        assert CENSUS[k] == test


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda").reshape(-1)          # (a copy: the shared cases are read-only)


def descriptor(N, xmin, dx, dtype):
    D = len(N)
    return _sffi.grid_descriptor(D, N, xmin, [x + (n - 1) * h for x, n, h in zip(xmin, N, dx)], dx, [0] * D, [0] * D, dtype)


def abi_extract(N, xmin, dx, flat, F, stride, level, dtype, test=None):
    """hjs_workspace_size / hjs_count / hjs_emit on `flat` (1-D device tensor holding F fields at `stride`): a list of
    (verts, faces) NumPy pairs.  With `test`, the launches are asserted through hjs_last_kernel."""
    lib = _sffi.lib()
    D = len(N)
    desc = descriptor(N, xmin, dx, dtype)
    need = C.c_size_t(0)
    _sffi.check(lib.hjs_workspace_size(C.byref(desc), F, C.byref(need)))
    nodes = int(np.prod(N))
    assert 6 * nodes * F <= need.value <= (6 * nodes + 16 * (nodes // 1024 + 2)) * F          # "5-9 bytes per node"
    work = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
    counts = torch.full((F, 2), -1, dtype=torch.int64, device="cuda")
    _sffi.check(lib.hjs_count(C.byref(desc), _p(flat), F, stride, float(level), _p(work), need.value, _p(counts), _stream()))
    if test:
        launched(["classify_kernel<%s, %d>" % (CT[dtype], D), "scan_blocks_kernel"], test)
    host = counts.cpu().numpy()
    nv, nf = host[:, 0], host[:, 1]
    verts = torch.full((int(nv.sum()), D), float("nan"), dtype=torch.float64, device="cuda")
    faces = torch.full((int(nf.sum()), D), -1, dtype=torch.int32, device="cuda")
    hc = (C.c_int64 * (2 * F))(*[int(v) for v in host.ravel()])
    _sffi.check(lib.hjs_emit(C.byref(desc), _p(flat), F, stride, float(level), _p(work), need.value, hc,
                             _p(verts) if verts.numel() else None, _p(faces) if faces.numel() else None, _stream()))
    if test:
        launched(["emit_kernel<%s, %d>" % (CT[dtype], D)] if int(host.sum()) else [], test)
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    v0, f0 = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])
    return [(verts[v0[f]:v0[f + 1]], faces[f0[f]:f0[f + 1]]) for f in range(F)]


def assert_same_mesh(got, ref, what):
    (gv, gf), (rv, rf) = got, ref
    assert gv.shape == rv.shape and gf.shape == rf.shape, (what, gv.shape, rv.shape, gf.shape, rf.shape)
    assert gv.dtype == np.float64 and gf.dtype == np.int32
    assert np.array_equal(gv.view(np.int64), rv.view(np.int64)), (what, "verts", int((gv != rv).any(axis=1).sum()))
    assert np.array_equal(S.canonical(gf), S.canonical(rf)), (what, "faces", int((S.canonical(gf) != S.canonical(rf)).any(axis=1).sum()))


# ------------------------------------------------------------------------------------------ the fields, computed once
def grid_of(N):
    """A non-cubic, off-origin geometry for the node counts N."""
    D = len(N)
    return [-0.7, 0.4, -1.1][:D], [0.13, 0.21, 0.17][:D]


def generic_fields(N):
    """name -> (phi fp64, level) on grid_of(N): every cell active, a shifted level, non-finite nodes, empty results, a plane
    lying exactly on a node plane."""
    rng = np.random.default_rng(sum(N) * 7 + len(N))
    xmin, dx = grid_of(N)
    noise = rng.standard_normal(N)
    bad = noise.copy()
    flat = bad.reshape(-1)
    k = max(1, flat.size // 25)
    flat[rng.integers(0, flat.size, k)] = np.nan
    flat[rng.integers(0, flat.size, k)] = np.inf
    flat[rng.integers(0, flat.size, k)] = -np.inf
    X = S.mesh_grid(N, xmin, dx)
    k0 = (N[0] - 1) // 2
    plane = X[0] - X[0][(k0,) + (0,) * (len(N) - 1)]
    assert (plane[k0] == 0).all()
    smooth = np.sqrt(sum((x - x.mean()) ** 2 for x in X)) - 0.3 * (N[-1] - 1) * dx[-1]
    return {"noise": (noise, 0.0), "noise_level": (noise, 0.37), "nonfinite": (bad, 0.0), "all_inside": (np.full(N, -1.0), 0.0),
            "all_outside": (np.full(N, 1.0), 0.0), "plane_on_nodes": (plane, 0.0), "smooth_level": (smooth, -0.05)}


_REFS = {}


def reference(key, N, xmin, dx, phi, level, dtype):
    """level_set_ref of the data as the device sees it (rounded to fp32 first for fp32): computed once, never modified."""
    k = (key, dtype)
    if k not in _REFS:
        data = np.ascontiguousarray(phi.astype(ND[dtype]))
        data.setflags(write=False)
        _REFS[k] = (data, S.level_set_ref(N, xmin, dx, data, level))
    return _REFS[k]


# ------------------------------------------------------------------------------------------ 1. the kernels, through the C ABI
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", GRIDS3 + GRIDS2, ids=lambda N: "x".join(map(str, N)))
def test_grids_and_fields_bitwise(N, dtype):
    xmin, dx = grid_of(N)
    nonempty = 0
    for name, (phi, level) in generic_fields(N).items():
        data, ref = reference((N, name), N, xmin, dx, phi, level, dtype)
        got = abi_extract(N, xmin, dx, dev(data), 1, data.size, level, dtype,
                          test="test_grids_and_fields_bitwise")
        assert_same_mesh(got[0], ref, (N, name, dtype))
        if name in ("all_inside", "all_outside"):
            assert got[0][0].shape == (0, len(N)) and got[0][1].shape == (0, len(N))
        nonempty += len(ref[1]) > 0
    assert nonempty >= 3
    # white noise: every cell is crossed
    cells = int(np.prod([n - 1 for n in N]))
    assert len(_REFS[((N, "noise"), dtype)][1][1]) >= cells


CLOSED_FORM = {"sphere9": lambda: S.sphere(9), "sphere17": lambda: S.sphere(17), "torus": S.torus, "sphere_on_nodes": S.sphere_on_nodes,
               "anisotropic": S.anisotropic, "cut_sphere": S.cut_sphere, "ellipse": S.ellipse}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", sorted(CLOSED_FORM))
def test_closed_form_cases_bitwise(name, dtype):
    """Cases a-f of tests/test_surface_ref.py on the device; in fp64 the properties proved there hold for the device's mesh
    because it is the same mesh."""
    case = CLOSED_FORM[name]()
    N, xmin, dx, level = case["N"], case["xmin"], case["dx"], case["level"]
    data, ref = reference(name, N, xmin, dx, case["phi"], level, dtype)
    got = abi_extract(N, xmin, dx, dev(data), 1, data.size, level, dtype)
    assert_same_mesh(got[0], ref, (name, dtype))
    assert len(ref[1]) > 0
    if name in ("sphere9", "sphere17", "anisotropic", "sphere_on_nodes", "torus"):
        _, ucount, dmax = S.edge_census(got[0][1])
        assert np.all(ucount == 2) and dmax == 1
        assert S.euler_characteristic(len(got[0][0]), got[0][1]) == (0 if name == "torus" else 2)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", [(9, 11, 13), (130, 67)], ids=lambda N: "x".join(map(str, N)))
def test_two_fields_with_a_stride_larger_than_the_grid(N, dtype):
    xmin, dx = grid_of(N)
    fields = generic_fields(N)
    nodes = int(np.prod(N))
    stride = nodes + 37
    flat = torch.full((2 * stride,), float("nan"), dtype=TD[dtype], device="cuda")
    refs = []
    for f, name in enumerate(("smooth_level", "noise")):
        phi, _ = fields[name]
        data = phi.astype(ND[dtype])
        flat[f * stride:f * stride + nodes] = dev(data)
        refs.append(S.level_set_ref(N, xmin, dx, data, 0.21))
    got = abi_extract(N, xmin, dx, flat, 2, stride, 0.21, dtype)
    for f in range(2):
        assert_same_mesh(got[f], refs[f], (N, f, dtype))
    assert len(refs[0][1]) != len(refs[1][1]) and len(refs[0][1]) > 0
    # one empty field between two others: its slot is skipped, the others land where they belong
    flat3 = torch.cat([flat[:stride], torch.full((stride,), 5.0, dtype=TD[dtype], device="cuda"), flat[stride:]])
    got = abi_extract(N, xmin, dx, flat3, 3, stride, 0.21, dtype)
    assert got[1][0].shape[0] == 0 and got[1][1].shape[0] == 0
    assert_same_mesh(got[0], refs[0], "first of three")
    assert_same_mesh(got[2], refs[1], "third of three")


def test_entry_points_refuse_bad_arguments():
    lib = _sffi.lib()
    N, (xmin, dx) = (9, 11, 13), grid_of((9, 11, 13))
    nodes = int(np.prod(N))
    d_t = torch.zeros(2 * nodes, dtype=torch.float64, device="cuda")
    need = C.c_size_t(0)
    desc = descriptor(N, xmin, dx, "float64")
    assert lib.hjs_workspace_size(C.byref(desc), 2, C.byref(need)) == 0
    work = torch.empty(need.value // 8 + 2, dtype=torch.int64, device="cuda")
    counts = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    hc = (C.c_int64 * 4)(0, 0, 0, 0)

    def count(desc, data=d_t, F=1, stride=nodes, w=_p(work), wb=None, c=counts):
        return lib.hjs_count(C.byref(desc), _p(data) if data is not None else None, F, stride, 0.0, w, need.value if wb is None else wb,
                             _p(c) if c is not None else None, _stream())

    assert count(desc) == 0
    assert count(desc, data=None) == _ffi_code("EINVAL") and b"null" in lib.hjs_last_error()
    assert count(desc, c=None) == _ffi_code("EINVAL")
    assert count(desc, w=None) == _ffi_code("EINVAL")
    assert count(desc, F=2, stride=nodes - 1) == _ffi_code("EINVAL") and b"field_stride" in lib.hjs_last_error()
    assert count(desc, F=0) == _ffi_code("EINVAL")
    assert count(desc, F=2, wb=need.value - 1) == _ffi_code("EINVAL") and b"workspace" in lib.hjs_last_error()
    assert count(desc, w=C.c_void_p(work.data_ptr() + 4)) == _ffi_code("EINVAL")              # not 8-byte aligned
    for nd, NN in ((1, (50,)), (4, (5, 6, 4, 7))):
        bad = descriptor(NN, [0.0] * nd, [1.0] * nd, "float64")
        assert count(bad) == _ffi_code("EUNSUPPORTED"), nd
        assert lib.hjs_workspace_size(C.byref(bad), 1, C.byref(need)) == _ffi_code("EUNSUPPORTED")
        assert lib.hjs_emit(C.byref(bad), _p(d_t), 1, nodes, 0.0, _p(work), need.value, hc, None, None, _stream()) == _ffi_code("EUNSUPPORTED")
    for nd in (0, 5):
        bad = descriptor(N, xmin, dx, "float64")
        bad.ndim = nd
        assert count(bad) == _ffi_code("EINVAL")
    for NN in ((1, 11, 13), (9, 11, 1), (9, 0, 13)):
        assert count(descriptor(NN, xmin, dx, "float64")) == _ffi_code("EINVAL"), NN
    assert count(descriptor((9, 1), xmin[:2], dx[:2], "float64")) == _ffi_code("EINVAL")
    bad = descriptor(N, xmin, dx, "float64")
    bad.dtype = 7
    assert count(bad) == _ffi_code("EINVAL")
    # emit: counts beyond int32 indices are refused before anything is launched; missing outputs too
    big = (C.c_int64 * 2)(2 ** 31, 0)
    assert lib.hjs_emit(C.byref(desc), _p(d_t), 1, nodes, 0.0, _p(work), need.value, big, _p(work), _p(work), _stream()) == _ffi_code("EUNSUPPORTED")
    big = (C.c_int64 * 2)(5, 2 ** 31)
    assert lib.hjs_emit(C.byref(desc), _p(d_t), 1, nodes, 0.0, _p(work), need.value, big, _p(work), _p(work), _stream()) == _ffi_code("EUNSUPPORTED")
    some = (C.c_int64 * 2)(3, 1)
    assert lib.hjs_emit(C.byref(desc), _p(d_t), 1, nodes, 0.0, _p(work), need.value, some, None, None, _stream()) == _ffi_code("EINVAL")
    assert lib.hjs_emit(C.byref(desc), _p(d_t), 1, nodes, 0.0, _p(work), need.value, None, None, None, _stream()) == _ffi_code("EINVAL")
    # empty results: no launch, null outputs accepted
    assert lib.hjs_emit(C.byref(desc), _p(d_t), 1, nodes, 0.0, _p(work), need.value, hc, None, None, _stream()) == 0
    assert _sffi.last_kernels() == []
    torch.cuda.synchronize()
    # the Python front end
    g4 = L.createGrid(np.zeros((4, 1)), np.ones((4, 1)), 5 * np.ones((4, 1), dtype=np.int64), None)
    with pytest.raises(Exception, match="proj"):
        extract_level_set(g4, np.zeros((5,) * 4))
    g3 = L.createGrid(-np.ones((3, 1)), np.ones((3, 1)), np.array([[9], [11], [13]]), None)
    with pytest.raises(Exception):
        extract_level_set(g3, np.zeros((9, 11, 12)))


def _ffi_code(name):
    return {"EINVAL": -1, "EHIP": -2, "EUNSUPPORTED": -3}[name]


# ------------------------------------------------------------------------------------------ 2. bounds
_POOLS = {}


def pools():
    if not _POOLS:
        for k in TD:
            _POOLS[k] = GuardedPool(TD[k], "cuda", 300 * 1000)
    return _POOLS["float64"], _POOLS["float32"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", [(9, 11, 13), (130, 67)], ids=lambda N: "x".join(map(str, N)))
def test_kernels_stay_inside_their_arrays(N, dtype):
    """count + emit of a two-field stack on views carved from tests/guarded_pool.py's pools, at element offsets 0-3 and with
    guards of NaN and +-1e30.  verts, the counts and the workspace (8-byte quantities) come from the fp64 pool, faces from the
    fp32 pool (int32 behind a float32 view), the data from the pool of its dtype.  Guards intact, inputs unchanged, every
    element of verts / faces / counts written, the same bits as on fresh arrays -- and as the restatement."""
    lib = _sffi.lib()
    D = len(N)
    xmin, dx = grid_of(N)
    fields = generic_fields(N)
    nodes = int(np.prod(N))
    stride = nodes + 5
    level = 0.0
    stack = torch.zeros(2 * stride, dtype=TD[dtype], device="cuda")
    refs = []
    for f, name in enumerate(("nonfinite", "smooth_level")):
        data = fields[name][0].astype(ND[dtype])
        stack[f * stride:f * stride + nodes] = dev(data)
        refs.append(S.level_set_ref(N, xmin, dx, data, level))
    nv = [len(r[0]) for r in refs]
    nf = [len(r[1]) for r in refs]
    assert min(nv) > 0 and min(nf) > 0
    desc = descriptor(N, xmin, dx, dtype)
    need = C.c_size_t(0)
    _sffi.check(lib.hjs_workspace_size(C.byref(desc), 2, C.byref(need)))

    def op(a64, a32):
        data = (a64 if dtype == "float64" else a32).inp("data", stack)
        work = a64.scratch("workspace", ((need.value + 7) // 8,))
        counts = a64.out("counts", (2, 2))
        verts = a64.out("verts", (sum(nv), D))
        faces = a32.out("faces", (sum(nf), D))
        a64.arm()
        a32.arm()
        _sffi.check(lib.hjs_count(C.byref(desc), data.ptr, 2, stride, level, work.ptr, need.value, counts.ptr, _stream()))
        host = counts.view.view(torch.int64).cpu().numpy()
        assert host[:, 0].tolist() == nv and host[:, 1].tolist() == nf, (host, nv, nf)
        hc = (C.c_int64 * 4)(*[int(v) for v in host.ravel()])
        _sffi.check(lib.hjs_emit(C.byref(desc), data.ptr, 2, stride, level, work.ptr, need.value, hc, verts.ptr, faces.ptr, _stream()))
        return {"kernels": tuple(_sffi.last_kernels())}

    p64, p32 = pools()
    plain64, plain32 = PlainAlloc(torch.float64, "cuda"), PlainAlloc(torch.float32, "cuda")
    ref = op(plain64, plain32)
    torch.cuda.synchronize()
    assert ref["kernels"] == ("emit_kernel<%s, %d>" % (CT[dtype], D),) * 2          # one launch per field
    ref64, ref32 = plain64.results(), plain32.results()
    # the reference run is the restatement's mesh
    rv = ref64["verts"].cpu().numpy().reshape(-1, D)
    rf = ref32["faces"].view(torch.int32).cpu().numpy().reshape(-1, D)
    assert_same_mesh((rv[:nv[0]], rf[:nf[0]]), refs[0], "field 0")
    assert_same_mesh((rv[nv[0]:], rf[nf[0]:]), refs[1], "field 1")
    for k in OFFSETS:
        for fname, fill in FILLS.items():
            tag = "%s %s offset %d fill %s" % (N, dtype, k, fname)
            p64.begin(fill, k)
            p32.begin(fill, k)
            try:
                got = op(p64, p32)
                p64.check()
                p32.check()
                same_bits(got, ref, tag)
                same_bits(p64.results(), ref64, tag)
                same_bits(p32.results(), ref32, tag)
            except BoundsError as e:
                raise BoundsError(e.kind, "%s: %s" % (tag, str(e)))


# ------------------------------------------------------------------------------------------ 3. census
def test_census_of_the_surface_library():
    """Every __device_stub__ of `nm -D libhj_surface.so` is in CENSUS, and every entry names a test of this file that asserts
    the launch through hjs_last_kernel (the `launched(kernels, test)` calls)."""
    out = subprocess.check_output(["nm", "-D", "-C", _sffi.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", out))
    assert stubs, "no kernels found in %s" % _sffi.LIB_PATH
    assert stubs == set(CENSUS), (sorted(stubs - set(CENSUS)), sorted(set(CENSUS) - stubs))
    src = open(os.path.abspath(__file__)).read()
    for kernel, test in CENSUS.items():
        fn = globals().get(test)
        assert callable(fn), test
        body = src[src.index("def %s(" % test):]
        body = body[:body.index("\n\n\n")]
        assert 'abi_extract(' in body and 'test="%s"' % test in body, test


# ------------------------------------------------------------------------------------------ 4. the Python front end
def _grid3():
    return L.createGrid(-np.ones((3, 1)), np.ones((3, 1)), np.array([[9], [11], [13]]), None)


def test_numpy_tensor_hostview_in_and_out_and_the_tau_stack():
    g = _grid3()
    case = S.anisotropic()
    phi = np.array(case["phi"])
    xmin = [float(np.asarray(v).ravel()[0]) for v in g.vs]
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    rv, rf = S.level_set_ref(case["N"], xmin, dx, phi, 0.1)
    out = extract_level_set(g, phi, 0.1)
    assert isinstance(out.verts, np.ndarray) and isinstance(out.faces, np.ndarray)
    assert_same_mesh((out.verts, out.faces), (rv, rf), "numpy")
    t = torch.as_tensor(phi, device="cuda")
    for arg in (t, HostView(t)):
        out = extract_level_set(g, arg, 0.1)
        assert torch.is_tensor(out.verts) and out.verts.is_cuda and out.verts.dtype == torch.float64
        assert torch.is_tensor(out.faces) and out.faces.is_cuda and out.faces.dtype == torch.int32
        assert_same_mesh((out.verts.cpu().numpy(), out.faces.cpu().numpy()), (rv, rf), type(arg).__name__)
    # level defaults to 0; fp32 data is meshed as fp32
    r0 = S.level_set_ref(case["N"], xmin, dx, phi, 0.0)
    out = extract_level_set(g, phi)
    assert_same_mesh((out.verts, out.faces), r0, "default level")
    r32 = S.level_set_ref(case["N"], xmin, dx, phi.astype(np.float32), 0.1)
    out = extract_level_set(g, t.float(), 0.1)
    assert_same_mesh((out.verts.cpu().numpy(), out.faces.cpu().numpy()), r32, "fp32")
    # a stack with a leading time axis: a list, each entry the array's own mesh (one of them empty)
    stack = np.stack([phi, phi + 0.15, np.full_like(phi, 3.0), 0.5 * phi])
    outs = extract_level_set(g, torch.as_tensor(stack, device="cuda"), 0.1)
    assert isinstance(outs, list) and len(outs) == 4
    for a, o in zip(stack, outs):
        assert_same_mesh((o.verts.cpu().numpy(), o.faces.cpu().numpy()), S.level_set_ref(case["N"], xmin, dx, a, 0.1), "stack")
    assert outs[2].verts.shape == (0, 3) and outs[2].faces.shape == (0, 3)
    outs = extract_level_set(g, stack, 0.1)
    assert isinstance(outs, list) and isinstance(outs[1].verts, np.ndarray) and np.array_equal(outs[0].verts, rv)
    # length / area and enclosed area / volume, torch and NumPy alike, against the restatement's own formulas
    area, vol = level_set_measure(out.verts, out.faces)
    assert (area, vol) == pytest.approx(S.measure(*r32), rel=1e-12)
    assert level_set_measure(rv, rf) == pytest.approx(S.measure(rv, rf), rel=1e-12)
    assert abs(level_set_measure(rv, rf)[1] - 4 / 3 * np.pi * 0.6 ** 3) < 0.1 * 0.9
    # 2-D: segments; augmentPeriodicData's longer axis is honoured (vs, not N, gives the node count)
    e = S.ellipse()
    g2 = L.createGrid(np.array([[-1.], [-1.5]]), np.array([[1.], [1.]]), np.array([[23], [31]]), None)
    x2 = [float(np.asarray(v).ravel()[0]) for v in g2.vs]
    d2 = [float(v) for v in np.asarray(g2.dx).ravel()]
    out = extract_level_set(g2, np.array(e["phi"]))
    assert_same_mesh((out.verts, out.faces), S.level_set_ref(e["N"], x2, d2, e["phi"], 0.0), "2-D")
    length, area = level_set_measure(out.verts, out.faces)
    assert abs(area - np.pi * 0.36 / 0.8) < 0.005 * np.pi * 0.36 / 0.8 and length > 0
    gp = L.createGrid(np.array([[-1.], [-1.5]]), np.array([[1.], [1.]]), np.array([[23], [31]]), 1)
    gA, dA = L.augmentPeriodicData(gp, np.array(e["phi"]))
    assert dA.shape == (23, 32)
    out = extract_level_set(gA, dA)
    xa = [float(np.asarray(v).ravel()[0]) for v in gA.vs]
    da = [float(v) for v in np.asarray(gA.dx).ravel()]
    assert_same_mesh((out.verts, out.faces), S.level_set_ref((23, 32), xa, da, dA, 0.0), "augmented")


def test_implicit_mesh_has_the_reference_s_signature():
    pytest.importorskip("matplotlib")
    from mpl_toolkits.mplot3d.art3d import Poly3DCollection
    case = S.anisotropic()
    phi = np.array(case["phi"])
    spacing = (0.5, 2.0, 1.25)
    mid = 0.5 * (phi.min() + phi.max())
    out = implicit_mesh(phi, None, spacing)                                   # positional, as the reference is called
    assert isinstance(out.mesh, Poly3DCollection) and isinstance(out.verts, np.ndarray)
    rv, rf = S.level_set_ref(case["N"], [0.0] * 3, spacing, phi, mid)
    assert_same_mesh((out.verts, out.faces), (rv, rf), "level=None")
    # verts in units of spacing: inside the box [0, (N - 1) * spacing], and spacing scales them exactly (powers of two)
    assert np.all(out.verts >= 0) and np.all(out.verts <= (np.array(case["N"]) - 1) * np.array(spacing))
    unit = implicit_mesh(phi, level=mid)                                      # spacing defaults to (1, 1, 1)
    twice = implicit_mesh(phi, level=mid, spacing=(2., 2., 2.))
    assert np.array_equal(twice.verts, 2.0 * unit.verts) and np.array_equal(twice.faces, unit.faces)
    down = implicit_mesh(torch.as_tensor(phi, device="cuda"), level=0.1, spacing=spacing, gd='descent', edge_color='b', face_color='g')
    up = implicit_mesh(phi, level=0.1, spacing=spacing, gd='ascent')
    assert np.array_equal(down.verts, up.verts) and np.array_equal(down.faces, up.faces[:, ::-1])
    assert level_set_measure(up.verts, up.faces)[1] > 0 > level_set_measure(down.verts, down.faces)[1]
    with pytest.raises(Exception):
        implicit_mesh(phi, gd='sideways')
    with pytest.raises(Exception):
        implicit_mesh(phi[0])


def test_the_example_runs():
    """examples/reachable_tube_mesh.py at n = 31: a mesh per tau slice, the tube grows, the .obj holds the last slice."""
    obj = os.path.join(os.environ.get("TMPDIR", "/tmp"), "reachable_tube_mesh_%d.obj" % os.getpid())
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "reachable_tube_mesh.py"), "31", "0.5", obj],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rows = [l.split() for l in out.stdout.splitlines() if re.match(r"^\s*\d+\.\d+\s+\d+\s+\d+\s", l)]
        assert len(rows) == 6, out.stdout
        nv, nf = [int(r[1]) for r in rows], [int(r[2]) for r in rows]
        area, vol, counted = [float(r[3]) for r in rows], [float(r[4]) for r in rows], [float(r[5]) for r in rows]
        assert min(nv) > 0 and min(nf) > 0 and vol[-1] > vol[0] > 0
        # tau = 0 is the cylinder of radius 0.5 over the whole period.  The chords of a circle of radius r at spacing h enclose
        # less than the disc by at most about (h / r)^2 / 2 of its area: h = 4 / 30, r = 0.5 gives 3.6 %; 5 % allowed
        exact = np.pi * 0.25 * 2 * np.pi
        assert 0 <= exact - vol[0] <= 0.05 * exact, (vol[0], exact)
        # counting nodes misplaces the boundary by at most half a cell: |difference| <= area * max(dx) / 2, plus the 5 % above
        for a, v, c in zip(area, vol, counted):
            assert abs(v - c) <= 0.5 * a * (4.0 / 30) + 0.05 * v, (a, v, c)
        lines = open(obj).read().splitlines()
        assert sum(l.startswith("v ") for l in lines) == nv[-1] and sum(l.startswith("f ") for l in lines) == nf[-1]
    finally:
        if os.path.exists(obj):
            os.remove(obj)
