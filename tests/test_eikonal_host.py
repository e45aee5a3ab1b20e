"""CPU-only: the argument checks of libhj_eikonal.so (include/hj_eikonal.h) through ctypes, in the manner of
tests/test_decomp_host.py.  Every refusal comes before the first HIP call, so no device is touched: a bad argument is a
message, never a launch.  Also: the binding, the header and the export table name the same functions, the binding's
constants are the header's and the source's, and the front end refuses bad shapes, dtypes, speeds and bands without a device.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd  # noqa: E402
from levelsetpy_amd import _effi, _ffi, _qffi  # noqa: E402
from levelsetpy_amd import eikonal as front  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
FAKE = 0x1000                       # a non-null, 8-byte aligned address: only compared with null, never read
E = _effi
INF, NAN = float("inf"), float("nan")


def grid(N=(8, 6), dtype="float64", dx=None, bc=None):
    nd = len(N)
    return _qffi.grid_descriptor(nd, list(N), [0.0] * nd, [0.0] * nd, dx or [0.1] * nd, bc or [0] * nd, [0] * nd, dtype)


def call(N=(8, 6), K=1, stride=None, level=0.0, band=INF, speed=None, speed_scalar=1.0, data=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 40,
         max_passes=10, null=False, ndim=None, dtype_=None, dx=None, bc=None):
    lib = E.lib()
    g = grid(N, dx=dx, bc=bc)
    if ndim is not None:
        g.ndim = ndim
    if dtype_ is not None:
        g.dtype = dtype_
    total = 1
    for n in N:
        total *= n
    before = lib.hje_last_kernel()
    passes = C.c_int64(-1)
    rc = lib.hje_signed_distance(None if null else C.byref(g), data, K, total if stride is None else stride, level, band, speed, speed_scalar,
                                 out, ws, ws_bytes, max_passes, C.byref(passes), None)
    assert lib.hje_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hje_last_error().decode()


REFUSALS = [
    ("null-descriptor", dict(null=True), "null grid descriptor"),
    ("ndim0", dict(ndim=0), "ndim 0"),
    ("ndim5", dict(ndim=5), "ndim 5"),
    ("dtype7", dict(dtype_=7), "dtype 7"),
    ("K0", dict(K=0), "K = 0"),
    ("N-negative", dict(N=(8, -6)), "N[1] = -6"),
    ("dx-zero", dict(dx=[0.1, 0.0]), "dx[1] = 0"),
    ("dx-nan", dict(dx=[NAN, 0.1]), "dx[0] = nan"),
    ("bc7", dict(bc=[0, 7]), "bc[1] = 7"),
    ("field-stride", dict(stride=47), "field_stride 47"),
    ("level-nan", dict(level=NAN), "level is NaN"),
    ("band-zero", dict(band=0.0), "band = 0"),
    ("band-negative", dict(band=-1.0), "band = -1"),
    ("band-nan", dict(band=NAN), "band = nan"),
    ("max-passes0", dict(max_passes=0), "max_passes = 0"),
    ("workspace-small", dict(ws_bytes=100), "workspace of 100 bytes"),
    ("null-data", dict(data=None), "null argument"),
    ("null-out", dict(out=None), "null argument"),
    ("null-workspace", dict(ws=None), "null argument"),
    ("workspace-misaligned", dict(ws=FAKE + 4), "8-byte aligned"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    _, kw, word = case
    rc, err = call(**kw)
    assert rc == EINVAL and word in err, (rc, err)


def test_an_empty_grid_launches_nothing():
    assert call(N=(0, 6), data=None, out=None, ws=None)[0] == OK


def test_workspace_size():
    """64 bytes of counters and K int32 of sign flags, the fp64 work array, two int32 flag arrays of K x tiles, each part
    rounded up to 256 bytes."""
    lib = E.lib()
    up = lambda v: -(-v // 256) * 256           # noqa: E731
    for N, K in (((8, 6), 1), ((33, 27, 29), 3), ((3, 3), 65537), ((300,), 2), ((7, 6, 5, 9), 1)):
        need = C.c_int64(-1)
        assert lib.hje_workspace_size(C.byref(grid(N)), K, C.byref(need)) == OK
        total = int(np.prod(N))
        assert need.value == up(64 + 4 * K) + up(8 * K * total) + up(8 * K * E.tile_count(N)), (N, K)
    assert lib.hje_workspace_size(C.byref(grid((8, 6))), 1, None) == EINVAL
    assert lib.hje_workspace_size(None, 1, C.byref(need)) == EINVAL and "null grid" in lib.hje_last_error().decode()


def test_check_maps_the_codes():
    rc, err = call(ndim=9)
    with pytest.raises(ValueError) as info:
        E.check(rc)
    assert str(info.value) == "%s (code %d)" % (err, EINVAL) and not isinstance(info.value, _ffi.Unsupported)
    E.check(0)


def test_a_refusal_leaves_the_other_libraries_records_alone():
    from levelsetpy_amd import _tffi
    _tffi.lib().hjt_ttr_init(7, None, 1, 0.0, 0.0, None, None, None)
    before = _tffi.lib().hjt_last_error()
    assert b"dtype" in before
    rc, err = call(K=0)
    assert rc == EINVAL and "K = 0" in err and _tffi.lib().hjt_last_error() == before


# ------------------------------------------------------------------------------------------ header, binding, export table
def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_eikonal.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hje_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(E.SIGNATURES) == ["hje_last_error", "hje_last_kernel", "hje_signed_distance", "hje_workspace_size"]
    out = subprocess.check_output(["nm", "-D", E.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (hje_[a-z0-9_]+)", out)))
    assert exported == declared, (exported, declared)
    assert not re.findall(r" T (hj[a-df-z]?_[a-z0-9_]+)", out)            # one translation unit: nothing of another library
    lib = E.lib()
    for name, (_, args) in E.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_constants_are_the_headers_and_the_sources():
    code = header_code()
    for name, val in (("HJE_NEG", E.NEG), ("HJE_POS", E.POS), ("HJE_ZERO", E.ZERO), ("HJE_FLAGS_OFFSET", E.FLAGS_OFFSET)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    src = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "hj_eikonal.hip")).read()
    assert "256 | 16 x 32 | 4 x 8 x 16 | 4 x 4 x 4 x 8" in src
    assert E.TILES == {1: (256,), 2: (16, 32), 3: (4, 8, 16), 4: (4, 4, 4, 8)}
    assert "constexpr int GROUP = %d;" % E.GROUP in src
    assert [E.launched_passes(p, 100) for p in (1, 8, 9, 43)] == [8, 8, 16, 48] and E.launched_passes(43, 45) == 45 and E.launched_passes(1, 1) == 1
    assert E.default_max_passes((33, 27, 29)) == 8 * (9 + 4 + 2) + 64 and E.tile_count((33, 27, 29)) == 9 * 4 * 2


def test_the_makefile_builds_and_cleans_the_library():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\blibhj_eikonal\.so\b", mk, re.M) and re.search(r"^\trm -f .*\blibhj_eikonal\.so\b", mk, re.M)
    assert re.search(r"^libhj_eikonal\.so: hj_eikonal\.hip hj_tool_host\.h", mk, re.M) and "hj_eikonal.hip" in mk.split("HIPCC ?=")[0]
    assert re.search(r"^resource-usage-eikonal:", mk, re.M)


# ------------------------------------------------------------------------------------------ the front end, before any device
class G(object):
    """What signedDistance reads of a grid: N, dx, bdry."""

    def __init__(self, N):
        self.N = np.array(N, dtype=np.int64).reshape(-1, 1)
        self.dx = np.full((len(N), 1), 0.1)
        self.dim = len(N)
        self.bdry = [levelsetpy_amd.addGhostExtrapolate] * len(N)


FRONT = [
    ("shape", dict(data=np.zeros((8, 7))), "does not agree in array size"),
    ("shape-members", dict(data=np.zeros((2, 3, 8, 6))), "does not agree in array size"),
    ("level-nan", dict(level=NAN), "level"),
    ("band-zero", dict(band=0.0), "band"),
    ("band-nan", dict(band=NAN), "band"),
    ("speed-negative", dict(speed=-1.0), "speed"),
    ("speed-zero", dict(speed=0.0), "speed"),
    ("speed-shape", dict(speed=np.ones((6, 8))), "speed"),
    ("speed-members", dict(speed=np.ones((2, 8, 6))), "speed"),
    ("dtype", dict(dtype="float16"), "dtype"),
    ("max-passes", dict(max_passes=0), "max_passes"),
    ("max-passes-fraction", dict(max_passes=2.5), "max_passes"),
]


@pytest.mark.parametrize("case", FRONT, ids=[c[0] for c in FRONT])
def test_front_end_refusals(case):
    _, kw, word = case
    kw = dict(kw)
    data = kw.pop("data", np.zeros((8, 6)))
    with pytest.raises(ValueError) as info:
        levelsetpy_amd.signedDistance(G((8, 6)), data, **kw)
    assert word in str(info.value), str(info.value)


def test_front_end_refuses_five_dimensions():
    with pytest.raises(ValueError) as info:
        levelsetpy_amd.signedDistance(G((3,) * 5), np.zeros((3,) * 5))
    assert "dimensions" in str(info.value)


def test_exports():
    assert levelsetpy_amd.signedDistance is front.signedDistance and levelsetpy_amd.addCRadius is front.addCRadius
    assert front.last_path() == "" or "eikonal" in front.last_path()
