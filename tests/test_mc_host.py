"""CPU-only: libhj_mc.so without a device (levelsetpy_amd/_nffi.py, include/hj_mc.h).

  * hjn_normals_host: the Philox words equal tests/mc_ref.py's exactly, the normals are within 1e-12 (the project's rule wherever
    libm enters: log, cos and sin are each side's own; sqrt and the products are exact operations);
  * every refusal of hjn_rollout and hjn_normals returns its code and leaves the sentinel-filled outputs untouched: every check
    comes before the first HIP call, so host arrays stand in for the device's;
  * the header, the binding and the export table name the same functions; the Makefile builds the library; the trajectory and the
    plants have one source each.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mc_ref as MC  # noqa: E402
from levelsetpy_amd import _ffi, _nffi, _qffi, _rffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3


@pytest.mark.parametrize("nd", [1, 2, 3, 4])
@pytest.mark.parametrize("first", [0, 2 ** 32 - 3, 2 ** 40, 2 ** 64 - 2])
def test_host_generator_equals_the_restatement(first, nd):
    seed = 0x299f31d0a4093822
    z, w = _nffi.normals_host(seed, first, 6, 5, 7, nd, words=True)
    rw = MC.words(seed, first, 6, 5, 7, nd)
    assert w.dtype == rw.dtype and np.array_equal(w, rw)
    rz = MC.normals_of(rw, nd)
    err = float(np.max(np.abs(z - rz)))
    print("first %d nd %d: max|normal - restatement| %.3e" % (first, nd, err))
    assert z.shape == (6, 7, nd) and err <= 1e-12
    if first == 2 ** 32 - 3:                                   # the carry into the counter's second word
        assert not np.array_equal(w[2], w[3]) and np.array_equal(w[3], MC.words(seed, 2 ** 32, 1, 5, 7, nd)[0])


def test_known_answer_through_the_library():
    """counter (243f6a88 85a308d3 13198a2e 03707344), key (a4093822 299f31d0): realisation, step and the pair index 0x03707344 are
    reachable only for pairs 0 and 1, so the published vector is checked in the restatement; here the all-zero one."""
    _, w = _nffi.normals_host(0, 0, 1, 0, 1, 2, words=True)
    assert [int(v) for v in w.ravel()] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def _grid(nd=2, n=9):
    return _qffi.grid_descriptor(nd, [n] * nd, [-1.0] * nd, [1.0] * nd, [2.0 / (n - 1)] * nd, [_ffi.BC_EXTRAPOLATE] * nd, [0.0] * nd, "float64")


def test_rollout_refusals_touch_nothing():
    lib = _nffi.lib()
    M, R, T, nd, n = 3, 2, 4, 2, 81
    data = np.zeros((T, 9, 9))
    x0 = np.zeros((M, nd))
    G = np.eye(2)
    f64 = {k: np.full(s, 5.0) for k, s in dict(final=(M, R, nd), vend=(M, R), vmin=(M, R), traj=(M, R, nd, T)).items()}
    i32 = {k: np.full(s, -77, dtype=np.int32) for k, s in dict(length=(M, R), status=(M, R), te=(M, R, T)).items()}
    desc, desc3 = _grid(2), _grid(3)
    di = _rffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 0, 0, [1.0])
    dub = _rffi.plant_descriptor(_ffi.HAM_DUBINS_REL, 1, 0, [1.0, 1.0, 1.0])
    ad = lambda a: a.ctypes.data                                            # noqa: E731

    def call(desc=desc, scheme=_ffi.ENO2, data=ad(data), T=T, stride=n, x0=ad(x0), M=M, R=R, first=0, seed=1, normals=None,
             G=ad(G), sq=0.1, policy=0, sub=2, dt=0.01, plant=di, final=ad(f64["final"]), length=ad(i32["length"]),
             status=ad(i32["status"]), vend=ad(f64["vend"]), vmin=ad(f64["vmin"]), traj=ad(f64["traj"]), te=ad(i32["te"])):
        return lib.hjn_rollout(C.byref(desc) if desc is not None else None, scheme, data, T, stride, x0, M, R, first, seed, normals,
                               G, sq, policy, sub, dt, C.byref(plant) if plant is not None else None, final, length, status,
                               vend, vmin, traj, te, None)
    bad_G = np.array([[1.0, np.inf], [0.0, 1.0]])
    einval = [dict(data=None), dict(x0=None), dict(final=None), dict(length=None), dict(status=None), dict(vend=None),
              dict(vmin=None), dict(desc=None), dict(plant=None), dict(T=1), dict(sub=0), dict(plant=dub), dict(desc=desc3),
              dict(stride=n - 1), dict(M=-1), dict(dt=float("nan")), dict(R=0), dict(R=-4), dict(G=None), dict(G=ad(bad_G)),
              dict(sq=float("inf")), dict(sq=float("nan")), dict(policy=2), dict(policy=-1),
              dict(M=2 ** 29, R=2), dict(M=1, R=2 ** 30), dict(M=2 ** 33, R=1),
              dict(plant=_rffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 2, 0, [1.0]))]
    for kw in einval:
        assert call(**kw) == EINVAL, kw
        assert lib.hjn_last_error(), kw
    assert b"G[0][1]" in (call(G=ad(bad_G)), lib.hjn_last_error())[1]
    assert b"split over states" in (call(M=2 ** 29, R=2), lib.hjn_last_error())[1]
    for kw, word in ((dict(scheme=_ffi.WENO5), b"scheme"), (dict(scheme=9), b"scheme"),
                     (dict(plant=_rffi.plant_descriptor(_ffi.HAM_USER_BASE, 0, 0, [1.0])), b"plant")):
        assert call(**kw) == EUNSUPPORTED, kw
        assert word in lib.hjn_last_error()
    with pytest.raises(_ffi.Unsupported):
        _nffi.check(call(scheme=_ffi.WENO5))
    with pytest.raises(ValueError):
        _nffi.check(call(R=0))
    assert call(M=0) == 0 and _nffi.last_kernel() == ""               # nothing to do: fine, and launches nothing
    assert all((a == 5.0).all() for a in f64.values()) and all((a == -77).all() for a in i32.values())


def test_normals_refusals_touch_nothing():
    lib = _nffi.lib()
    z, w = np.full((4, 3, 2), 5.0), np.full((4, 3, 1, 4), 7, dtype=np.uint32)
    for fn, tail in ((lib.hjn_normals, (None,)), (lib.hjn_normals_host, ())):
        for count, step0, nsteps, nd, pw, pz in ((4, 0, 3, 0, w, z), (4, 0, 3, 5, w, z), (-1, 0, 3, 2, w, z), (4, 0, -3, 2, w, z),
                                                 (4, -1, 3, 2, w, z), (4, 2 ** 32 - 2, 3, 2, w, z), (4, 0, 3, 2, None, None),
                                                 (2 ** 40, 0, 3, 2, w, z)):
            rc = fn(1, 0, count, step0, nsteps, nd, pw.ctypes.data if pw is not None else None,
                    pz.ctypes.data if pz is not None else None, *tail)
            assert rc == EINVAL and lib.hjn_last_error(), (count, step0, nsteps, nd)
        assert fn(1, 0, 0, 0, 3, 2, None, None, *tail) == 0 and fn(1, 0, 4, 0, 0, 2, None, None, *tail) == 0
    assert (z == 5.0).all() and (w == 7).all()
    assert lib.hjn_normals_host(1, 0, 4, 2 ** 32 - 3, 3, 2, w.ctypes.data, None) == 0 and (z == 5.0).all() and not (w == 7).all()


def test_binding_header_and_exports_name_the_same_functions():
    txt = open(os.path.join(ROOT, "include", "hj_mc.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    declared = sorted(set(re.findall(r"\b(hjn_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_nffi.SIGNATURES) == ["hjn_last_error", "hjn_last_kernel", "hjn_normals", "hjn_normals_host", "hjn_rollout"]
    out = subprocess.check_output(["nm", "-D", _nffi.LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (hjn_[a-z0-9_]+)", out))) == declared
    for name, (_, args) in _nffi.SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        assert (0 if decl in ("", "void") else decl.count(",") + 1) == len(args), name
    for name, val in (("HJN_POLICY_EARLIEST", _nffi.POLICY_EARLIEST), ("HJN_POLICY_CLOCK", _nffi.POLICY_CLOCK)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, code).group(1)) == val
    stubs = set(re.findall(r"__device_stub__(\w+)", subprocess.check_output(["nm", "-D", "-C", _nffi.LIB_PATH]).decode()))
    assert stubs == {"noisy_rollout_kernel", "normals_kernel"}


def test_the_makefile_builds_the_library_and_the_trajectory_has_one_source():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libhj_mc\.so: hj_mc\.hip hj_mc_dev\.h hj_tool_host\.h hj_query_dev\.h hj_rollout_dev\.h", mk, re.M)
    assert re.search(r"^resource-usage-mc:.*\n\t.*-Rpass-analysis=kernel-resource-usage .*hj_mc\.hip$", mk, re.M)
    assert re.search(r"^\trm -f .*\blibhj_mc\.so\b", mk, re.M) and "libhj_mc.so" in mk.split("\n")[0]
    for goal in ([], ["libs"]):
        out = subprocess.check_output(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "-n", "-B"] + goal).decode()
        assert "-o libhj_mc.so hj_mc.hip" in out and "-o libhj_stoch.so hj_stoch.hip" in out
    # one trajectory, one set of plants: hj_mc.hip instantiates hj_rollout_dev.h's rollout_body around hj_plants_dev.h's plants
    csrc = os.path.join(ROOT, "levelsetpy_amd", "csrc")
    roll = open(os.path.join(csrc, "hj_rollout.hip")).read()
    body = open(os.path.join(csrc, "hj_rollout_dev.h")).read()
    assert "hjr::rollout_body<" in open(os.path.join(csrc, "hj_mc.hip")).read() and "struct NoHooks { static constexpr bool plain = true; };" in body
    assert '#include "hj_plants_dev.h"' in roll and "struct Plant<" not in roll
    assert '#include "hj_plants_dev.h"' in open(os.path.join(csrc, "hj_mc_dev.h")).read() and "struct Plant<" not in open(os.path.join(csrc, "hj_mc_dev.h")).read()
    assert open(os.path.join(csrc, "hj_plants_dev.h")).read().count("template <> struct Plant<") == 3
    # the generator is written once, for both sides
    dev = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "hj_mc_dev.h")).read()
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "hj_mc.hip")).read())
    assert "__host__ __device__ __forceinline__ void philox4x32_10(" in dev and "0xD2511F53" not in src and "atomic" not in src + dev
    assert src.count("pair_words(") == 2 and src.count("pair_normals(") == 2
