"""CPU-only: the host layer the stateless libraries share (levelsetpy_amd/csrc/hj_tool_host.h, levelsetpy_amd/_ffi.bind).

  * every argument check of tests/tool_lib_cases.py: the return code and a word of <prefix>_last_error().  Every data pointer
    is null and every check comes before the first HIP call, so no device is touched;
  * each library keeps an error text and a last-kernel record of its own;
  * per library, the functions its header declares are the keys of SIGNATURES and the hj?_ symbols it exports, argument counts
    included; the constants of the rollout and time-to-reach bindings are their headers'.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tool_lib_cases as T  # noqa: E402
from levelsetpy_amd import _ffi, rollout  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = T.modules()
LIB_NAMES = sorted(T.LIBS)


# ------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("lib_name", LIB_NAMES)
def test_argument_checks(lib_name):
    mine = [c for c in T.CASES if c[0] == lib_name]
    assert len(mine) >= 10
    read = getattr(MODS[lib_name].lib(), T.LIBS[lib_name] + "_last_kernel")
    for case in mine:
        before = read().decode()
        rc, err, kernel = T.run(case, MODS)
        assert rc == case[4], T.line(case, rc, err, kernel)
        if rc != T.OK:
            assert case[5] and case[5] in err, T.line(case, rc, err, kernel)
        # no call launches anything: the record stays, except that an emit of nothing empties the list
        assert kernel == ("" if case[1] == "emit-nothing" else before), T.line(case, rc, err, kernel)


@pytest.mark.parametrize("lib_name", LIB_NAMES)
def test_mapping_of_return_codes(lib_name):
    """check(): HJ_EUNSUPPORTED -> Unsupported, every other code -> ValueError, the library's message and the code in the text."""
    mod = MODS[lib_name]
    for code, exc in ((T.EINVAL, ValueError), (T.EUNSUPPORTED, _ffi.Unsupported)):
        case = next(c for c in T.CASES if c[0] == lib_name and c[4] == code)
        rc, err, _ = T.run(case, MODS)
        with pytest.raises(exc) as info:
            mod.check(rc)
        assert str(info.value) == "%s (code %d)" % (err, code) and (exc is _ffi.Unsupported or not isinstance(info.value, _ffi.Unsupported))
    mod.check(0)


@pytest.mark.parametrize("lib_name", LIB_NAMES)
def test_a_refusal_leaves_the_other_libraries_records_alone(lib_name):
    others = [n for n in LIB_NAMES if n != lib_name]
    for n in others:                                                  # every other library holds a text first
        T.run(next(c for c in T.CASES if c[0] == n and c[1].endswith("dtype7")), MODS)
    read = lambda n: getattr(MODS[n].lib(), T.LIBS[n] + "_last_error")().decode()       # noqa: E731
    before = {n: read(n) for n in others}
    assert all("dtype" in v for v in before.values())
    told = 0
    for case in (c for c in T.CASES if c[0] == lib_name and c[4] != T.OK):
        rc, err, _ = T.run(case, MODS)
        assert rc != T.OK and read(lib_name) == err
        assert {n: read(n) for n in others} == before, case[1]
        told += err not in before.values()                            # a text that would show if the records were one
    assert told >= 5


def test_rollout_of_no_state_keeps_the_last_kernel_record():
    lib = MODS["rollout"].lib()
    before = lib.hjr_last_kernel()
    case = next(c for c in T.CASES if c[1] == "rollout-nostates")
    assert T.run(case, MODS)[0] == T.OK and lib.hjr_last_kernel() == before


def test_emit_of_no_vertex_leaves_the_kernel_list_empty():
    case = next(c for c in T.CASES if c[1] == "emit-nothing")
    assert T.run(case, MODS)[0] == T.OK and MODS["surface"].last_kernels() == []


# ------------------------------------------------------------------------------------------ header, binding, export table
REQUIRED = {"query": ["hjq_interp_points", "hjq_costate_points", "hjq_project_minmax"],
            "surface": ["hjs_workspace_size", "hjs_count", "hjs_emit"],
            "ttr": ["hjt_ttr_init", "hjt_ttr_update", "hjt_ttr_from_stack"],
            "rollout": ["hjr_rollout"],
            "batch": ["hjb_step_bounds", "hjb_substep", "hjb_integrate"],
            "hiquery": ["hjx_interp_points", "hjx_costate_points", "hjx_project_minmax", "hjx_rollout"],
            "plant": ["hjp_plant_register", "hjp_rollout", "hjp_rollout_hi"],
            "shapes": ["hjg_evaluate"],
            "hishapes": ["hjk_evaluate", "hjk_plan", "hjk_decode"]}


def header_code(lib_name):
    txt = open(os.path.join(ROOT, "include", "hj_%s.h" % lib_name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


@pytest.mark.parametrize("lib_name", LIB_NAMES)
def test_binding_header_and_exports_name_the_same_functions(lib_name):
    mod, pre, code = MODS[lib_name], T.LIBS[lib_name], header_code(lib_name)
    declared = sorted(set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % pre, code)))
    assert declared and declared == sorted(mod.SIGNATURES), (declared, sorted(mod.SIGNATURES))
    for need in REQUIRED[lib_name] + [pre + "_last_error", pre + "_last_kernel"]:
        assert need in declared
    if lib_name == "rollout":
        assert len(declared) == 3
    out = subprocess.check_output(["nm", "-D", mod.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (%s_[a-z0-9_]+)" % pre, out)))
    assert exported == declared, (exported, declared)
    lib = mod.lib()
    for name, (_, args) in mod.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_rollout_constants_are_the_headers():
    import rollout_ref as R
    from levelsetpy_amd import _rffi
    code = header_code("rollout")
    for name, val in (("HJR_MODE_MIN", _rffi.MODE_MIN), ("HJR_MODE_MAX", _rffi.MODE_MAX), ("HJR_REACHED", _rffi.REACHED),
                      ("HJR_EXHAUSTED", _rffi.EXHAUSTED), ("HJR_LEFT_GRID", _rffi.LEFT_GRID)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert C.sizeof(_rffi.Plant) == 48
    assert (rollout.REACHED, rollout.EXHAUSTED, rollout.LEFT_GRID) == (R.REACHED, R.EXHAUSTED, R.LEFT_GRID)


def test_ttr_mode_bits_are_the_headers():
    import ttr_ref as R
    from levelsetpy_amd import _tffi
    code = header_code("ttr")
    assert (_tffi.FIRST, _tffi.NO_INTERP) == (R.FIRST, R.NO_INTERP)
    assert re.search(r"HJT_FIRST\s*=\s*1\b", code) and re.search(r"HJT_NO_INTERP\s*=\s*2\b", code)


def test_one_table_of_state_dimensions():
    from levelsetpy_amd import _bffi, _rffi
    assert _rffi.PLANT_DIMS is _ffi.HAM_DIMS and _bffi.HAM_DIMS is _ffi.HAM_DIMS
    assert _ffi.HAM_DIMS == {_ffi.HAM_DUBINS_REL: 3, _ffi.HAM_DOUBLE_INTEGRATOR: 2, _ffi.HAM_DOUBLE_PENDULUM: 4}
