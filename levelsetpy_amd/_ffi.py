"""ctypes binding of libhj_mi355x.so (include/hj_mi355x.h).

The product path is HIP only: if the shared library is missing or cannot be
loaded, every compute entry point raises.  bind() below is the one loader: the bindings of
the stateless libraries (the other _?ffi modules) go through it too.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# enums of include/hj_mi355x.h
BC_EXTRAPOLATE, BC_PERIODIC = 0, 1
DISS_GLF, DISS_LOCAL = 0, 1
DISS_LLF, DISS_LLLF = 1, 2          # distinguished by run-time Hamiltonians that read the costate range (hj_mi355x.h)
POST_NONE, POST_MIN_PREV, POST_MAX_PREV = 0, 1, 2
ENO2, ENO3, WENO5, WENO5_ASSHIPPED = 0, 1, 2, 3
HAM_DUBINS_REL, HAM_DOUBLE_INTEGRATOR, HAM_DOUBLE_PENDULUM = 0, 1, 2
HAM_USER_BASE = 100
HAM_DIMS = {HAM_DUBINS_REL: 3, HAM_DOUBLE_INTEGRATOR: 2, HAM_DOUBLE_PENDULUM: 4}      # state dimension of the built-in systems
F64, F32 = 0, 1
STAGE_YDOT, STAGE_EULER, STAGE_RK3_HALF, STAGE_RK3_FULL, STAGE_RK2_FULL = 0, 1, 2, 3, 4
OP_MIN, OP_MAX, OP_MAX_NEG = 0, 1, 2
STENCIL = 3
BOUND_SLOTS = 64

SCHEME_IDS = {"ENO2": ENO2, "ENO3": ENO3, "WENO5": WENO5, "WENO5_ASSHIPPED": WENO5_ASSHIPPED, "ENO2_FAST": 4, "ENO3_FAST": 5}

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pd, _pi, _pi64 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hj_ctx_create": (_i, [C.POINTER(_vp), _i, _pi64, _pd, _pd, _pi, _pi, _i, _i]),
    "hj_ctx_destroy": (None, [_vp]),
    "hj_ctx_set_stream": (_i, [_vp, _vp]),
    "hj_ctx_set_coords": (_i, [_vp, _i, _pd]),
    "hj_ctx_set_aux": (_i, [_vp, _i, _pd, _i64]),
    "hj_ctx_set_slab": (_i, [_vp, _i, _i]),
    "hj_ghost": (_i, [_vp, _i, _i, _vp, _vp]),
    "hj_upwind": (_i, [_vp, _i, _i, _vp, _vp, _vp, _pd]),
    "hj_lf_split_begin": (_i, [_vp, _i, _vp, C.POINTER(_vp), C.POINTER(_vp), _pd]),
    "hj_lf_split_end": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _pd, _vp, _vp, _pd, _pd]),
    "hj_rk_combine": (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _i64]),
    "hj_lf_term": (_i, [_vp, _i, _i, _pd, _d, _i, _vp, _vp, _pd]),
    "hj_rk_substep": (_i, [_vp, _i, _i, _pd, _d, _i, _d, _i, _vp, _vp, _vp, _i, _i64, _i64]),
    "hj_read_step_bound": (_i, [_vp, _i, _pd, _pd]),
    "hj_rk_step": (_i, [_vp, _i, _i, _i, _pd, _d, _d, _d, _d, _i, _vp, _vp, _vp, _vp, _pd, _pd]),
    "hj_rk_stage12": (_i, [_vp, _i, _i, _pd, _d, _d, _d, _vp, _vp, _i]),
    "hj_rk_plan": (_i, [_vp, _i, _i, _i, _pd, _i, _pi, _pi]),
    "hj_rk_integrate": (_i, [_vp, _i, _i, _i, _pd, _d, _d, _d, _d, _i, _vp, _vp, _vp, _vp, _i64, _d, _pd, _pi64, _pi]),
    "hj_ctx_set_post_step": (_i, [_vp, _i]),
    "hj_ctx_set_post_arrays": (_i, [_vp, _i, _vp, _i, _vp]),
    "hj_static_step_bound": (_i, [_vp, _i, _pd, _pd, _pd]),
    "hj_ctx_set_dissipation": (_i, [_vp, _i]),
    "hj_max_d1sq": (_i, [_vp, _vp, _vp]),
    "hj_ctx_set_weno_eps_source": (_i, [_vp, _vp]),
    "hj_minmax_with": (_i, [_vp, _i, _vp, _vp, _i64]),
    "hj_any_nan": (_i, [_vp, _vp, _i64, _pi]),
    "hj_comm_unique_id": (_i, [C.c_char_p, _vp]),
    "hj_comm_init": (_i, [_vp, C.c_char_p, _i, _i, _vp, _i, _i]),
    "hj_comm_destroy": (_i, [_vp]),
    "hj_comm_info": (_i, [_vp, _pi, _pi, _pi, _pi]),
    "hj_halo_exchange": (_i, [_vp, _vp]),
    "hj_slab_join": (_i, [_vp]),
    "hj_slab_rk_step": (_i, [_vp, _i, _i, _i, _pd, _d, _i, _vp, _vp, _vp, _vp]),
    "hj_ctx_set_axis0_pad": (_i, [_vp, _i, _pd, _pd, _pd]),
    "hj_comm_init_external": (_i, [_vp, _i, _i, _i, _i]),
    "hj_halo_exchange_depth": (_i, [_vp, _vp, _i]),
    "hj_slab_rk_step_deep": (_i, [_vp, _i, _i, _i, _pd, _d, _i, _vp, _vp, _vp, _vp]),
    "hj_term_normal": (_i, [_vp, _i, _vp, _vp, _d, _vp, _pd]),
    "hj_term_reinit": (_i, [_vp, _i, _vp, _vp, _i, _vp, _pd]),
    "hj_term_convection": (_i, [_vp, _i, _vp, _vp, _pd, _vp, _pd]),
    "hj_term_curvature": (_i, [_vp, _vp, _vp, _d, _vp, _pd]),
    "hj_curvature_second": (_i, [_vp, _vp, _vp, _vp]),
    "hj_hessian_second": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "hj_laplacian_second": (_i, [_vp, _vp, _vp]),
    "hj_centered_first_second": (_i, [_vp, _i, _vp, _vp]),
    "hj_term_trace_hessian": (_i, [_vp, _vp, C.POINTER(_vp), _pd, C.POINTER(_vp), _pd, _vp, _pd]),
    "hj_ham_register": (_i, [C.c_char_p, _i, _i, C.c_char_p, C.c_char_p, _i, C.c_char_p, C.c_char_p, _pi]),
    "hj_ham_register2": (_i, [C.c_char_p, _i, _i, C.c_char_p, C.c_char_p, _i, _i, C.c_char_p, C.c_char_p, _pi]),
    "hj_ham_flags": (_i, [_i, _pi]),
    "hj_rk_last_bounds": (_i, [_vp, _pd, _pi]),
    "hj_rk_prev_bounds": (_i, [_vp, _pd, _pi, _pd]),
    "hj_range_pass": (_i, [_vp, _i, _i, _pd, _vp, _vp]),
    "hj_bound_pass": (_i, [_vp, _i, _i, _pd, _vp, _pd]),
    "hj_ctx_set_range_source": (_i, [_vp, _vp]),
    "hj_range_alpha_max": (_i, [_vp, _i, _pd, _pd]),
    "hj_ham_info": (_i, [_i, _pi, _pi, _pi]),
    "hj_ham_compile_check": (_i, [_i, _i]),
    "hj_ham_cache_stats": (_i, [_pi, _pi]),
    "hj_sync": (_i, [_vp]),
    "hj_last_error": (C.c_char_p, []),
    "hj_last_kernel": (C.c_char_p, [C.c_void_p]),
    "hj_last_launch": (_i, [_vp, _pi, _pi]),
    "hj_last_tile": (_i, [_vp, _pi]),
    "hj_ctx_state_generation": (C.c_uint64, [_vp]),
    "hj_plan_substep": (_i, [_i, _pi64, _pi, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _pi64, C.c_char_p, _i]),
    "hj_plan_substep_symbols": (_i, [_i, _pi64, _pi, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _pi64, C.c_char_p, _i]),
    "hj_launch_record": (_i, [_vp, _i]),
    "hj_launch_record_read": (_i, [_vp, C.c_char_p, _i]),
    "hj_version": (C.c_char_p, []),
}

HAM_RANGE = 1          # hj_ham_register2 flag: alpha reads the costate range (dmin / dmax)


class Unsupported(ValueError):
    """HJ_EUNSUPPORTED: the library has no kernel for this combination (callers with another path may take it)."""


def bind(env_var, file_name, prefix, fallback_text, signatures):
    """The loader of one shared library of levelsetpy_amd/csrc: -> (path, lib, check, last_kernel).

      path           the environment variable's value, or the library beside this package's sources
      lib()          the loaded library, its functions typed by `signatures`; RuntimeError (loudly) if it is not built
      check(rc)      non-zero return code -> ValueError with <prefix>_last_error() (Unsupported for HJ_EUNSUPPORTED),
                     as the reference's error() (matlab_utils.py:134-137)
      last_kernel()  <prefix>_last_kernel() of the calling thread as text (the stateless libraries)
    """
    path = os.environ.get(env_var) or os.path.join(HERE, "csrc", file_name)
    loaded = []

    def lib():
        if not loaded:
            if not os.path.exists(path):
                raise RuntimeError(
                    "levelsetpy_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` (or `make -C levelsetpy_amd/csrc`). There is no CPU fallback." % path)
            # torch first: its wheel bundles the HIP/HSA runtime the process must share.  Loaded the other way
            # round, the library would bring in /opt/rocm's copy and torch a second one, and the later of the
            # two runtimes to initialise finds "no ROCm-capable device" (seen with build() followed by smoke()).
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            L = C.CDLL(path)
            for name, (res, args) in signatures.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            loaded.append(L)
        return loaded[0]

    def check(rc):
        if rc != 0:
            msg = getattr(lib(), prefix + "_last_error")()
            text = (msg or fallback_text.encode()).decode("utf-8", "replace") + " (code %d)" % rc
            raise (Unsupported if rc == -3 else ValueError)(text)

    def last_kernel():
        return (getattr(lib(), prefix + "_last_kernel")() or b"").decode()

    return path, lib, check, last_kernel


LIB_PATH, lib, check, _ = bind("HJ_LIB", "libhj_mi355x.so", "hj", "hj_mi355x error", SIGNATURES)   # HJ_LIB: tuning builds


def darr(values):
    values = [float(v) for v in values]
    return (C.c_double * max(1, len(values)))(*values)


def grid_descriptor(cls, width, ndim, N, xmin, xlast, dx, bc, tz, dtype_name):
    """A grid descriptor of struct class `cls` with room for `width` axes (hjq_grid: 4, hjh_grid: 6), unused axes neutral."""
    g = cls()
    g.ndim = int(ndim)
    g.dtype = F64 if dtype_name == "float64" else F32
    for d in range(width):
        inside = d < ndim
        g.N[d] = int(N[d]) if inside else 1
        g.xmin[d] = float(xmin[d]) if inside else 0.0
        g.xlast[d] = float(xlast[d]) if inside else 0.0
        g.dx[d] = float(dx[d]) if inside else 1.0
        g.bc[d] = int(bc[d]) if inside else 0
        g.toward_zero[d] = int(tz[d]) if inside else 0
    return g
