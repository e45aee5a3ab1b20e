/* libhj_hidim.so: Hamilton-Jacobi problems on 5-D and 6-D grids (gfx950).
 *
 * The solver of hj_mi355x.h stops at HJ_MAX_DIM = 4 axes, and that constant is part of every struct of the other ABIs.
 * This library is the substep, the step bound, the whole-interval integrator and the derivative pass for grids of
 * HJH_MIN_DIM .. HJH_MAX_DIM axes, with a grid descriptor and coordinate tables of its own.  The entry points are
 * stateless -- no hj_ctx: a descriptor, the tables and a HIP stream per call.  Every array pointer is DEVICE memory owned
 * by the caller unless it is called *_host; inputs are never written.  Return value: HJ_OK (0) or a negative HJ_E* code
 * of hj_mi355x.h; hjh_last_error() holds the text.  A call that returns an error has launched nothing.  All index
 * arithmetic is 64-bit.
 *
 * A substep is the solver's: one thread per cell, the cell's stencils gathered straight from global memory (ghost cells
 * as hj_mi355x.h describes them), upwind derivatives of `scheme`, the Lax-Friedrichs term of the built-in system `ham`
 * with global dissipation, the stage expression of HJ_STAGE_*.  The per-cell device functions are the ones
 * libhj_mi355x.so compiles (csrc/hj_device.h, csrc/hj_split.h), instantiated at 5 and 6 axes.
 *     scheme   HJ_ENO2 | HJ_ENO3 | HJ_WENO5_ASSHIPPED   (HJ_EUNSUPPORTED otherwise: the intended WENO5's epsilon is a
 *              reduction over the whole grid)
 *     ham      HJH_HAM_PLANE5D (5-D) | HJH_HAM_DUBINS_PAIR6D (6-D)
 *     dtype    g->dtype, HJ_F64 | HJ_F32: the element type of every state array and of the tables
 *
 * params_host: HJH_PAR_SLOTS fp64 on the HOST (unused slots 0), rounded to the grid's dtype where they are used; they
 * travel in the kernel arguments.
 *     HJH_HAM_PLANE5D         state (x, y, theta, v, omega); { a_max, alpha_max, s } with s = -1 (the control minimises) or +1
 *                             H = p0 (x3 cos x2) + p1 (x3 sin x2) + p2 x4 + s (a_max |p3|) + s (alpha_max |p4|)
 *                             alpha = { |x3 cos x2|, |x3 sin x2|, |x4|, a_max, alpha_max }
 *                             aux0 = cos(vs[2]), aux1 = sin(vs[2])
 *     HJH_HAM_DUBINS_PAIR6D   evader (x0, x1, x2), pursuer (x3, x4, x5); { v_e, v_p, w_e, w_p }
 *                             H = -( p0 (v_e cos x2) + p1 (v_e sin x2) + p3 (v_p cos x5) + p4 (v_p sin x5) + w_e |p2| - w_p |p5| )
 *                             alpha = { |v_e cos x2|, |v_e sin x2|, w_e, |v_p cos x5|, |v_p sin x5|, w_p }
 *                             aux0 = cos(vs[2]), aux1 = sin(vs[2]), aux2 = cos(vs[5]), aux3 = sin(vs[5])
 * Sums run left to right.  With HJ_ENO2 / HJ_ENO3 every operation is rounded on its own, in that order.
 * HJ_F32 (contract, as hj_mi355x.h states it for the solver; tests/test_gpu_fp32_exact.py): the tables (coordinates, cos / sin)
 * are the caller's, of the grid's dtype -- the package forms them in fp64 and rounds once --; each parameter is rounded once and
 * an alpha that is a parameter (a_max, alpha_max, w_e, w_p) enters hjh_step_bound as that rounded value, widened exactly; dt is
 * converted once per launch, (float)dt; the bound 1 / sum_d (max alpha_d / dx_d) is formed in fp64 in axis order.  With HJ_ENO2 /
 * HJ_ENO3 a float substep and hjh_upwind are then bit for bit the float32 mode of oracle/hj_oracle.py.
 *
 * Any other system: hjh_ham_register (below) compiles the caller's H / alpha expression into these kernels at run time; its
 * id (>= HJH_HAM_USER_BASE) is a `ham` like the two above.
 */
#ifndef HJ_HIDIM_H
#define HJ_HIDIM_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else                                  /* hipRTC (hjh_ham_register) has no system headers; hj_mi355x.h brings int64_t */
typedef signed int int32_t;
#endif
#include "hj_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJH_MIN_DIM = 5, HJH_MAX_DIM = 6 };
enum { HJH_HAM_PLANE5D = 50, HJH_HAM_DUBINS_PAIR6D = 51 };
enum { HJH_HAM_USER_BASE = 1000 };     /* ids >= this: systems registered at run time (hjh_ham_register) */
#define HJH_PAR_SLOTS 8

/* hjq_grid (hj_query.h) with room for six axes */
typedef struct hjh_grid {
    int32_t ndim;                      /* HJH_MIN_DIM .. HJH_MAX_DIM */
    int32_t dtype;                     /* HJ_F64 | HJ_F32 */
    int64_t N[6];                      /* nodes per axis, row-major arrays (last axis fastest) */
    double xmin[6];
    double xlast[6];
    double dx[6];
    int32_t bc[6];                     /* HJ_BC_EXTRAPOLATE | HJ_BC_PERIODIC */
    int32_t toward_zero[6];
} hjh_grid;

/* 1-D tables of the grid's dtype */
typedef struct hjh_tables {
    const void* coord[6];              /* grid.vs[d]: N[d] values */
    const void* aux[4];                /* the cos / sin tables of `ham`, listed above; a registered system's own tables */
} hjh_tables;

/* post-step operators against arrays, numbered as hjb_entry's (hj_batch.h) */
enum { HJH_ARR_NONE = 0, HJH_ARR_MIN = 1, HJH_ARR_MAX = 2, HJH_ARR_MAX_NEG = 3 /* max(y, -array): obstacle mask */ };

/* One stage (HJ_STAGE_*, HJ_STAGE_YDOT included): dst = stage(y0, src + dt * ydot(src)).  restrict_sign as hj_rk_substep.
 * After the stage expression, in this order: post_prev (HJ_POST_MIN_PREV / HJ_POST_MAX_PREV: min / max with y0 where the
 * stage reads y0, with src otherwise), then op_a against post_a, then op_b against post_b -- NaN propagating as NumPy's
 * minimum / maximum.  HJ_STAGE_YDOT applies none of them.  dst must not alias src.  Asynchronous on `stream`. */
int hjh_substep(const hjh_grid* g, const hjh_tables* tab, int scheme, int ham, int stage, int restrict_sign,
                const double* params_host, const void* src, const void* y0, void* dst, double dt, int post_prev,
                int op_a, const void* post_a, int op_b, const void* post_b, void* stream);

/* stepBound = 1 / sum_d max_x alpha_d(x) / dx_d with the system's alpha at zero costate (it ignores the data), summed
 * in axis order: the meaning of hjb_step_bounds.  keys: HJH_MAX_DIM 64-bit words of device scratch.  sb_host: one value;
 * amax_host (may be null): HJH_MAX_DIM values, the per-axis maxima.  The call waits for `stream`. */
int hjh_step_bound(const hjh_grid* g, const hjh_tables* tab, int ham, const double* params_host, void* keys,
                   double* sb_host, double* amax_host, void* stream);

/* A whole interval: hj_rk_integrate's schedule (order 1..3; the time arithmetic is hjb_plan's, stop_tol as there) with
 * the steps planned on the host before the first launch.  Step sizes and parameters travel as kernel arguments: nothing
 * but scalars is copied, and the host does not wait between launches or at the end.  post_prev and the array operators
 * are applied by the last stage of every step.  y_in is never written; buf_a, buf_b and work (orders 2 and 3) are
 * distinct arrays of the grid's size.  t_host / steps_host: the time reached and the number of steps.  result_in_host:
 * where the result is -- 0: y_in (no step), 1: buf_a, 2: buf_b. */
int hjh_integrate(const hjh_grid* g, const hjh_tables* tab, int scheme, int ham, int order, int restrict_sign,
                  int post_prev, const double* params_host, double sb, const void* y_in, void* buf_a, void* buf_b,
                  void* work, int op_a, const void* post_a, int op_b, const void* post_b, double t0, double tf,
                  double factor_cfl, double max_step, double stop_tol, double* t_host, int64_t* steps_host,
                  int32_t* result_in_host, void* stream);

/* derivL[d] and derivR[d] (upwindFirst* of `scheme`) for every axis d whose bit is set in axis_mask, from one gather per
 * cell.  derivL_host / derivR_host: HJH_MAX_DIM device pointers in host memory (those of unnamed axes are not read).
 * keys (may be null): 4 * HJH_MAX_DIM 64-bit words, zeroed by the call; keys[4 d + k] receives the order-preserving key
 * of { -min L, max L, -min R, max R } of axis d, as upwind_all_kernel leaves them.  With HJ_ENO2 / HJ_ENO3 the values are
 * the substep's own one-sided derivatives, every operation rounded on its own.  Asynchronous on `stream`. */
int hjh_upwind(const hjh_grid* g, int scheme, const void* src, unsigned axis_mask, void* const* derivL_host,
               void* const* derivR_host, void* keys, void* stream);

/* ---- systems registered at run time.  `body` is a device expression (C++ statements) that assigns H and every alpha[d] from
 *     x[d]    node coordinates, d = 0 .. ndim-1          p[d]    costates (the reference's derivC)
 *     par[k]  the call's params_host, k < nparams        aux[k]  the value of the call's table tab->aux[k] (k < naux) at this cell's
 *     T       the element type                                   index along axis aux_axes[k]: N[aux_axes[k]] values of the grid's dtype
 * and device math functions.  It sees neither the time, the data nor the costate range (alpha must not depend on them: the step
 * bound is a property of the grid).  hipRTC compiles hidim_substep_kernel / hidim_bound_kernel (csrc/hj_hidim_dev.h, found in
 * include_dir) around it for gfx950, lazily at the first launch on each device, and keeps the code objects in the on-disk cache
 * hj_mi355x.h describes.  With HJ_ENO2 / HJ_ENO3 the expression is compiled with contraction off: every operation is rounded on
 * its own, as a NumPy callback written the same way rounds.  hjh_substep, hjh_step_bound and hjh_integrate take the id as `ham`;
 * a null tab->aux[k], k < naux, is refused.  The same (name, ndim, nparams, body, axes) registered again gives the same id.
 * hiprtc_path (may be null): the libhiprtc.so to load. */
int hjh_ham_register(const char* name, int ndim, int nparams, const char* body, int naux, const int32_t* aux_axes,
                     const char* include_dir, const char* hiprtc_path, int* ham_id);
/* what was registered (any pointer may be null); aux_axes: 4 values, -1 past naux; kernels_built: on all devices */
int hjh_ham_info(int ham_id, int* ndim, int* nparams, int* naux, int32_t* aux_axes, int* kernels_built);
/* compile the substep kernel of (scheme, dtype) and the bound kernel now, without a launch (needs no GPU); HJ_EINVAL with the
 * compiler's message, which names the registration and the line of `body` */
int hjh_ham_compile_check(int ham_id, int scheme, int dtype);
/* the generated translation unit, 0-terminated, for offline inspection (hipcc -I csrc -I include); n: the buffer's size */
int hjh_ham_source(int ham_id, char* buf, int64_t n);
/* kernels compiled with hipRTC / loaded from the disk cache by this library in this process */
int hjh_ham_cache_stats(int* compiled, int* loaded_from_cache);

const char* hjh_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g.
 * "hidim_substep_kernel<double, HamDubinsPair6D, 3>" (element type, system, scheme) */
const char* hjh_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
