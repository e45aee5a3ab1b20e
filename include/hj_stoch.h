/* libhj_stoch.so: stochastic reachability, phi_t + H(x, grad phi) = trace(sigma^T D^2phi sigma), fused (gfx950).
 *
 * What HJIPDE_solve runs for extraArgs.addGaussianNoiseStandardDeviation = sigma (reference ValueFuncs/hji_solver.py:449-471:
 * termSum of the Lax-Friedrichs term and termTraceHessian with L = sigma^T, R = sigma, hessianFunc = hessianSecond), for a
 * constant sigma and a built-in system, as ONE launch of stoch_substep_kernel per Runge-Kutta stage.  The entry points are
 * stateless in the style of hj_batch.h: the grid descriptor of hj_query.h, the coordinate / aux tables of hj_batch.h and a HIP
 * stream per call.  Every array pointer inside a struct is DEVICE memory owned by the caller; pointers called *_host are host
 * memory; inputs are never written.  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjw_last_error() holds
 * the text.  A call that returns an error has launched nothing.  All index arithmetic is 64-bit.
 *
 * A cell's substep: the upwind derivatives of `scheme`, the Lax-Friedrichs ydot of `ham` with global dissipation and the
 * termRestrictUpdate clamp (all as libhj_batch.so forms them, from the solver's own device functions), then the Hessian of
 * hessianSecond on the ghost cells of addGhostAllDims (csrc/hj_curv.h's device functions), ydot += trace(sigma^T P sigma) in
 * cellMatrixMultiply / cellMatrixTrace order, the stage expression of HJ_STAGE_* and the post-step operators of hjb_entry.
 *     scheme   HJ_ENO2 | HJ_ENO3 | HJ_WENO5_ASSHIPPED   (the intended WENO5: HJ_EUNSUPPORTED)
 *     ham      HJ_HAM_DOUBLE_INTEGRATOR (2-D) | HJ_HAM_DUBINS_REL (3-D) | HJ_HAM_DOUBLE_PENDULUM (4-D)
 *     dtype    g->dtype must be HJ_F64   (HJ_F32: HJ_EUNSUPPORTED)
 *     sigma    ndim x ndim finite numbers, row-major, on the host
 *     form     which instantiation runs:
 *                HJW_FORM_AUTO      the diagonal one when every off-diagonal entry of sigma is zero, else the general one
 *                HJW_FORM_GENERAL   the general one (every entry of sigma, 2 ndim (ndim - 1) diagonal-neighbour loads per cell)
 *                HJW_FORM_DIAGONAL  the diagonal one (sigma_ii P_ii sigma_ii summed over ascending i, no diagonal-neighbour
 *                                   load); HJ_EINVAL when sigma has a non-zero off-diagonal entry
 * params_host: HJB_PAR_SLOTS fp64, the parameters of `ham` as hj_mi355x.h lists them (unused slots 0).
 */
#ifndef HJ_STOCH_H
#define HJ_STOCH_H
#include <stdint.h>
#include "hj_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJW_FORM_AUTO = 0, HJW_FORM_GENERAL = 1, HJW_FORM_DIAGONAL = 2 };

/* termSum's stepBound of the two terms: inv = 0; inv += 1 / sb_LF; inv += 1 / sb_TH; sb = 1 / inv, with
 *     sb_LF   the value hj_static_step_bound / hjb_step_bounds give: 1 / sum_d max_x alpha_d(x) / dx_d
 *     sb_TH   termTraceHessian's for L = sigma^T, R = sigma: 1 / (2 |trace((L D) R)|), D[m][k] = 1 / (dx_m dx_k); inf when 0
 * keys: HJ_MAX_DIM 64-bit words of device scratch.  sb_host[0] = sb, [1] = sb_LF, [2] = sb_TH.  The call waits for `stream`. */
int hjw_step_bound(const hjq_grid* g, const hjb_tables* tab, int ham, const double* params_host, const double* sigma_host,
                   void* keys, double* sb_host, void* stream);

/* One stage (HJ_STAGE_*, HJ_STAGE_YDOT included).  entry_host: the stage's arrays, dt and post-step operators as hjb_entry
 * describes them (`active` is not read; with HJ_STAGE_YDOT no operator is applied).  dst must alias none of the arrays read.
 * restrict_sign as hj_rk_substep: it clamps the Lax-Friedrichs term only, as termRestrictUpdate inside termSum does.
 * Asynchronous on `stream`. */
int hjw_substep(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int stage, int restrict_sign,
                const double* params_host, const double* sigma_host, int form, const hjb_entry* entry_host, void* stream);

/* hjb_plan for one problem: the schedule of one interval on the host, launching nothing. */
int hjw_plan(int order, double sb, double t0, double tf, double factor_cfl, double max_step, double stop_tol,
             double* t_host, int64_t* steps_host);

/* A whole interval: the steps hjw_plan gives for `sb` (hjw_step_bound's), order x steps launches enqueued on `stream` without
 * a host wait between them (or before them: a stage's arrays and dt ride in its launch arguments).  problem_host as
 * hjb_integrate takes it; post_prev (HJ_POST_*) and the problem's array operators are applied by the last stage of every step.
 * *result_in_host: where the result is -- 0: y_in (no step), 1: buf_a, 2: buf_b. */
int hjw_integrate(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int order, int restrict_sign, int post_prev,
                  const double* params_host, const double* sigma_host, int form, double sb, const hjb_problem* problem_host,
                  double t0, double tf, double factor_cfl, double max_step, double stop_tol, double* t_host,
                  int64_t* steps_host, int32_t* result_in_host, void* stream);

const char* hjw_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g.
 * "stoch_substep_kernel<double, HamDubinsRel, 3, 0>" (element type, system, scheme, DIAG) */
const char* hjw_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
