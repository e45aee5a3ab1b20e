/* libhj_batch.so: many Hamilton-Jacobi problems on one grid, advanced together (gfx950).
 *
 * B value functions on the same grid, each with its own Hamiltonian parameters, time step and post-step operators:
 * every Runge-Kutta stage is ONE launch of batch_substep_kernel for all of them (gridDim.y = the problem).  The entry
 * points are stateless -- no hj_ctx: the grid descriptor of hj_query.h, the grid's coordinate tables and a HIP stream
 * per call.  Every array pointer is DEVICE memory owned by the caller unless it is called *_host; inputs are never
 * written.  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjb_last_error() holds the text.  A call
 * that returns HJ_EINVAL / HJ_EUNSUPPORTED has launched nothing.  All index arithmetic is 64-bit.
 *
 * A problem's substep is the solver's: one thread per cell, the cell's stencils gathered straight from global memory
 * (ghost cells as hj_mi355x.h describes them), upwind derivatives of `scheme`, the Lax-Friedrichs term of the built-in
 * system `ham` with global dissipation, the stage expression of HJ_STAGE_*.  The device functions are the ones
 * libhj_mi355x.so compiles (csrc/hj_device.h, csrc/hj_split.h), so a problem's result has the bits hj_rk_substep /
 * hj_rk_integrate give for it alone.
 *     scheme   HJ_ENO2 | HJ_ENO3 | HJ_WENO5_ASSHIPPED   (HJ_EUNSUPPORTED otherwise: the intended WENO5's epsilon is a
 *              reduction over each problem's whole grid)
 *     ham      HJ_HAM_DUBINS_REL (3-D) | HJ_HAM_DOUBLE_INTEGRATOR (2-D) | HJ_HAM_DOUBLE_PENDULUM (4-D)
 *     dtype    g->dtype, HJ_F64 | HJ_F32: the element type of every state array and of the tables
 *
 * params: B x HJB_PAR_SLOTS fp64 on the device, row b the parameters of problem b as hj_mi355x.h lists them for `ham`
 * (unused slots 0); rounded to the grid's dtype where they are used (once each); an entry's dt is converted once, (float)dt.
 * The HJ_F32 rounding points are the solver's (hj_mi355x.h, "what an HJ_F32 context computes").
 *
 * A problem whose entry has active == 0 costs nothing: its workgroups return before they read or write anything of it.
 */
#ifndef HJ_BATCH_H
#define HJ_BATCH_H
#include <stdint.h>
#include "hj_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HJB_PAR_SLOTS 8

/* what the problems share besides the grid: 1-D tables of the grid's dtype */
typedef struct hjb_tables {
    const void* coord[HJ_MAX_DIM];     /* grid.vs[d]: N[d] values */
    const void* aux[4];                /* the tables of `ham` (hj_mi355x.h, HJ_HAM_*): cos / sin of vs[2] (Dubins), sin / cos of
                                          vs[0] and of vs[2] (pendulum); null where the system reads none */
} hjb_tables;

/* post-step operators against arrays, as hj_ctx_set_post_arrays numbers them */
enum { HJB_ARR_NONE = 0, HJB_ARR_MIN = 1, HJB_ARR_MAX = 2, HJB_ARR_MAX_NEG = 3 /* max(y, -array): obstacle mask */ };

/* one problem's share of one launch (64 bytes).  After the stage expression the kernel applies, in this order:
 * post_prev (HJ_POST_MIN_PREV / HJ_POST_MAX_PREV: min / max with y0 where the stage reads y0, with src otherwise),
 * then op_a against post_a, then op_b against post_b -- NaN propagating as NumPy's minimum / maximum. */
typedef struct hjb_entry {
    const void* src;                   /* the stage's stencil input */
    const void* y0;                    /* the state the step started from (stages RK3_HALF, RK3_FULL, RK2_FULL), else unused */
    void* dst;                         /* the stage's output; must not alias src */
    const void* post_a;                /* arrays of the post-step operators, or null */
    const void* post_b;
    double dt;
    int32_t active;                    /* 0: the problem sits this launch out */
    int32_t post_prev;                 /* HJ_POST_* */
    int32_t op_a, op_b;                /* HJB_ARR_* */
} hjb_entry;

/* the buffers of one problem for hjb_integrate, as hj_rk_integrate takes them: y_in is never written; buf_a, buf_b and
 * work (orders 2 and 3) are distinct arrays of the grid's size */
typedef struct hjb_problem {
    const void* y_in;
    void* buf_a;
    void* buf_b;
    void* work;
    const void* post_a;                /* applied after every step, as hjb_entry describes */
    const void* post_b;
    int32_t op_a, op_b;
} hjb_problem;

/* stepBound of every problem: 1 / sum_d max_x alpha_d(x) / dx_d with the system's alpha at zero costate (it ignores the
 * data), the value hj_static_step_bound gives.  keys: B x HJ_MAX_DIM 64-bit words of device scratch.  sb_host: B values;
 * amax_host (may be null): B x HJ_MAX_DIM, the per-dimension maxima.  The call waits for `stream`. */
int hjb_step_bounds(const hjq_grid* g, const hjb_tables* tab, int ham, const double* params, int64_t B,
                    void* keys, double* sb_host, double* amax_host, void* stream);

/* one stage (HJ_STAGE_*, HJ_STAGE_YDOT included) for B problems: problem b reads entries[b].  restrict_sign as
 * hj_rk_substep.  Asynchronous on `stream`.  B above the grid-dimension limit of a launch (65535) is chunked inside. */
int hjb_substep(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int stage, int restrict_sign,
                const double* params, const hjb_entry* entries, int64_t B, void* stream);

/* The schedule of one interval, on the host, launching nothing: problem b steps from t0 while
 *     stop_tol < 0:  tf - t >= 100 eps |tf|     (the integrators' own test)
 *     stop_tol >= 0: t < tf - stop_tol          (HJIPDE_solve's)
 * with deltaT = min(factor_cfl * sb_host[b], tf - t, max_step) and the time expressions of odeCFL1/2/3, as
 * hj_rk_integrate.  t_host[b] / steps_host[b]: the time reached and the number of steps.  HJ_ESTATE when a step does
 * not advance the time. */
int hjb_plan(int order, const double* sb_host, int64_t B, double t0, double tf, double factor_cfl, double max_step,
             double stop_tol, double* t_host, int64_t* steps_host);

/* A whole interval for B problems: hj_rk_integrate (order 1..3) for each, the stages of all problems sharing launches.
 * The schedule is known before the first launch (alpha ignores the data): the call writes the entries of every (step,
 * stage, problem) into `table` with one copy, waits for `stream` once, then enqueues order x max_b steps[b] launches
 * and returns.  A problem that has reached tf is inactive in the remaining launches.  post_prev (HJ_POST_*) and the
 * problems' array operators are applied by the last stage of every step.
 * table: device scratch of table_bytes >= order * max_b steps[b] * B * sizeof(hjb_entry) (hjb_plan gives steps).
 * t_host / steps_host: as hjb_plan.  result_in_host[b]: where problem b's result is -- 0: y_in (no step), 1: buf_a,
 * 2: buf_b. */
int hjb_integrate(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int order, int restrict_sign,
                  int post_prev, const double* params, const double* sb_host, const hjb_problem* problems_host,
                  int64_t B, double t0, double tf, double factor_cfl, double max_step, double stop_tol,
                  void* table, int64_t table_bytes, double* t_host, int64_t* steps_host, int32_t* result_in_host,
                  void* stream);

/* flags[b] = 1 if entries[b].src holds a NaN among its first n elements, else 0 (inactive entries: 0).  Asynchronous. */
int hjb_nan_flags(int dtype, const hjb_entry* entries, int64_t B, int64_t n, int32_t* flags, void* stream);

const char* hjb_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g.
 * "batch_substep_kernel<double, HamDubinsRel, 3>" (element type, system, scheme) */
const char* hjb_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
