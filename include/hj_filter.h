/* libhj_filter.so: the least-restrictive safety filter -- filtered rollouts through a stored value function in one launch, and the
 * filter's decision at states (gfx950).
 *
 * A nominal controller runs while V(x) is on the safe side of `level` by more than `margin`; the value function's optimal control
 * takes over once the margin is used up.  The entry points are stateless -- no hj_ctx: the grid descriptor of hj_query.h and a HIP
 * stream per call.  Every array pointer is DEVICE memory owned by the caller; inputs are never written.  The calls are asynchronous
 * on `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjf_last_error() holds the
 * text.  A call that returns an error has launched nothing and touched no output.
 *
 * A filtered trajectory is the trajectory of hj_rollout.h (the same 2^ND lanes, the state in fp64, every operation rounded on its
 * own) that never stops early and chooses its held values (c0, c1) differently.  With T = ntimes and x = x0[m]:
 *     column 0 = x
 *     for it = 0 .. T-2:
 *         sl = HJF_SLICE_CLOCK ? it : slice
 *         for s = 0 .. sub_samples-1:
 *             v = V[sl](x);  p = grad V[sl](x)                     (hjq_interp_points' / hjq_costate_points' fp64 values)
 *             gap = u_mode == HJR_MODE_MAX ? v - level : level - v (one subtraction)
 *             gap_min = first evaluation ? gap : nmin(gap_min, gap)        (hj_mc.h's nmin: NaN if either is NaN)
 *             (c0, c1) = the plant's controls for p at x           (hj_rollout.h, u_mode / d_mode)
 *             act = !(gap > margin)                                (a NaN gap acts)
 *             if !act, for every held value that is a CONTROL of the plant (table below), j its index among the controls:
 *                 HJF_NOMINAL_TABLE:  c_j = u_nom[m][it][j]        (as given: keeping it inside the bounds the value function was
 *                                                                  solved for is the caller's)
 *                 HJF_NOMINAL_VALUE:  sn = nom_ntimes == 1 ? 0 : it;  q = grad Vn[sn](x);
 *                                     (n0, n1) = the plant's controls for q at x with u_mode = nom_u_mode;  c_j = n_j
 *             if HJF_DSTB_ZERO: every held value that is a DISTURBANCE = 0.0       (HJF_DSTB_WORST: left as computed)
 *             step = it sub_samples + s:  active[m][step] = act;  applied[m][step] = (c0, c1)
 *             x = RK4(x, dt_small; c0, c1 held)
 *         column it+1 = x
 *     sl = HJF_SLICE_CLOCK ? T-1 : slice;  v = V[sl](x);  gap as above;  gap_min = nmin(gap_min, gap);  value_end = v
 *
 *   plant                      controls   disturbance                              NU
 *   HJ_HAM_DUBINS_REL          c0         c1                                       1
 *   HJ_HAM_DOUBLE_INTEGRATOR   c0         none (c1 stays the plant's 0.0)          1
 *   HJ_HAM_DOUBLE_PENDULUM     c0, c1     none                                     2
 *
 * status: HJF_LEFT_GRID if one of the recorded states is outside an extrapolated axis or not finite (hj_rollout.h's rule; such a
 * state has a NaN gap, so the optimal controls act on NaN costates and every later state is NaN: no state between two columns
 * leaves the grid unrecorded); otherwise HJF_VIOLATED if !(gap_min > 0); otherwise HJF_SAFE.
 */
#ifndef HJ_FILTER_H
#define HJ_FILTER_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else                                  /* hipRTC has no system headers and declares the signed widths alone */
typedef __UINT8_TYPE__ uint8_t;
#endif
#include "hj_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJF_SAFE = 0, HJF_VIOLATED = 1, HJF_LEFT_GRID = 2 };
enum { HJF_NOMINAL_TABLE = 0, HJF_NOMINAL_VALUE = 1 };
enum { HJF_SLICE_CLOCK = 0, HJF_SLICE_STATIC = 1 };
enum { HJF_DSTB_WORST = 0, HJF_DSTB_ZERO = 1 };

/* g, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant: as hjr_rollout, with its checks in its order.
 * field_stride == 0 is legal with HJF_SLICE_STATIC only: one converged field serves every time stamp, and `slice` must then be 0.
 * slice_policy: HJF_SLICE_*; slice: the field HJF_SLICE_STATIC reads, 0 .. ntimes-1 (ignored by HJF_SLICE_CLOCK).
 * nominal: HJF_NOMINAL_*.  u_nom (HJF_NOMINAL_TABLE): nstates x (ntimes-1) x NU fp64.  nom_data (HJF_NOMINAL_VALUE): nom_ntimes (1 or
 * ntimes) value functions on grid g of g's element type, nom_field_stride elements apart (at least the grid where nom_ntimes > 1);
 * nom_u_mode: HJR_MODE_*.  level: finite.  margin: not NaN; +inf always acts, -inf never does.  dstb: HJF_DSTB_*.
 * Outputs, every element written:
 *   final nstates x ndim fp64: the last state;  gap_min, value_end nstates fp64;  interventions nstates int32: the number of
 *   sub-steps with act;  first_intervention nstates int32: the step index of the first of them, -1 if none;  length nstates int32:
 *   always ntimes;  status nstates int32: HJF_*;
 *   traj (may be null) nstates x ndim x ntimes fp64;  active (may be null) nstates x nsteps uint8;  applied (may be null) nstates x
 *   nsteps x 2 fp64, nsteps = (ntimes-1) sub_samples.
 * nstates * 2^ndim must be below 2^32 (HJ_EINVAL otherwise; the caller splits over states: the bits do not depend on the split).
 * nstates == 0 returns HJ_OK and launches nothing. */
int hjf_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant, int slice_policy, int64_t slice,
                int nominal, const double* u_nom, const void* nom_data, int64_t nom_ntimes, int64_t nom_field_stride,
                int nom_u_mode, double level, double margin, int dstb, double* final_state, double* gap_min, double* value_end,
                int32_t* interventions, int32_t* first_intervention, int32_t* length, int32_t* status, double* traj,
                uint8_t* active, double* applied, void* stream);

/* The decision of one sub-step at nstates states xs (nstates x ndim fp64), without the RK4 step: field `slice` of the stack
 * (nfields fields, field_stride apart; field_stride is not read where nfields == 1), the table nominal u_nom (nstates x NU fp64).
 * Outputs, every element written: applied nstates x 2 fp64, active nstates uint8, value nstates fp64 (v), gap nstates fp64,
 * costate (may be null) nstates x ndim fp64 (p).  The other arguments and the checks as hjf_rollout's. */
int hjf_decide(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice,
               const double* xs, int64_t nstates, const hjr_plant* plant, const double* u_nom, double level, double margin,
               int dstb, double* applied, uint8_t* active, double* value, double* gap, double* costate, void* stream);

const char* hjf_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g. "filtered_rollout_kernel<double, 1, 0>" or
 * "decide_points_kernel<float, 3, 2>" (element type, scheme, plant id) */
const char* hjf_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
