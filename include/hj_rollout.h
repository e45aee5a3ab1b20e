/* libhj_rollout.so: many optimal trajectories through a stored value function in one launch (gfx950).
 *
 * computeOptTraj for M initial states at once: every trajectory stays on the device from its first state to its
 * last.  The entry point is stateless -- no hj_ctx: the grid descriptor of hj_query.h and a HIP stream per call.
 * Every array pointer is DEVICE memory owned by the caller; inputs are never written.  The call is asynchronous on
 * `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h;
 * hjr_last_error() holds the text.  A call that returns an error has launched nothing and touched no output.
 *
 * Per trajectory, with T = ntimes, the state x (fp64) and tE = 0 at the start:
 *     for it = 0 .. T-2:
 *         tE = the index the bisection over [tE, T-1] settles on: lower = tE, upper = T-1;
 *              while upper > lower: mid = (upper + lower + 1) / 2; V[mid](x) < 1e-4 ? lower = mid : upper = mid - 1
 *              (V[mid](x) as hjq_interp_points gives it in fp64; NaN compares false)
 *         if tE == T-1: stop (the state is inside the last stored set, the target)
 *         sub_samples times: p = grad V[tE](x) as hjq_costate_points gives it in fp64 (NaN outside the grid);
 *                            u, d = the plant's optimal control and disturbance for p at x; x = RK4(x, dt_small; u, d held)
 *         column it+1 of traj = x
 * The state, the weights, the controls and the dynamics are fp64, every operation rounded on its own; the stencil
 * arithmetic of the costate runs in the data's type.  A state outside an extrapolated axis, or not finite, has NaN
 * costates, hence NaN controls and NaN states from then on: it runs to full length.
 *
 * sgn(s) is +1 for s >= 0, -1 for s < 0, NaN for NaN.  RK4 with f(x) = f(x; u, d), h = 0.5 dt:
 *     k1 = f(x); k2 = f(x + h k1); k3 = f(x + h k2); k4 = f(x + dt k3); x + (dt / 6) (((k1 + 2 k2) + 2 k3) + k4)
 *
 * Plants (id as hj_mi355x.h's Hamiltonians, params as the Python classes' native() returns them):
 *   HJ_HAM_DUBINS_REL {v_e, v_p, w, .}     f = ((-v_e + v_p cos x3) + a x2,  v_p sin x3 - a x1,  b - a)
 *                                          a = w sgn((p1 x2 - p2 x1) - p3) for u_mode max, negated for min
 *                                          b = -w sgn(p3) for d_mode min, negated for max
 *   HJ_HAM_DOUBLE_INTEGRATOR {u_bound}     f = (x2, u);  u = -u_bound sgn(p2) for min, negated for max
 *   HJ_HAM_DOUBLE_PENDULUM {u_max}         f = drift(x) + (0, u1, 0, u2);  u_i = u_max sgn(p_i) for max, negated for min
 *                                          (p_i the costates of the two angular velocities; drift as DoublePendulum4D._drift)
 */
#ifndef HJ_ROLLOUT_H
#define HJ_ROLLOUT_H
#ifndef __HIPCC_RTC__                  /* hipRTC (hjp_plant_register) has no system headers */
#include <stdint.h>
#endif
#include "hj_query.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJR_MODE_MIN = 0, HJR_MODE_MAX = 1 };
/* status of a trajectory.  HJR_LEFT_GRID: one of its recorded states is outside an extrapolated axis or not finite */
enum { HJR_REACHED = 0, HJR_EXHAUSTED = 1, HJR_LEFT_GRID = 2 };

typedef struct hjr_plant {
    int32_t id;                        /* HJ_HAM_DUBINS_REL | HJ_HAM_DOUBLE_INTEGRATOR | HJ_HAM_DOUBLE_PENDULUM */
    int32_t u_mode;                    /* HJR_MODE_MIN | HJR_MODE_MAX */
    int32_t d_mode;                    /* the same for the disturbance (read by HJ_HAM_DUBINS_REL only) */
    int32_t reserved;
    double params[4];
} hjr_plant;

/* data: ntimes value functions on grid g, time first, slice k at data + k*field_stride elements (element type
 * g->dtype), the sets shrinking along the time axis (index 0 the full horizon, the last index the target).
 * scheme: HJ_ENO2 | HJ_ENO3 | HJ_WENO5_ASSHIPPED (HJ_EUNSUPPORTED otherwise, as hjq_costate_points).
 * x0: nstates x ndim fp64, row-major.  dt_small: the caller's (tau[1] - tau[0]) / sub_samples.
 * traj: nstates x ndim x ntimes fp64; the columns past length[m] hold NaN.  length: nstates, the number of recorded
 * states (1 .. ntimes).  t_earliest (may be null): nstates x ntimes, entry it = the index the bisection at column it
 * settled on, -1 where none ran.  status: nstates, HJR_*.  Every element of every output is written.
 * nstates == 0 returns HJ_OK and launches nothing. */
int hjr_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride,
                const double* x0, int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant,
                double* traj, int32_t* length, int32_t* t_earliest, int32_t* status, void* stream);

const char* hjr_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g. "rollout_kernel<double, 1, 0>"
 * (element type, scheme, plant id) */
const char* hjr_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
