/* libhj_hiquery.so: value-function queries and rollouts on 5-D and 6-D grids (gfx950).
 *
 * hj_query.h and hj_rollout.h stop at HJ_MAX_DIM = 4 axes.  This library is their entry points for grids of HJH_MIN_DIM ..
 * HJH_MAX_DIM axes, with the grid descriptor of hj_hidim.h (hjh_grid) -- what a caller does with the array hjh_integrate
 * leaves: V and grad V at many states, min / max projections, optimal trajectories.  The entry points are stateless -- no
 * hj_ctx: a descriptor and a HIP stream per call.  Every array pointer is DEVICE memory owned by the caller; inputs are
 * never written.  Calls are asynchronous on `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E*
 * code of hj_mi355x.h; hjx_last_error() holds the text.  A call that returns an error has launched nothing.  ndim outside
 * HJH_MIN_DIM .. HJH_MAX_DIM is HJ_EINVAL.  All index arithmetic is 64-bit.
 *
 * The semantics are, word for word, those of hj_query.h (interpolation: wrap on a periodic axis, NaN outside an extrapolated
 * one, corners in ascending corner number, corners of weight exactly 0 skipped, fp64 accumulation with a separate multiply
 * and add, one rounding to the output type) and of hj_rollout.h (the bisection over the stored sets, the costate, sgn, RK4),
 * at 5 and 6 axes: the device functions are the ones libhj_query.so and libhj_rollout.so compile (csrc/hj_query_dev.h,
 * csrc/hj_rollout_dev.h), instantiated at six axes.
 *
 * Plants of hjx_rollout (id as hj_hidim.h's systems; hjr_plant of hj_rollout.h, params as listed; sgn(0) = +1, sgn(NaN) = NaN):
 *   HJH_HAM_PLANE5D {a_max, alpha_max}          f = (x3 cos x2, x3 sin x2, x4, a, al)
 *                                               a = a_max sgn(p3), al = alpha_max sgn(p4) for u_mode max, both negated for min
 *                                               no disturbance (d_mode is checked, not read)
 *   HJH_HAM_DUBINS_PAIR6D {v_e, v_p, w_e, w_p}  f = (v_e cos x2, v_e sin x2, u, v_p cos x5, v_p sin x5, d)
 *                                               u = w_e sgn(p2) for u_mode max, negated for min
 *                                               d = w_p sgn(p5) for d_mode max, negated for min
 * (states and costates numbered from 0, as the Python classes Plane5D / DubinsPair6D number them.)
 */
#ifndef HJ_HIQUERY_H
#define HJ_HIQUERY_H
#include <stdint.h>
#include "hj_hidim.h"
#include "hj_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hjq_interp_points on an hjh_grid: one thread per (field, state).  out: nfields x nstates, state index fastest; element
 * type of the grid, or fp64 when out_f64 is nonzero (the unrounded sum). */
int hjx_interp_points(const hjh_grid* g, const void* data, int64_t nfields, int64_t field_stride,
                      const double* xs, int64_t nstates, void* out, int out_f64, void* stream);

/* hjq_costate_points on an hjh_grid: 2^ndim lanes per (field, state) -- 32 at 5-D, a whole wavefront at 6-D.
 * scheme: HJ_ENO2 | HJ_ENO3 | HJ_WENO5_ASSHIPPED (HJ_EUNSUPPORTED otherwise).  Non-finite data as hjq_costate_points.
 * costate: nfields x nstates x ndim.  derivL / derivR (same shape) and value (nfields x nstates) may be null. */
int hjx_costate_points(const hjh_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride,
                       const double* xs, int64_t nstates, void* costate, void* derivL, void* derivR, void* value,
                       int out_f64, void* stream);

/* hjq_project_minmax on an hjh_grid: min (HJQ_MIN) or max (HJQ_MAX) over the axes whose bit is set in remove_mask, a
 * non-empty proper subset.  out: nfields x (kept axes in order), contiguous.  Any NaN in a reduced set gives NaN. */
int hjx_project_minmax(const hjh_grid* g, const void* data, int64_t nfields, int64_t field_stride,
                       unsigned remove_mask, int op, void* out, void* stream);

/* hjr_rollout on an hjh_grid, for the two plants above.  plant->id: HJH_HAM_PLANE5D (5-D grids) | HJH_HAM_DUBINS_PAIR6D
 * (6-D grids); a plant on a grid of another dimension is HJ_EINVAL, any other id HJ_EUNSUPPORTED.  Arguments, outputs and
 * status codes as hjr_rollout.  nstates == 0 returns HJ_OK and launches nothing. */
int hjx_rollout(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride,
                const double* x0, int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant,
                double* traj, int32_t* length, int32_t* t_earliest, int32_t* status, void* stream);

const char* hjx_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g. "hi_costate_points_kernel<double, 6, 1>"
 * (element type, axes, scheme) or "hi_rollout_kernel<float, 0, 51>" (element type, scheme, plant id) */
const char* hjx_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
