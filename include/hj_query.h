/* libhj_query.so: value-function queries at states (gfx950).
 *
 * What a caller does with a stored value function after the solve: V and grad V at many states, min / max
 * projections.  The entry points are stateless -- no hj_ctx: a plain grid descriptor and a HIP stream per call.
 * Every array pointer is DEVICE memory owned by the caller; inputs are never written.  Calls are asynchronous on
 * `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h;
 * hjq_last_error() holds the text.
 *
 * Interpolation semantics (all three point kernels): multilinear on the 2^ndim corner nodes of the cell that
 * holds the state.
 *   periodic axis      x is wrapped into [xmin, xmin + N dx); cell index clamped to N-1; upper corner taken mod N
 *   extrapolated axis  x < xmin or x > xlast gives NaN; cell index clamped to N-2 (the last node is inside)
 *   weights            w = (x - (xmin + i dx)) / dx in fp64
 *   sum                corners in ascending corner number (bit d selects the upper node of axis d), weight = product
 *                      over d in axis order, corners of weight exactly 0 skipped, fp64 accumulation with a separate
 *                      multiply and add, one rounding to the output type.
 */
#ifndef HJ_QUERY_H
#define HJ_QUERY_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else                                  /* hipRTC (hjp_plant_register) has no system headers; hj_mi355x.h brings int64_t */
typedef signed int int32_t;
#endif
#include "hj_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hjq_grid {
    int32_t ndim;                      /* 1 .. HJ_MAX_DIM */
    int32_t dtype;                     /* HJ_F64 | HJ_F32: element type of the value arrays */
    int64_t N[HJ_MAX_DIM];             /* nodes per axis, row-major arrays (last axis fastest) */
    double xmin[HJ_MAX_DIM];           /* first node  (grid.vs[d][0])  */
    double xlast[HJ_MAX_DIM];          /* last node   (grid.vs[d][-1]): the upper limit of an extrapolated axis */
    double dx[HJ_MAX_DIM];
    int32_t bc[HJ_MAX_DIM];            /* HJ_BC_EXTRAPOLATE | HJ_BC_PERIODIC */
    int32_t toward_zero[HJ_MAX_DIM];   /* addGhostExtrapolate's towardZero (costates only) */
} hjq_grid;

enum { HJQ_MIN = 0, HJQ_MAX = 1 };

/* V at states.  data: nfields value functions on one grid, field f at data + f*field_stride elements.
 * xs: nstates x ndim fp64, row-major.  out: nfields x nstates, state index fastest; element type of the grid, or
 * fp64 when out_f64 is nonzero (the unrounded sum). */
int hjq_interp_points(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride,
                      const double* xs, int64_t nstates, void* out, int out_f64, void* stream);

/* grad V at states without full-grid derivative arrays: at each of the 2^ndim corner nodes the 7-point stencil of
 * every axis is gathered (ghost values as the solver's), upwind<scheme> gives L and R, the corner costate is
 * 0.5 (L + R), and the corners are interpolated as above.  scheme: HJ_ENO2 | HJ_ENO3 | HJ_WENO5_ASSHIPPED
 * (HJ_EUNSUPPORTED otherwise: the intended WENO5 needs a grid-wide epsilon).  Non-finite data as computeGradients:
 * a stencil entry that is NaN / +-inf is read as 1e6; a corner node that is NaN / +-inf itself contributes NaN / +inf.
 * costate: nfields x nstates x ndim.  derivL / derivR (same shape) and value (nfields x nstates) may be null. */
int hjq_costate_points(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride,
                       const double* xs, int64_t nstates, void* costate, void* derivL, void* derivR, void* value,
                       int out_f64, void* stream);

/* min or max over the axes whose bit is set in remove_mask (bit d = axis d; a non-empty proper subset).
 * out: nfields x (kept axes in order), contiguous.  Any NaN in a reduced set gives NaN (np.amin / np.amax). */
int hjq_project_minmax(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride,
                       unsigned remove_mask, int op, void* out, void* stream);

const char* hjq_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g. "costate_points_kernel<double, 1>" */
const char* hjq_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
