/* libhj_ttr.so: time-to-reach functions (gfx950).
 *
 * For every node, the time at which the sublevel set {y <= level} first (or last) swept over it; +inf where it never
 * did.  The entry points are stateless -- no hj_ctx: plain pointers and a HIP stream per call.  Every array pointer
 * is DEVICE memory owned by the caller; inputs are never written.  Calls are asynchronous on `stream` (0: the null
 * stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjt_last_error() holds the text.
 *
 * dtype is the element type of the data (y, last_y, data): HJ_F64 | HJ_F32.  ttr is ALWAYS fp64 (times are fp64
 * everywhere).  n == 0 returns HJ_OK and launches nothing.  All index arithmetic is 64-bit.
 *
 * The recurrence of one step from (t_last, last_y) to (t, y), in fp64 (fp32 data widened first), every operation
 * rounded on its own, in this order:
 *     a = last_y - level;  b = y - level
 *     changed = (y <= level) && (last_y > level)          a NaN compares false: a NaN node never changes
 *     if (mode & HJT_FIRST) changed = changed && (ttr == +inf)
 *     tc = (mode & HJT_NO_INTERP) ? t : t_last - ((t - t_last) * a) / (b - a)
 *     if (changed) ttr = tc;   last_y = y
 * (changed implies b - a < 0: no division by zero is ever used.)  mode 0 is the toolbox's postTimestepTTR: every
 * inward crossing overwrites; HJT_FIRST keeps the earliest crossing (the minimum time to reach).
 */
#ifndef HJ_TTR_H
#define HJ_TTR_H
#include <stdint.h>
#include "hj_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJT_FIRST = 1, HJT_NO_INTERP = 2 };

/* ttr[i] = (y[i] <= level) ? t : +inf;  last_y[i] = y[i]. */
int hjt_ttr_init(int dtype, const void* y, int64_t n, double t, double level, double* ttr, void* last_y, void* stream);

/* One step of the recurrence, in place on ttr and last_y.  y and last_y must be different arrays. */
int hjt_ttr_update(int dtype, const void* y, int64_t n, double t, double t_last, double level, int mode,
                   double* ttr, void* last_y, void* stream);

/* hjt_ttr_init on slice 0, then hjt_ttr_update on slices 1 .. T-1, in ONE pass: slice k is data + k*field_stride
 * elements (field_stride >= n) at time tau_dev[k] (T fp64 values on the device, T >= 1).  Every value of the stack is
 * read once, ttr is written once. */
int hjt_ttr_from_stack(int dtype, const void* data, int64_t T, int64_t field_stride, int64_t n, const double* tau_dev,
                       double level, int mode, double* ttr, void* stream);

const char* hjt_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g. "ttr_from_stack_kernel<double>" */
const char* hjt_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
