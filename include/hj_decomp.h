/* libhj_decomp.so: decomposed value functions put back together on the device (gfx950).
 *
 * A system of ndim <= HJD_MAX_DIM state axes is solved as nsubs <= HJD_MAX_SUBS self-contained subsystems of at most
 * HJ_MAX_DIM axes each, every one on an ordinary grid of its own.  The full-dimensional value is
 *
 *     V(x) = op_s V_s(x[axis_s])        op = max (HJQ_MAX): the intersection of the back-projections
 *                                       op = min (HJQ_MIN): their union
 *
 * and this library evaluates it: on the nodes of a full grid (one streaming pass, every element stored once, no
 * intermediate array) or at arbitrary states (the full array never exists).  The entry points are stateless -- no hj_ctx:
 * a descriptor and a HIP stream per call.  Every array pointer is DEVICE memory owned by the caller unless stated
 * otherwise; inputs are never written.  Calls are asynchronous on `stream` (0: the null stream).  Return value: HJ_OK (0)
 * or a negative HJ_E* code of hj_mi355x.h; hjd_last_error() holds the text.
 *
 * Arithmetic, as hj_shapes.h: every subsystem value is widened to fp64; min / max give NaN when either side is NaN
 * (np.minimum / np.maximum); the fold runs left to right over s = 0 .. nsubs-1; an fp32 output is the fp64 result rounded
 * once at the store.  The ACTIVE subsystem of a node or state is the lowest s whose (widened) value equals the fp64
 * result, -1 where the result is NaN.
 *
 * Fields: every subsystem holds 1 or `nfields` value functions (a time stack), field f at data + f * field_stride
 * elements; a subsystem with one field is broadcast over the fields of the result.
 */
#ifndef HJ_DECOMP_H
#define HJ_DECOMP_H
#include <stdint.h>
#include "hj_mi355x.h"
#include "hj_query.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJD_MAX_DIM = 8, HJD_MAX_SUBS = 8 };

typedef struct hjd_sub {
    hjq_grid grid;                     /* the subsystem's own grid; grid.dtype is the element type of `data` */
    const void* data;                  /* nfields arrays of grid.N, row-major */
    int64_t nfields;                   /* 1, or the nfields of the call */
    int64_t field_stride;              /* elements from one field to the next */
    int32_t axis[HJ_MAX_DIM];          /* axis[k]: the full axis that axis k of `grid` stands for; distinct, any order */
} hjd_sub;

typedef struct hjd_decomp {
    int32_t ndim;                      /* axes of the full space, 1 .. HJD_MAX_DIM */
    int32_t nsubs;                     /* 1 .. HJD_MAX_SUBS */
    int32_t op;                        /* HJQ_MIN (union) | HJQ_MAX (intersection) */
    int32_t reserved;
    hjd_sub sub[HJD_MAX_SUBS];         /* a subsystem array holds at most 2^31 - 1 elements per field */
} hjd_decomp;

/* The conforming case: the full grid has N[a] nodes on axis a and N[axis_s[k]] == grid_s.N[k] for every subsystem and
 * axis, node for node.  A pure index gather, exact:
 *     out[f, i] = op_s data_s[f_s, sum_k i[axis_s[k]] * stride_s[k]]
 * N: ndim HOST values.  out: nfields x prod(N) elements of out_dtype (HJ_F64 | HJ_F32), row-major, last axis fastest.
 * active: int32 of the same shape, or null.  An axis no subsystem covers is a broadcast.  prod(N) == 0 launches nothing. */
int hjd_backproject_nodes(const hjd_decomp* decomp, const int64_t* N, int64_t nfields, void* out, int out_dtype,
                          int32_t* active, void* stream);

/* The general case: the full grid's nodes are coord[a][0 .. N[a]-1] (coord: ndim HOST pointers to DEVICE fp64 tables)
 * and the value at node i is op_s interp_s(x[axis_s]) with x_a = coord[a][i_a]; interp_s is the multilinear interpolant of
 * hj_query.h on the subsystem's grid (periodic axes wrap, NaN outside an extrapolated axis, the same corner order and
 * skipping of zero weights).  N[a] == 1 with a one-element table is a slice. */
int hjd_backproject_coords(const hjd_decomp* decomp, const int64_t* N, const double* const* coord, int64_t nfields,
                           void* out, int out_dtype, int32_t* active, void* stream);

/* V and the active subsystem at states.  xs: nstates x ndim fp64, row-major.  out: nfields x nstates, fp64 when out_f64
 * is nonzero, fp32 otherwise.  active: int32 of the same shape, or null.  A non-finite coordinate on a covered axis gives
 * NaN.  nstates == 0 launches nothing. */
int hjd_points(const hjd_decomp* decomp, const double* xs, int64_t nstates, int64_t nfields, void* out, int out_f64,
               int32_t* active, void* stream);

const char* hjd_last_error(void);
/* name of the kernel the calling thread's last successful launch ran: "backproject_nodes_kernel<double>" | "...<float>",
 * "backproject_coords_kernel<double>" | "...<float>", "decomp_points_kernel<double>" | "...<float>" */
const char* hjd_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
