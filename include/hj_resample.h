/* libhj_resample.so: value functions resampled across grids and frames on the device, on grids of 1 to 6 dimensions (gfx950).
 *
 * Every node of a DESTINATION grid takes the multilinear interpolant of a stored array on a SOURCE grid at an affine image of
 * its own coordinates: coarse-to-fine migration (the identity map), a shift, a rotation, and the union / intersection of one
 * function placed at K poses, folded in registers.  The destination is walked from its coordinate vectors alone: no dense
 * coordinate array exists.  The entry points are stateless -- no hj_ctx: two grid descriptors of hj_hidim.h and a HIP stream
 * per call.  Every array pointer is DEVICE memory owned by the caller; inputs are never written.  Calls are asynchronous on
 * `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjm_last_error() holds the
 * text.  A call that returns HJ_EINVAL or HJ_EUNSUPPORTED has made no HIP call.
 *
 * THE RULE.  All arithmetic is fp64 whatever the element types, every product and sum rounded on its own.  For the node with
 * multi-index (i_0 .. i_D-1) of the destination, member k (map A, b: row k of `maps`) and one field:
 *     x_d = coord[d][i_d]
 *     y_i = (((A_i0 x_0) + (A_i1 x_1)) + ... + (A_i,D-1 x_D-1)) + b_i       all D products taken, zero coefficients included
 *                                                                          (A = I, finite x: y = x + b exactly); null maps: y = x
 *     v_k = the interpolant of hj_query.h at y on the source grid (csrc/hj_query_dev.h: interp_value, the function
 *           hjq_interp_points and hjx_interp_points run): y wrapped by whole periods on periodic axes, corners in ascending
 *           number, corners of weight exactly 0 skipped, a multiply and an add per corner
 *     member k is OUTSIDE at the node when y lies outside an extrapolated axis of the source or is not finite.
 *   HJM_REDUCE_NONE   out[k][field][node] = v_k; the node is FILLED when member k is inside.
 *   HJM_REDUCE_MIN / HJM_REDUCE_MAX
 *                     out[field][node] = the fold, k ascending, over the members that are inside, by NumPy's minimum / maximum
 *                     (NaN on either side gives NaN): a NaN stored in the data propagates, an outside member is skipped.  The
 *                     node is FILLED when at least one member is inside.
 *   A node that is not filled takes HJM_FILL_NAN: NaN; HJM_FILL_VALUE: fill_value; HJM_FILL_MAX: the largest non-NaN value
 *   among the filled nodes of the same output array (an output array: one [k][field] or [field] slice of `out`), NaN when that
 *   array has no filled node or only NaN ones.  inside_counts[array] receives the number of filled nodes of every output array.
 *   An fp32 output is the fp64 result rounded once at the store (the maximum of HJM_FILL_MAX is taken in fp64).
 *
 * The counts are summed by a small launch of their own.  HJM_FILL_MAX takes a further launch on the same stream, which finds the unfilled nodes again from the geometry alone (the
 * data may hold NaN) and stores the maximum there; neither the maximum nor a count crosses to the host.  Every element of `out`
 * is stored exactly once.
 *
 * INDEXING is hj_hishapes.h's: the destination's axes are split into a tail (the longest suffix below 2^31 nodes) and a head, a
 * workgroup owns 256 consecutive tail nodes of one head index, blockIdx.x = head' * chunks + chunk is split in 32 bits, and the
 * kernel divides by nothing (one host-prepared 64-bit reciprocal per axis).  blockIdx.y is the output array; more than 65535
 * of them take further launches.  Source offsets are 64-bit.
 *
 * A TEST FACILITY, hj_hishapes.h's: the environment variables HJ_INDEX_TAIL_BELOW (the tail stays below this many nodes, 1 .. 2^31)
 * and HJ_INDEX_LAUNCH_BLOCKS (workgroups of one launch at most, 1 .. 2^24 - 1) lower the plan's two limits so that small
 * destinations take the head axes and several launches.  hjm_resample, hjm_plan and hjm_decode read them once per call; the
 * destination's last axis stays in the tail and a launch holds a whole head index whatever they say; a value outside its range is
 * refused with HJ_EINVAL before anything is launched; unset, the plan is the one above.
 */
#ifndef HJ_RESAMPLE_H
#define HJ_RESAMPLE_H
#include <stdint.h>
#include "hj_mi355x.h"
#include "hj_hidim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJM_MAX_DIM = 6 };
enum { HJM_REDUCE_NONE = 0, HJM_REDUCE_MIN = 1, HJM_REDUCE_MAX = 2 };
enum { HJM_FILL_NAN = 0, HJM_FILL_VALUE = 1, HJM_FILL_MAX = 2 };
enum { HJM_COUNT_SLOTS = 32 };          /* partial counts per output array in the workspace */

typedef struct hjm_launch_plan {       /* hjk_launch_plan over the destination's nodes, and the output arrays */
    int32_t first_tail;                /* axes first_tail .. ndim - 1 are the tail, 0 .. first_tail - 1 the head */
    int32_t array_launches;            /* ceil(arrays / 65535): gridDim.y ends at 65535 */
    int64_t arrays;                    /* output arrays: K * nfields (HJM_REDUCE_NONE) or nfields (a fold) */
    int64_t total, tail, head;         /* nodes of the destination = head * tail */
    int64_t chunks;                    /* workgroups per head index: ceil(tail / 256) */
    int64_t heads_per_launch;          /* head indices of a full launch */
    int64_t launches;                  /* launches along the head, each repeated array_launches times */
    int64_t blocks_full, blocks_last;  /* gridDim.x of launches 0 .. launches - 2, and of the last one */
} hjm_launch_plan;

/* Resample `data` from grid src onto grid dst (both of ndim D = 1 .. 6).
 *   src        N, xmin, xlast, dx, bc are read; src->dtype is the element type of `data`.  N[d] >= 2 on an extrapolated axis.
 *   dst        ndim and N (1 .. 2^31 - 1 per axis) are read
 *   coord      D device pointers in HOST memory: coord[d] = the N[d] fp64 node coordinates of the destination's axis d
 *   data       nfields arrays of src's nodes, field_stride elements apart (>= the source's node count when nfields > 1);
 *              nfields <= 2^31 - 1.  All fields share the maps
 *   maps       K x (D D + D) fp64, row-major A then b per row; null with K = 1: the identity
 *   out        K x nfields x dst nodes (HJM_REDUCE_NONE) or nfields x dst nodes (a fold) elements of out_dtype (HJ_F64 | HJ_F32)
 *   inside_counts  one int64 per output array, written by the call
 *   workspace  hjm_workspace_size(arrays) bytes, zeroed by the call
 * K x nfields above 65535 is chunked. */
int hjm_resample(const hjh_grid* src, const hjh_grid* dst, const double* const* coord, const void* data, int64_t nfields,
                 int64_t field_stride, const double* maps, int64_t K, int reduce, int fill_mode, double fill_value, void* out,
                 int out_dtype, int64_t* inside_counts, void* workspace, void* stream);

/* bytes of workspace for `arrays` output arrays: one order-preserving 64-bit key of the running maximum each, then
 * HJM_COUNT_SLOTS partial counts of filled nodes each (the waves of a launch add to different ones; a last small launch adds them) */
int64_t hjm_workspace_size(int64_t arrays);

/* The launches hjm_resample would make onto grid dst.  No device is touched. */
int hjm_plan(const hjh_grid* dst, int64_t nfields, int64_t K, int reduce, hjm_launch_plan* plan);

/* A host run of the DEVICE decode function: the multi-index the kernel computes for flat node `node` of dst (last axis
 * fastest), through the launch, workgroup and thread that own it.  idx[d] of d >= ndim is 0. */
int hjm_decode(const hjh_grid* dst, int64_t node, int32_t idx[6]);

const char* hjm_last_error(void);
/* names of the kernels the calling thread's last successful call launched, joined by ';':
 * "resample_kernel<double, 3, 0>;resample_counts_kernel" (element type of the data, D, reduce) [";resample_fill_kernel<3, 0>" (D, 1 with a fold)] */
const char* hjm_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
