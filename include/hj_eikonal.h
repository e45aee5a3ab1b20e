/* libhj_eikonal.so: signed distance and first-arrival time from a level set (gfx950).
 *
 * Solves |grad u| = 1 / speed outward from the interface {data == level} with Godunov's first-order upwind scheme
 * (a fast iterative method on tiles) and returns sign(data - level) * u.  The entry points are stateless -- no hj_ctx:
 * the grid descriptor of hj_query.h (ndim, N, dx and bc are read) and a HIP stream per call.  Every array pointer is
 * DEVICE memory owned by the caller; inputs are never written.  Return value: HJ_OK (0) or a negative HJ_E* code of
 * hj_mi355x.h; hje_last_error() holds the text.  hje_signed_distance waits for `stream` after every group of passes (its
 * loop reads a counter back), so it cannot be captured into a graph; its last kernel is asynchronous on `stream`.
 *
 * THE DISCRETE PROBLEM.  All arithmetic is fp64 whatever the data type (fp32 is widened first), every product, sum,
 * quotient and square root rounded on its own, in the order written here.
 *
 *   phi_i = data_i - level.  speed_i is speed[i], or speed_scalar when speed is null;  s_i = 1 / speed_i.
 *   Node i is a WALL if phi_i is NaN or if speed_i > 0 is false (zero, negative, NaN).  A wall is NaN in the output,
 *   is read as +inf by its neighbours and never makes a neighbour near.
 *
 * 1. Near set and frozen values.  A node that is no wall is NEAR if phi_i == 0, or if for some axis d and side the
 *    neighbour j exists (index +-1, wrapped on a periodic axis), is no wall, and (phi_i > 0) != (phi_j > 0).  For such a
 *    pair   t = (dx_d * |phi_i|) / |phi_i - phi_j|,   or t = dx_d / 2 when phi_i or phi_j is infinite;
 *    t_d is the smaller t of the two sides of axis d.  Over the axes that have a crossing, in axis order,
 *        q = t_d * t_d;  r = 1 / q;  S = S + r  (the first term starts S);      u_i = s_i / sqrt(S)
 *    and u_i = 0 where phi_i == 0.  Near nodes never change afterwards; every other node that is no wall starts at +inf.
 * 2. Update of a node that is neither near nor a wall.  a_d = min of the two neighbours' u along axis d (a neighbour
 *    outside a non-periodic axis, or a wall, counts as +inf), h_d = dx_d, w_d = 1 / (h_d * h_d).  Sort (a, h, w)
 *    ascending by a, ties in axis order; below the sorted entries are numbered 1 .. D.
 *        candidate_1 = a_1 + h_1 * s_i
 *        A = w_1;  B = 0;  Q = 0
 *        for k = 2 .. D:   b = a_k - a_1;  p = w_k * b;  A = A + w_k;  B = B + p;  Q = Q + p * b
 *                          C = Q - s_i * s_i
 *                          candidate_k = a_1 + (B + sqrt(B * B - A * C)) / A
 *    (the shift by a_1 is part of the rule: it makes the result independent of the order of updates).  candidate_k is
 *    looked at only if no earlier one was accepted.  It is accepted if it is <= a_{k+1}; candidate_D is accepted unless
 *    it is NaN; a NaN candidate is never accepted.  The new value is the accepted candidate if a_1 is finite and the
 *    candidate is <= band and < the old value; the old value otherwise.
 * 3. Result.  The fixed point of 2 (no node changes).  Then  v = min(u, band)  (+inf becomes band),
 *        out_i = NaN at a wall,  +v where phi_i > 0,  -v where phi_i < 0,  +0 where phi_i == 0,
 *    rounded once to the element type of `out`.  A member without an interface is +-inf (or +-band) everywhere.
 *
 * WORKSPACE (hje_workspace_size bytes, 8-byte aligned, contents unspecified on entry).  Its start is readable after
 * the call:  uint64 counters[8] at byte 0 -- [0] tile launches that did work, [1] tile launches that changed a value,
 * [2] 1 + the index of the last pass that changed a value;  then at byte 64, K int32 of sign flags, the OR over
 * member k's nodes that are no walls of HJE_NEG (phi < 0), HJE_POS (phi > 0), HJE_ZERO (phi == 0).  The fp64 work array
 * and the tile flags follow; `out` is never used as work space.
 */
#ifndef HJ_EIKONAL_H
#define HJ_EIKONAL_H
#include <stdint.h>
#include "hj_mi355x.h"
#include "hj_query.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJE_NEG = 1, HJE_POS = 2, HJE_ZERO = 4 };
enum { HJE_FLAGS_OFFSET = 64 };        /* byte offset of the sign flags in the workspace */

/* Bytes of workspace for K members on grid g. */
int hje_workspace_size(const hjq_grid* g, int64_t K, int64_t* bytes);

/* K members: member k reads data + k * field_stride elements (field_stride >= nodes) of g->dtype and writes
 * out + k * nodes elements of the same type.  speed: nodes fp64 values shared by the members, or null for speed_scalar.
 * band: > 0, +inf for none.  max_passes >= 1: the call fails with HJ_ESTATE when the last of them still changed a value.
 * passes_host (may be null): the number of passes up to and including the first that changed nothing.
 * K >= 1.  N[d] may be 0 (an empty grid): nothing is launched. */
int hje_signed_distance(const hjq_grid* g, const void* data, int64_t K, int64_t field_stride, double level, double band,
                        const double* speed, double speed_scalar, void* out, void* workspace, int64_t workspace_bytes,
                        int64_t max_passes, int64_t* passes_host, void* stream);

const char* hje_last_error(void);
/* names of the kernels the calling thread's last successful call launched, joined by ';', e.g.
 * "eikonal_init_kernel<double>;eikonal_tile_kernel<3>;eikonal_finish_kernel<double>" */
const char* hje_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
