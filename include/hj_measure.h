/* libhj_measure.so: the size of a sublevel set, the overlap of two and the box that holds one, on grids of 1 to 6 dimensions (gfx950).
 *
 * The set is that of the piecewise-linear interpolant on the Kuhn subdivision, the one hj_surface.h extracts a mesh of: inside a
 * simplex the volume of { phi <= level } has a closed, cancellation-free recursion, and its fraction is kept as an INTEGER (2^52 the
 * whole simplex).  Every sum is an integer sum, so a result does not depend on the order of summation and is compared with ==.
 * The entry points are stateless -- no hj_ctx: a grid descriptor of hj_hidim.h and a HIP stream per call.  Every array pointer is
 * DEVICE memory owned by the caller; inputs are never written.  hjv_measure is asynchronous on `stream` (0: the null stream) and
 * leaves its records in device memory.  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjv_last_error() holds the
 * text.  A call that returns HJ_EINVAL or HJ_EUNSUPPORTED has made no HIP call and written nothing.
 *
 * THE RULE, for one field `data` (tests/measure_ref.py restates it with NumPy and Python integers).
 *   GRID     D = 1 .. 6 axes, N[d] >= 2 nodes each, `level` finite.  Of the descriptor ndim, dtype, N and bc are read.
 *   CELLS    N[d] - 1 per extrapolated axis; N[d] per periodic axis, the last one from node N[d] - 1 to node 0 (a full period).
 *            A cell is named by its base node (the lower one on every axis).
 *   VALUES   f = (double)data[node] - level: fp32 data widened, then ONE fp64 subtraction.
 *   CORNERS  bit d of corner b selects the upper node of axis d.  SIMPLICES: the D! permutations p of (0 .. D-1) in lexicographic
 *            order, vertices v_0 = 0, v_k = v_{k-1} | 1 << p[k-1]: exactly hj_surface.h's.
 *   CLASS    invalid  some corner's f is NaN or +-inf        contributes nothing; counted
 *            full     no corner has f > 0                    contributes D! 2^52 (through the count)
 *            empty    no corner has f < 0                    contributes nothing
 *            cut      otherwise                              contributes the sum of its D! simplices' q
 *   SIMPLEX  q = simplex_q(f_0 .. f_D), the values at v_0 .. v_D.  m = the number of f > 0, k = the number of f < 0.
 *            m == 0: q = 2^52.  m > 0 and k == 0: q = 0.  Otherwise a[0..k) the negatives and b[0..m) the positives, both in path
 *            order (zeros belong to neither), F(i, m) = 1, F(k, j) = 0 and
 *                theta = (-a_i) / (b_j - a_i)        F(i, j) = (theta F(i, j+1)) + ((1 - theta) F(i+1, j))
 *            every operation rounded on its own, no contraction; q = min(2^52, (uint64) rint(F(0, 0) 2^52)).
 *   RECORD   HJV_RECORD_WORDS 64-bit words:
 *                [HJV_CELLS] [HJV_FULL] [HJV_CUT] [HJV_INVALID]   int64 counts of cells (empty = cells - full - cut - invalid)
 *                [HJV_QLO] [HJV_QHI]                              Q_cut, the sum of q over all simplices of all cut cells, 128 bits
 *                [HJV_INSIDE]                                     nodes with f <= 0 (-inf is inside, NaN is not)
 *                [HJV_NAN]                                        nodes whose f is NaN
 *                [HJV_LO + d] [HJV_HI + d]                        smallest / largest index along axis d of an inside node;
 *                                                                 N[d] and -1 when there is none (axes past ndim: 1 and -1)
 *            Q = full D! 2^52 + Q_cut, and the volume is (Q / (D! 2^52)) times the cell volume: the caller's arithmetic.
 *   COMPARE  with a second input b (either may be fp32 or fp64; one field of b may be broadcast over the fields of a), one pass
 *            reads each once and leaves four records per field: [HJV_SET_A] a, [HJV_SET_B] b, [HJV_SET_UNION] nmin(a, b),
 *            [HJV_SET_INTERSECTION] nmax(a, b) -- hj_shapes_dev.h's NaN-propagating minimum / maximum of the WIDENED values,
 *            taken before `level` is subtracted.  No temporary array exists.
 *
 * KERNELS.  measure_kernel<TA, TB, D, COMPARE>: a thread owns one node (the node statistics); where the node is a cell's base it
 * classifies the cell from its 2^D corners.  The cut cells of a workgroup are compacted by wave ballots into a list in LDS, their
 * corner values are gathered into LDS, and (cell, simplex) pairs are spread over the lanes, a lane unranking its permutation from
 * the simplex number: one cut 6-D cell is 720 lanes' worth of work, not one lane's.  Sums: wave ballots and shuffles, then one
 * integer atomic add per workgroup and counter into one of the workspace's slots; Q_cut is added low word first, the carry into the
 * high word from the value the atomic returns.  measure_fold_kernel adds the slots into the records.  No float atomic exists.
 *
 * INDEXING is hj_hishapes.h's, as in hj_resample.h: tail / head split of the axes, a workgroup owns 256 consecutive tail nodes of
 * one head index, blockIdx.x is split in 32 bits, one host-prepared reciprocal per axis and nothing divides.  blockIdx.y is the
 * field; more than 65535 fields take further launches inside the call.  Node offsets are 64-bit.
 *
 * A TEST FACILITY, hj_hishapes.h's: the environment variables HJ_INDEX_TAIL_BELOW (the tail stays below this many nodes, 1 .. 2^31)
 * and HJ_INDEX_LAUNCH_BLOCKS (workgroups of one launch at most, 1 .. 2^24 - 1) lower the plan's two limits so that small grids
 * take the head axes and several launches.  hjv_measure, hjv_workspace_size, hjv_plan and hjv_decode read them once per call (the
 * slots follow the plan: size the workspace under the values the measurement runs with); the grid's last axis stays in the tail
 * and a launch holds a whole head index whatever they say; a value outside its range is refused with HJ_EINVAL before anything is
 * launched (hjv_workspace_size: 0); unset, the plan is the one above.
 */
#ifndef HJ_MEASURE_H
#define HJ_MEASURE_H
#include <stdint.h>
#include "hj_mi355x.h"
#include "hj_hidim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJV_MAX_DIM = 6 };
enum { HJV_RECORD_WORDS = 20 };
enum { HJV_CELLS = 0, HJV_FULL = 1, HJV_CUT = 2, HJV_INVALID = 3, HJV_QLO = 4, HJV_QHI = 5, HJV_INSIDE = 6, HJV_NAN = 7, HJV_LO = 8, HJV_HI = 14 };
enum { HJV_SET_A = 0, HJV_SET_B = 1, HJV_SET_UNION = 2, HJV_SET_INTERSECTION = 3 };
enum { HJV_MAX_SLOTS = 32 };           /* partial sums per record in the workspace, at most */

typedef struct hjv_launch_plan {       /* hjm_launch_plan (hj_resample.h) over the grid's nodes, and the fields */
    int32_t first_tail;                /* axes first_tail .. ndim - 1 are the tail, 0 .. first_tail - 1 the head */
    int32_t field_launches;            /* ceil(nfields / 65535): gridDim.y ends at 65535 */
    int64_t nfields;
    int64_t total, tail, head;         /* nodes of the grid = head * tail */
    int64_t chunks;                    /* workgroups per head index: ceil(tail / 256) */
    int64_t heads_per_launch;          /* head indices of a full launch */
    int64_t launches;                  /* launches along the head, each repeated field_launches times */
    int64_t blocks_full, blocks_last;  /* gridDim.x of launches 0 .. launches - 2, and of the last one */
    int64_t slots;                     /* partial sums per record: the power of two >= min(HJV_MAX_SLOTS, workgroups per field) */
} hjv_launch_plan;

/* Measure the fields of `a` (b null), or compare them with those of `b`.
 *   g          ndim, N, bc are read; g->dtype is the element type of `a`
 *   a          nfields arrays of the grid's nodes, stride_a elements apart (>= the node count when nfields > 1); nfields <= 2^31 - 1
 *   b          null, or nfields_b (1: broadcast, or nfields) arrays of b_dtype (HJ_F64 | HJ_F32), stride_b elements apart
 *   records    nfields (b null) or nfields x 4 records of HJV_RECORD_WORDS words, written by the call
 *   workspace  hjv_workspace_size(g, nfields, b != null) bytes, zeroed by the call */
int hjv_measure(const hjh_grid* g, const void* a, int64_t nfields, int64_t stride_a, const void* b, int b_dtype, int64_t nfields_b,
                int64_t stride_b, double level, void* records, void* workspace, void* stream);

/* bytes of workspace: per record `slots` (hjv_plan) partial sums of HJV_RECORD_WORDS words.  0 for a grid or a field count
 * hjv_measure would refuse. */
int64_t hjv_workspace_size(const hjh_grid* g, int64_t nfields, int compare);

/* The launches hjv_measure would make.  No device is touched. */
int hjv_plan(const hjh_grid* g, int64_t nfields, hjv_launch_plan* plan);

/* A host run of the DEVICE decode function: the multi-index the kernel computes for flat node `node` of g (last axis fastest),
 * through the launch, workgroup and thread that own it.  idx[d] of d >= ndim is 0. */
int hjv_decode(const hjh_grid* g, int64_t node, int32_t idx[6]);

/* A host run of the DEVICE per-simplex function: *q = simplex_q(f[0] .. f[D]), D = 1 .. 6.  No device is needed. */
int hjv_simplex_q_host(int D, const double* f, uint64_t* q);

const char* hjv_last_error(void);
/* names of the kernels the calling thread's last successful call launched, joined by ';':
 * "measure_kernel<double, double, 3, 0>;measure_fold_kernel" (element types of a and b -- a's twice without b --, D, 1: compare) */
const char* hjv_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
