/* libhj_hishapes.so: implicit surface functions built on the device on grids of 1 to 6 dimensions (gfx950).
 *
 * Targets, obstacles and their set algebra -- what a solve starts from and is clamped against -- written once, straight
 * into device memory, from the grid's coordinate vectors alone (no dense coordinate arrays, no host pass, no copy).
 * The entry points are stateless -- no hj_ctx: the grid descriptor of hj_hidim.h, a program and a HIP stream per call.
 * Every array pointer is DEVICE memory owned by the caller; inputs are never written.  Calls are asynchronous on
 * `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjk_last_error()
 * holds the text.
 *
 * A SCENE is a postfix program of at most HJG_MAX_OPS instructions over an evaluation stack at most HJG_MAX_DEPTH deep
 * (the limits, instructions, opcodes and array slots of hj_shapes.h).  A leaf pushes one value per node, an operator
 * replaces the top one or two.  A leaf's parameters are `off` fp64 values into the row of its MEMBER in a K x P table:
 * one launch evaluates K scenes that differ only in their numbers and writes member k to out + k * total.
 *
 *   leaf        parameters at row[off ...]          value at node x
 *   SPHERE      c[ndim], r                          sqrt(sum_d (x_d - c_d)(x_d - c_d)) - r
 *   CYLINDER    c[ndim], r; arg = ignored-axes mask the same, over the axes whose bit is clear
 *   RECT        l[ndim], u[ndim]                    m = max(x_0 - u_0, l_0 - x_0); then per further axis
 *                                                   m = max(m, x_d - u_d); m = max(m, l_d - x_d).  Corners may be +-inf
 *   HALFSPACE   n[ndim], p[ndim]                    sum_d n_d (x_d - p_d); n is taken as given (a unit normal)
 *   ARRAY       none; arg = slot of arrays[]        the array's value at the node, fp32 widened
 *   SPHERE_OF   A[J][ndim] row-major, c[J], r;      a sphere in J linear images of the coordinates, 1 <= J <= 6:
 *               arg = J                             e_j = (((A_j0 x_0) + (A_j1 x_1)) + ... + (A_j,ndim-1 x_ndim-1)) - c_j, all
 *                                                   ndim terms taken (a zero coefficient is not skipped);
 *                                                   s = e_0 e_0, then s = s + e_j e_j; the value is sqrt(s) - r
 *   operator
 *   UNION       min(a, b)      INTERSECT  max(a, b)      DIFFERENCE  max(a, -b)      COMPLEMENT  -a
 *
 * All arithmetic is fp64 whatever the output type, every operation rounded on its own, sums left to right from the
 * first term; sqrt is correctly rounded.  min / max give NaN when either side is NaN (np.minimum / np.maximum).  x_d is
 * coord[d][i_d], the grid's own coordinate vector: periodic axes get plain coordinates.  An fp32 output is the fp64
 * result rounded once at the store.  The interpreter and the leaves hj_shapes.h has are ONE source with
 * libhj_shapes.so's (hj_shapes_dev.h): a program without SPHERE_OF gives the bits hjg_evaluate gives.
 *
 * flags[k] (int32, zeroed by the caller) receives the OR of what member k's STORED values showed: HJG_NEG a value < 0,
 * HJG_POS a value > 0, HJG_ZERO a zero or a NaN.  "No sign change on the grid" is flags[k] == HJG_NEG or == HJG_POS.
 *
 * INDEXING, and its limits.  The axes are split into a TAIL -- the longest suffix of axes whose product of extents stays
 * below 2^31 -- and the HEAD, the axes before it.  A workgroup owns 256 consecutive tail nodes of one head index; it takes
 * `chunks` = ceil(tail / 256) workgroups per head index, and blockIdx.x = head' * chunks + chunk is split in 32 bits.
 * One launch has fewer than 2^32 threads -- the runtime takes gridDim.x * blockDim.x modulo 2^32 and reports nothing, so a
 * larger launch would run a part of its threads only -- and so covers at most heads_per_launch = floor((2^24 - 1) / chunks)
 * head indices (a head index is at most 2^23 workgroups); a grid with more, every grid past 2^32 nodes among them, takes
 * further launches, each given the multi-index of its first head index by the host, to which the kernel adds head' by add
 * and carry.  A thread divides its own tail node through the tail axes.  No number the kernel divides exceeds 32 bits and it
 * divides by nothing: the host prepares one 64-bit reciprocal per axis, and a quotient is one multiply-high.  So a grid may
 * have up to 2^63 - 1 nodes, an axis up to 2^31 - 1; what is NOT done is to pack several head indices into one workgroup:
 * a grid whose last axis alone is short and whose last two axes together pass 2^31 runs workgroups that are mostly idle.
 * hjk_plan refuses what the grid check refuses (an axis of 2^31 nodes or more, more than 2^63 - 1 nodes) and nothing else.
 *
 * A TEST FACILITY: the plan's two limits can be lowered, so that a grid of a few thousand nodes takes the head axes' carry, the
 * 64-bit node of a head index and the walk over several launches, which otherwise need more than 2^31 nodes or 2^24 workgroups.
 * Two environment variables, decimal whole numbers, read once by every call of hjk_evaluate, hjk_plan and hjk_decode (a call's
 * plan, decode and launches see the same values):
 *   HJ_INDEX_TAIL_BELOW     the tail stays below this many nodes           (1 .. 2^31, unset: 2^31)
 *   HJ_INDEX_LAUNCH_BLOCKS  one launch has at most this many workgroups    (1 .. 2^24 - 1, unset: 2^24 - 1)
 * The grid's last axis is the tail's whatever the first says (a value at or below N[ndim - 1] counts as just above it), and a
 * launch holds one whole head index whatever the second says (a value below `chunks` counts as `chunks`).  Anything else -- 0, a
 * negative number, a number above the constant, text that is no number -- is refused with HJ_EINVAL, the variable named, before
 * anything is launched.  Unset, the plan is the one described above.  The kernels are the same either way: the limits change
 * kernel arguments and launch counts alone.
 */
#ifndef HJ_HISHAPES_H
#define HJ_HISHAPES_H
#include <stdint.h>
#include "hj_mi355x.h"
#include "hj_hidim.h"
#include "hj_shapes.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJK_MAX_DIM = 6 };
enum { HJG_SPHERE_OF = 10 };           /* the leaf libhj_shapes.so does not know: arg = J */

typedef struct hjk_program {           /* hjg_program with six coordinate tables */
    int32_t n_ops, n_arrays;
    hjg_op ops[HJG_MAX_OPS];
    hjg_array arrays[HJG_MAX_ARRAYS];
    const double* coord[6];            /* coord[d]: the N[d] fp64 node coordinates of axis d (grid.vs[d]) */
} hjk_program;

typedef struct hjk_launch_plan {
    int32_t first_tail;                /* axes first_tail .. ndim - 1 are the tail, 0 .. first_tail - 1 the head */
    int32_t member_launches;           /* ceil(K / 65535): gridDim.y ends at 65535 */
    int64_t total, tail, head;         /* nodes of the grid = head * tail */
    int64_t chunks;                    /* workgroups per head index: ceil(tail / 256) */
    int64_t heads_per_launch;          /* head indices of a full launch */
    int64_t launches;                  /* launches along the head, each repeated member_launches times */
    int64_t blocks_full, blocks_last;  /* gridDim.x of launches 0 .. launches - 2, and of the last one */
} hjk_launch_plan;

/* Evaluate K members of the scene on grid g (ndim 1 .. 6; only ndim, dtype and N are read).  g->dtype must be HJ_F64 or
 * HJ_F32 as in every descriptor, but it does not choose the output's element type: out_dtype does.  N[d] may be 0 (an empty grid).
 * params: K x P fp64, row-major (may be null when P == 0).  out: K x total elements of out_dtype.  flags: K int32.
 * The program is validated before anything is launched: opcodes, stack underflow / overflow, exactly one value left,
 * parameter offsets inside P, cylinder masks inside ndim, J of SPHERE_OF in 1 .. 6 and its J ndim + J + 1 values inside
 * P, array slots used and non-null, K >= 1.  K above 65535 is chunked.  K * total == 0 launches nothing. */
int hjk_evaluate(const hjh_grid* g, const hjk_program* program, const double* params, int64_t K, int64_t P,
                 void* out, int out_dtype, int32_t* flags, void* stream);

/* The launches hjk_evaluate would make for K members on grid g.  No device is touched.  An empty grid: all zero. */
int hjk_plan(const hjh_grid* g, int64_t K, hjk_launch_plan* plan);

/* A host run of the DEVICE decode function: the multi-index the kernel computes for flat node `node` (last axis
 * fastest), through the launch, workgroup and thread that own it.  idx[d] of d >= ndim is 0. */
int hjk_decode(const hjh_grid* g, int64_t node, int32_t idx[6]);

const char* hjk_last_error(void);
/* name of the kernel the calling thread's last successful launch ran: "hi_scene_kernel<double>" | "hi_scene_kernel<float>" */
const char* hjk_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
