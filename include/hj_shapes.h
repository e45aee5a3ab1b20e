/* libhj_shapes.so: implicit surface functions built on the device (gfx950).
 *
 * Targets, obstacles and their set algebra -- what a solve starts from and is clamped against -- written once, straight
 * into device memory, from the grid's coordinate vectors alone (no dense coordinate arrays, no host pass, no copy).
 * The entry point is stateless -- no hj_ctx: the grid descriptor of hj_query.h, a program and a HIP stream per call.
 * Every array pointer is DEVICE memory owned by the caller; inputs are never written.  Calls are asynchronous on
 * `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h; hjg_last_error()
 * holds the text.
 *
 * A SCENE is a postfix program of at most HJG_MAX_OPS instructions over an evaluation stack at most HJG_MAX_DEPTH deep.
 * A leaf pushes one value per node, an operator replaces the top one or two.  A leaf's parameters are `off` fp64 values
 * into the row of its MEMBER in a K x P table: one launch evaluates K scenes that differ only in their numbers (a sweep
 * over radii, an obstacle that moves along the leading axis) and writes member k to out + k * total.
 *
 *   leaf        parameters at row[off ...]          value at node x
 *   SPHERE      c[ndim], r                          sqrt(sum_d (x_d - c_d)(x_d - c_d)) - r
 *   CYLINDER    c[ndim], r; arg = ignored-axes mask the same, over the axes whose bit is clear
 *   RECT        l[ndim], u[ndim]                    m = max(x_0 - u_0, l_0 - x_0); then per further axis
 *                                                   m = max(m, x_d - u_d); m = max(m, l_d - x_d).  Corners may be +-inf
 *   HALFSPACE   n[ndim], p[ndim]                    sum_d n_d (x_d - p_d); n is taken as given (a unit normal)
 *   ARRAY       none; arg = slot of arrays[]        the array's value at the node, fp32 widened
 *   operator
 *   UNION       min(a, b)      INTERSECT  max(a, b)      DIFFERENCE  max(a, -b)      COMPLEMENT  -a
 *
 * All arithmetic is fp64 whatever the output type, every operation rounded on its own, sums left to right from the
 * first term; sqrt is correctly rounded.  min / max give NaN when either side is NaN (np.minimum / np.maximum).  x_d is
 * coord[d][i_d], the grid's own coordinate vector: periodic axes get plain coordinates.  An fp32 output is the fp64
 * result rounded once at the store.
 *
 * flags[k] (int32, zeroed by the caller) receives the OR of what member k's STORED values showed: HJG_NEG a value < 0,
 * HJG_POS a value > 0, HJG_ZERO a zero or a NaN.  "No sign change on the grid" is flags[k] == HJG_NEG or == HJG_POS.
 */
#ifndef HJ_SHAPES_H
#define HJ_SHAPES_H
#include <stdint.h>
#include "hj_mi355x.h"
#include "hj_query.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJG_MAX_OPS = 64, HJG_MAX_DEPTH = 8, HJG_MAX_ARRAYS = 8 };
enum { HJG_SPHERE = 1, HJG_CYLINDER = 2, HJG_RECT = 3, HJG_HALFSPACE = 4, HJG_ARRAY = 5,
       HJG_UNION = 6, HJG_INTERSECT = 7, HJG_DIFFERENCE = 8, HJG_COMPLEMENT = 9 };
enum { HJG_NEG = 1, HJG_POS = 2, HJG_ZERO = 4 };

typedef struct hjg_op {
    int16_t code;                      /* HJG_SPHERE .. HJG_COMPLEMENT */
    int16_t arg;                       /* CYLINDER: mask of ignored axes (bit d = axis d); ARRAY: slot; otherwise 0 */
    int32_t off;                       /* leaves with parameters: first value in the member's row */
} hjg_op;

typedef struct hjg_array {
    const void* data;                  /* total elements, or K x total when per_member */
    int32_t dtype;                     /* HJ_F64 | HJ_F32 */
    int32_t per_member;                /* nonzero: member k reads data + k * total */
} hjg_array;

typedef struct hjg_program {
    int32_t n_ops, n_arrays;
    hjg_op ops[HJG_MAX_OPS];
    hjg_array arrays[HJG_MAX_ARRAYS];
    const double* coord[HJ_MAX_DIM];   /* coord[d]: the N[d] fp64 node coordinates of axis d (grid.vs[d]) */
} hjg_program;

/* Evaluate K members of the scene on grid g.  g->dtype must be HJ_F64 or HJ_F32 as in every descriptor, but it does not choose
 * the output's element type: out_dtype does.  N[d] may be 0 (an empty grid).
 * params: K x P fp64, row-major (may be null when P == 0).  out: K x total elements of out_dtype.  flags: K int32.
 * The program is validated before anything is launched: opcodes, stack underflow / overflow, exactly one value left,
 * parameter offsets inside P, cylinder masks inside ndim, array slots used and non-null, K >= 1.  K * total == 0
 * launches nothing. */
int hjg_evaluate(const hjq_grid* g, const hjg_program* program, const double* params, int64_t K, int64_t P,
                 void* out, int out_dtype, int32_t* flags, void* stream);

const char* hjg_last_error(void);
/* name of the kernel the calling thread's last successful launch ran: "scene_kernel<double>" | "scene_kernel<float>" */
const char* hjg_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
