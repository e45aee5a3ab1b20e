// A scene (include/hj_shapes.h, include/hj_hishapes.h) as libhj_shapes.so (hj_shapes.hip, MD = 4 axes) and libhj_hishapes.so
// (hj_hishapes.hip, MD = 6) evaluate it: the leaves and the two folds, the postfix interpreter (run_program), the store with the sign-flag
// vote (store_and_vote) and, at the end, the host side the two libraries share -- the descriptor's and the program's checks, the entry
// point up to its launch, the member-chunk loop.  ONE source, so a program gives the same bits in either library.
// Every leaf is written one operation per statement with contraction off: the results are NumPy's, bit for bit.
#ifndef HJ_SHAPES_DEV_H
#define HJ_SHAPES_DEV_H
#include <hip/hip_runtime.h>
#include "../../include/hj_hishapes.h"      // HJG_SPHERE_OF and hjk_program; it includes hj_shapes.h

namespace hjg_dev {

// NaN on either side gives NaN, as np.minimum / np.maximum (and array_op of hj_stage_dev.h)
__device__ __forceinline__ double nmin(double a, double b) {
    double r;
    if (a != a) r = a;
    else if (b != b) r = b;
    else r = a < b ? a : b;
    return r;
}

__device__ __forceinline__ double nmax(double a, double b) {
    double r;
    if (a != a) r = a;
    else if (b != b) r = b;
    else r = a > b ? a : b;
    return r;
}

// sqrt(sum over the axes not in `ignore` of (x_d - c_d)(x_d - c_d)) - r;  p = c[ndim], r
template <int MD>
__device__ __forceinline__ double ball(const double (&x)[MD], int ndim, int ignore, const double* __restrict__ p) {
#pragma clang fp contract(off)
    double s = 0.0;                     // 0 + first term is the first term: the terms are squares
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        if (d < ndim && !((ignore >> d) & 1)) {
            const double e = x[d] - p[d];
            const double q = e * e;
            s = s + q;
        }
    }
    const double root = __builtin_sqrt(s);
    return root - p[ndim];
}

// p = l[ndim], u[ndim]
template <int MD>
__device__ __forceinline__ double rect(const double (&x)[MD], int ndim, const double* __restrict__ p) {
#pragma clang fp contract(off)
    const double a0 = x[0] - p[ndim];
    const double b0 = p[0] - x[0];
    double m = nmax(a0, b0);
#pragma unroll
    for (int d = 1; d < MD; ++d) {
        if (d < ndim) {
            const double a = x[d] - p[ndim + d];
            m = nmax(m, a);
            const double b = p[d] - x[d];
            m = nmax(m, b);
        }
    }
    return m;
}

// p = n[ndim], point[ndim]
template <int MD>
__device__ __forceinline__ double halfspace(const double (&x)[MD], int ndim, const double* __restrict__ p) {
#pragma clang fp contract(off)
    const double e0 = x[0] - p[ndim];
    double s = p[0] * e0;
#pragma unroll
    for (int d = 1; d < MD; ++d) {
        if (d < ndim) {
            const double e = x[d] - p[ndim + d];
            const double q = p[d] * e;
            s = s + q;
        }
    }
    return s;
}

// a sphere in J linear images of the coordinates;  p = A[J][ndim] row-major, c[J], r.  Every image takes all ndim terms, left to
// right from the first; the squares are summed from the first image on
template <int MD>
__device__ __forceinline__ double ball_of(const double (&x)[MD], int ndim, int J, const double* __restrict__ p) {
#pragma clang fp contract(off)
    const double* __restrict__ c = p + J * ndim;
    double s = 0.0;
    for (int j = 0; j < J; ++j) {
        const double* __restrict__ a = p + j * ndim;
        double e = a[0] * x[0];
#pragma unroll
        for (int d = 1; d < MD; ++d) {
            if (d < ndim) {
                const double q = a[d] * x[d];
                e = e + q;
            }
        }
        e = e - c[j];
        const double q = e * e;
        s = j == 0 ? q : s + q;
    }
    const double root = __builtin_sqrt(s);
    return root - c[J];
}

// ---- the interpreter: the body of scene_kernel (hj_shapes.hip) and hi_scene_kernel (hj_hishapes.hip), which decode the node,
// fill x[] and store.  A thread owns one node of one member and runs the postfix program on it; no intermediate array exists in
// global memory.
// The program rides in the kernel arguments and the member's parameter row is read through blockIdx.y: opcodes, offsets and
// parameters are wave-uniform, so the interpreter's branches never diverge and its parameter reads are scalar loads.
// The evaluation stack: the top value in a register, the values below it in LDS, one column per thread ([depth - 1][256]
// doubles, 14 KB; each kernel declares its own).  A stack indexed at run time in registers goes to scratch; the LDS column is
// indexed by the uniform stack pointer, costs one ds access per instruction of the program, and needs no barrier (a thread reads
// only what it wrote).
// The kernels' stores are ONE element per lane, neighbouring lanes on neighbouring elements: a wave-instruction covers 512
// contiguous bytes of fp64 whatever the alignment -- with an odd node count every second member starts off 16-byte alignment, and
// callers pass views at any element offset, so nothing there is wider than an element and no head or tail needs peeling.
// ARGS: the kernel's argument struct (SceneArgs, HiArgs), of which prog (hjg_program or hjk_program) and ndim are read.  row: the
// member's parameters (the kernel's `__restrict__` is not repeated here).  base: the member's first element, member x nodes -- of
// the output and of a per-member array leaf; the kernel forms it once.  OF: whether HJG_SPHERE_OF is a leaf (libhj_hishapes.so only).
constexpr int SCENE_BLOCK = 256;
using Below = double[HJG_MAX_DEPTH - 1][SCENE_BLOCK];   // the stack under its top value, one column per thread

template <bool OF, typename ARGS, int MD>
__device__ __forceinline__ double run_program(const ARGS& A, const double (&x)[MD], const double* row, long long base, long long node,
                                              Below& below, int tid) {
    const auto& prog = A.prog;
    const int ndim = A.ndim;
    double top = 0.0;
    int sp = 0;                                                  // values on the stack, the one in `top` included
    for (int i = 0; i < prog.n_ops; ++i) {
        const hjg_op op = prog.ops[i];
        if (op.code <= HJG_ARRAY || (OF && op.code == HJG_SPHERE_OF)) {      // a leaf: the old top goes under the new one
            if (sp > 0) below[sp - 1][tid] = top;
            ++sp;
            if (op.code == HJG_SPHERE) {
                top = ball(x, ndim, 0, row + op.off);
            } else if (op.code == HJG_CYLINDER) {
                top = ball(x, ndim, op.arg, row + op.off);
            } else if (op.code == HJG_RECT) {
                top = rect(x, ndim, row + op.off);
            } else if (op.code == HJG_HALFSPACE) {
                top = halfspace(x, ndim, row + op.off);
            } else if (OF && op.code == HJG_SPHERE_OF) {
                top = ball_of(x, ndim, op.arg, row + op.off);
            } else {
                const hjg_array a = prog.arrays[op.arg];
                const long long at = (a.per_member ? base : 0ll) + node;
                top = a.dtype == HJ_F64 ? ((const double*)a.data)[at] : (double)((const float*)a.data)[at];
            }
        } else if (op.code == HJG_COMPLEMENT) {
            top = -top;
        } else {
            --sp;
            const double a = below[sp - 1][tid];
            if (op.code == HJG_UNION) top = nmin(a, top);
            else if (op.code == HJG_INTERSECT) top = nmax(a, top);
            else top = nmax(a, -top);
        }
    }
    return top;
}

// The end of both kernels: the store, and what the member's stored values showed -- one vote per wave, and an atomic only when
// it would add a bit.  inside: whether this lane stores (to out[at]); f: the member's flag word.  The store and the lane's sign
// class are one function so that they stay ONE `inside` region of the kernel: a vote shared on its own compiled to a second one
// and cost the one-leaf programs 1 % to 4 % (profiles/refactor_shapes.txt).
template <typename T>
__device__ __forceinline__ void store_and_vote(bool inside, T* out, long long at, T stored, int tid, int* f) {
    if (inside) out[at] = stored;
    const int mine = inside ? (stored < T(0) ? HJG_NEG : (stored > T(0) ? HJG_POS : HJG_ZERO)) : 0;
    const int seen = (__any(mine & HJG_NEG) ? HJG_NEG : 0) | (__any(mine & HJG_POS) ? HJG_POS : 0) | (__any(mine & HJG_ZERO) ? HJG_ZERO : 0);
    if ((tid & 63) == 0 && seen) {                               // the first lane of the wave
        if (seen & ~__atomic_load_n(f, __ATOMIC_RELAXED)) atomicOr(f, seen);
    }
}

// ---------------------------------------------------------------------------------------------- host side
// Refusals go to the including library's own error record: hj_tool_host.h comes before this header.
#ifndef HJ_TOOL_HOST_H
#error "include hj_tool_host.h before hj_shapes_dev.h"
#endif
using hj_tool::fail;

constexpr long long MAX_Y = 65535;      // gridDim.y of one launch

static int null_argument() { return fail(HJ_EINVAL, "null argument"); }

static int check_members(int64_t K) {
    if (K < 1) return fail(HJ_EINVAL, "K = %lld: a scene has at least one member", (long long)K);
    return HJ_OK;
}

// what the libraries read of a descriptor: GD is hjq_grid (MD = 4) or hjh_grid (MD = 6); total = the number of nodes
template <int MD, typename GD>
static int check_extents(const GD* g, long long& total) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->ndim < 1 || g->ndim > MD) return fail(HJ_EINVAL, "ndim %d: grids of 1 .. %d dimensions", g->ndim, MD);
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "dtype %d: fp64 (%d) or fp32 (%d)", g->dtype, (int)HJ_F64, (int)HJ_F32);
    total = 1;
    for (int d = 0; d < g->ndim; ++d) {
        if (g->N[d] < 0 || g->N[d] > 0x7fffffffll) return fail(HJ_EINVAL, "N[%d] = %lld: 0 .. 2^31 - 1 nodes per axis", d, (long long)g->N[d]);
        if (total && g->N[d] > 0x7fffffffffffffffll / total) return fail(HJ_EINVAL, "the grid has more than 2^63 - 1 nodes");
        total *= g->N[d];
    }
    return HJ_OK;
}

static const char* const OP_NAMES[] = {"", "SPHERE", "CYLINDER", "RECT", "HALFSPACE", "ARRAY", "UNION", "INTERSECT", "DIFFERENCE", "COMPLEMENT",
                                       "SPHERE_OF"};

// everything the kernel would trust: after this, no instruction can leave the stack, the parameter row or the array table.
// Without OF opcode 10 is unknown, as every one past HJG_COMPLEMENT; MD: the most images SPHERE_OF takes
template <bool OF, int MD, typename PROG>
static int check_program(const PROG* p, int ndim, int64_t K, int64_t P) {
    if (!p) return fail(HJ_EINVAL, "null program");
    if (int rc = check_members(K)) return rc;
    if (P < 0) return fail(HJ_EINVAL, "P = %lld is negative", (long long)P);
    if (p->n_ops < 1 || p->n_ops > HJG_MAX_OPS)
        return fail(HJ_EINVAL, "a program has 1 .. %d instructions (got %d): evaluate a subtree first and pass it as an array leaf", (int)HJG_MAX_OPS, p->n_ops);
    if (p->n_arrays < 0 || p->n_arrays > HJG_MAX_ARRAYS) return fail(HJ_EINVAL, "a scene has at most %d array leaves (got %d)", (int)HJG_MAX_ARRAYS, p->n_arrays);
    for (int s = 0; s < p->n_arrays; ++s) {
        if (!p->arrays[s].data) return fail(HJ_EINVAL, "array leaf %d is null", s);
        if (p->arrays[s].dtype != HJ_F64 && p->arrays[s].dtype != HJ_F32)
            return fail(HJ_EINVAL, "array leaf %d has dtype %d: fp64 (%d) or fp32 (%d)", s, p->arrays[s].dtype, (int)HJ_F64, (int)HJ_F32);
    }
    int depth = 0;
    for (int i = 0; i < p->n_ops; ++i) {
        const hjg_op& op = p->ops[i];
        if (op.code < HJG_SPHERE || op.code > (OF ? HJG_SPHERE_OF : HJG_COMPLEMENT)) return fail(HJ_EINVAL, "instruction %d: unknown opcode %d", i, (int)op.code);
        const char* name = OP_NAMES[op.code];
        const bool of = OF && op.code == HJG_SPHERE_OF;
        if (op.code <= HJG_ARRAY || of) {
            if (++depth > HJG_MAX_DEPTH)
                return fail(HJ_EINVAL, "instruction %d (%s): stack overflow, the evaluation stack is %d deep: evaluate a subtree first and pass it as an array leaf",
                            i, name, (int)HJG_MAX_DEPTH);
            if (op.code == HJG_ARRAY) {
                if (op.arg < 0 || op.arg >= p->n_arrays) return fail(HJ_EINVAL, "instruction %d (ARRAY): slot %d of %d array leaves", i, (int)op.arg, p->n_arrays);
                continue;
            }
            if (of && (op.arg < 1 || op.arg > MD))
                return fail(HJ_EINVAL, "instruction %d (SPHERE_OF): J = %d: a sphere in 1 .. %d images of the coordinates", i, (int)op.arg, MD);
            const int64_t need = of ? (int64_t)op.arg * ndim + op.arg + 1 : ((op.code == HJG_SPHERE || op.code == HJG_CYLINDER) ? ndim + 1 : 2 * ndim);
            if (op.off < 0 || (int64_t)op.off + need > P)
                return fail(HJ_EINVAL, "instruction %d (%s): parameter offset %d + %lld values lies outside a row of P = %lld", i, name, op.off,
                            (long long)need, (long long)P);
            if (op.code == HJG_CYLINDER && (op.arg < 0 || op.arg >= (1 << ndim)))
                return fail(HJ_EINVAL, "instruction %d (CYLINDER): mask %#x names an axis outside the %d of the grid", i, (unsigned)op.arg, ndim);
        } else {
            const int takes = op.code == HJG_COMPLEMENT ? 1 : 2;
            if (depth < takes) return fail(HJ_EINVAL, "instruction %d (%s): stack underflow, it takes %d value(s) and %d are there", i, name, takes, depth);
            depth -= takes - 1;
        }
    }
    if (depth != 1) return fail(HJ_EINVAL, "the program leaves %d values on the stack: exactly one is the result", depth);
    for (int d = 0; d < ndim; ++d)
        if (!p->coord[d]) return fail(HJ_EINVAL, "null coordinate table of axis %d", d);
    return HJ_OK;
}

// gridDim.y ends at 65535: further members take further launches.  launch(nk): one launch of nk members from A.k0 on
template <typename ARGS, typename F>
static int member_launches(ARGS& A, int64_t K, F&& launch) {
    for (long long k0 = 0; k0 < K; k0 += MAX_Y) {
        A.k0 = k0;
        launch((unsigned)(K - k0 < MAX_Y ? K - k0 : MAX_Y));
        HIP_TRY(hipGetLastError());
    }
    return HJ_OK;
}

// hjg_evaluate and hjk_evaluate up to their launches: every check, in the order the refusals are documented in, and what both
// kernels' arguments (ARGS: SceneArgs, HiArgs) hold.  launch(type_tag<T>): the library's own launches into an output of T
template <bool OF, int MD, typename GD, typename PROG, typename ARGS, typename F>
static int evaluate(const GD* g, const PROG* program, const double* params, int64_t K, int64_t P, const void* out, int out_dtype,
                    int32_t* flags, ARGS& A, F&& launch) {
    long long total = 0;
    int rc = check_extents<MD>(g, total);
    if (rc) return rc;
    if (out_dtype != HJ_F64 && out_dtype != HJ_F32)
        return fail(HJ_EUNSUPPORTED, "out_dtype %d: the output must be fp64 (%d) or fp32 (%d)", out_dtype, (int)HJ_F64, (int)HJ_F32);
    rc = check_program<OF, MD>(program, g->ndim, K, P);
    if (rc) return rc;
    if (total == 0) return HJ_OK;
    if (K > 0x7fffffffffffffffll / total) return fail(HJ_EINVAL, "K x nodes exceeds 2^63 - 1");
    if (!out || !flags || (P > 0 && !params)) return null_argument();
    A.prog = *program;
    A.total = total;
    A.P = P;
    A.k0 = 0;
    A.params = params;
    A.flags = flags;
    A.ndim = g->ndim;
    if (out_dtype == HJ_F64) return launch(hj_tool::type_tag<double>{});
    return launch(hj_tool::type_tag<float>{});
}

}  // namespace hjg_dev
#endif
