// libhj_shapes.so (include/hj_shapes.h): implicit surface functions for gfx950.
//   scene_kernel<T>  one pass over K members of a scene: a thread owns one node of one member (blockIdx.y the member), runs
//                    the postfix program on it and stores the result once.  No intermediate array exists in global memory.
// The program rides in the kernel arguments and the member's parameter row is read through blockIdx.y: opcodes, offsets and
// parameters are wave-uniform, so the interpreter's branches never diverge and its parameter reads are scalar loads.
// The evaluation stack: the top value in a register, the values below it in LDS, one column per thread ([depth - 1][256]
// doubles, 14 KB).  A stack indexed at run time in registers goes to scratch; the LDS column is indexed by the uniform stack
// pointer, costs one ds access per instruction of the program, and needs no barrier (a thread reads only what it wrote).
// Stores are ONE element per lane, neighbouring lanes on neighbouring elements: a wave-instruction covers 512 contiguous bytes
// of fp64 whatever the alignment -- with an odd node count every second member starts off 16-byte alignment, and callers pass
// views at any element offset, so nothing here is wider than an element and no head or tail needs peeling.
// The leaves are hj_shapes_dev.h's (shared with hj_hishapes.hip), written one operation per statement with contraction off: the
// results are NumPy's, bit for bit.
#include <hip/hip_runtime.h>
#include "hj_tool_host.h"
#include "hj_shapes_dev.h"
#include "../../include/hj_shapes.h"

namespace hjg {

using namespace hj_tool;
using namespace hjg_dev;        // nmin, nmax and the leaves: hj_shapes_dev.h, compiled here at HJ_MAX_DIM axes

constexpr int BLOCK = 256;
constexpr long long MAX_Y = 65535;      // gridDim.y of one launch

struct SceneArgs {
    hjg_program prog;
    long long total;                    // nodes of the grid
    long long P;                        // values per parameter row
    long long k0;                       // first member of this launch
    const double* params;
    int* flags;
    int n[HJ_MAX_DIM];
    int ndim;
};

template <typename T>
__global__ __launch_bounds__(BLOCK) void scene_kernel(const SceneArgs A, T* __restrict__ out) {
    __shared__ double below[HJG_MAX_DEPTH - 1][BLOCK];          // the stack under its top value, one column per thread
    const int tid = threadIdx.x;
    const long long member = A.k0 + blockIdx.y;
    const long long t = blockIdx.x * (long long)BLOCK + tid;
    const bool inside = t < A.total;
    const long long node = inside ? t : A.total - 1;             // a thread past the end evaluates the last node and stores nothing

    // the node's index per axis, last axis fastest; 32-bit divisions whenever the grid allows them
    int idx[HJ_MAX_DIM] = {0, 0, 0, 0};
    if (A.total <= 0xffffffffll) {
        unsigned r = (unsigned)node;
#pragma unroll
        for (int d = HJ_MAX_DIM - 1; d >= 1; --d) {
            if (d < A.ndim) {
                const unsigned q = r / (unsigned)A.n[d];
                idx[d] = (int)(r - q * (unsigned)A.n[d]);
                r = q;
            }
        }
        idx[0] = (int)r;
    } else {
        long long r = node;
#pragma unroll
        for (int d = HJ_MAX_DIM - 1; d >= 1; --d) {
            if (d < A.ndim) {
                const long long q = r / A.n[d];
                idx[d] = (int)(r - q * A.n[d]);
                r = q;
            }
        }
        idx[0] = (int)r;
    }
    double x[HJ_MAX_DIM] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < HJ_MAX_DIM; ++d)
        if (d < A.ndim) x[d] = A.prog.coord[d][idx[d]];

    const double* __restrict__ row = A.params + member * A.P;
    double top = 0.0;
    int sp = 0;                                                  // values on the stack, the one in `top` included
    for (int i = 0; i < A.prog.n_ops; ++i) {
        const hjg_op op = A.prog.ops[i];
        if (op.code <= HJG_ARRAY) {                              // a leaf: the old top goes under the new one
            if (sp > 0) below[sp - 1][tid] = top;
            ++sp;
            if (op.code == HJG_SPHERE) {
                top = ball(x, A.ndim, 0, row + op.off);
            } else if (op.code == HJG_CYLINDER) {
                top = ball(x, A.ndim, op.arg, row + op.off);
            } else if (op.code == HJG_RECT) {
                top = rect(x, A.ndim, row + op.off);
            } else if (op.code == HJG_HALFSPACE) {
                top = halfspace(x, A.ndim, row + op.off);
            } else {
                const hjg_array a = A.prog.arrays[op.arg];
                const long long at = (a.per_member ? member * A.total : 0ll) + node;
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

    const T stored = (T)top;
    if (inside) out[member * A.total + t] = stored;

    // what the member's stored values showed: one vote per wave, and an atomic only when it would add a bit
    const int mine = inside ? (stored < T(0) ? HJG_NEG : (stored > T(0) ? HJG_POS : HJG_ZERO)) : 0;
    const int seen = (__any(mine & HJG_NEG) ? HJG_NEG : 0) | (__any(mine & HJG_POS) ? HJG_POS : 0) | (__any(mine & HJG_ZERO) ? HJG_ZERO : 0);
    if ((tid & 63) == 0 && seen) {
        int* f = A.flags + member;
        if (seen & ~__atomic_load_n(f, __ATOMIC_RELAXED)) atomicOr(f, seen);
    }
}

// ---------------------------------------------------------------------------------------------- host side
static int check_grid(const hjq_grid* g, long long& total) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->ndim < 1 || g->ndim > HJ_MAX_DIM) return fail(HJ_EINVAL, "ndim %d: grids of 1 .. %d dimensions", g->ndim, HJ_MAX_DIM);
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "dtype %d: fp64 (%d) or fp32 (%d)", g->dtype, (int)HJ_F64, (int)HJ_F32);
    total = 1;
    for (int d = 0; d < g->ndim; ++d) {
        if (g->N[d] < 0 || g->N[d] > 0x7fffffffll) return fail(HJ_EINVAL, "N[%d] = %lld: 0 .. 2^31 - 1 nodes per axis", d, (long long)g->N[d]);
        if (total && g->N[d] > 0x7fffffffffffffffll / total) return fail(HJ_EINVAL, "the grid has more than 2^63 - 1 nodes");
        total *= g->N[d];
    }
    return HJ_OK;
}

static const char* const OP_NAMES[] = {"", "SPHERE", "CYLINDER", "RECT", "HALFSPACE", "ARRAY", "UNION", "INTERSECT", "DIFFERENCE", "COMPLEMENT"};

// everything the kernel would trust: after this, no instruction can leave the stack, the parameter row or the array table
static int check_program(const hjg_program* p, int ndim, int64_t K, int64_t P) {
    if (!p) return fail(HJ_EINVAL, "null program");
    if (K < 1) return fail(HJ_EINVAL, "K = %lld: a scene has at least one member", (long long)K);
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
        if (op.code < HJG_SPHERE || op.code > HJG_COMPLEMENT) return fail(HJ_EINVAL, "instruction %d: unknown opcode %d", i, (int)op.code);
        const char* name = OP_NAMES[op.code];
        if (op.code <= HJG_ARRAY) {
            if (++depth > HJG_MAX_DEPTH)
                return fail(HJ_EINVAL, "instruction %d (%s): stack overflow, the evaluation stack is %d deep: evaluate a subtree first and pass it as an array leaf",
                            i, name, (int)HJG_MAX_DEPTH);
            if (op.code == HJG_ARRAY) {
                if (op.arg < 0 || op.arg >= p->n_arrays) return fail(HJ_EINVAL, "instruction %d (ARRAY): slot %d of %d array leaves", i, (int)op.arg, p->n_arrays);
                continue;
            }
            const int64_t need = (op.code == HJG_SPHERE || op.code == HJG_CYLINDER) ? ndim + 1 : 2 * ndim;
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

template <typename T>
static int scene_launch(SceneArgs& A, int64_t K, void* out, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for(A.total, "too many nodes for one launch", blocks);
    if (rc) return rc;
    for (long long k0 = 0; k0 < K; k0 += MAX_Y) {               // gridDim.y ends at 65535: further members take further launches
        const long long nk = K - k0 < MAX_Y ? K - k0 : MAX_Y;
        A.k0 = k0;
        hipLaunchKernelGGL((scene_kernel<T>), dim3(blocks, (unsigned)nk), dim3(BLOCK), 0, stream, A, (T*)out);
        HIP_TRY(hipGetLastError());
    }
    launched(name);
    return HJ_OK;
}

}  // namespace hjg

using namespace hjg;

extern "C" {

int hjg_evaluate(const hjq_grid* g, const hjg_program* program, const double* params, int64_t K, int64_t P, void* out, int out_dtype,
                 int32_t* flags, void* stream) {
    long long total = 0;
    int rc = check_grid(g, total);
    if (rc) return rc;
    if (out_dtype != HJ_F64 && out_dtype != HJ_F32)
        return fail(HJ_EUNSUPPORTED, "out_dtype %d: the output must be fp64 (%d) or fp32 (%d)", out_dtype, (int)HJ_F64, (int)HJ_F32);
    rc = check_program(program, g->ndim, K, P);
    if (rc) return rc;
    if (total == 0) return HJ_OK;
    if (K > 0x7fffffffffffffffll / total) return fail(HJ_EINVAL, "K x nodes exceeds 2^63 - 1");
    if (!out || !flags || (P > 0 && !params)) return fail(HJ_EINVAL, "null argument");
    SceneArgs A;
    A.prog = *program;
    A.total = total;
    A.P = P;
    A.k0 = 0;
    A.params = params;
    A.flags = flags;
    A.ndim = g->ndim;
    for (int d = 0; d < HJ_MAX_DIM; ++d) A.n[d] = d < g->ndim ? (int)g->N[d] : 1;
    if (out_dtype == HJ_F64) return scene_launch<double>(A, K, out, (hipStream_t)stream, "scene_kernel<double>");
    return scene_launch<float>(A, K, out, (hipStream_t)stream, "scene_kernel<float>");
}

HJ_TOOL_LAST_SYMBOLS(hjg)

}  // extern "C"
