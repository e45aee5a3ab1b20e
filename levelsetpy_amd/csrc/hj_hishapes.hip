// libhj_hishapes.so (include/hj_hishapes.h): implicit surface functions on grids of 1 to 6 dimensions, for gfx950.
//   hi_scene_kernel<T>  one pass over K members of a scene: a thread owns one node of one member (blockIdx.y the member), runs
//                       the postfix program on it and stores the result once.  No intermediate array exists in global memory.
// The interpreter is scene_kernel's (hj_shapes.hip): the program rides in the kernel arguments and the member's parameter row is
// read through blockIdx.y, so opcodes, offsets and parameters are wave-uniform, the branches never diverge and the parameter reads
// are scalar loads; the top of the evaluation stack is a register, the values below it one LDS column per thread ([depth - 1][256]
// doubles, 14 KB), indexed by the uniform stack pointer, no barrier; stores are ONE element per lane, so a view at any element
// offset needs no head or tail; the leaves are hj_shapes_dev.h's, the source scene_kernel compiles.
// The indexing is new: NOTHING here divides or takes a remainder by a run-time extent, in 32 or in 64 bits.
//   * the host splits the axes into a tail (the longest suffix with fewer than 2^31 nodes) and a head; a workgroup owns 256
//     consecutive tail nodes of ONE head index, so blockIdx.x = head' * chunks + chunk and every linear index is below 2^32;
//   * `quotient` divides a 32-bit value by an extent with the 64-bit reciprocal the host prepared: one multiply-high, exact for
//     every 32-bit dividend;
//   * blockIdx.x is split, and the head index decoded, ONCE per wave from wave-uniform values (scalar registers): the head index
//     of a launch's first workgroup arrives decoded (the host divides) and head' is added to it with carry;
//   * every lane divides its OWN tail node through the tail axes, on the vector unit.  Decoding the wave's first node on the
//     scalar unit and moving the lanes on by add-and-carry was built first and measured slower (profiles/hishapes_timing.txt):
//     the interpreter already keeps the scalar unit, which the four SIMDs of a compute unit share, busier than the vector units.
// `split_block` and `node_index` are __host__ __device__: hjk_decode runs them on the host for any node of any grid.
#include <hip/hip_runtime.h>
#include "hj_tool_host.h"
#include "hj_shapes_dev.h"
#include "../../include/hj_hishapes.h"

namespace hjk {

using namespace hj_tool;
using namespace hjg_dev;

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int MD = HJK_MAX_DIM;
constexpr long long MAX_X = 0x7fffffffll;   // gridDim.x of one launch
constexpr long long MAX_Y = 65535;          // gridDim.y of one launch

// what the decode reads: the extents (1 past ndim), their reciprocals and the split of blockIdx.x
struct HiIndex {
    unsigned long long recip[MD];           // floor(2^64 / n) + 1 for n > 1 (2^64 / n for a power of two): quotient
    unsigned long long chunk_recip;         // the same of `chunks`
    unsigned n[MD];                         // nodes per axis
    unsigned h0[MD];                        // multi-index of this launch's first head index (tail axes: 0)
    unsigned chunks;                        // workgroups per head index
    unsigned tail;                          // nodes of the tail, below 2^31
    int first_tail;                         // axes first_tail .. MD - 1 are the tail
};

struct HiArgs {
    hjk_program prog;
    HiIndex X;
    long long total;                        // nodes of the grid
    long long P;                            // values per parameter row
    long long k0;                           // first member of this launch
    long long node0;                        // flat node of this launch's first head index at tail node 0
    const double* params;
    int* flags;
    int ndim;
};
static_assert(sizeof(HiArgs) <= 4096, "the program and the index must fit the kernel-argument segment");

// floor(v / n) for any 32-bit v by the reciprocal r = floor(2^64 / n) + 1 of n > 1: the high 64 bits of v * r, exact because
// v * (r * n - 2^64) <= v * n < 2^64
__host__ __device__ __forceinline__ unsigned quotient(unsigned v, unsigned long long r) {
    const unsigned long long lo = (unsigned long long)v * (unsigned)r;
    const unsigned long long hi = (unsigned long long)v * (unsigned)(r >> 32);
    return (unsigned)((hi + (lo >> 32)) >> 32);
}

// blockIdx.x = head' * chunks + chunk -> head' (the head index counted from this launch's first) and the chunk; wave-uniform
__host__ __device__ __forceinline__ void split_block(const HiIndex& X, unsigned block, unsigned& hl, unsigned& chunk) {
    hl = block;
    chunk = 0u;
    if (X.chunks > 1u) {
        hl = quotient(block, X.chunk_recip);
        chunk = block - hl * X.chunks;
    }
}

// The multi-index of tail node t of head index h0 + hl.  The tail axes divide t, a lane's own value: vector arithmetic, one
// multiply-high per axis.  The head axes add hl to the launch's first head index with carry: wave-uniform, scalar arithmetic.
__host__ __device__ __forceinline__ void node_index(const HiIndex& X, unsigned hl, unsigned t, unsigned (&idx)[MD]) {
    unsigned up = hl;
#pragma unroll
    for (int d = MD - 1; d >= 0; --d) {
        if (d > X.first_tail) {                                  // a tail axis below the tail's first: divide the tail node
            idx[d] = 0u;
            if (X.n[d] > 1u) {
                const unsigned q = quotient(t, X.recip[d]);
                idx[d] = t - q * X.n[d];
                t = q;
            }
        } else if (d == X.first_tail) {
            idx[d] = t;
        } else if (d > 0) {                                      // a head axis: the launch's first head index plus head', with carry
            const unsigned v = X.h0[d] + up;                     // both below 2^31
            idx[d] = 0u;
            up = v;                                              // an axis of one node passes the carry on
            if (X.n[d] > 1u) {
                up = quotient(v, X.recip[d]);
                idx[d] = v - up * X.n[d];
            }
        } else {
            idx[0] = X.h0[0] + up;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void hi_scene_kernel(const HiArgs A, T* __restrict__ out) {
    __shared__ double below[HJG_MAX_DEPTH - 1][BLOCK];          // the stack under its top value, one column per thread
    const int tid = threadIdx.x;
    const unsigned lane = (unsigned)tid & (WAVE - 1);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid / WAVE);
    const long long member = A.k0 + blockIdx.y;

    unsigned hl, chunk;
    split_block(A.X, blockIdx.x, hl, chunk);
    if (chunk * (unsigned)BLOCK + wave * WAVE >= A.X.tail) return;           // wave-uniform: the whole wave is past the tail's end
    const unsigned mine = chunk * (unsigned)BLOCK + (unsigned)tid;
    const bool inside = mine < A.X.tail;
    const unsigned t = inside ? mine : A.X.tail - 1u;            // a lane past the end evaluates the last node and stores nothing
    unsigned idx[MD];
    node_index(A.X, hl, t, idx);

    double x[MD] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < MD; ++d)
        if (d < A.ndim) x[d] = A.prog.coord[d][idx[d]];
    // the flat node: this launch's first, head' tails on (wave-uniform, one 64-bit multiply), and the lane's place in the tail
    const long long node = A.node0 + (long long)hl * (long long)A.X.tail + (long long)t;

    const double* __restrict__ row = A.params + member * A.P;
    double top = 0.0;
    int sp = 0;                                                  // values on the stack, the one in `top` included
    for (int i = 0; i < A.prog.n_ops; ++i) {
        const hjg_op op = A.prog.ops[i];
        if (op.code <= HJG_ARRAY || op.code == HJG_SPHERE_OF) {  // a leaf: the old top goes under the new one
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
            } else if (op.code == HJG_SPHERE_OF) {
                top = ball_of(x, A.ndim, op.arg, row + op.off);
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
    if (inside) out[member * A.total + node] = stored;

    // what the member's stored values showed: one vote per wave, and an atomic only when it would add a bit
    const int sign = inside ? (stored < T(0) ? HJG_NEG : (stored > T(0) ? HJG_POS : HJG_ZERO)) : 0;
    const int seen = (__any(sign & HJG_NEG) ? HJG_NEG : 0) | (__any(sign & HJG_POS) ? HJG_POS : 0) | (__any(sign & HJG_ZERO) ? HJG_ZERO : 0);
    if (lane == 0u && seen) {
        int* f = A.flags + member;
        if (seen & ~__atomic_load_n(f, __ATOMIC_RELAXED)) atomicOr(f, seen);
    }
}

// ---------------------------------------------------------------------------------------------- host side
static int check_grid(const hjh_grid* g, long long& total) {
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

static bool is_leaf(int code) { return code <= HJG_ARRAY || code == HJG_SPHERE_OF; }

// everything the kernel would trust: after this, no instruction can leave the stack, the parameter row or the array table
static int check_program(const hjk_program* p, int ndim, int64_t K, int64_t P) {
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
        if (op.code < HJG_SPHERE || op.code > HJG_SPHERE_OF) return fail(HJ_EINVAL, "instruction %d: unknown opcode %d", i, (int)op.code);
        const char* name = OP_NAMES[op.code];
        if (is_leaf(op.code)) {
            if (++depth > HJG_MAX_DEPTH)
                return fail(HJ_EINVAL, "instruction %d (%s): stack overflow, the evaluation stack is %d deep: evaluate a subtree first and pass it as an array leaf",
                            i, name, (int)HJG_MAX_DEPTH);
            if (op.code == HJG_ARRAY) {
                if (op.arg < 0 || op.arg >= p->n_arrays) return fail(HJ_EINVAL, "instruction %d (ARRAY): slot %d of %d array leaves", i, (int)op.arg, p->n_arrays);
                continue;
            }
            if (op.code == HJG_SPHERE_OF && (op.arg < 1 || op.arg > MD))
                return fail(HJ_EINVAL, "instruction %d (SPHERE_OF): J = %d: a sphere in 1 .. %d images of the coordinates", i, (int)op.arg, MD);
            const int64_t need = op.code == HJG_SPHERE_OF ? (int64_t)op.arg * ndim + op.arg + 1
                                                          : ((op.code == HJG_SPHERE || op.code == HJG_CYLINDER) ? ndim + 1 : 2 * ndim);
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

static unsigned long long recip64(unsigned n) { return n > 1u ? 0xffffffffffffffffull / n + 1ull : 0ull; }

// the split of the axes, the launches and what the decode reads of them (X.h0 is set per launch)
static void make_plan(const hjh_grid* g, long long total, int64_t K, hjk_launch_plan& L, HiIndex& X) {
    L = hjk_launch_plan{};
    X = HiIndex{};
    for (int d = 0; d < MD; ++d) {
        X.n[d] = d < g->ndim ? (unsigned)g->N[d] : 1u;
        X.recip[d] = recip64(X.n[d]);
    }
    L.member_launches = (int32_t)((K + MAX_Y - 1) / MAX_Y);
    L.total = total;
    if (total == 0) return;
    long long tail = 1;
    int ft = MD;
    while (ft > 0 && tail * (long long)X.n[ft - 1] < 0x80000000ll) tail *= (long long)X.n[--ft];       // the last axis always fits
    L.first_tail = ft;
    L.tail = tail;
    L.head = total / tail;
    L.chunks = (tail + BLOCK - 1) / BLOCK;
    L.heads_per_launch = std::min<long long>(L.head, MAX_X / L.chunks);
    L.launches = (L.head + L.heads_per_launch - 1) / L.heads_per_launch;
    L.blocks_full = L.heads_per_launch * L.chunks;
    L.blocks_last = (L.head - (L.launches - 1) * L.heads_per_launch) * L.chunks;
    if (L.launches == 1) L.blocks_full = L.blocks_last;
    X.chunks = (unsigned)L.chunks;
    X.chunk_recip = recip64(X.chunks);
    X.tail = (unsigned)tail;
    X.first_tail = ft;
}

// the multi-index of head index `head` into X.h0: the one place that divides, on the host
static void set_head(HiIndex& X, long long head) {
    for (int d = MD - 1; d >= 0; --d) {
        X.h0[d] = 0u;
        if (d < X.first_tail) {
            X.h0[d] = (unsigned)(head % (long long)X.n[d]);
            head /= (long long)X.n[d];
        }
    }
}

template <typename T>
static int scene_launch(HiArgs& A, const hjk_launch_plan& L, int64_t K, void* out, hipStream_t stream, const char* name) {
    for (long long l = 0; l < L.launches; ++l) {
        const long long head = l * L.heads_per_launch;
        set_head(A.X, head);
        A.node0 = head * L.tail;
        const unsigned blocks = (unsigned)(l + 1 < L.launches ? L.blocks_full : L.blocks_last);
        for (long long k0 = 0; k0 < K; k0 += MAX_Y) {           // gridDim.y ends at 65535: further members take further launches
            const long long nk = K - k0 < MAX_Y ? K - k0 : MAX_Y;
            A.k0 = k0;
            hipLaunchKernelGGL((hi_scene_kernel<T>), dim3(blocks, (unsigned)nk), dim3(BLOCK), 0, stream, A, (T*)out);
            HIP_TRY(hipGetLastError());
        }
    }
    launched(name);
    return HJ_OK;
}

}  // namespace hjk

using namespace hjk;

extern "C" {

int hjk_evaluate(const hjh_grid* g, const hjk_program* program, const double* params, int64_t K, int64_t P, void* out, int out_dtype,
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
    HiArgs A;
    hjk_launch_plan L;
    make_plan(g, total, K, L, A.X);
    A.prog = *program;
    A.total = total;
    A.P = P;
    A.k0 = 0;
    A.node0 = 0;
    A.params = params;
    A.flags = flags;
    A.ndim = g->ndim;
    if (out_dtype == HJ_F64) return scene_launch<double>(A, L, K, out, (hipStream_t)stream, "hi_scene_kernel<double>");
    return scene_launch<float>(A, L, K, out, (hipStream_t)stream, "hi_scene_kernel<float>");
}

int hjk_plan(const hjh_grid* g, int64_t K, hjk_launch_plan* plan) {
    long long total = 0;
    int rc = check_grid(g, total);
    if (rc) return rc;
    if (K < 1) return fail(HJ_EINVAL, "K = %lld: a scene has at least one member", (long long)K);
    if (!plan) return fail(HJ_EINVAL, "null argument");
    HiIndex X;
    make_plan(g, total, K, *plan, X);
    return HJ_OK;
}

int hjk_decode(const hjh_grid* g, int64_t node, int32_t idx[6]) {
    long long total = 0;
    int rc = check_grid(g, total);
    if (rc) return rc;
    if (!idx) return fail(HJ_EINVAL, "null argument");
    if (node < 0 || node >= total) return fail(HJ_EINVAL, "node %lld: the grid has nodes 0 .. %lld", (long long)node, total - 1);
    hjk_launch_plan L;
    HiIndex X;
    make_plan(g, total, 1, L, X);
    // the launch, workgroup and thread that own the node, as scene_launch and the kernel lay them out
    const long long head = node / L.tail, t = node % L.tail;
    const long long launch = head / L.heads_per_launch;
    set_head(X, launch * L.heads_per_launch);
    const unsigned block = (unsigned)((head - launch * L.heads_per_launch) * L.chunks + t / BLOCK);
    unsigned mine[MD], hl = 0u, chunk = 0u;
    split_block(X, block, hl, chunk);
    node_index(X, hl, chunk * (unsigned)BLOCK + (unsigned)(t % BLOCK), mine);
    for (int d = 0; d < MD; ++d) idx[d] = (int32_t)mine[d];
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjk)

}  // extern "C"
