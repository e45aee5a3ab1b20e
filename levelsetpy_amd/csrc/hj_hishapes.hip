// libhj_hishapes.so (include/hj_hishapes.h): implicit surface functions on grids of 1 to 6 dimensions, for gfx950.
//   hi_scene_kernel<T>  one pass over K members of a scene: a thread owns one node of one member (blockIdx.y the member), runs
//                       the postfix program on it and stores the result once.  No intermediate array exists in global memory.
// The kernel is a frame around hj_shapes_dev.h's interpreter, vote, leaves and checks, the source scene_kernel (hj_shapes.hip)
// compiles; the reasons for their shape stand there.
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

constexpr int BLOCK = SCENE_BLOCK;
constexpr int WAVE = 64;
constexpr int MD = HJK_MAX_DIM;
constexpr long long MAX_X = 0x7fffffffll;   // gridDim.x of one launch

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
    __shared__ double below[HJG_MAX_DEPTH - 1][BLOCK];          // run_program's stack under its top value
    const int tid = threadIdx.x;
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
    const long long base = member * A.total;                     // the member's first element: of the output, of a per-member array leaf
    const T stored = (T)run_program<true>(A, x, row, base, node, below, tid);
    store_and_vote(inside, out, base + node, stored, tid, A.flags + member);
}

// ---------------------------------------------------------------------------------------------- host side
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
static int scene_launch(HiArgs& A, const hjk_launch_plan& L, int64_t K, void* out, hipStream_t stream) {
    for (long long l = 0; l < L.launches; ++l) {
        const long long head = l * L.heads_per_launch;
        set_head(A.X, head);
        A.node0 = head * L.tail;
        const unsigned blocks = (unsigned)(l + 1 < L.launches ? L.blocks_full : L.blocks_last);
        int rc = member_launches(A, K, [&](unsigned nk) { hipLaunchKernelGGL((hi_scene_kernel<T>), dim3(blocks, nk), dim3(BLOCK), 0, stream, A, (T*)out); });
        if (rc) return rc;
    }
    launched(kernel_name("hi_scene_kernel", type_tag<T>::name(), {}).c_str());
    return HJ_OK;
}

}  // namespace hjk

using namespace hjk;

extern "C" {

int hjk_evaluate(const hjh_grid* g, const hjk_program* program, const double* params, int64_t K, int64_t P, void* out, int out_dtype,
                 int32_t* flags, void* stream) {
    HiArgs A;
    return evaluate<true, MD>(g, program, params, K, P, out, out_dtype, flags, A, [&](auto t) {
        hjk_launch_plan L;
        make_plan(g, A.total, K, L, A.X);
        A.node0 = 0;
        return scene_launch<typename decltype(t)::type>(A, L, K, out, (hipStream_t)stream);
    });
}

int hjk_plan(const hjh_grid* g, int64_t K, hjk_launch_plan* plan) {
    long long total = 0;
    int rc = check_extents<MD>(g, total);
    if (rc) return rc;
    if ((rc = check_members(K))) return rc;
    if (!plan) return null_argument();
    HiIndex X;
    make_plan(g, total, K, *plan, X);
    return HJ_OK;
}

int hjk_decode(const hjh_grid* g, int64_t node, int32_t idx[6]) {
    long long total = 0;
    int rc = check_extents<MD>(g, total);
    if (rc) return rc;
    if (!idx) return null_argument();
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
