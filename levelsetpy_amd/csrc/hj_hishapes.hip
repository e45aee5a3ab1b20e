// libhj_hishapes.so (include/hj_hishapes.h): implicit surface functions on grids of 1 to 6 dimensions, for gfx950.
//   hi_scene_kernel<T>  one pass over K members of a scene: a thread owns one node of one member (blockIdx.y the member), runs
//                       the postfix program on it and stores the result once.  No intermediate array exists in global memory.
// The kernel is a frame around hj_shapes_dev.h's interpreter, vote, leaves and checks, the source scene_kernel (hj_shapes.hip)
// compiles; the reasons for their shape stand there.
// The indexing is hj_index_dev.h's node walk (tail / head split, host-prepared reciprocals, blockIdx.x split in 32 bits: nothing
// divides), decoded at six axes whatever the grid's ndim: the interpreter already keeps the scalar unit, which the four SIMDs of a
// compute unit share, busier than the vector units, so every lane divides its own tail node on the vector unit.
#include <hip/hip_runtime.h>
#include "hj_tool_host.h"
#include "hj_shapes_dev.h"
#include "hj_index_dev.h"
#include "../../include/hj_hishapes.h"

namespace hjk {

using namespace hj_tool;
using namespace hjg_dev;
using namespace hj_index;

constexpr int BLOCK = SCENE_BLOCK;
constexpr int WAVE = 64;
constexpr int MD = HJK_MAX_DIM;

struct HiArgs {
    hjk_program prog;
    Index X;
    long long total;                        // nodes of the grid
    long long P;                            // values per parameter row
    long long k0;                           // first member of this launch
    long long node0;                        // flat node of this launch's first head index at tail node 0
    const double* params;
    int* flags;
    int ndim;
};
static_assert(sizeof(HiArgs) <= 4096, "the program and the index must fit the kernel-argument segment");

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
template <typename T>
static int scene_launch(HiArgs& A, const Plan& L, int64_t K, void* out, hipStream_t stream) {
    int rc = head_launches(L, A.X, A.node0, [&](unsigned blocks) {
        return member_launches(A, K, [&](unsigned nk) { hipLaunchKernelGGL((hi_scene_kernel<T>), dim3(blocks, nk), dim3(BLOCK), 0, stream, A, (T*)out); });
    });
    if (rc) return rc;
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
        Limits lim;
        if (int rc = read_limits(lim, BLOCK)) return rc;
        const Plan L = make_plan(g, A.total, BLOCK, A.X, lim);
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
    Limits lim;
    if ((rc = read_limits(lim, BLOCK))) return rc;
    Index X;
    publish(make_plan(g, total, BLOCK, X, lim), *plan);
    plan->member_launches = (int32_t)((K + MAX_Y - 1) / MAX_Y);
    return HJ_OK;
}

int hjk_decode(const hjh_grid* g, int64_t node, int32_t idx[6]) {
    long long total = 0;
    int rc = check_extents<MD>(g, total);
    if (rc) return rc;
    if (!idx) return null_argument();
    if ((rc = check_node(node, total))) return rc;
    Limits lim;
    if ((rc = read_limits(lim, BLOCK))) return rc;
    Index X;
    const Plan L = make_plan(g, total, BLOCK, X, lim);
    decode(L, X, MD, node, idx);                                 // at six axes, as the kernel decodes
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjk)

}  // extern "C"
