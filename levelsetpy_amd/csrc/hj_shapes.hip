// libhj_shapes.so (include/hj_shapes.h): implicit surface functions for gfx950.
//   scene_kernel<T>  one pass over K members of a scene: a thread owns one node of one member (blockIdx.y the member), runs
//                    the postfix program on it and stores the result once.
// The kernel is a frame: it decodes the node and fills x[]; the interpreter, the vote, the leaves and the checks are
// hj_shapes_dev.h's (shared with hj_hishapes.hip), where the reasons for their shape stand.
#include <hip/hip_runtime.h>
#include "hj_tool_host.h"
#include "hj_shapes_dev.h"
#include "../../include/hj_shapes.h"

namespace hjg {

using namespace hj_tool;
using namespace hjg_dev;        // nmin, nmax and the leaves: hj_shapes_dev.h, compiled here at HJ_MAX_DIM axes

constexpr int BLOCK = SCENE_BLOCK;

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

// The node's coordinates, from its index per axis, last axis fastest; 32-bit divisions whenever the grid allows them.  A function of
// its own, as node_index is in hj_hishapes.hip: with the interpreter a call, the same lines inside the kernel compiled to another
// block layout of the two division paths than the parent's (profiles/refactor_shapes.txt).
__device__ __forceinline__ void node_coords(const SceneArgs& A, long long node, double (&x)[HJ_MAX_DIM]) {
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
#pragma unroll
    for (int d = 0; d < HJ_MAX_DIM; ++d) {
        x[d] = 0.0;
        if (d < A.ndim) x[d] = A.prog.coord[d][idx[d]];
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void scene_kernel(const SceneArgs A, T* __restrict__ out) {
    __shared__ double below[HJG_MAX_DEPTH - 1][BLOCK];          // run_program's stack under its top value
    const int tid = threadIdx.x;
    const long long member = A.k0 + blockIdx.y;
    const long long t = blockIdx.x * (long long)BLOCK + tid;
    const bool inside = t < A.total;
    const long long node = inside ? t : A.total - 1;             // a thread past the end evaluates the last node and stores nothing

    double x[HJ_MAX_DIM];
    node_coords(A, node, x);

    const double* __restrict__ row = A.params + member * A.P;
    const long long base = member * A.total;                     // the member's first element: of the output, of a per-member array leaf
    const T stored = (T)run_program<false>(A, x, row, base, node, below, tid);
    store_and_vote(inside, out, base + t, stored, tid, A.flags + member);
}

// ---------------------------------------------------------------------------------------------- host side
template <typename T>
static int scene_launch(SceneArgs& A, int64_t K, void* out, hipStream_t stream) {
    unsigned blocks;
    int rc = blocks_for(A.total, "too many nodes for one launch", blocks);
    if (rc) return rc;
    rc = member_launches(A, K, [&](unsigned nk) { hipLaunchKernelGGL((scene_kernel<T>), dim3(blocks, nk), dim3(BLOCK), 0, stream, A, (T*)out); });
    if (rc) return rc;
    launched(kernel_name("scene_kernel", type_tag<T>::name(), {}).c_str());
    return HJ_OK;
}

}  // namespace hjg

using namespace hjg;

extern "C" {

int hjg_evaluate(const hjq_grid* g, const hjg_program* program, const double* params, int64_t K, int64_t P, void* out, int out_dtype,
                 int32_t* flags, void* stream) {
    SceneArgs A;
    return evaluate<false, HJ_MAX_DIM>(g, program, params, K, P, out, out_dtype, flags, A, [&](auto t) {
        for (int d = 0; d < HJ_MAX_DIM; ++d) A.n[d] = d < g->ndim ? (int)g->N[d] : 1;
        return scene_launch<typename decltype(t)::type>(A, K, out, (hipStream_t)stream);
    });
}

HJ_TOOL_LAST_SYMBOLS(hjg)

}  // extern "C"
