// Device source of libhj_hidim.so's substep and bound kernels (include/hj_hidim.h): what hj_hidim.hip instantiates for the two built-in systems
// and what hipRTC compiles around a registered expression (hjh_ham_register: the generated HamUser<T> includes this header).  Device code only:
// hipRTC must be able to read it, so nothing of the host layer (hj_tool_host.h) is named here.
//   hidim_substep_kernel<T, HAM, SCHEME>  batch_substep_kernel (hj_batch.hip) without the problem axis: one thread per cell, every stencil load
//                                         issued unconditionally, 256 threads per workgroup.  Everything rides in the kernel arguments.
//   hidim_bound_kernel<T, HAM>            the per-axis maxima of alpha at zero costate
// A system HAM has  ND, ID, struct Cell,  cell(P, idx, sc) -> Cell  and  eval<NP>(cell, q, H, alpha): interface and scaling as hj_device.h's --
// cell() folds the costate scales sc[d] into the cell's coefficients, eval() takes the UNSCALED costates q (p_d = sc[d] q_d), returns H(x, p)
// and alpha_s[d] = sc[d] alpha_d.
// What the two kernels share with batch_substep_kernel / stoch_substep_kernel and their bound kernels -- the clamp, what a stage stores
// (stage_result, array_op), the fold of the per-axis maxima -- is hj_stage_dev.h's, device code only like this header.
#ifndef HJ_HIDIM_DEV_H
#define HJ_HIDIM_DEV_H
#include "hj_split.h"
#include "hj_stage_dev.h"
#include "../../include/hj_hidim.h"

namespace hjh {

using namespace hj;

template <typename T> struct HiTables {
    const T* coord[HJH_MAX_DIM];       // grid.vs[d]
    const T* aux[4];                   // cos / sin tables (include/hj_hidim.h)
    T par[HJH_PAR_SLOTS];
};

// lf_ydot (hj_device.h) for a system that reads HiTables: ydot = -(H - sum_d hd_d alpha_d), the sum in axis order, NP as there
template <bool NP, typename HAM, typename T>
__device__ __forceinline__ T hidim_ydot(const typename HAM::Cell& c, const T* pc, const T* hd, T* alpha) {
    T H;
    HAM::template eval<NP>(c, pc, H, alpha);
    if constexpr (NP) {
#pragma clang fp contract(off)
        T diss = T(0);
#pragma unroll
        for (int d = 0; d < HAM::ND; ++d) diss = diss + hd[d] * alpha[d];
        return -(H - diss);
    } else {
        T diss = T(0);
#pragma unroll
        for (int d = 0; d < HAM::ND; ++d) diss += hd[d] * alpha[d];
        return -(H - diss);
    }
}

static_assert(HJH_ARR_NONE == 0 && HJH_ARR_MIN == 1 && HJH_ARR_MAX == 2 && HJH_ARR_MAX_NEG == 3, "array_op (hj_stage_dev.h) takes the numbers");

template <typename T, int ND> struct SubstepArgs {
    GridArgs<T, ND> G;
    T sc[ND];                          // costate scale of the scheme (hj_device.h)
    HiTables<T> P;
    const T* src;
    const T* y0;
    T* dst;
    const T* post_a;
    const T* post_b;
    T dt;
    int stage, restrict_sign, post_prev, op_a, op_b;
};

template <typename T, typename HAM, int SCHEME>
__global__ __launch_bounds__(256) void hidim_substep_kernel(const SubstepArgs<T, HAM::ND> A) {
    constexpr int ND = HAM::ND;
    constexpr bool NP = np_order(SCHEME);
    static_assert(SCHEME != HJ_WENO5, "the intended WENO5 needs an epsilon reduction over the grid");
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= A.G.total) return;
    const int stage = A.stage;
    WenoK<T> wk;
    wk.c13 = T(0); wk.c4 = T(0);
    T ca = T(0), cb = T(1);
    if (stage == HJ_STAGE_RK3_HALF) { ca = T(0.75); cb = T(0.25); }
    else if (stage == HJ_STAGE_RK3_FULL) { ca = T(1.0 / 3.0); cb = T(2.0 / 3.0); }
    else if (stage == HJ_STAGE_RK2_FULL) { ca = T(0.5); cb = T(0.5); }
    const bool use_y0 = stage >= HJ_STAGE_RK3_HALF;
    int idx[ND];
    decode<T, ND>(A.G, t, idx);
    const T* pc0 = A.src + t;
    T v[ND][7];
    const T centre = pc0[0];
    const T y0v = use_y0 ? A.y0[t] : T(0);
    const typename HAM::Cell hc = HAM::cell(A.P, idx, A.sc);
    gather_stencils<T, ND>(A.G, pc0, idx, centre, v);
    T pc[ND], hd[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) upwind_cd<SCHEME, T>(v[d], A.G.K[d], T(0), wk, pc[d], hd[d]);
    T alpha[ND];
    T ydot = hidim_ydot<NP, HAM>(hc, pc, hd, alpha);
    ydot = restrict_clamp(A.restrict_sign, ydot);
    A.dst[t] = stage_result<NP>(A, stage, ca, cb, use_y0, A.dt, y0v, centre, ydot, t);
}

// max over the grid of alpha_d at zero costate: batch_bound_kernel's evaluation (unit scales), one workgroup maximum per axis folded into
// keys[d] (order-preserving keys, zero at launch)
template <typename T, typename HAM>
__global__ __launch_bounds__(256) void hidim_bound_kernel(const GridArgs<T, HAM::ND> G, const HiTables<T> P, unsigned long long* keys) {
    constexpr int ND = HAM::ND;
    double m[ND];
    T one[ND], p[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) { m[d] = -1e300; one[d] = T(1); p[d] = T(0); }
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < G.total; t += (long long)gridDim.x * blockDim.x) {
        int idx[ND];
        decode<T, ND>(G, t, idx);
        T H, a[ND];
        HAM::template eval<false>(HAM::cell(P, idx, one), p, H, a);
#pragma unroll
        for (int d = 0; d < ND; ++d) m[d] = fmax(m[d], (double)a[d]);
    }
    fold_bound<ND>(m, keys);
}

}  // namespace hjh
#endif
