// What the substep and bound kernels of libhj_batch.so, libhj_stoch.so and libhj_hidim.so share (hj_batch.hip, hj_stoch.hip, hj_hidim_dev.h):
// the pieces around a stage's ydot that do not depend on the system or on where the arguments ride.  Device code only: hipRTC reads this
// header through hj_hidim_dev.h, so nothing of the host layer (hj_tool_host.h) is named here.  Every function is inlined into its kernel.
//   tables_of      the HamTables a built-in system reads, from the tables and parameters of a launch
//   restrict_clamp termRestrictUpdate
//   stage_result   rk_stage_out, post_step and the two array operators: what a stage stores
//   array_op       min / max against an array
//   fold_bound     the end of a bound kernel: the workgroup's per-axis maxima into the keys
// (The stage prologue -- ca, cb and use_y0 from the stage -- stays written out in the three substep kernels: as a function of its own the
// compiler simplifies the chain before it inlines it and the kernels' select order moves, so their code would no longer be the code
// tools/codeobj_diff.py has compared.  For the same reason stoch_substep_kernel keeps its own copy of the clamp.)
#ifndef HJ_STAGE_DEV_H
#define HJ_STAGE_DEV_H
#include "hj_split.h"

namespace hj {

template <typename T>
__device__ __forceinline__ HamTables<T> tables_of(const T* const* coord, const T* const* aux, const double* par) {
    HamTables<T> P;
#pragma unroll
    for (int d = 0; d < HJ_MAX_DIM; ++d) P.coord[d] = coord[d];
#pragma unroll
    for (int s = 0; s < 4; ++s) P.aux[s] = aux[s];
#pragma unroll
    for (int s = 0; s < HJ_PAR_SLOTS; ++s) P.par[s] = (T)par[s];     // rounded as the solver's host side rounds them (fill_ham)
    P.range = nullptr;
    P.local_mode = 0;
    return P;
}

// termRestrictUpdate clamp, written like direct_substep_kernel's (a NaN stays a NaN)
template <typename T>
__device__ __forceinline__ T restrict_clamp(int restrict_sign, T ydot) {
    if (restrict_sign > 0) ydot = (ydot < T(0)) ? T(0) : ydot;
    else if (restrict_sign < 0) ydot = (ydot > T(0)) ? T(0) : ydot;
    return ydot;
}

// min / max against an array: minmax_kernel's expression (hj_split.h), NaN propagating as NumPy's minimum / maximum.  op: 1 min, 2 max,
// 3 max(a, -b) -- HJB_ARR_* of include/hj_batch.h and HJH_ARR_* of include/hj_hidim.h (the libraries assert the numbers)
template <typename T>
__device__ __forceinline__ T array_op(int op, T a, T b) {
    T r;
    if (a != a) r = a;
    else if (b != b) r = b;
    else if (op == 1) r = a < b ? a : b;
    else if (op == 2) r = a > b ? a : b;
    else r = a > -b ? a : -b;
    return r;
}

// what a stage stores at cell t.  S holds the stage's post_prev, op_a, op_b, post_a, post_b: the kernel's argument block, or the problem's
// entry of a batched launch -- read where they are used, and not at all by HJ_STAGE_YDOT (dt, a reference, likewise)
template <bool NP, typename T, typename S>
__device__ __forceinline__ T stage_result(const S& s, int stage, T ca, T cb, bool use_y0, const T& dt, T y0v, T centre, T ydot, long long t) {
    T o;
    if (stage == HJ_STAGE_YDOT) o = ydot;
    else {
        o = rk_stage_out<NP>(stage, ca, cb, dt, y0v, centre, ydot);
        if (s.post_prev) o = post_step(s.post_prev, o, use_y0 ? y0v : centre);
        if (s.op_a) o = array_op(s.op_a, o, ((const T*)s.post_a)[t]);
        if (s.op_b) o = array_op(s.op_b, o, ((const T*)s.post_b)[t]);
    }
    return o;
}

// the end of a bound kernel of 256 threads: m[d] = this thread's maximum of alpha_d; one workgroup maximum per axis folded into keys[d]
// (order-preserving keys, zero at launch)
template <int ND>
__device__ __forceinline__ void fold_bound(const double* m, unsigned long long* keys) {
    __shared__ double red[4][ND];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const double w = wave_max(m[d]);
        if (lane == 0) red[wv][d] = w;
    }
    __syncthreads();
    if (threadIdx.x < ND) {
        const int d = threadIdx.x;
        const double w = fmax(fmax(red[0][d], red[1][d]), fmax(red[2][d], red[3][d]));
        if (w > -1e299) key_max(keys + d, w);
    }
}

}  // namespace hj
#endif
