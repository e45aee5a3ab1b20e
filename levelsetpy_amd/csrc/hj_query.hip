// libhj_query.so (include/hj_query.h): value-function queries at states for gfx950.
//   interp_points_kernel   V at states: one thread per (field, state)
//   costate_points_kernel  grad V at states: 2^ndim lanes per (field, state), one corner node each; the 7-point stencils of
//                          the corner go through hj_device.h's ghost_value and upwind<SCHEME> -- the solver's own source,
//                          so a corner costate has the bits computeGradients gives that node
//   project_minmax_kernel  min / max over a subset of axes, a thread or a wavefront per output node
// The interpolation arithmetic is hji_solver._eval_point's, operation by operation (contraction off: `v += wt * val`
// must stay a multiply and an add), so the fp64 results equal the host loop's bit for bit.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hj_tool_host.h"
#include "hj_query_dev.h"

namespace hjq {

using namespace hj_tool;

template <typename T>
__device__ __forceinline__ void put(void* out, long long i, double v, int out_f64) {
    if (out_f64) ((double*)out)[i] = v;
    else ((T*)out)[i] = (T)v;
}

// ---- (a) V at states: thread t -> field t / M, state t % M
template <typename T>
__global__ __launch_bounds__(256) void interp_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                            const double* __restrict__ xs, long long M, QGrid G,
                                                            void* __restrict__ out, int out_f64) {
#pragma clang fp contract(off)
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= nfields * M) return;
    const long long f = t / M, m = t - f * M;
    const double v = interp_value<T>(G, data + f * field_stride, xs + m * G.ndim);
    put<T>(out, t, v, out_f64);
}

// ---- (b) grad V at states
struct CostateOut {
    void* costate;
    void* derivL;
    void* derivR;
    void* value;
    int out_f64;
};

template <typename T, int SCHEME>
__global__ __launch_bounds__(256) void costate_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                             const double* __restrict__ xs, long long M, QGrid G, QStencil<T> S,
                                                             CostateOut O) {
    const int lanes = 1 << G.ndim;                 // 2 .. 16: divides the wavefront, groups never straddle one
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long grp = t / lanes;
    const int c = (int)(t - grp * lanes);
    if (grp >= nfields * M) return;                // whole groups leave together
    const long long f = grp / M, m = grp - f * M;
    int lo[MAXD];
    double w[MAXD];
    const bool inside = locate(G, xs + m * G.ndim, lo, w);
    long long off;
    const double wt = corner(G, lo, w, c, off);
    const int used = wt != 0.0;
    T cC[MAXD], cL[MAXD], cR[MAXD];
    T raw = T(0);
#pragma unroll
    for (int d = 0; d < MAXD; ++d) cC[d] = cL[d] = cR[d] = T(0);
    if (inside && used) {
        const T* pc0 = data + f * field_stride + off;
        raw = *pc0;
        if (!finite(raw)) {
            // the node's own NaN / inf is put back after the differences (computeGradients: NaN stays NaN, +-inf becomes +inf)
            const T back = raw != raw ? raw : T(__builtin_inf());
#pragma unroll
            for (int d = 0; d < MAXD; ++d) cC[d] = cL[d] = cR[d] = back;
        } else {
#pragma unroll
            for (int d = 0; d < MAXD; ++d) {
                if (d >= G.ndim) break;
                int j = lo[d] + ((c >> d) & 1);
                if (G.per[d] && j >= G.n[d]) j -= G.n[d];
                T v[7];
                gather_axis<T>(pc0, G.stride[d], j, G.n[d], G.per[d] != 0, S.km[d], raw, v);
                T L, R;
                hj::upwind<SCHEME, T>(v, S.K[d], T(0), L, R);
                cL[d] = L;
                cR[d] = R;
                cC[d] = T(0.5) * (L + R);
            }
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int d = 0; d < MAXD; ++d) {
        if (d >= G.ndim) break;
        double p, q, r;
        {
#pragma clang fp contract(off)
            p = wt * (double)cC[d];
            q = wt * (double)cL[d];
            r = wt * (double)cR[d];
        }
        const double sC = group_sum(p, used, lanes);
        if (c == 0) put<T>(O.costate, grp * G.ndim + d, inside ? sC : nan, O.out_f64);
        if (O.derivL) {
            const double sL = group_sum(q, used, lanes);
            if (c == 0) put<T>(O.derivL, grp * G.ndim + d, inside ? sL : nan, O.out_f64);
        }
        if (O.derivR) {
            const double sR = group_sum(r, used, lanes);
            if (c == 0) put<T>(O.derivR, grp * G.ndim + d, inside ? sR : nan, O.out_f64);
        }
    }
    if (O.value) {
        double p;
        {
#pragma clang fp contract(off)
            p = wt * (double)raw;
        }
        const double sV = group_sum(p, used, lanes);
        if (c == 0) put<T>(O.value, grp, inside ? sV : nan, O.out_f64);
    }
}

// ---- (c) min / max over a subset of axes (ProjArgs, Red, proj_base: hj_query_dev.h)
// WAVE = false: the last axis is kept -- one thread per output node, neighbouring threads read neighbouring elements.
// WAVE = true:  the last axis is removed -- one wavefront per output node; its lanes stride the last axis (neighbouring
//               lanes read neighbouring elements) inside loops over the other removed axes.
// The removed axes sit at the END of rem_n / rem_s (unused leading slots have n = 1), so the loops need no index division.
template <typename T, bool WAVE>
__global__ __launch_bounds__(256) void project_minmax_kernel(const T* __restrict__ data, T* __restrict__ out, ProjArgs A) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long node = WAVE ? t / 64 : t;
    const int lane = WAVE ? (int)(t & 63) : 0;
    if (node >= A.nfields * A.nout) return;         // WAVE: whole wavefronts leave together
    const long long f = node / A.nout, o = node - f * A.nout;
    const T* __restrict__ p = data + f * A.field_stride + proj_base<T>(A, o);
    const T start = A.op == HJQ_MIN ? T(__builtin_inf()) : -T(__builtin_inf());
    Red<T> acc{start, 0};
    static_assert(MAXD == 4, "three loops: at most MAXD - 1 removed axes");
    for (int i0 = 0; i0 < A.rem_n[1]; ++i0)
        for (int i1 = 0; i1 < A.rem_n[2]; ++i1) {
            const T* __restrict__ row = p + i0 * A.rem_s[1] + i1 * A.rem_s[2];
            for (int i2 = lane; i2 < A.rem_n[3]; i2 += WAVE ? 64 : 1) acc.take(row[i2 * A.rem_s[3]], A.op);
        }
    if (WAVE) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const T ov = __shfl_xor(acc.v, s, 64);
            const int on = __shfl_xor(acc.nan, s, 64);
            acc.nan |= on;
            acc.take(ov, A.op);
        }
        if (lane != 0) return;
    }
    out[node] = acc.nan ? T(__builtin_nan("")) : acc.v;
}

// ---------------------------------------------------------------------------------------------- host side
// (check_points, TOO_MANY: hj_query_dev.h)
template <typename T>
static int interp_launch(const QGrid& G, const void* data, int64_t nfields, int64_t field_stride, const double* xs, int64_t M,
                  void* out, int out_f64, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M, TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((interp_points_kernel<T>), dim3(blocks), dim3(256), 0, stream, (const T*)data, (long long)field_stride,
                       (long long)nfields, xs, (long long)M, G, out, out_f64);
    return launch_done(name);
}

template <typename T, int SCHEME>
static int costate_launch(const hjq_grid* g, const QGrid& G, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                   int64_t M, const CostateOut& O, hipStream_t stream, const char* name) {
    QStencil<T> S;
    for (int d = 0; d < MAXD; ++d) {
        S.km[d] = (d < G.ndim && g->toward_zero[d]) ? T(-1) : T(1);
        hj::fill_stencil_constants<T>(G.dx[d], S.K[d]);
    }
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M * (1ll << G.ndim), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((costate_points_kernel<T, SCHEME>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (long long)nfields, xs, (long long)M, G, S, O);
    return launch_done(name);
}

template <typename T, bool WAVE>
static int project_launch(const void* data, void* out, const ProjArgs& A, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for(A.nfields * A.nout * (WAVE ? 64 : 1), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((project_minmax_kernel<T, WAVE>), dim3(blocks), dim3(256), 0, stream, (const T*)data, (T*)out, A);
    return launch_done(name);
}

}  // namespace hjq

using namespace hjq;

extern "C" {

int hjq_interp_points(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                      int64_t nstates, void* out, int out_f64, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!out) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_points(g, G, total, data, nfields, field_stride, xs, nstates, false))) return rc;
    if (g->dtype == HJ_F64)
        return interp_launch<double>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "interp_points_kernel<double>");
    return interp_launch<float>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "interp_points_kernel<float>");
}

int hjq_costate_points(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                       int64_t nstates, void* costate, void* derivL, void* derivR, void* value, int out_f64, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!costate) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_point_scheme(scheme, "point"))) return rc;
    if ((rc = check_points(g, G, total, data, nfields, field_stride, xs, nstates, true))) return rc;
    const CostateOut O{costate, derivL, derivR, value, out_f64};
    hipStream_t s = (hipStream_t)stream;
#define HJQ_COSTATE(T, SCH) return costate_launch<T, SCH>(g, G, data, nfields, field_stride, xs, nstates, O, s, "costate_points_kernel<" #T ", " #SCH ">")
    if (g->dtype == HJ_F64) {
        if (scheme == HJ_ENO2) HJQ_COSTATE(double, 0);
        if (scheme == HJ_ENO3) HJQ_COSTATE(double, 1);
        HJQ_COSTATE(double, 3);
    }
    if (scheme == HJ_ENO2) HJQ_COSTATE(float, 0);
    if (scheme == HJ_ENO3) HJQ_COSTATE(float, 1);
    HJQ_COSTATE(float, 3);
#undef HJQ_COSTATE
}

int hjq_project_minmax(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, unsigned remove_mask, int op,
                       void* out, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!data || !out) return fail(HJ_EINVAL, "null argument");
    if (nfields < 1) return fail(HJ_EINVAL, "nfields must be positive");
    if (nfields > 1 && field_stride < total) return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, total);
    if (op != HJQ_MIN && op != HJQ_MAX) return fail(HJ_EINVAL, "unknown projection %d", op);
    const unsigned all = (1u << G.ndim) - 1u;
    if ((remove_mask & ~all) || remove_mask == 0 || remove_mask == all)
        return fail(HJ_EINVAL, "remove_mask %#x must name a non-empty proper subset of the %d axes", remove_mask, G.ndim);
    ProjArgs A;
    A.nkeep = A.nrem = 0;
    A.nout = 1;
    for (int d = 0; d < MAXD; ++d) { A.keep_n[d] = A.rem_n[d] = 1; A.keep_s[d] = A.rem_s[d] = 0; }
    for (int d = 0; d < G.ndim; ++d) {
        if (remove_mask >> d & 1u) {
            ++A.nrem;
        } else {
            A.keep_n[A.nkeep] = G.n[d]; A.keep_s[A.nkeep] = G.stride[d]; ++A.nkeep; A.nout *= G.n[d];
        }
    }
    for (int d = G.ndim - 1, k = MAXD - 1; d >= 0; --d)          // removed axes right-aligned: the last one is the innermost loop
        if (remove_mask >> d & 1u) { A.rem_n[k] = G.n[d]; A.rem_s[k] = G.stride[d]; --k; }
    A.field_stride = field_stride;
    A.nfields = nfields;
    A.op = op;
    const bool wave = remove_mask >> (G.ndim - 1) & 1u;
    hipStream_t s = (hipStream_t)stream;
    if (g->dtype == HJ_F64)
        return wave ? project_launch<double, true>(data, out, A, s, "project_minmax_kernel<double, true>")
                    : project_launch<double, false>(data, out, A, s, "project_minmax_kernel<double, false>");
    return wave ? project_launch<float, true>(data, out, A, s, "project_minmax_kernel<float, true>")
                : project_launch<float, false>(data, out, A, s, "project_minmax_kernel<float, false>");
}

HJ_TOOL_LAST_SYMBOLS(hjq)

}  // extern "C"
