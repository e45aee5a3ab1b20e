// libhj_query.so (include/hj_query.h): value-function queries at states for gfx950.
//   interp_points_kernel   V at states: one thread per (field, state)
//   costate_points_kernel  grad V at states: 2^ndim lanes per (field, state), one corner node each; the 7-point stencils of
//                          the corner go through hj_device.h's ghost_value and upwind<SCHEME> -- the solver's own source,
//                          so a corner costate has the bits computeGradients gives that node
//   project_minmax_kernel  min / max over a subset of axes, a thread or a wavefront per output node
// The interpolation arithmetic is hji_solver._eval_point's, operation by operation (contraction off: `v += wt * val`
// must stay a multiply and an add), so the fp64 results equal the host loop's bit for bit.
// The bodies of the costate and projection kernels and the entry points' checks are hj_query_dev.h's, which libhj_hiquery.so
// compiles at six axes; this file holds the kernels' frames at four axes and the launches.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hj_tool_host.h"
#include "hj_query_dev.h"

namespace hjq {

using namespace hj_tool;

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

// ---- (b) grad V at states: costate_body at a run-time number of axes, the solver's upwind rule
template <typename T, int SCHEME>
__global__ __launch_bounds__(256) void costate_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                             const double* __restrict__ xs, long long M, QGrid G, QStencil<T> S,
                                                             CostateOut O) {
    costate_body<T, SCHEME, 0, UpwindSolver>(data, field_stride, nfields, xs, M, G, S, O);
}

// ---- (c) min / max over a subset of axes: project_body, three loops over the removed axes
template <typename T, bool WAVE>
__global__ __launch_bounds__(256) void project_minmax_kernel(const T* __restrict__ data, T* __restrict__ out, ProjArgs A) {
    project_body<T, WAVE>(data, out, A);
}

// ---------------------------------------------------------------------------------------------- host side
// (the entry points' checks, fill_stencil, TOO_MANY: hj_query_dev.h)
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
                   int64_t M, const CostateOut& O, hipStream_t stream) {
    QStencil<T> S;
    fill_stencil(g, G, S);
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M * (1ll << G.ndim), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((costate_points_kernel<T, SCHEME>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (long long)nfields, xs, (long long)M, G, S, O);
    return launch_done(kernel_name("costate_points_kernel", type_tag<T>::name(), {SCHEME}).c_str());
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
    if (int rc = interp_points(g, data, nfields, field_stride, xs, nstates, out, G)) return rc;
    if (g->dtype == HJ_F64)
        return interp_launch<double>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "interp_points_kernel<double>");
    return interp_launch<float>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "interp_points_kernel<float>");
}

int hjq_costate_points(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                       int64_t nstates, void* costate, void* derivL, void* derivR, void* value, int out_f64, void* stream) {
    QGrid G;
    if (int rc = costate_points(g, scheme, data, nfields, field_stride, xs, nstates, costate, G)) return rc;
    const CostateOut O{costate, derivL, derivR, value, out_f64};
    return dispatch(g->dtype, scheme, [&](auto t, auto sch) {
        return costate_launch<typename decltype(t)::type, decltype(sch)::value>(g, G, data, nfields, field_stride, xs, nstates, O, (hipStream_t)stream);
    });
}

int hjq_project_minmax(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, unsigned remove_mask, int op,
                       void* out, void* stream) {
    ProjArgs A;
    bool wave;
    if (int rc = project_minmax(g, data, nfields, field_stride, remove_mask, op, out, A, wave)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (g->dtype == HJ_F64)
        return wave ? project_launch<double, true>(data, out, A, s, "project_minmax_kernel<double, true>")
                    : project_launch<double, false>(data, out, A, s, "project_minmax_kernel<double, false>");
    return wave ? project_launch<float, true>(data, out, A, s, "project_minmax_kernel<float, true>")
                : project_launch<float, false>(data, out, A, s, "project_minmax_kernel<float, false>");
}

HJ_TOOL_LAST_SYMBOLS(hjq)

}  // extern "C"
