// libhj_hiquery.so (include/hj_hiquery.h): value-function queries and rollouts on 5-D and 6-D grids, for gfx950.
//   hi_interp_points_kernel<T>              V at states: one thread per (field, state)
//   hi_costate_points_kernel<T, ND, SCHEME> grad V at states: 2^ND lanes per (field, state), one corner node each -- 32 lanes
//                                           at 5-D (two states per wavefront), the whole wavefront at 6-D
//   hi_project_minmax_kernel<T, WAVE>       min / max over a subset of axes, a thread or a wavefront per output node
//   hi_rollout_kernel<T, SCHEME, PLANT>     a trajectory per 2^ND lanes, from its first state to its last
// Neither the arithmetic nor the checks are restated here: the costate and projection kernels are hj_query_dev.h's costate_body and
// project_body, compiled at six axes (HJ_QUERY_MAXD), the trajectory is hj_rollout_dev.h's rollout_body, and the entry points'
// checks are those headers' host side -- the sources libhj_query.so and libhj_rollout.so compile.  What is this file's own: the
// kernels' frames at a compile-time number of axes, the two plants and the launches.
// The kernels take the grid with `ndim` overwritten by the template's constant (at<ND>), so every loop over axes of the
// shared functions unrolls and lo / w / cC / cL / cR stay in registers.
#include <hip/hip_runtime.h>
#include <cmath>
#define HJ_QUERY_MAXD 6
#define HJ_QUERY_MIND 5
#include "hj_tool_host.h"
#include "../../include/hj_hidim.h"
#include "hj_query_dev.h"
#include "hj_rollout_dev.h"
#include "../../include/hj_hiquery.h"

static_assert(HJ_QUERY_MAXD == HJH_MAX_DIM && HJ_QUERY_MIND == HJH_MIN_DIM, "the header's range is hj_hidim.h's");

namespace hjx {

using hjq::MAXD;
using hjq::QGrid;
using hjq::QStencil;
using hjq::ProjArgs;
using hjq::CostateOut;
using hjq::UpwindHidim;       // the one-sided derivatives of a corner's stencil at 5-D / 6-D
using hjq::at;
using hjq::put;
using hjq::fill_stencil;
using hjq::TOO_MANY;
using hjr::Plant;
using hjr::RolloutOut;
using hjr::TOO_MANY_TRAJ;
using namespace hj_tool;

// ---- (a) V at states: thread t -> field t / M, state t % M
template <typename T>
__global__ __launch_bounds__(256) void hi_interp_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                               const double* __restrict__ xs, long long M, QGrid G,
                                                               void* __restrict__ out, int out_f64) {
#pragma clang fp contract(off)
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= nfields * M) return;
    const long long f = t / M, m = t - f * M;
    double v;
    if (G.ndim == 5) v = hjq::interp_value<T>(at<5>(G), data + f * field_stride, xs + m * 5);
    else v = hjq::interp_value<T>(at<6>(G), data + f * field_stride, xs + m * 6);
    put<T>(out, t, v, out_f64);
}

// ---- (b) grad V at states: costate_body at a compile-time number of axes, the upwind rule of 5-D / 6-D
template <typename T, int ND, int SCHEME>
__global__ __launch_bounds__(256) void hi_costate_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                                const double* __restrict__ xs, long long M, QGrid G0, QStencil<T> S,
                                                                CostateOut O) {
    hjq::costate_body<T, SCHEME, ND, UpwindHidim>(data, field_stride, nfields, xs, M, at<ND>(G0), S, O);
}

// ---- (c) min / max over a subset of axes: project_body, five loops over the removed axes
template <typename T, bool WAVE>
__global__ __launch_bounds__(256) void hi_project_minmax_kernel(const T* __restrict__ data, T* __restrict__ out, ProjArgs A) {
    hjq::project_body<T, WAVE>(data, out, A);
}

}  // namespace hjx

// ---- (d) the plants of hjx_rollout: controls(costate p, state x) -> (c0, c1), f(x; c0, c1) -> xdot, as dynamics.py's
// get_opt_u / get_opt_v / dynamics.  One operation per statement.
namespace hjr {

template <> struct Plant<HJH_HAM_PLANE5D> {
    static constexpr int ND = 5;
    // c0 = a, the acceleration; c1 = al, the angular acceleration: both are the control
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& a, double& al) {
#pragma clang fp contract(off)
        a = P.params[0] * sgn(p[3]);
        al = P.params[1] * sgn(p[4]);
        if (P.u_mode == HJR_MODE_MIN) { a = -a; al = -al; }
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double a, double al, double* k) {
#pragma clang fp contract(off)
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        k[0] = x[3] * c;
        k[1] = x[3] * s;
        k[2] = x[4];
        k[3] = a;
        k[4] = al;
    }
};

template <> struct Plant<HJH_HAM_DUBINS_PAIR6D> {
    static constexpr int ND = 6;
    // c0 = u, the evader's turn rate (the control); c1 = d, the pursuer's (the disturbance)
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& u, double& d) {
#pragma clang fp contract(off)
        u = P.params[2] * sgn(p[2]);
        if (P.u_mode == HJR_MODE_MIN) u = -u;
        d = P.params[3] * sgn(p[5]);
        if (P.d_mode == HJR_MODE_MIN) d = -d;
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double u, double d, double* k) {
#pragma clang fp contract(off)
        const double ve = P.params[0], vp = P.params[1];
        const double c2 = cos(x[2]);
        const double s2 = sin(x[2]);
        const double c5 = cos(x[5]);
        const double s5 = sin(x[5]);
        k[0] = ve * c2;
        k[1] = ve * s2;
        k[2] = u;
        k[3] = vp * c5;
        k[4] = vp * s5;
        k[5] = d;
    }
};

}  // namespace hjr

namespace hjx {

// A finished trajectory idles in its wavefront (rollout_body never returns early), so every __shfl of group_sum runs with all
// lanes of its group active.
template <typename T, int SCHEME, int PLANT>
__global__ __launch_bounds__(256) void hi_rollout_kernel(const T* __restrict__ data, long long field_stride, int ntimes,
                                                         const double* __restrict__ x0, long long M, QGrid G0, QStencil<T> S,
                                                         int sub_samples, double dt_small, hjr_plant P, RolloutOut O) {
    const QGrid G = at<Plant<PLANT>::ND>(G0);
    hjr::rollout_body<T, SCHEME, Plant<PLANT>, UpwindHidim>(data, field_stride, ntimes, x0, M, G, S, sub_samples, dt_small, P, O);
}

// ---------------------------------------------------------------------------------------------- host side
template <typename T>
static int interp_launch(const QGrid& G, const void* data, int64_t nfields, int64_t field_stride, const double* xs, int64_t M,
                         void* out, int out_f64, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M, TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_interp_points_kernel<T>), dim3(blocks), dim3(256), 0, stream, (const T*)data, (long long)field_stride,
                       (long long)nfields, xs, (long long)M, G, out, out_f64);
    return launch_done(name);
}

template <typename T, int ND, int SCHEME>
static int costate_launch(const hjh_grid* g, const QGrid& G, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                          int64_t M, const CostateOut& O, hipStream_t stream) {
    QStencil<T> S;
    fill_stencil(g, G, S);
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M * (1ll << ND), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_costate_points_kernel<T, ND, SCHEME>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (long long)nfields, xs, (long long)M, G, S, O);
    return launch_done(kernel_name("hi_costate_points_kernel", type_tag<T>::name(), {ND, SCHEME}).c_str());
}

template <typename T, bool WAVE>
static int project_launch(const void* data, void* out, const ProjArgs& A, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for(A.nfields * A.nout * (WAVE ? 64 : 1), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_project_minmax_kernel<T, WAVE>), dim3(blocks), dim3(256), 0, stream, (const T*)data, (T*)out, A);
    return launch_done(name);
}

template <typename T, int SCHEME, int PLANT>
static int rollout_launch(const hjh_grid* g, const QGrid& G, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                          int64_t M, int sub_samples, double dt_small, const hjr_plant& P, const RolloutOut& O, hipStream_t stream) {
    QStencil<T> S;
    fill_stencil(g, G, S);
    unsigned blocks;
    int rc = blocks_for((long long)M * (1ll << G.ndim), TOO_MANY_TRAJ, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_rollout_kernel<T, SCHEME, PLANT>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (int)ntimes, x0, (long long)M, G, S, sub_samples, dt_small, P, O);
    return launch_done(kernel_name("hi_rollout_kernel", type_tag<T>::name(), {SCHEME, PLANT}).c_str());
}

// state dimension of a plant of this library, 0 for any other id
static int plant_ndim(int id) { return id == HJH_HAM_PLANE5D ? 5 : (id == HJH_HAM_DUBINS_PAIR6D ? 6 : 0); }

}  // namespace hjx

using namespace hjx;

extern "C" {

int hjx_interp_points(const hjh_grid* g, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                      int64_t nstates, void* out, int out_f64, void* stream) {
    QGrid G;
    if (int rc = hjq::interp_points(g, data, nfields, field_stride, xs, nstates, out, G)) return rc;
    if (g->dtype == HJ_F64)
        return interp_launch<double>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "hi_interp_points_kernel<double>");
    return interp_launch<float>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "hi_interp_points_kernel<float>");
}

int hjx_costate_points(const hjh_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                       int64_t nstates, void* costate, void* derivL, void* derivR, void* value, int out_f64, void* stream) {
    QGrid G;
    if (int rc = hjq::costate_points(g, scheme, data, nfields, field_stride, xs, nstates, costate, G)) return rc;
    const CostateOut O{costate, derivL, derivR, value, out_f64};
    return dispatch(g->dtype, scheme, [&](auto t, auto sch) {
        using T = typename decltype(t)::type;
        constexpr int SCH = decltype(sch)::value;
        if (G.ndim == 5) return costate_launch<T, 5, SCH>(g, G, data, nfields, field_stride, xs, nstates, O, (hipStream_t)stream);
        return costate_launch<T, 6, SCH>(g, G, data, nfields, field_stride, xs, nstates, O, (hipStream_t)stream);
    });
}

int hjx_project_minmax(const hjh_grid* g, const void* data, int64_t nfields, int64_t field_stride, unsigned remove_mask, int op,
                       void* out, void* stream) {
    ProjArgs A;
    bool wave;
    if (int rc = hjq::project_minmax(g, data, nfields, field_stride, remove_mask, op, out, A, wave)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (g->dtype == HJ_F64)
        return wave ? project_launch<double, true>(data, out, A, s, "hi_project_minmax_kernel<double, true>")
                    : project_launch<double, false>(data, out, A, s, "hi_project_minmax_kernel<double, false>");
    return wave ? project_launch<float, true>(data, out, A, s, "hi_project_minmax_kernel<float, true>")
                : project_launch<float, false>(data, out, A, s, "hi_project_minmax_kernel<float, false>");
}

int hjx_rollout(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant, double* traj, int32_t* length,
                int32_t* t_earliest, int32_t* status, void* stream) {
    QGrid G;
    long long total;
    int rc = hjq::make_grid(g, G, total);
    if (rc) return rc;
    bool go;
    rc = hjr::check_rollout(G, total, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, traj, length, status, [&]() {
        const int nd = plant_ndim(plant->id);
        if (nd == 0) return fail(HJ_EUNSUPPORTED, "plant %d has no rollout kernel on 5-D / 6-D grids", (int)plant->id);
        if (nd != G.ndim) return fail(HJ_EINVAL, "plant %d has %d states, the grid %d dimensions", (int)plant->id, nd, G.ndim);
        return (int)HJ_OK;
    }, go);
    if (rc || !go) return rc;
    const RolloutOut O{traj, length, t_earliest, status};
    static_assert(HJH_HAM_PLANE5D == 50 && HJH_HAM_DUBINS_PAIR6D == 51, "plant ids name the kernels");
    return dispatch(g->dtype, scheme, [&](auto t, auto sch) {
        using T = typename decltype(t)::type;
        constexpr int SCH = decltype(sch)::value;
        if (plant->id == HJH_HAM_PLANE5D)
            return rollout_launch<T, SCH, 50>(g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, O, (hipStream_t)stream);
        return rollout_launch<T, SCH, 51>(g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, O, (hipStream_t)stream);
    });
}

HJ_TOOL_LAST_SYMBOLS(hjx)

}  // extern "C"
