// libhj_rollout.so (include/hj_rollout.h): computeOptTraj for many initial states in one launch, for gfx950.
//   rollout_kernel<T, SCHEME, PLANT>  2^ndim lanes per trajectory, as costate_points_kernel: lane c owns corner c of the cell
//                                     that holds the state, every lane of the group carries the state redundantly, and the
//                                     corners' terms are added by hj_query_dev.h's group_sum in ascending corner order.  An
//                                     interpolated value or costate therefore has the bits interp_points_kernel and
//                                     costate_points_kernel give for that state, and the trajectory the bits computeOptTraj
//                                     gives with the built-in system's own methods (levelsetpy_amd/dynamics.py).
// Control flow is uniform inside a group (every lane holds the same state, bounds and flags) and predicated across groups: a
// finished trajectory sets `done` and idles through the remaining time stamps, it never returns or breaks, so every __shfl of
// group_sum runs with all lanes of its group active.  State, weights, controls and dynamics are fp64 with contraction off;
// the stencil arithmetic is T, as in the costate kernel.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hj_tool_host.h"
#include "hj_query_dev.h"
#include "hj_rollout_dev.h"

namespace hjr {

using hjq::make_grid;
using hjq::fill_stencil;
using namespace hj_tool;

// sgn, rk4, RolloutOut, the trajectory itself (rollout_body) and the entry point's checks (check_rollout): hj_rollout_dev.h, shared
// with libhj_hiquery.so and libhj_plant.so

template <> struct Plant<HJ_HAM_DUBINS_REL> {
    static constexpr int ND = 3;
    // c0 = a, the evader's turn rate (the control); c1 = b, the pursuer's (the disturbance)
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& a, double& b) {
#pragma clang fp contract(off)
        const double w = P.params[2];
        const double s1 = p[0] * x[1];
        const double s2 = p[1] * x[0];
        double s = s1 - s2;
        s = s - p[2];
        a = w * sgn(s);
        if (P.u_mode == HJR_MODE_MIN) a = -a;
        b = w * sgn(p[2]);
        if (P.d_mode == HJR_MODE_MIN) b = -b;
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double a, double b, double* k) {
#pragma clang fp contract(off)
        const double ve = P.params[0], vp = P.params[1];
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        const double vc = vp * c;
        const double drift = -ve + vc;
        const double ax2 = a * x[1];
        k[0] = drift + ax2;
        const double vs = vp * s;
        const double ax1 = a * x[0];
        k[1] = vs - ax1;
        k[2] = b - a;
    }
};

template <> struct Plant<HJ_HAM_DOUBLE_INTEGRATOR> {
    static constexpr int ND = 2;
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& u, double& unused) {
#pragma clang fp contract(off)
        u = P.params[0] * sgn(p[1]);
        if (P.u_mode == HJR_MODE_MIN) u = -u;
        unused = 0.0;
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double u, double, double* k) {
        k[0] = x[1];
        k[1] = u;
    }
};

template <> struct Plant<HJ_HAM_DOUBLE_PENDULUM> {
    static constexpr int ND = 4;
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& u1, double& u2) {
#pragma clang fp contract(off)
        u1 = P.params[0] * sgn(p[1]);
        u2 = P.params[0] * sgn(p[3]);
        if (P.u_mode == HJR_MODE_MIN) { u1 = -u1; u2 = -u2; }
    }
    // the drift in the expression order of DoublePendulum4D._drift (every product and sum left to right)
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double u1, double u2, double* k) {
#pragma clang fp contract(off)
        constexpr double G = 9.8, L1 = 1.0, L2 = 1.0, M1 = 1.0, M2 = 1.0;
        const double w1 = x[1], w2 = x[3];
        const double s1 = sin(x[0]), c1 = cos(x[0]), s2 = sin(x[2]), c2 = cos(x[2]);
        const double a0 = s2 * c1, a1 = c2 * s1;
        const double sd = a0 - a1;
        const double b0 = c2 * c1, b1 = s2 * s1;
        const double cd = b0 + b1;
        const double m12 = M1 + M2;
        double t = M2 * L1; t = t * cd; t = t * cd;
        const double den1 = m12 * L1 - t;
        double q1 = M2 * L1; q1 = q1 * w1; q1 = q1 * w1; q1 = q1 * sd; q1 = q1 * cd;
        double q2 = M2 * G; q2 = q2 * s2; q2 = q2 * cd;
        double q3 = M2 * L2; q3 = q3 * w2; q3 = q3 * w2; q3 = q3 * sd;
        double q4 = m12 * G; q4 = q4 * s1;
        double n1 = q1 + q2; n1 = n1 + q3; n1 = n1 - q4;
        const double f1 = n1 / den1;
        const double den2 = (L2 / L1) * den1;
        double r1 = -M2 * L2; r1 = r1 * w2; r1 = r1 * w2; r1 = r1 * sd; r1 = r1 * cd;
        double r2 = m12 * G; r2 = r2 * s1; r2 = r2 * cd;
        double r3 = m12 * L1; r3 = r3 * w1; r3 = r3 * w1; r3 = r3 * sd;
        double r4 = m12 * G; r4 = r4 * s2;
        double n3 = r1 + r2; n3 = n3 - r3; n3 = n3 - r4;
        const double f3 = n3 / den2;
        k[0] = w1;
        k[1] = f1 + u1;
        k[2] = w2;
        k[3] = f3 + u2;
    }
};

template <typename T, int SCHEME, int PLANT>
__global__ __launch_bounds__(256) void rollout_kernel(const T* __restrict__ data, long long field_stride, int ntimes,
                                                      const double* __restrict__ x0, long long M, QGrid G, QStencil<T> S,
                                                      int sub_samples, double dt_small, hjr_plant P, RolloutOut O) {
    rollout_body<T, SCHEME, Plant<PLANT>, UpwindSolver>(data, field_stride, ntimes, x0, M, G, S, sub_samples, dt_small, P, O);
}

// ---------------------------------------------------------------------------------------------- host side
template <typename T, int SCHEME, int PLANT>
static int launch(const hjq_grid* g, const QGrid& G, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                  int64_t M, int sub_samples, double dt_small, const hjr_plant& P, const RolloutOut& O, hipStream_t stream) {
    QStencil<T> S;
    fill_stencil(g, G, S);
    unsigned blocks;
    int rc = blocks_for((long long)M * (1ll << G.ndim), TOO_MANY_TRAJ, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((rollout_kernel<T, SCHEME, PLANT>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (int)ntimes, x0, (long long)M, G, S, sub_samples, dt_small, P, O);
    return launch_done(kernel_name("rollout_kernel", type_tag<T>::name(), {SCHEME, PLANT}).c_str());
}

}  // namespace hjr

using namespace hjr;

extern "C" {

int hjr_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant, double* traj, int32_t* length,
                int32_t* t_earliest, int32_t* status, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    bool go;
    rc = check_rollout(G, total, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, traj, length, status, [&]() {
        const int nd = ham_ndim(plant->id);
        if (nd == 0) return fail(HJ_EUNSUPPORTED, "plant %d has no rollout kernel", (int)plant->id);
        if (nd != G.ndim) return fail(HJ_EINVAL, "plant %d has %d states, the grid %d dimensions", (int)plant->id, nd, G.ndim);
        return (int)HJ_OK;
    }, go);
    if (rc || !go) return rc;
    const RolloutOut O{traj, length, t_earliest, status};
    static_assert(HJ_HAM_DUBINS_REL == 0 && HJ_HAM_DOUBLE_INTEGRATOR == 1 && HJ_HAM_DOUBLE_PENDULUM == 2, "plant ids name the kernels");
    return dispatch(g->dtype, scheme, [&](auto t, auto sch) {
        using T = typename decltype(t)::type;
        constexpr int SCH = decltype(sch)::value;
        hipStream_t s = (hipStream_t)stream;
        if (plant->id == 0) return launch<T, SCH, 0>(g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, O, s);
        if (plant->id == 1) return launch<T, SCH, 1>(g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, O, s);
        return launch<T, SCH, 2>(g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, O, s);
    });
}

HJ_TOOL_LAST_SYMBOLS(hjr)

}  // extern "C"
