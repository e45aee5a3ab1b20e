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
#include "hj_plants_dev.h"

namespace hjr {

using hjq::make_grid;
using hjq::fill_stencil;
using namespace hj_tool;

// sgn, rk4, RolloutOut, the trajectory itself (rollout_body) and the entry point's checks (check_rollout): hj_rollout_dev.h, shared
// with libhj_hiquery.so, libhj_plant.so and libhj_mc.so; the three Plant<> specialisations: hj_plants_dev.h, shared with libhj_mc.so

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
