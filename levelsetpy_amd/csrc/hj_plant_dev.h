// What the host code of libhj_plant.so (hj_plant.hip) and the translation units it generates for hipRTC share: the argument block
// of user_rollout_kernel, and -- device side -- the kernel's body around a plant type.  The block holds hj_query_dev.h's grid and
// stencil structs at the width MD: one host file fills it for both widths (four axes for 2-D .. 4-D plants, six for 5-D / 6-D
// ones), a generated unit reads it at its own (HJ_QUERY_MAXD).
#ifndef HJ_PLANT_DEV_H
#define HJ_PLANT_DEV_H
#include "hj_query_dev.h"
#include "hj_rollout_dev.h"
#include "../../include/hj_plant.h"

namespace hjp {

template <typename T, int MD> struct RolloutArgs {
    const T* data;
    long long field_stride;
    const double* x0;
    long long M;
    int ntimes, sub_samples;
    double dt_small;
    hjq::QGridT<MD> G;
    hjq::QStencilT<T, MD> S;
    hjp_plant P;
    double* traj;
    int* length;
    int* t_earliest;
    int* status;
};

// The body of user_rollout_kernel<T, SCHEME> around the plant PL: rollout_body with the number of axes a compile-time constant
// (A.G.ndim is PL::ND, checked by the host: every loop over axes of the shared functions unrolls) and the upwind rule of that
// dimension.  256 threads, 2^ND lanes per trajectory, 64-bit indexing of traj: all rollout_body's.
template <typename T, int SCHEME, typename PL>
__device__ __forceinline__ void user_rollout(const RolloutArgs<T, hjq::MAXD>& A) {
    constexpr int ND = PL::ND;
    static_assert(ND >= hjq::MIND && ND <= hjq::MAXD, "the unit's HJ_QUERY_MAXD / HJ_QUERY_MIND fit the plant");
    const hjq::QGrid G = hjq::at<ND>(A.G);
    const hjr::RolloutOut O{A.traj, A.length, A.t_earliest, A.status};
    if constexpr (ND <= HJ_MAX_DIM)
        hjr::rollout_body<T, SCHEME, PL, hjr::UpwindSolver>(A.data, A.field_stride, A.ntimes, A.x0, A.M, G, A.S, A.sub_samples, A.dt_small, A.P, O);
    else
        hjr::rollout_body<T, SCHEME, PL, hjr::UpwindHidim>(A.data, A.field_stride, A.ntimes, A.x0, A.M, G, A.S, A.sub_samples, A.dt_small, A.P, O);
}

}  // namespace hjp
#endif
