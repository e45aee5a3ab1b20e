// What the host code of libhj_plant.so (hj_plant.hip) and the translation units it generates for hipRTC share: the argument block
// of user_rollout_kernel, and -- device side, when hj_query_dev.h and hj_rollout_dev.h came first -- the kernel's body around a
// plant type.  The block restates QGrid and QStencil<T> of hj_query_dev.h field by field with the number of axes as a template
// parameter, because one host file fills it for both widths (four axes for 2-D .. 4-D plants, six for 5-D / 6-D ones), while
// that header has one width per translation unit.
#ifndef HJ_PLANT_DEV_H
#define HJ_PLANT_DEV_H
#include "hj_device.h"
#include "../../include/hj_plant.h"

namespace hjp {

template <typename T, int MD> struct RolloutArgs {
    const T* data;
    long long field_stride;
    const double* x0;
    long long M;
    int ntimes, sub_samples;
    double dt_small;
    // QGrid
    int n[MD], per[MD];
    long long stride[MD];
    double xmin[MD], xlast[MD], dx[MD];
    // QStencil<T>
    T km[MD];
    T K[MD][hj::HJ_NK];
    hjp_plant P;
    double* traj;
    int* length;
    int* t_earliest;
    int* status;
};

#ifdef HJ_ROLLOUT_DEV_H
// The body of user_rollout_kernel<T, SCHEME> around the plant PL: rollout_body with the number of axes a compile-time constant
// (every loop over axes of the shared functions unrolls) and the upwind rule of that dimension.  256 threads, 2^ND lanes per
// trajectory, 64-bit indexing of traj: all rollout_body's.
template <typename T, int SCHEME, typename PL>
__device__ __forceinline__ void user_rollout(const RolloutArgs<T, hjq::MAXD>& A) {
    constexpr int ND = PL::ND;
    static_assert(ND >= hjq::MIND && ND <= hjq::MAXD, "the unit's HJ_QUERY_MAXD / HJ_QUERY_MIND fit the plant");
    hjq::QGrid G;
    hjq::QStencil<T> S;
    G.ndim = ND;
#pragma unroll
    for (int d = 0; d < hjq::MAXD; ++d) {
        G.n[d] = A.n[d]; G.per[d] = A.per[d]; G.stride[d] = A.stride[d];
        G.xmin[d] = A.xmin[d]; G.xlast[d] = A.xlast[d]; G.dx[d] = A.dx[d];
        S.km[d] = A.km[d];
#pragma unroll
        for (int k = 0; k < hj::HJ_NK; ++k) S.K[d][k] = A.K[d][k];
    }
    const hjr::RolloutOut O{A.traj, A.length, A.t_earliest, A.status};
    if constexpr (ND <= HJ_MAX_DIM)
        hjr::rollout_body<T, SCHEME, PL, hjr::UpwindSolver>(A.data, A.field_stride, A.ntimes, A.x0, A.M, G, S, A.sub_samples, A.dt_small, A.P, O);
    else
        hjr::rollout_body<T, SCHEME, PL, hjr::UpwindHidim>(A.data, A.field_stride, A.ntimes, A.x0, A.M, G, S, A.sub_samples, A.dt_small, A.P, O);
}
#endif

}  // namespace hjp
#endif
