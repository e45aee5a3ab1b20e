// What the host code of libhj_plant.so (hj_plant.hip) and the translation units it generates for hipRTC share: the argument blocks
// of user_rollout_kernel, user_noisy_rollout_kernel, user_filtered_rollout_kernel and user_decide_points_kernel, and -- device side --
// the kernels' bodies around a plant type: rollout_body plain, with hj_mc_dev.h's NoisyHooks, with hj_filter_dev.h's HooksOf.  The block holds hj_query_dev.h's grid and
// stencil structs at the width MD: one host file fills it for both widths (four axes for 2-D .. 4-D plants, six for 5-D / 6-D
// ones), a generated unit reads it at its own (HJ_QUERY_MAXD).
#ifndef HJ_PLANT_DEV_H
#define HJ_PLANT_DEV_H
#include "hj_query_dev.h"
#include "hj_rollout_dev.h"
#include "hj_filter_dev.h"
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

// user_noisy_rollout_kernel's: a rollout of R.M = nstates * nreal groups and hj_mc_dev.h's Noise and McOut, member by member.  G is MD x MD
// HERE, so `policy` and the outputs lie where the unit of that width reads them (hjn::Noise is as wide as the unit that compiles it).
template <typename T, int MD> struct NoisyArgs {
    RolloutArgs<T, MD> R;
    long long nreal;
    const double* normals;
    unsigned long long first, seed;
    long long nsteps;
    double sq;
    double G[MD * MD];                  // ND x ND, row-major, from element 0
    int policy;
    double* final_state;
    double* value_end;
    double* value_min;
};

// user_filtered_rollout_kernel's and user_decide_points_kernel's (R.ntimes: the number of fields, one sub-step, a zero step)
template <typename T, int MD> struct FilterArgs {
    RolloutArgs<T, MD> R;
    hjf::Filter F;
    hjf::FilterOut E;
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

// rollout_body around PL with a hook type: the same two choices
template <typename T, int SCHEME, typename PL, typename HK>
__device__ __forceinline__ void user_hooked(const RolloutArgs<T, hjq::MAXD>& A, const hjr::RolloutOut& O, HK&& H) {
    constexpr int ND = PL::ND;
    static_assert(ND >= hjq::MIND && ND <= hjq::MAXD, "the unit's HJ_QUERY_MAXD / HJ_QUERY_MIND fit the plant");
    const hjq::QGrid G = hjq::at<ND>(A.G);
    if constexpr (ND <= HJ_MAX_DIM)
        hjr::rollout_body<T, SCHEME, PL, hjr::UpwindSolver, hjp_plant, HK>(A.data, A.field_stride, A.ntimes, A.x0, A.M, G, A.S, A.sub_samples, A.dt_small,
                                                                           A.P, O, static_cast<HK&&>(H));
    else
        hjr::rollout_body<T, SCHEME, PL, hjr::UpwindHidim, hjp_plant, HK>(A.data, A.field_stride, A.ntimes, A.x0, A.M, G, A.S, A.sub_samples, A.dt_small,
                                                                          A.P, O, static_cast<HK&&>(H));
}

// user_noisy_rollout_kernel<T, SCHEME>: hj_mc.h's realisation
template <typename T, int SCHEME, typename PL>
__device__ __forceinline__ void user_noisy_rollout(const NoisyArgs<T, hjq::MAXD>& A) {
    hjn::Noise N;
    N.normals = A.normals;
    N.first = A.first;
    N.seed = A.seed;
    N.nsteps = A.nsteps;
    N.sq = A.sq;
#pragma unroll
    for (int k = 0; k < hjq::MAXD * hjq::MAXD; ++k) N.G[k] = A.G[k];
    N.policy = A.policy;
    const hjn::McOut E{A.final_state, A.value_end, A.value_min};
    const hjr::RolloutOut O{A.R.traj, A.R.length, A.R.t_earliest, A.R.status};
    using HK = hjn::NoisyHooks<PL::ND>;
    user_hooked<T, SCHEME, PL, HK>(A.R, O, HK{N, E, A.nreal, A.R.sub_samples, 0, 0.0, 0.0});
}

// user_filtered_rollout_kernel<T, SCHEME> (POINT false) and user_decide_points_kernel<T, SCHEME> (true): hj_filter.h's trajectory and decision
template <typename T, int SCHEME, typename PL, bool POINT>
__device__ __forceinline__ void user_filtered(const FilterArgs<T, hjq::MAXD>& A) {
    using HK = hjf::HooksOf<T, hjf::OwnControl<PL, hjp_plant>, POINT>;
    const hjr::RolloutOut O{A.R.traj, A.R.length, nullptr, A.R.status};
    user_hooked<T, SCHEME, PL, HK>(A.R, O, HK{A.F, A.E, 0.0, 0.0, 0, -1, false, false});
}

}  // namespace hjp
#endif
