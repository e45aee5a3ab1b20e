// libhj_mc.so (include/hj_mc.h): Monte Carlo rollouts of dx = f dt + G dW through a stored value function, for gfx950.
//   noisy_rollout_kernel<T, SCHEME, PLANT>  2^ndim lanes per realisation, as rollout_kernel: hj_rollout_dev.h's rollout_body with hj_mc_dev.h's
//                                           NoisyHooks (noise after a sub-step, the clock policy, the values at recorded columns).  Every lane of a
//                                           group carries the state and computes the realisation's normals redundantly -- the inputs
//                                           are the same, so the bits are; no shuffle, no divergence.
//   normals_kernel                          the generator alone: one thread per (realisation, step, pair of normals)
// hjn_normals_host runs the same __host__ __device__ generator on the host.  No float atomics, no reduction: the sums of a
// probability are the caller's.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hj_tool_host.h"
#include "hj_query_dev.h"
#include "hj_mc_dev.h"

namespace hjn {

using hjq::make_grid;
using hjq::fill_stencil;
using hjq::UpwindSolver;
using namespace hj_tool;

template <typename T, int SCHEME, int PLANT>
__global__ __launch_bounds__(256) void noisy_rollout_kernel(const T* __restrict__ data, long long field_stride, int ntimes,
                                                            const double* __restrict__ x0, long long groups, long long R, QGrid G,
                                                            QStencil<T> S, int sub_samples, double dt_small, hjr_plant P, Noise N,
                                                            hjr::RolloutOut O, McOut E) {
    using PL = hjr::Plant<PLANT>;
    hjr::rollout_body<T, SCHEME, PL, UpwindSolver, hjr_plant, NoisyHooks<PL::ND>>(data, field_stride, ntimes, x0, groups, G, S, sub_samples, dt_small,
                                                                                  P, O, NoisyHooks<PL::ND>{N, E, R, sub_samples, 0, 0.0, 0.0});
}

// thread t = (i * nsteps + s) * npairs + j: the words and the normals of pair j of (first + i, step0 + s)
__global__ __launch_bounds__(256) void normals_kernel(unsigned long long seed, unsigned long long first, long long total,
                                                      long long step0, long long nsteps, int nd, int npairs,
                                                      unsigned* __restrict__ words, double* __restrict__ normals) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long is = t / npairs;
    const int j = (int)(t - is * npairs);
    const long long i = is / nsteps;
    const long long s = is - i * nsteps;
    uint32_t w[4];
    pair_words(seed, first + (unsigned long long)i, (uint32_t)(step0 + s), (uint32_t)j, w);
    if (words) {
#pragma unroll
        for (int k = 0; k < 4; ++k) words[t * 4 + k] = w[k];
    }
    if (normals) {
        double z0, z1;
        pair_normals(w, z0, z1);
        normals[is * nd + 2 * j] = z0;
        if (2 * j + 1 < nd) normals[is * nd + 2 * j + 1] = z1;
    }
}

// ---------------------------------------------------------------------------------------------- host side (the noise's checks: hj_mc_dev.h)
template <typename T, int SCHEME, int PLANT>
static int launch(const hjq_grid* g, const QGrid& G, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                  long long groups, long long R, int sub_samples, double dt_small, const hjr_plant& P, const Noise& N,
                  const hjr::RolloutOut& O, const McOut& E, hipStream_t stream) {
    QStencil<T> S;
    fill_stencil(g, G, S);
    unsigned blocks;
    int rc = blocks_for(groups * (1ll << G.ndim), TOO_MANY_REAL, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((noisy_rollout_kernel<T, SCHEME, PLANT>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (int)ntimes, x0, groups, R, G, S, sub_samples, dt_small, P, N, O, E);
    return launch_done(kernel_name("noisy_rollout_kernel", type_tag<T>::name(), {SCHEME, PLANT}).c_str());
}

// the checks hjn_normals and hjn_normals_host share
static int check_normals(int64_t count, int64_t step0, int64_t nsteps, int nd, const void* words, const void* normals, bool& go) {
    go = false;
    if (nd < 1 || nd > MAXD) return fail(HJ_EINVAL, "nd %d: a step has 1 .. %d normals", nd, MAXD);
    if (count < 0 || nsteps < 0) return fail(HJ_EINVAL, "count and nsteps must not be negative");
    if (step0 < 0 || step0 > 0x100000000ll || nsteps > 0x100000000ll - step0)
        return fail(HJ_EINVAL, "steps %lld .. %lld: the counter holds a step in 32 bits", (long long)step0, (long long)(step0 + nsteps));
    if (count == 0 || nsteps == 0) return HJ_OK;
    if (!words && !normals) return fail(HJ_EINVAL, "null argument: one of out_words and out_normals is needed");
    if (count > (1ll << 40) / nsteps) return fail(HJ_EINVAL, "count * nsteps is too large for one call");
    go = true;
    return HJ_OK;
}

}  // namespace hjn

using namespace hjn;

extern "C" {

int hjn_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals, const double* Gm,
                double sq, int policy, int sub_samples, double dt_small, const hjr_plant* plant, double* final_state,
                int32_t* length, int32_t* status, double* value_end, double* value_min, double* traj, int32_t* t_earliest,
                void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    bool go;
    // check_rollout asks for a trajectory array; here it is optional, so the final states stand in for it
    rc = hjr::check_rollout(G, total, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, final_state, length,
                            status, [&]() {
        const int nd = ham_ndim(plant->id);
        if (nd == 0) return fail(HJ_EUNSUPPORTED, "plant %d has no noisy rollout kernel", (int)plant->id);
        if (nd != G.ndim) return fail(HJ_EINVAL, "plant %d has %d states, the grid %d dimensions", (int)plant->id, nd, G.ndim);
        return (int)HJ_OK;
    }, go);
    if (rc) return rc;
    if ((rc = check_noise(G.ndim, ntimes, sub_samples, nreal, policy, sq, Gm))) return rc;
    if (!go) return HJ_OK;
    if ((rc = check_realisations(G.ndim, nstates, nreal, value_end, value_min))) return rc;
    Noise N;
    N.normals = normals;
    N.first = first_realisation;
    N.seed = seed;
    N.nsteps = (ntimes - 1) * (long long)sub_samples;
    N.sq = sq;
    for (int k = 0; k < MAXD * MAXD; ++k) N.G[k] = k < G.ndim * G.ndim ? Gm[k] : 0.0;
    N.policy = policy;
    const hjr::RolloutOut O{traj, length, t_earliest, status};
    const McOut E{final_state, value_end, value_min};
    static_assert(HJ_HAM_DUBINS_REL == 0 && HJ_HAM_DOUBLE_INTEGRATOR == 1 && HJ_HAM_DOUBLE_PENDULUM == 2, "plant ids name the kernels");
    const long long groups = nstates * nreal;
    return dispatch(g->dtype, scheme, [&](auto t, auto sch) {
        using T = typename decltype(t)::type;
        constexpr int SCH = decltype(sch)::value;
        hipStream_t s = (hipStream_t)stream;
        if (plant->id == 0) return launch<T, SCH, 0>(g, G, data, ntimes, field_stride, x0, groups, nreal, sub_samples, dt_small, *plant, N, O, E, s);
        if (plant->id == 1) return launch<T, SCH, 1>(g, G, data, ntimes, field_stride, x0, groups, nreal, sub_samples, dt_small, *plant, N, O, E, s);
        return launch<T, SCH, 2>(g, G, data, ntimes, field_stride, x0, groups, nreal, sub_samples, dt_small, *plant, N, O, E, s);
    });
}

int hjn_normals(uint64_t seed, uint64_t first, int64_t count, int64_t step0, int64_t nsteps, int nd, uint32_t* out_words,
                double* out_normals, void* stream) {
    bool go;
    int rc = check_normals(count, step0, nsteps, nd, out_words, out_normals, go);
    if (rc || !go) return rc;
    const int npairs = (nd + 1) / 2;
    const long long total = count * nsteps * npairs;
    unsigned blocks;
    rc = blocks_for(total, "too many normals for one launch", blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(normals_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (unsigned long long)first, total, (long long)step0, (long long)nsteps, nd, npairs, (unsigned*)out_words, out_normals);
    return launch_done("normals_kernel");
}

int hjn_normals_host(uint64_t seed, uint64_t first, int64_t count, int64_t step0, int64_t nsteps, int nd, uint32_t* out_words,
                     double* out_normals) {
    bool go;
    int rc = check_normals(count, step0, nsteps, nd, out_words, out_normals, go);
    if (rc || !go) return rc;
    const int npairs = (nd + 1) / 2;
    for (int64_t i = 0; i < count; ++i)
        for (int64_t s = 0; s < nsteps; ++s)
            for (int j = 0; j < npairs; ++j) {
                const int64_t is = i * nsteps + s;
                uint32_t w[4];
                pair_words(seed, first + (uint64_t)i, (uint32_t)(step0 + s), (uint32_t)j, w);
                if (out_words)
                    for (int k = 0; k < 4; ++k) out_words[(is * npairs + j) * 4 + k] = w[k];
                if (out_normals) {
                    double z0, z1;
                    pair_normals(w, z0, z1);
                    out_normals[is * nd + 2 * j] = z0;
                    if (2 * j + 1 < nd) out_normals[is * nd + 2 * j + 1] = z1;
                }
            }
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjn)

}  // extern "C"
