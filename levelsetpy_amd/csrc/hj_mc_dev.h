// Device code of libhj_mc.so (hj_mc.hip, include/hj_mc.h): the counter-based generator, written once for the host and the device,
// and the hooks that turn hj_rollout_dev.h's rollout_body into a noisy realisation.  There is ONE source of the trajectory: the noise, the
// clock policy and the per-realisation outputs enter rollout_body through its hook type (NoisyHooks below), the plants are hj_plants_dev.h's,
// shared with libhj_rollout.so.  tests/mc_ref.py restates the result.
// Include after hj_query_dev.h.
#ifndef HJ_MC_DEV_H
#define HJ_MC_DEV_H
#include "hj_rollout_dev.h"
#include "hj_plants_dev.h"
#include "../../include/hj_mc.h"

namespace hjn {

// ---------------------------------------------------------------------------------------------- the generator
__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32-10: counter c[4], key k[2] -> w[4]
__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t* c, const uint32_t* k, uint32_t* w) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        if (round) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the words of pair j of (realisation r, step): counter (r_lo, r_hi, step, j), key (seed_lo, seed_hi)
__host__ __device__ __forceinline__ void pair_words(uint64_t seed, uint64_t r, uint32_t step, uint32_t j, uint32_t* w) {
    const uint32_t c[4] = {(uint32_t)r, (uint32_t)(r >> 32), step, j};
    const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32_10(c, k, w);
}

// Box-Muller on 53-bit uniforms, one operation per statement
__host__ __device__ __forceinline__ void pair_normals(const uint32_t* w, double& z0, double& z1) {
#pragma clang fp contract(off)
    const uint64_t k1 = ((uint64_t)(w[0] >> 5) << 26) + (uint64_t)(w[1] >> 6);
    const uint64_t k2 = ((uint64_t)(w[2] >> 5) << 26) + (uint64_t)(w[3] >> 6);
    const double two53 = 1.1102230246251565e-16;          // 2^-53
    const double u1 = (double)(k1 + 1) * two53;           // (0, 1]: k1 + 1 <= 2^53 is exact
    const double u2 = (double)k2 * two53;                 // [0, 1)
    const double l = log(u1);
    const double m = -2.0 * l;
    const double rad = sqrt(m);
    const double a = 6.283185307179586 * u2;
    const double ca = cos(a);
    const double sa = sin(a);
    z0 = rad * ca;
    z1 = rad * sa;
}

// the nd normals of (r, step) into xi (room for an even count)
template <int ND> __host__ __device__ __forceinline__ void step_normals(uint64_t seed, uint64_t r, uint32_t step, double* xi) {
#pragma unroll
    for (int j = 0; j < (ND + 1) / 2; ++j) {
        uint32_t w[4];
        pair_words(seed, r, step, (uint32_t)j, w);
        pair_normals(w, xi[2 * j], xi[2 * j + 1]);
    }
}

// NaN if either is NaN, else the smaller
__host__ __device__ __forceinline__ double nmin(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (b < a ? b : a); }

}  // namespace hjn

// ---------------------------------------------------------------------------------------------- a realisation
namespace hjn {

using hjq::MAXD;
using hjq::QGrid;
using hjq::QStencil;

// what the noise needs (kernel argument)
struct Noise {
    const double* normals;              // null: generate
    unsigned long long first, seed;
    long long nsteps;                   // (ntimes - 1) * sub_samples: the stride of a realisation in `normals`
    double sq;
    double G[MAXD * MAXD];              // ND x ND, row-major
    int policy;
};

// the outputs a realisation has beside a trajectory's (hjr::RolloutOut: traj, here nullable, length, t_earliest, status)
struct McOut {
    double* final_state;
    double* value_end;
    double* value_min;
};

// rollout_body's hooks for group q = m R + k of 2^ND lanes: realisation k of state m.  The policy flag is wave-uniform (a kernel argument);
// every lane of the group computes the normals redundantly, so no shuffle is needed and control flow stays uniform inside a group.
template <int ND> struct NoisyHooks {
    static constexpr bool plain = false;
    const Noise& N;
    const McOut& O;
    long long R;
    int sub_samples;
    long long q;
    double vend, vmin;

    __device__ __forceinline__ long long state_of(long long group) {
        q = group;
        return group / R;
    }
    // HJN_POLICY_CLOCK reads slice `it` at column `it` and never stops early; HJN_POLICY_EARLIEST leaves the choice to the bisection
    __device__ __forceinline__ bool slice(int it, int& tE) const {
        if (N.policy != HJN_POLICY_CLOCK) return false;
        tE = it;
        return true;
    }
    // x = x + sq (G xi): the normals of (first + q, it sub_samples + s), supplied or generated
    __device__ __forceinline__ void after_substep(double* x, int it, int s) const {
#pragma clang fp contract(off)
        const unsigned step = (unsigned)it * (unsigned)sub_samples + (unsigned)s;
        double xi[ND + (ND & 1)];
        if (N.normals) {
            const double* src = N.normals + (q * N.nsteps + (long long)step) * ND;
#pragma unroll
            for (int i = 0; i < ND; ++i) xi[i] = src[i];
        } else {
            step_normals<ND>(N.seed, N.first + (unsigned long long)q, step, xi);
        }
        double tt[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            double n = N.G[i * ND] * xi[0];
#pragma unroll
            for (int j = 1; j < ND; ++j) {
                const double pr = N.G[i * ND + j] * xi[j];
                n = n + pr;
            }
            tt[i] = N.sq * n;
        }
#pragma unroll
        for (int i = 0; i < ND; ++i) x[i] = x[i] + tt[i];
    }
    // v = V[T-1] at the column just recorded
    __device__ __forceinline__ void recorded(double v, bool first) {
        vend = v;
        vmin = first ? v : nmin(vmin, v);
    }
    __device__ __forceinline__ void finish(long long group, const double* x) const {
#pragma unroll
        for (int d = 0; d < ND; ++d) O.final_state[group * ND + d] = x[d];
        O.value_end[group] = vend;
        O.value_min[group] = vmin;
    }
};

// ---------------------------------------------------------------------------------------------- host side
#ifndef HJ_RTC
// The checks of a noisy rollout's entry point (hjn_rollout; hjp_noisy_rollout / _hi of libhj_plant.so) after check_rollout's, in the
// order the refusals are documented in: check_noise before the look at `go`, check_realisations after it.
static const char TOO_MANY_REAL[] = "too many realisations for one launch (nstates * nreal * 2^ndim must be below 2^32): split over states";

static int check_noise(int ndim, int64_t ntimes, int sub_samples, int64_t nreal, int policy, double sq, const double* Gm) {
    using hj_tool::fail;
    if (nreal < 1) return fail(HJ_EINVAL, "nreal must be at least 1");
    if (policy != HJN_POLICY_EARLIEST && policy != HJN_POLICY_CLOCK) return fail(HJ_EINVAL, "policy %d is neither HJN_POLICY_EARLIEST nor HJN_POLICY_CLOCK", policy);
    if (!std::isfinite(sq)) return fail(HJ_EINVAL, "sq must be finite");
    if (!Gm) return fail(HJ_EINVAL, "null argument: G");
    for (int k = 0; k < ndim * ndim; ++k)
        if (!std::isfinite(Gm[k])) return fail(HJ_EINVAL, "G[%d][%d] is not finite", k / ndim, k % ndim);
    if ((ntimes - 1) * (long long)sub_samples > 0x100000000ll)
        return fail(HJ_EINVAL, "(ntimes - 1) * sub_samples = %lld: the counter holds a step in 32 bits", (long long)((ntimes - 1) * (long long)sub_samples));
    return HJ_OK;
}

static int check_realisations(int ndim, int64_t nstates, int64_t nreal, const void* value_end, const void* value_min) {
    using hj_tool::fail;
    if (!value_end || !value_min) return fail(HJ_EINVAL, "null argument");
    if (nreal > 0xffffffffll || nstates > 0xffffffffll || nstates * nreal > (0xffffffffll >> ndim)) return fail(HJ_EINVAL, "%s", TOO_MANY_REAL);
    return HJ_OK;
}
#endif  // HJ_RTC

}  // namespace hjn
#endif
