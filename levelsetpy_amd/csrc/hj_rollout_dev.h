// Device code shared by the rollout kernels of libhj_rollout.so (hj_rollout.hip), libhj_hiquery.so (hj_hiquery.hip), libhj_mc.so (hj_mc.hip,
// through the hook type below), libhj_filter.so (hj_filter.hip, through a hook type with the filter's points) and the ones libhj_plant.so has hipRTC compile (hj_plant.hip): what does not depend on the plant -- sgn, the RK4 step, and a trajectory from
// its first state to its last (the bisection over the stored sets, the costate, the sub-steps).  One source, so a 5-D / 6-D
// trajectory is stepped by the statements a 2-D .. 4-D one is.  At the end, the host side the three share: check_rollout.
// A plant is a specialisation of Plant<ID> in the including file: ND, controls(P, p, x, c0, c1), f(P, x, c0, c1, k).  A plant with
// more than two held values names a type of its own, Control, and takes it whole: controls(P, p, x, Control&), f(P, x, const
// Control&, k) -- libhj_plant.so's PlantUser, compiled at run time (hj_plant.hip); its descriptor is whatever type the kernel hands on.
// Include after hj_query_dev.h.
#ifndef HJ_ROLLOUT_DEV_H
#define HJ_ROLLOUT_DEV_H
#include "hj_query_dev.h"
#include "../../include/hj_rollout.h"

namespace hjr {

using hjq::MAXD;
using hjq::QGrid;
using hjq::QStencil;
using hjq::UpwindSolver;      // the one-sided derivatives of a corner's stencil up to 4-D, and
using hjq::UpwindHidim;       // at 5-D / 6-D: hj_query_dev.h

// +1 for s >= 0, -1 for s < 0, NaN for NaN: an exact zero is deterministic, a NaN costate poisons the state
__device__ __forceinline__ double sgn(double s) { return s >= 0.0 ? 1.0 : (s < 0.0 ? -1.0 : __builtin_nan("")); }

// ---- the plants: controls(costate p, state x) -> (c0, c1), f(x; c0, c1) -> xdot.  One operation per statement.
template <int ID> struct Plant;

// What a step holds fixed: two scalars (the built-in plants), or the plant's own Control type.
struct Control2 { double c0, c1; };
template <typename...> struct void_of { using type = void; };
template <typename PL, typename = void> struct control_of { using type = Control2; };
template <typename PL> struct control_of<PL, typename void_of<typename PL::Control>::type> { using type = typename PL::Control; };

template <typename PL, typename PD>
__device__ __forceinline__ void plant_controls(const PD& P, const double* p, const double* x, Control2& c) { PL::controls(P, p, x, c.c0, c.c1); }
template <typename PL, typename PD, typename CT>
__device__ __forceinline__ void plant_controls(const PD& P, const double* p, const double* x, CT& c) { PL::controls(P, p, x, c); }
template <typename PL, typename PD>
__device__ __forceinline__ void plant_f(const PD& P, const double* x, const Control2& c, double* k) { PL::f(P, x, c.c0, c.c1, k); }
template <typename PL, typename PD, typename CT>
__device__ __forceinline__ void plant_f(const PD& P, const double* x, const CT& c, double* k) { PL::f(P, x, c, k); }

// one classical RK4 step with the controls held, in the expression order of the Python systems' update_state
template <typename PL, typename PD, typename CT>
__device__ __forceinline__ void rk4(const PD& P, double* x, double dt, const CT& c) {
#pragma clang fp contract(off)
    constexpr int N = PL::ND;
    double k1[N], k2[N], k3[N], k4[N], xa[N];
    const double h = 0.5 * dt;
    plant_f<PL>(P, x, c, k1);
#pragma unroll
    for (int d = 0; d < N; ++d) { const double t = h * k1[d]; xa[d] = x[d] + t; }
    plant_f<PL>(P, xa, c, k2);
#pragma unroll
    for (int d = 0; d < N; ++d) { const double t = h * k2[d]; xa[d] = x[d] + t; }
    plant_f<PL>(P, xa, c, k3);
#pragma unroll
    for (int d = 0; d < N; ++d) { const double t = dt * k3[d]; xa[d] = x[d] + t; }
    plant_f<PL>(P, xa, c, k4);
    const double sixth = dt / 6.0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        const double a = 2.0 * k2[d];
        double s = k1[d] + a;
        const double b = 2.0 * k3[d];
        s = s + b;
        s = s + k4[d];
        s = sixth * s;
        x[d] = x[d] + s;
    }
}

struct RolloutOut {
    double* traj;
    int* length;
    int* t_earliest;
    int* status;
};

// What a caller may add to a trajectory, the way Control was introduced: a hook type with `plain` false is asked after every sub-step
// (after_substep: libhj_mc.so's noise), which slice to read (slice: true where it chose tE itself and no bisection runs), and told of every
// recorded column (recorded: the target function's value there); it maps a group to its row of x0 (state_of), may leave traj out
// (a null O.traj) and writes its own outputs at the end (finish).  Every use below is an `if constexpr (!HK::plain)`: with the
// default the statements are discarded, and the kernels of libhj_rollout.so, libhj_hiquery.so and libhj_plant.so are what they were.
struct NoHooks { static constexpr bool plain = true; };

// A hook type that names a member type Filter has three more points (libhj_filter.so's FilterHooks, hj_filter_dev.h), detected the way
// control_of detects Control, so NoHooks and hj_mc_dev.h's NoisyHooks stay as they are and their kernels keep their code: decide(),
// between the plant's controls and the RK4 step, sees the column, the sub-step, the slice, the state, the held values and the body's own
// value and costate queries (the costate of any stack on the grid) and may replace the held values; at_end(), before the outputs,
// sees the same queries and whether the trajectory left the grid; a type whose `point` is true is answered at the first state alone:
// decided(), and no step is taken.
template <typename HK, typename = void> struct filter_of { static constexpr bool value = false, point = false; };
template <typename HK> struct filter_of<HK, typename void_of<typename HK::Filter>::type> {
    static constexpr bool value = true, point = HK::point;
};

// The body of a rollout kernel: the thread's trajectory (2^ND lanes per trajectory, this thread one corner of its cell).
// Control flow is uniform inside a group and predicated across groups: see hj_rollout.hip.
template <typename T, int SCHEME, typename PL, typename UP, typename PD = hjr_plant, typename HK = NoHooks>
__device__ __forceinline__ void rollout_body(const T* __restrict__ data, long long field_stride, int ntimes,
                                             const double* __restrict__ x0, long long M, const QGrid& G, const QStencil<T>& S,
                                             int sub_samples, double dt_small, const PD& P, const RolloutOut& O, HK&& H = HK()) {
    constexpr int ND = PL::ND;                     // == G.ndim (checked by the host)
    constexpr int lanes = 1 << ND;                 // 4 .. 64: divides the wavefront, groups never straddle one
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long m = t / lanes;
    const int c = (int)(t - m * lanes);
    if (m >= M) return;                            // whole groups leave together
    const double nan = __builtin_nan("");
    const double small = 1e-4;
    double x[MAXD];
    long long xr = m;                              // the row of x0: a hook may run several groups from one
    if constexpr (!HK::plain) xr = H.state_of(m);
#pragma unroll
    for (int d = 0; d < MAXD; ++d) x[d] = d < ND ? x0[xr * ND + d] : 0.0;

    // where the state is: the cell, this lane's corner of it and the corner's weight
    int lo[MAXD];
    double w[MAXD];
    bool inside;
    long long off;
    double wt;
    int used;
    auto find = [&]() {
        inside = hjq::locate(G, x, lo, w);
        wt = hjq::corner(G, lo, w, c, off);
        used = wt != 0.0;
    };
    // V[f](x) in fp64: costate_points_kernel's `value`, the bits of interp_points_kernel
    auto value_at = [&](int f) -> double {
        T raw = T(0);
        if (inside && used) raw = data[(long long)f * field_stride + off];
        double p;
        {
#pragma clang fp contract(off)
            p = wt * (double)raw;
        }
        const double v = hjq::group_sum(p, used, lanes);
        return inside ? v : nan;
    };
    // grad V[f](x) in fp64: costate_points_kernel's `costate`.  The middle block is hjq::corner_derivs' statements, written out: calling it
    // here costs the 4-D kernels two VGPRs and 36 bytes of scratch (profiles/refactor_query_rollout.txt).
    auto costate_in = [&](const T* __restrict__ base, long long stride, int f, double* p) {
        T cC[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) cC[d] = T(0);
        if (inside && used) {
            const T* pc0 = base + (long long)f * stride + off;
            const T raw = *pc0;
            if (!hjq::finite(raw)) {
                // the node's own NaN / inf is put back after the differences (computeGradients: NaN stays NaN, +-inf becomes +inf)
                const T back = raw != raw ? raw : T(__builtin_inf());
#pragma unroll
                for (int d = 0; d < ND; ++d) cC[d] = back;
            } else {
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    int j = lo[d] + ((c >> d) & 1);
                    if (G.per[d] && j >= G.n[d]) j -= G.n[d];
                    T v[7];
                    hjq::gather_axis<T>(pc0, G.stride[d], j, G.n[d], G.per[d] != 0, S.km[d], raw, v);
                    T L, R;
                    UP::template lr<SCHEME, T>(v, S.K[d], L, R);
                    cC[d] = T(0.5) * (L + R);
                }
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            double q;
            {
#pragma clang fp contract(off)
                q = wt * (double)cC[d];
            }
            const double sC = hjq::group_sum(q, used, lanes);
            p[d] = inside ? sC : nan;
        }
    };
    auto costate_at = [&](int f, double* p) { costate_in(data, field_stride, f, p); };

    double* __restrict__ row = O.traj + m * ND * (long long)ntimes;         // traj[m][d][col] = row[d * ntimes + col]
    bool paths = true;                             // a hook may run without traj
    if constexpr (!HK::plain) paths = O.traj != nullptr;
    int* __restrict__ te_row = O.t_earliest ? O.t_earliest + m * (long long)ntimes : nullptr;
    find();
    if constexpr (filter_of<HK>::point) {
        double p[ND];
        typename control_of<PL>::type ctl;
        const int f = H.field();
        costate_at(f, p);
        plant_controls<PL>(P, p, x, ctl);
        H.decided(m, c, x, p, ctl, P, value_at(f));
        return;
    }
    if (c == 0 && paths) {
#pragma unroll
        for (int d = 0; d < ND; ++d) row[d * (long long)ntimes] = x[d];
    }
    if constexpr (!HK::plain) H.recorded(value_at(ntimes - 1), true);
    int tE = 0, len = 1;
    bool done = false, reached = false, left = !inside;
    for (int it = 0; it < ntimes - 1; ++it) {
        // the largest index of [tE, ntimes-1] whose set holds x: only the visited slices are interpolated
        const bool active = !done;
        bool chosen = false;
        if constexpr (!HK::plain) chosen = H.slice(it, tE);
        if (!chosen) {
            int lower = tE, upper = active ? ntimes - 1 : tE;
            while (upper > lower) {
                const int mid = (upper + lower + 1) / 2;
                if (value_at(mid) < small) lower = mid;
                else upper = mid - 1;
            }
            if (active) {
                tE = upper;
                if (tE == ntimes - 1) done = reached = true;
            }
        }
        if (te_row && c == 0) te_row[it] = active ? tE : -1;
        if (!done) {
            for (int s = 0; s < sub_samples; ++s) {
                double p[ND];
                typename control_of<PL>::type ctl;
                costate_at(tE, p);
                plant_controls<PL>(P, p, x, ctl);
                if constexpr (filter_of<HK>::value) H.decide(m, c, it, s, tE, x, ctl, P, value_at, costate_in);
                rk4<PL>(P, x, dt_small, ctl);
                if constexpr (!HK::plain) H.after_substep(x, it, s);
                find();
            }
            len = it + 2;
            left = left || !inside;
            if constexpr (!HK::plain) H.recorded(value_at(ntimes - 1), false);
        }
        if (c == 0 && paths) {
#pragma unroll
            for (int d = 0; d < ND; ++d) row[d * (long long)ntimes + it + 1] = done ? nan : x[d];
        }
    }
    if constexpr (filter_of<HK>::value) H.at_end(P, value_at, left);
    if (c == 0) {
        if (te_row) te_row[ntimes - 1] = -1;
        O.length[m] = len;
        O.status[m] = left ? HJR_LEFT_GRID : (reached ? HJR_REACHED : HJR_EXHAUSTED);
        if constexpr (!HK::plain) H.finish(m, x);       // a finished trajectory's state no longer moves: x is the last recorded one
    }
}

// ---------------------------------------------------------------------------------------------- host side
#ifndef HJ_RTC
// The checks of a rollout entry point (hjr_rollout, hjx_rollout, hjp_rollout / hjp_rollout_hi) after make_grid, in the order the
// refusals are documented in.  plant_checks(): what the library asks of its own plants, between the scheme and the modes.
// go: false where the call is in order and there is nothing to launch (no state).
template <int MD, typename PD, typename F>
static int check_rollout(const hjq::QGridT<MD>& G, long long total, int scheme, const void* data, int64_t ntimes, int64_t field_stride,
                         const double* x0, int64_t nstates, int sub_samples, double dt_small, const PD* plant, const void* traj,
                         const void* length, const void* status, F&& plant_checks, bool& go) {
    using hj_tool::fail;
    go = false;
    if (!plant) return fail(HJ_EINVAL, "null plant descriptor");
    if (nstates < 0) return fail(HJ_EINVAL, "nstates must not be negative");
    if (ntimes < 2 || ntimes > 0x7fffffffll) return fail(HJ_EINVAL, "ntimes %lld: a rollout needs at least two stored sets", (long long)ntimes);
    if (sub_samples < 1) return fail(HJ_EINVAL, "sub_samples must be positive");
    if (!std::isfinite(dt_small)) return fail(HJ_EINVAL, "dt_small must be finite");
    if (field_stride < total) return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, total);
    int rc = hj_tool::check_point_scheme(scheme, "rollout");
    if (rc || (rc = plant_checks())) return rc;
    if ((plant->u_mode != HJR_MODE_MIN && plant->u_mode != HJR_MODE_MAX) || (plant->d_mode != HJR_MODE_MIN && plant->d_mode != HJR_MODE_MAX))
        return fail(HJ_EINVAL, "u_mode / d_mode must be HJR_MODE_MIN or HJR_MODE_MAX");
    for (int d = 0; d < G.ndim; ++d)
        if (G.n[d] < HJ_STENCIL) return fail(HJ_EINVAL, "grid too small along dim %d (N=%d, need %d)", d, G.n[d], HJ_STENCIL);
    if (nstates == 0) return HJ_OK;
    if (!data || !x0 || !traj || !length || !status) return fail(HJ_EINVAL, "null argument");
    go = true;
    return HJ_OK;
}

static const char TOO_MANY_TRAJ[] = "too many trajectories for one launch";
#endif  // HJ_RTC

}  // namespace hjr
#endif
