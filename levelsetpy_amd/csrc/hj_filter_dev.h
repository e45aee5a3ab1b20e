// Device code of libhj_filter.so (hj_filter.hip, include/hj_filter.h): which held values of a plant are controls, the filter's decision --
// ONE function, called at every sub-step of a filtered rollout and by the point query -- and the hooks that turn hj_rollout_dev.h's
// rollout_body into a filtered trajectory.  There is ONE source of the trajectory: the decision, the slice policy and the per-trajectory
// outputs enter rollout_body through its hook type (FilterHooks below), the cell search, the value and the costates are the body's own, the
// plants are hj_plants_dev.h's, nmin is hj_mc_dev.h's.  tests/filter_ref.py restates the result.
// Include after hj_query_dev.h.
#ifndef HJ_FILTER_DEV_H
#define HJ_FILTER_DEV_H
#include "hj_rollout_dev.h"
#include "hj_plants_dev.h"
#include "hj_mc_dev.h"
#include "../../include/hj_filter.h"

namespace hjf {

// ---- include/hj_filter.h's table: what each held value of a built-in plant is, and the number of controls
enum { HELD_NOTHING = 0, HELD_CONTROL = 1, HELD_DISTURBANCE = 2 };
template <int ID> struct Held;
template <> struct Held<HJ_HAM_DUBINS_REL> { static constexpr int c0 = HELD_CONTROL, c1 = HELD_DISTURBANCE, NU = 1; };
template <> struct Held<HJ_HAM_DOUBLE_INTEGRATOR> { static constexpr int c0 = HELD_CONTROL, c1 = HELD_NOTHING, NU = 1; };
template <> struct Held<HJ_HAM_DOUBLE_PENDULUM> { static constexpr int c0 = HELD_CONTROL, c1 = HELD_CONTROL, NU = 2; };

// what the filter needs (kernel argument: the kinds are wave-uniform branches)
struct Filter {
    const double* u_nom;                // HJF_NOMINAL_TABLE
    const void* nom_data;               // HJF_NOMINAL_VALUE: the stack's element type is the kernel's T
    long long nom_stride;
    int nom_ntimes, nom_u_mode;
    double level, margin;
    int nominal, slice_policy, slice, dstb;
    int ntimes, sub_samples;
};

// the outputs beside hjr::RolloutOut's traj and length: a rollout's, then the point query's (applied and active are both's)
struct FilterOut {
    double* final_state;
    double* gap_min;
    double* value_end;
    int* interventions;
    int* first;
    int* status;
    unsigned char* active;
    double* applied;
    double* value;
    double* gap;
    double* costate;
};

// gap of a value: on which side of `level` the safe set lies follows from what the control does to V
__device__ __forceinline__ double gap_of(const Filter& F, const hjr_plant& P, double v) {
#pragma clang fp contract(off)
    return P.u_mode == HJR_MODE_MAX ? v - F.level : F.level - v;
}

// The decision of one sub-step.  c: the plant's controls for the costate of V at x, replaced where the nominal runs; u_row: the
// table's NU values of this (state, column); nominal_costate(q): grad Vn at x, asked only where the value nominal runs (the branch is
// uniform inside a group of lanes: every lane holds the same gap).  -> act
template <int PLANT, typename NQ>
__device__ __forceinline__ bool decide(const Filter& F, const hjr_plant& P, double v, const double* x, const double* u_row,
                                       NQ&& nominal_costate, hjr::Control2& c, double& gap) {
    using PL = hjr::Plant<PLANT>;
    using HV = Held<PLANT>;
    gap = gap_of(F, P, v);
    const bool act = !(gap > F.margin);
    if (!act) {
        if (F.nominal == HJF_NOMINAL_TABLE) {
            if (HV::c0 == HELD_CONTROL) c.c0 = u_row[0];
            if (HV::c1 == HELD_CONTROL) c.c1 = u_row[HV::c0 == HELD_CONTROL ? 1 : 0];
        } else {
            double q[PL::ND];
            nominal_costate(q);
            hjr_plant Q = P;
            Q.u_mode = F.nom_u_mode;
            hjr::Control2 n;
            hjr::plant_controls<PL>(Q, q, x, n);
            if (HV::c0 == HELD_CONTROL) c.c0 = n.c0;
            if (HV::c1 == HELD_CONTROL) c.c1 = n.c1;
        }
    }
    if (F.dstb == HJF_DSTB_ZERO) {
        if (HV::c0 == HELD_DISTURBANCE) c.c0 = 0.0;
        if (HV::c1 == HELD_DISTURBANCE) c.c1 = 0.0;
    }
    return act;
}

// rollout_body's hooks.  POINT false: a filtered trajectory (group m of 2^ND lanes: state m).  POINT true: the decision at the state alone.
template <typename T, int PLANT, bool POINT> struct FilterHooks {
    using Filter = hjf::Filter;         // names the filter's hook points to rollout_body (hjr::filter_of)
    static constexpr bool plain = false;
    static constexpr bool point = POINT;
    static constexpr int NU = Held<PLANT>::NU;
    static constexpr int ND = hjr::Plant<PLANT>::ND;
    const Filter& F;
    const FilterOut& O;
    double gmin, vend;
    int count, first;
    bool seen, left;

    __device__ __forceinline__ long long state_of(long long group) const { return group; }
    // the clock reads slice `it` at column `it`, the static policy one slice throughout: no bisection, and it never stops early
    __device__ __forceinline__ bool slice(int it, int& tE) const {
        tE = F.slice_policy == HJF_SLICE_CLOCK ? it : F.slice;
        return true;
    }
    __device__ __forceinline__ void after_substep(double*, int, int) const {}
    __device__ __forceinline__ void recorded(double, bool) const {}

    __device__ __forceinline__ void take(double gap) {
        gmin = seen ? hjn::nmin(gmin, gap) : gap;
        seen = true;
    }
    template <typename VQ, typename CQ>
    __device__ __forceinline__ void decide(long long m, int c, int it, int s, int sl, const double* x, hjr::Control2& ctl,
                                           const hjr_plant& P, VQ&& value_at, CQ&& costate_in) {
        const double v = value_at(sl);
        const int step = it * F.sub_samples + s;
        const long long nsteps = (long long)(F.ntimes - 1) * F.sub_samples;
        const double* u_row = F.u_nom + (m * (F.ntimes - 1) + it) * NU;
        double gap;
        const bool act = hjf::decide<PLANT>(F, P, v, x, u_row, [&](double* q) {
            costate_in((const T*)F.nom_data, F.nom_stride, F.nom_ntimes == 1 ? 0 : it, q);
        }, ctl, gap);
        take(gap);
        if (act) {
            if (count == 0) first = step;
            ++count;
        }
        if (c == 0) {
            if (O.active) O.active[m * nsteps + step] = act ? 1 : 0;
            if (O.applied) {
                O.applied[(m * nsteps + step) * 2] = ctl.c0;
                O.applied[(m * nsteps + step) * 2 + 1] = ctl.c1;
            }
        }
    }
    template <typename VQ> __device__ __forceinline__ void at_end(const hjr_plant& P, VQ&& value_at, bool left_grid) {
        const double v = value_at(F.slice_policy == HJF_SLICE_CLOCK ? F.ntimes - 1 : F.slice);
        take(gap_of(F, P, v));
        vend = v;
        left = left_grid;
    }
    __device__ __forceinline__ void finish(long long m, const double* x) const {
#pragma unroll
        for (int d = 0; d < ND; ++d) O.final_state[m * ND + d] = x[d];
        O.gap_min[m] = gmin;
        O.value_end[m] = vend;
        O.interventions[m] = count;
        O.first[m] = first;
        O.status[m] = left ? HJF_LEFT_GRID : (!(gmin > 0.0) ? HJF_VIOLATED : HJF_SAFE);
    }

    // POINT: the field to read, and the answer (v and p of that field at x, ctl the plant's controls for p)
    __device__ __forceinline__ int field() const { return F.slice; }
    __device__ __forceinline__ void decided(long long m, int c, const double* x, const double* p, hjr::Control2& ctl, const hjr_plant& P,
                                            double v) const {
        double gap;
        const bool act = hjf::decide<PLANT>(F, P, v, x, F.u_nom + m * NU, [&](double* q) {
#pragma unroll
            for (int d = 0; d < ND; ++d) q[d] = __builtin_nan("");      // the point query has the table nominal only (checked by the host)
        }, ctl, gap);
        if (c != 0) return;
        O.applied[m * 2] = ctl.c0;
        O.applied[m * 2 + 1] = ctl.c1;
        O.active[m] = act ? 1 : 0;
        O.value[m] = v;
        O.gap[m] = gap;
        if (O.costate) {
#pragma unroll
            for (int d = 0; d < ND; ++d) O.costate[m * ND + d] = p[d];
        }
    }
};

}  // namespace hjf
#endif
