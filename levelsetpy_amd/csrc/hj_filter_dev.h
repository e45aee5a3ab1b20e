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

// How a plant's held values meet the filter: what the plant, its descriptor and its control value are, NU, the width W of a row of
// `applied`, and how a control value takes a table row, takes the nominal plant's controls, loses its disturbances and is stored.
// BuiltIn<ID>: Held<ID> over hjr::Control2.  OwnControl<PL>: a plant with a Control type of its own, u[NU] then dst[NDST] (libhj_plant.so's
// PlantUser around a registered plant, descriptor hjp_plant -- named by the including unit, PD).
template <int ID> struct BuiltIn {
    using PL = hjr::Plant<ID>;
    using PD = hjr_plant;
    using CT = hjr::Control2;
    using HV = Held<ID>;
    static constexpr int NU = HV::NU, W = 2;
    __device__ __forceinline__ static void take_row(CT& c, const double* u_row) {
        if (HV::c0 == HELD_CONTROL) c.c0 = u_row[0];
        if (HV::c1 == HELD_CONTROL) c.c1 = u_row[HV::c0 == HELD_CONTROL ? 1 : 0];
    }
    __device__ __forceinline__ static void take_nominal(CT& c, const CT& n) {
        if (HV::c0 == HELD_CONTROL) c.c0 = n.c0;
        if (HV::c1 == HELD_CONTROL) c.c1 = n.c1;
    }
    __device__ __forceinline__ static void zero_disturbances(CT& c) {
        if (HV::c0 == HELD_DISTURBANCE) c.c0 = 0.0;
        if (HV::c1 == HELD_DISTURBANCE) c.c1 = 0.0;
    }
    __device__ __forceinline__ static void store(const CT& c, double* row) {
        row[0] = c.c0;
        row[1] = c.c1;
    }
};
template <typename PLT, typename PDT> struct OwnControl {
    using PL = PLT;
    using PD = PDT;
    using CT = typename PLT::Control;
    static constexpr int NU = PLT::NU, NDST = PLT::NDST, W = NU + NDST > 2 ? NU + NDST : 2;
    __device__ __forceinline__ static void take_row(CT& c, const double* u_row) {
#pragma unroll
        for (int i = 0; i < NU; ++i) c.u[i] = u_row[i];
    }
    __device__ __forceinline__ static void take_nominal(CT& c, const CT& n) {
#pragma unroll
        for (int i = 0; i < NU; ++i) c.u[i] = n.u[i];
    }
    __device__ __forceinline__ static void zero_disturbances(CT& c) {
#pragma unroll
        for (int j = 0; j < NDST; ++j) c.dst[j] = 0.0;
    }
    __device__ __forceinline__ static void store(const CT& c, double* row) {
#pragma unroll
        for (int i = 0; i < NU; ++i) row[i] = c.u[i];
#pragma unroll
        for (int j = 0; j < NDST; ++j) row[NU + j] = c.dst[j];
#pragma unroll
        for (int k = NU + NDST; k < W; ++k) row[k] = 0.0;
    }
};

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
template <typename PD> __device__ __forceinline__ double gap_of(const Filter& F, const PD& P, double v) {
#pragma clang fp contract(off)
    return P.u_mode == HJR_MODE_MAX ? v - F.level : F.level - v;
}

// The decision of one sub-step.  c: the plant's controls for the costate of V at x, replaced where the nominal runs; u_row: the
// table's NU values of this (state, column); nominal_costate(q): grad Vn at x, asked only where the value nominal runs (the branch is
// uniform inside a group of lanes: every lane holds the same gap).  -> act
// PLANT: the adaptor above.
template <typename PLANT, typename NQ>
__device__ __forceinline__ bool decide(const Filter& F, const typename PLANT::PD& P, double v, const double* x, const double* u_row,
                                       NQ&& nominal_costate, typename PLANT::CT& c, double& gap) {
    using PL = typename PLANT::PL;
    gap = gap_of(F, P, v);
    const bool act = !(gap > F.margin);
    if (!act) {
        if (F.nominal == HJF_NOMINAL_TABLE) {
            PLANT::take_row(c, u_row);
        } else {
            double q[PL::ND];
            nominal_costate(q);
            typename PLANT::PD Q = P;
            Q.u_mode = F.nom_u_mode;
            typename PLANT::CT n;
            hjr::plant_controls<PL>(Q, q, x, n);
            PLANT::take_nominal(c, n);
        }
    }
    if (F.dstb == HJF_DSTB_ZERO) PLANT::zero_disturbances(c);
    return act;
}

// rollout_body's hooks.  POINT false: a filtered trajectory (group m of 2^ND lanes: state m).  POINT true: the decision at the state alone.
// PLANT: the adaptor of the plant's held values; FilterHooks<T, ID, POINT> below names the built-in plants' by their id.
template <typename T, typename PLANT, bool POINT> struct HooksOf {
    using Filter = hjf::Filter;         // names the filter's hook points to rollout_body (hjr::filter_of)
    using PD = typename PLANT::PD;
    using CT = typename PLANT::CT;
    static constexpr bool plain = false;
    static constexpr bool point = POINT;
    static constexpr int NU = PLANT::NU, W = PLANT::W;
    static constexpr int ND = PLANT::PL::ND;
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
    __device__ __forceinline__ void decide(long long m, int c, int it, int s, int sl, const double* x, CT& ctl,
                                           const PD& P, VQ&& value_at, CQ&& costate_in) {
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
            if (O.applied) PLANT::store(ctl, O.applied + (m * nsteps + step) * W);
        }
    }
    template <typename VQ> __device__ __forceinline__ void at_end(const PD& P, VQ&& value_at, bool left_grid) {
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
    __device__ __forceinline__ void decided(long long m, int c, const double* x, const double* p, CT& ctl, const PD& P,
                                            double v) const {
        double gap;
        const bool act = hjf::decide<PLANT>(F, P, v, x, F.u_nom + m * NU, [&](double* q) {
#pragma unroll
            for (int d = 0; d < ND; ++d) q[d] = __builtin_nan("");      // the point query has the table nominal only (checked by the host)
        }, ctl, gap);
        if (c != 0) return;
        PLANT::store(ctl, O.applied + m * W);
        O.active[m] = act ? 1 : 0;
        O.value[m] = v;
        O.gap[m] = gap;
        if (O.costate) {
#pragma unroll
            for (int d = 0; d < ND; ++d) O.costate[m * ND + d] = p[d];
        }
    }
};
template <typename T, int PLANT, bool POINT> using FilterHooks = HooksOf<T, BuiltIn<PLANT>, POINT>;

}  // namespace hjf
#endif
