// libhj_filter.so (include/hj_filter.h): the least-restrictive safety filter on a stored value function, for gfx950.
//   filtered_rollout_kernel<T, SCHEME, PLANT>  2^ndim lanes per trajectory, as rollout_kernel: hj_rollout_dev.h's rollout_body with
//                                              hj_filter_dev.h's FilterHooks (the decision between the plant's controls and the RK4 step, the
//                                              clock or static slice, the gap's minimum, the per-trajectory outputs)
//   decide_points_kernel<T, SCHEME, PLANT>     the same lanes per state: rollout_body's cell search, value and costate at the state, the same
//                                              decision, no step
// The nominal kind, the slice policy and the disturbance rule are kernel arguments: wave-uniform branches.  Control flow is uniform inside a
// group of lanes (every lane holds the same gap bits) and predicated across groups.  No shared memory, no reduction across trajectories.
// The filter's checks stand in this file alone.  hj_plant.hip, whose filter kernels for registered plants are compiled at run time, reads
// them from here: it includes this file with HJ_FILTER_CHECKS_ONLY defined, which leaves out the kernels and the entry points.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hj_tool_host.h"
#include "hj_query_dev.h"
#include "hj_filter_dev.h"

namespace hjf {

using hjq::make_grid;
using hjq::fill_stencil;
using hjq::QGrid;
using hjq::QStencil;
using hjq::UpwindSolver;
using namespace hj_tool;

#ifndef HJ_FILTER_CHECKS_ONLY
template <typename T, int SCHEME, int PLANT>
__global__ __launch_bounds__(256) void filtered_rollout_kernel(const T* __restrict__ data, long long field_stride, int ntimes,
                                                               const double* __restrict__ x0, long long M, QGrid G, QStencil<T> S,
                                                               int sub_samples, double dt_small, hjr_plant P, Filter F,
                                                               hjr::RolloutOut O, FilterOut E) {
    using PL = hjr::Plant<PLANT>;
    using HK = FilterHooks<T, PLANT, false>;
    hjr::rollout_body<T, SCHEME, PL, UpwindSolver, hjr_plant, HK>(data, field_stride, ntimes, x0, M, G, S, sub_samples, dt_small, P, O,
                                                                  HK{F, E, 0.0, 0.0, 0, -1, false, false});
}

template <typename T, int SCHEME, int PLANT>
__global__ __launch_bounds__(256) void decide_points_kernel(const T* __restrict__ data, long long field_stride, int nfields,
                                                            const double* __restrict__ xs, long long M, QGrid G, QStencil<T> S,
                                                            hjr_plant P, Filter F, FilterOut E) {
    using PL = hjr::Plant<PLANT>;
    using HK = FilterHooks<T, PLANT, true>;
    hjr::rollout_body<T, SCHEME, PL, UpwindSolver, hjr_plant, HK>(data, field_stride, nfields, xs, M, G, S, 1, 0.0, P,
                                                                  hjr::RolloutOut{nullptr, nullptr, nullptr, nullptr},
                                                                  HK{F, E, 0.0, 0.0, 0, -1, false, false});
}

#endif  // HJ_FILTER_CHECKS_ONLY

// ---------------------------------------------------------------------------------------------- host side
static const char TOO_MANY_STATES[] = "too many states for one launch (nstates * 2^ndim must be below 2^32): split over states";

// what the library asks of its own plants (check_rollout's plant_checks)
static int check_plant(const hjr_plant* plant, const QGrid& G) {
    const int nd = ham_ndim(plant->id);
    if (nd == 0) return fail(HJ_EUNSUPPORTED, "plant %d has no filter kernel", (int)plant->id);
    if (nd != G.ndim) return fail(HJ_EINVAL, "plant %d has %d states, the grid %d dimensions", (int)plant->id, nd, G.ndim);
    return HJ_OK;
}

// the refusals the two entry points share after check_rollout's
static int check_filter(int64_t nfields, int64_t slice, double level, double margin, int dstb) {
    if (slice < 0 || slice >= nfields) return fail(HJ_EINVAL, "slice %lld outside 0..%lld", (long long)slice, (long long)nfields - 1);
    if (!std::isfinite(level)) return fail(HJ_EINVAL, "level must be finite");
    if (margin != margin) return fail(HJ_EINVAL, "margin must not be NaN (+inf always acts, -inf never does)");
    if (dstb != HJF_DSTB_WORST && dstb != HJF_DSTB_ZERO) return fail(HJ_EINVAL, "dstb %d is neither HJF_DSTB_WORST nor HJF_DSTB_ZERO", dstb);
    return HJ_OK;
}

static int check_states(int64_t nstates, int ndim) {
    if (nstates > (0xffffffffll >> ndim)) return fail(HJ_EINVAL, "%s", TOO_MANY_STATES);
    return HJ_OK;
}

// hjf_rollout's refusals after check_rollout's and before the look at `go`; single: one field serves every time stamp.  CLOCK: slice <- 0
static int check_rollout_filter(long long total, int64_t ntimes, int sub_samples, bool single, int slice_policy, int64_t& slice, int nominal,
                                int64_t nom_ntimes, int64_t nom_field_stride, int nom_u_mode, double level, double margin, int dstb) {
    if (slice_policy != HJF_SLICE_CLOCK && slice_policy != HJF_SLICE_STATIC)
        return fail(HJ_EINVAL, "slice_policy %d is neither HJF_SLICE_CLOCK nor HJF_SLICE_STATIC", slice_policy);
    if (slice_policy == HJF_SLICE_CLOCK) slice = 0;               // not read
    int rc = check_filter(single ? 1 : ntimes, slice, level, margin, dstb);
    if (rc) return rc;
    if (nominal != HJF_NOMINAL_TABLE && nominal != HJF_NOMINAL_VALUE)
        return fail(HJ_EINVAL, "nominal %d is neither HJF_NOMINAL_TABLE nor HJF_NOMINAL_VALUE", nominal);
    if (nominal == HJF_NOMINAL_VALUE) {
        if (nom_ntimes != 1 && nom_ntimes != ntimes)
            return fail(HJ_EINVAL, "nom_ntimes %lld: the nominal value function has one field or ntimes (%lld)", (long long)nom_ntimes, (long long)ntimes);
        if (nom_ntimes > 1 && nom_field_stride < total)
            return fail(HJ_EINVAL, "nom_field_stride %lld is smaller than the grid (%lld)", (long long)nom_field_stride, total);
        if (nom_u_mode != HJR_MODE_MIN && nom_u_mode != HJR_MODE_MAX) return fail(HJ_EINVAL, "nom_u_mode must be HJR_MODE_MIN or HJR_MODE_MAX");
    }
    if ((ntimes - 1) * (long long)sub_samples > 0x7fffffffll)
        return fail(HJ_EINVAL, "(ntimes - 1) * sub_samples = %lld: a step index is an int32", (long long)((ntimes - 1) * (long long)sub_samples));
    return HJ_OK;
}

// hjf_decide's
static int check_decide_filter(long long total, int64_t nfields, int64_t field_stride, int64_t slice, double level, double margin, int dstb) {
    if (nfields < 1 || nfields > 0x7fffffffll) return fail(HJ_EINVAL, "nfields %lld: a decision needs a stored set", (long long)nfields);
    if (nfields > 1 && field_stride < total)
        return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, total);
    return check_filter(nfields, slice, level, margin, dstb);
}

#ifndef HJ_FILTER_CHECKS_ONLY
template <typename F3> static int dispatch_plant(const hjq_grid* g, int scheme, const hjr_plant* plant, F3&& f) {
    static_assert(HJ_HAM_DUBINS_REL == 0 && HJ_HAM_DOUBLE_INTEGRATOR == 1 && HJ_HAM_DOUBLE_PENDULUM == 2, "plant ids name the kernels");
    return dispatch(g->dtype, scheme, [&](auto t, auto sch) {
        if (plant->id == 0) return f(t, sch, int_c<0>{});
        if (plant->id == 1) return f(t, sch, int_c<1>{});
        return f(t, sch, int_c<2>{});
    });
}

#endif  // HJ_FILTER_CHECKS_ONLY

}  // namespace hjf

#ifndef HJ_FILTER_CHECKS_ONLY
using namespace hjf;

extern "C" {

int hjf_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant, int slice_policy, int64_t slice,
                int nominal, const double* u_nom, const void* nom_data, int64_t nom_ntimes, int64_t nom_field_stride,
                int nom_u_mode, double level, double margin, int dstb, double* final_state, double* gap_min, double* value_end,
                int32_t* interventions, int32_t* first_intervention, int32_t* length, int32_t* status, double* traj,
                uint8_t* active, double* applied, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    bool go;
    // one converged field for every time stamp (stride 0) is the static policy's alone: anything else meets check_rollout's refusal.
    // check_rollout asks for a trajectory array; here it is optional, so the final states stand in for it
    const bool single = field_stride == 0 && slice_policy == HJF_SLICE_STATIC;
    rc = hjr::check_rollout(G, total, scheme, data, ntimes, single ? (int64_t)total : field_stride, x0, nstates, sub_samples, dt_small,
                            plant, final_state, length, status, [&]() { return check_plant(plant, G); }, go);
    if (rc) return rc;
    if ((rc = check_rollout_filter(total, ntimes, sub_samples, single, slice_policy, slice, nominal, nom_ntimes, nom_field_stride, nom_u_mode, level,
                                   margin, dstb)))
        return rc;
    if (!go) {
        launched_none();
        return HJ_OK;
    }
    if (!gap_min || !value_end || !interventions || !first_intervention || (nominal == HJF_NOMINAL_TABLE ? !u_nom : !nom_data))
        return fail(HJ_EINVAL, "null argument");
    if ((rc = check_states(nstates, G.ndim))) return rc;
    const Filter F{u_nom, nom_data, (long long)nom_field_stride, (int)nom_ntimes, nom_u_mode, level, margin, nominal, slice_policy,
                   (int)slice, dstb, (int)ntimes, sub_samples};
    const hjr::RolloutOut O{traj, length, nullptr, status};
    const FilterOut E{final_state, gap_min, value_end, interventions, first_intervention, status, active, applied, nullptr, nullptr, nullptr};
    return dispatch_plant(g, scheme, plant, [&](auto t, auto sch, auto pl) {
        using T = typename decltype(t)::type;
        constexpr int SCH = decltype(sch)::value, PLANT = decltype(pl)::value;
        QStencil<T> S;
        fill_stencil(g, G, S);
        unsigned blocks;
        int r = blocks_for(nstates * (1ll << G.ndim), TOO_MANY_STATES, blocks);
        if (r) return r;
        hipLaunchKernelGGL((filtered_rollout_kernel<T, SCH, PLANT>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)data,
                           (long long)field_stride, (int)ntimes, x0, (long long)nstates, G, S, sub_samples, dt_small, *plant, F, O, E);
        return launch_done(kernel_name("filtered_rollout_kernel", type_tag<T>::name(), {SCH, PLANT}).c_str());
    });
}

int hjf_decide(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice,
               const double* xs, int64_t nstates, const hjr_plant* plant, const double* u_nom, double level, double margin,
               int dstb, double* applied, uint8_t* active, double* value, double* gap, double* costate, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    bool go;
    // check_rollout with what a point does not have held at values it accepts: two sets a grid apart, one sub-step, a zero step
    rc = hjr::check_rollout(G, total, scheme, data, 2, (int64_t)total, xs, nstates, 1, 0.0, plant, applied, active, value,
                            [&]() { return check_plant(plant, G); }, go);
    if (rc) return rc;
    if ((rc = check_decide_filter(total, nfields, field_stride, slice, level, margin, dstb))) return rc;
    if (!go) {
        launched_none();
        return HJ_OK;
    }
    if (!gap || !u_nom) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_states(nstates, G.ndim))) return rc;
    const Filter F{u_nom, nullptr, 0, 1, HJR_MODE_MIN, level, margin, HJF_NOMINAL_TABLE, HJF_SLICE_STATIC, (int)slice, dstb, (int)nfields, 1};
    const FilterOut E{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, active, applied, value, gap, costate};
    return dispatch_plant(g, scheme, plant, [&](auto t, auto sch, auto pl) {
        using T = typename decltype(t)::type;
        constexpr int SCH = decltype(sch)::value, PLANT = decltype(pl)::value;
        QStencil<T> S;
        fill_stencil(g, G, S);
        unsigned blocks;
        int r = blocks_for(nstates * (1ll << G.ndim), TOO_MANY_STATES, blocks);
        if (r) return r;
        hipLaunchKernelGGL((decide_points_kernel<T, SCH, PLANT>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)data,
                           nfields > 1 ? (long long)field_stride : 0ll, (int)nfields, xs, (long long)nstates, G, S, *plant, F, E);
        return launch_done(kernel_name("decide_points_kernel", type_tag<T>::name(), {SCH, PLANT}).c_str());
    });
}

HJ_TOOL_LAST_SYMBOLS(hjf)

}  // extern "C"
#endif  // HJ_FILTER_CHECKS_ONLY
