// Host side of what libhj_batch.so, libhj_stoch.so and libhj_hidim.so share: the three libraries that integrate with ONE launch per RK
// stage (hj_batch.hip, hj_stoch.hip, hj_hidim.hip).  Include after hj_tool_host.h (fail, the error record; plan_problem / step_time, the
// time arithmetic, stay there) and hj_split.h (GridArgs).  Host code only.
//   fill_grid            a grid descriptor (hjq_grid, hjh_grid) as the kernels' GridArgs
//   check_axes, check_coord, check_aux    the descriptor's and the tables' checks
//   step_bound_of_keys   1 / sum_d max alpha_d / dx_d from the keys a bound kernel leaves
//   Stage, rk_schedule, rk_stage_id, result_in    an interval's launches: the RK1 / RK2 / RK3 buffer rotation, stated once
//   check_stage_id, check_y0, check_order, check_post_prev, check_array_ops, check_buffers    a stage's and an interval's checks
// Each library calls the checks in its own order -- the order decides which refusal a call with two faults gets -- and keeps the
// checks only it makes.
#ifndef HJ_STAGE_HOST_H
#define HJ_STAGE_HOST_H

namespace hj_tool {

// fill_grid of the solver (hj_host.h) from the descriptor: a single domain, no slab halos
template <typename T, int ND, typename GRID> static void fill_grid(const GRID* g, hj::GridArgs<T, ND>& G) {
    long long s = 1;
    for (int d = ND - 1; d >= 0; --d) {
        G.n[d] = (int)g->N[d];
        G.bc[d] = g->bc[d];
        G.km[d] = g->toward_zero[d] ? T(-1) : T(1);
        G.inv_dx[d] = (T)(1.0 / g->dx[d]);
        hj::fill_stencil_constants<T>(g->dx[d], G.K[d]);
        G.stride[d] = s;
        s *= g->N[d];
    }
    G.halo_lo = 0;
    G.halo_hi = 0;
    G.total = s;
}

// ---- the descriptor and the tables
static int null_coord(int d) { return fail(HJ_EINVAL, "null coordinate table of axis %d", d); }
static int check_coord(const void* const* coord, int n) {
    for (int d = 0; d < n; ++d)
        if (!coord[d]) return null_coord(d);
    return HJ_OK;
}

// the first nd axes of a descriptor; total = the number of cells.  With `coord`, every axis's coordinate table is checked with the axis
// (libhj_batch.so, libhj_stoch.so); libhj_hidim.so checks its tables once it knows the system (check_coord)
template <typename GRID> static int check_axes(const GRID* g, int nd, const void* const* coord, long long& total) {
    total = 1;
    for (int d = 0; d < nd; ++d) {
        if (g->N[d] < HJ_STENCIL || g->N[d] > (1ll << 30)) return fail(HJ_EINVAL, "N[%d] = %lld out of range (need %d .. 2^30)", d, (long long)g->N[d], HJ_STENCIL);
        if (g->bc[d] != HJ_BC_EXTRAPOLATE && g->bc[d] != HJ_BC_PERIODIC) return fail(HJ_EINVAL, "unknown boundary kind %d on axis %d", (int)g->bc[d], d);
        if (!(g->dx[d] > 0.0) || !std::isfinite(g->dx[d])) return fail(HJ_EINVAL, "axis %d: dx must be positive and finite", d);
        if (coord && !coord[d]) return null_coord(d);
        total *= g->N[d];
        if (total > (1ll << 38)) return fail(HJ_EINVAL, "grid too large");
    }
    return HJ_OK;
}

static int check_aux(const void* const* aux, int naux, int ham) {
    for (int s = 0; s < naux; ++s)
        if (!aux[s]) return fail(HJ_EINVAL, "Hamiltonian %d reads aux table %d, which is null", ham, s);
    return HJ_OK;
}

// the aux tables a built-in system of hj_mi355x.h reads (hjb_tables)
static int builtin_naux(int ham) { return ham == HJ_HAM_DUBINS_REL ? 2 : (ham == HJ_HAM_DOUBLE_PENDULUM ? 4 : 0); }

// ---- stepBound = 1 / sum_d max alpha_d / dx_d, summed in dimension order (hj_static_step_bound), from the ndim keys of a bound kernel;
// amax (may be null) gets the maxima, its slots ndim .. slots - 1 zero
static double step_bound_of_keys(const unsigned long long* keys, const double* dx, int ndim, double* amax, int slots) {
    double inv = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double a = hj::key_to_double(keys[d]);
        if (amax) amax[d] = a;
        inv += a / dx[d];
    }
    for (int d = ndim; d < slots && amax; ++d) amax[d] = 0.0;
    return 1.0 / inv;
}

// ---- one launch of an interval: the stage, its arrays and scalars
struct Stage {
    int stage;
    const void* src;
    const void* y0;
    void* dst;
    double dt;
    int post_prev, op_a, op_b;
    const void* post_a;
    const void* post_b;
};

// the stage a step of `order` runs as its j-th launch
static int rk_stage_id(int order, int j) {
    return j == 0 ? HJ_STAGE_EULER : (order == 2 ? HJ_STAGE_RK2_FULL : (j == 1 ? HJ_STAGE_RK3_HALF : HJ_STAGE_RK3_FULL));
}

// The stages of dts.size() steps in launch order, `order` per step: step k reads the state of step k - 1 (y_in first) and leaves its own in
// buf_a (k even) or buf_b (k odd).  RK3: the first stage buffer doubles as the output; RK2: `work` is the first stage buffer
// (hj_rk_integrate).  The post-step operators act on a step's last stage only.
static void rk_schedule(int order, const void* y_in, void* buf_a, void* buf_b, void* work, const std::vector<double>& dts, int post_prev,
                        int op_a, const void* post_a, int op_b, const void* post_b, std::vector<Stage>& st) {
    st.clear();
    st.reserve(dts.size() * (size_t)order);
    void* outs[2] = {buf_a, buf_b};
    const void* cur = y_in;
    for (size_t k = 0; k < dts.size(); ++k) {
        void* nxt = outs[k & 1];
        void* first = order == 2 ? work : nxt;
        const void* src[3] = {cur, first, work};
        void* dst[3] = {first, order == 2 ? nxt : work, nxt};
        for (int j = 0; j < order; ++j)
            st.push_back(Stage{rk_stage_id(order, j), src[j], j ? cur : nullptr, dst[j], dts[k], 0, 0, 0, nullptr, nullptr});
        Stage& last = st.back();
        last.post_prev = post_prev;
        last.op_a = op_a; last.post_a = op_a ? post_a : nullptr;
        last.op_b = op_b; last.post_b = op_b ? post_b : nullptr;
        cur = nxt;
    }
}

// where the state is after n steps: 0 = y_in, 1 = buf_a, 2 = buf_b
static int32_t result_in(int64_t n) { return n == 0 ? 0 : 1 + (int32_t)((n - 1) & 1); }

// ---- checks of a stage and of an interval.  `problem` >= 0: a batched problem, named in front of the refusal
static int refuse(long long problem, const char* what) {
    return problem < 0 ? fail(HJ_EINVAL, "%s", what) : fail(HJ_EINVAL, "problem %lld: %s", problem, what);
}

static int check_stage_id(int stage) {
    return (stage < HJ_STAGE_YDOT || stage > HJ_STAGE_RK2_FULL) ? fail(HJ_EINVAL, "unknown stage %d", stage) : HJ_OK;
}
static int check_y0(int stage, const void* y0) {
    return (stage >= HJ_STAGE_RK3_HALF && !y0) ? fail(HJ_EINVAL, "stage %d reads y0, which is null", stage) : HJ_OK;
}
static int check_order(int order) { return (order < 1 || order > 3) ? fail(HJ_EINVAL, "order must be 1, 2 or 3") : HJ_OK; }
static int check_post_prev(int post_prev) {
    return (post_prev < HJ_POST_NONE || post_prev > HJ_POST_MAX_PREV) ? fail(HJ_EINVAL, "unknown post-step operator %d", post_prev) : HJ_OK;
}
// op: 0 none, 1 min, 2 max, 3 max(y, -array) -- HJB_ARR_* and HJH_ARR_*
static int check_array_ops(int op_a, const void* post_a, int op_b, const void* post_b, long long problem = -1) {
    if (op_a < 0 || op_a > 3 || op_b < 0 || op_b > 3) return refuse(problem, "unknown array operator");
    if ((op_a && !post_a) || (op_b && !post_b)) return refuse(problem, "an array operator without its array");
    return HJ_OK;
}
static int check_buffers(int order, const void* y_in, const void* buf_a, const void* buf_b, const void* work, long long problem = -1) {
    if (!y_in || !buf_a || !buf_b) return refuse(problem, "null buffer");
    if (order >= 2 && !work) return refuse(problem, "work buffer required for order >= 2");
    if (buf_a == buf_b || buf_a == y_in || buf_b == y_in || work == y_in || work == buf_a || work == buf_b)
        return refuse(problem, "buffers must be distinct");
    return HJ_OK;
}

}  // namespace hj_tool
#endif
