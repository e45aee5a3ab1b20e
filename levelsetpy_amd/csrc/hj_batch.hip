// libhj_batch.so (include/hj_batch.h): B Hamilton-Jacobi problems on one grid, every RK stage ONE launch for all of them, for gfx950.
//   batch_substep_kernel<T, HAM, SCHEME>  direct_substep_kernel (hj_split.h) with a problem axis: one thread per cell, every stencil load
//                                         issued unconditionally, blockIdx.y the problem.  The grid, the coordinate and aux tables and the
//                                         stage ride in the kernel arguments; what differs per problem -- the Hamiltonian's parameters, dt,
//                                         the source / y0 / destination pointers, the post-step operators -- is read from a device table
//                                         through blockIdx.y: wave-uniform plain loads.  A problem whose entry is inactive returns at once.
//   batch_bound_kernel<T, HAM>            per problem, the per-dimension maxima of alpha at zero costate (alpha_bound_kernel's evaluation)
//   batch_nan_kernel<T>                   per problem, "does the state hold a NaN"
// The per-cell functions (gather_stencils, upwind_cd, HAM::cell / plane / eval, lf_ydot, rk_stage_out, post_step) are the solver's own
// source, compiled with the solver's flags: a problem's result has the bits direct_substep_kernel gives for it alone.  The library links
// nothing of libhj_mi355x.so.
// What this library shares with libhj_stoch.so and libhj_hidim.so is in two headers.  hj_stage_dev.h: tables_of, the clamp, what a stage
// stores (stage_result, array_op), the fold that ends the bound kernel.  hj_stage_host.h: the descriptor as GridArgs (fill_grid) and its
// checks, the step bound from the keys, a stage's and an interval's checks, and the RK schedule (rk_schedule) whose stages hjb_integrate
// writes into its table.  Here: the problem axis, the device table and the per-problem prefix of the refusals.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "hj_tool_host.h"
#include "hj_split.h"
#include "hj_stage_host.h"
#include "hj_stage_dev.h"
#include "../../include/hj_batch.h"

namespace hjb {

using namespace hj;
using namespace hj_tool;

constexpr long long MAX_Y = 65535;      // gridDim.y of one launch

static_assert(sizeof(hjb_entry) == 64, "hjb_entry is 64 bytes (include/hj_batch.h)");
static_assert(HJB_ARR_NONE == 0 && HJB_ARR_MIN == 1 && HJB_ARR_MAX == 2 && HJB_ARR_MAX_NEG == 3, "array_op and check_array_ops take the numbers");

// what every problem of a launch shares
template <typename T, int ND> struct BatchArgs {
    GridArgs<T, ND> G;
    T sc[ND];                          // costate scale of the scheme (hj_device.h)
    const T* coord[HJ_MAX_DIM];
    const T* aux[4];
    const double* par;                 // HJB_PAR_SLOTS per problem, first problem of this launch
    const hjb_entry* tab;              // one entry per problem, first problem of this launch
    int stage, restrict_sign;
};

template <typename T, typename HAM, int SCHEME>
__global__ __launch_bounds__(256) void batch_substep_kernel(const BatchArgs<T, HAM::ND> A) {
    constexpr int ND = HAM::ND;
    constexpr bool NP = np_order(SCHEME);
    static_assert(SCHEME != HJ_WENO5, "the intended WENO5 needs a per-problem epsilon reduction");
    // the problem's entry: a uniform index, so these are scalar loads.  A finished problem leaves before anything of it is touched
    const hjb_entry* __restrict__ e = A.tab + blockIdx.y;
    if (e->active == 0) return;
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= A.G.total) return;
    const HamTables<T> P = tables_of<T>(A.coord, A.aux, A.par + (long long)blockIdx.y * HJB_PAR_SLOTS);
    const T* __restrict__ y = (const T*)e->src;
    const T* __restrict__ y0 = (const T*)e->y0;
    T* __restrict__ out = (T*)e->dst;
    const T dt = (T)e->dt;
    const int stage = A.stage;
    T eps[ND];
    WenoK<T> wk[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        eps[d] = T(0);
        wk[d].c13 = T(0); wk[d].c4 = T(0);
    }
    T ca = T(0), cb = T(1);
    if (stage == HJ_STAGE_RK3_HALF) { ca = T(0.75); cb = T(0.25); }
    else if (stage == HJ_STAGE_RK3_FULL) { ca = T(1.0 / 3.0); cb = T(2.0 / 3.0); }
    else if (stage == HJ_STAGE_RK2_FULL) { ca = T(0.5); cb = T(0.5); }
    const bool use_y0 = stage >= HJ_STAGE_RK3_HALF;
    int idx[ND];
    decode<T, ND>(A.G, t, idx);
    const T* pc0 = y + t;
    T v[ND][7];
    const T centre = pc0[0];
    const T y0v = use_y0 ? y0[t] : T(0);
    const typename HAM::Cell hc = HAM::cell(P, idx, A.sc);
    const typename HAM::Plane hp = HAM::plane(P, idx[0], A.sc);
    gather_stencils<T, ND>(A.G, pc0, idx, centre, v);
    T pc[ND], hd[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) upwind_cd<SCHEME, T>(v[d], A.G.K[d], eps[d], wk[d], pc[d], hd[d]);
    T alpha[ND];
    T ydot = lf_ydot<NP, HAM>(P, hc, hp, A.sc, pc, hd, alpha);
    ydot = restrict_clamp(A.restrict_sign, ydot);
    out[t] = stage_result<NP>(*e, stage, ca, cb, use_y0, dt, y0v, centre, ydot, t);
}

// max over the grid of alpha_d at zero costate, per problem: the evaluation of alpha_bound_kernel (hj_split.h) -- HAM::eval with unit scales --
// one workgroup maximum per dimension folded into keys[problem][d] (order-preserving keys, zero at launch)
template <typename T, typename HAM>
__global__ __launch_bounds__(256) void batch_bound_kernel(const GridArgs<T, HAM::ND> G, const hjb_tables tab, const double* par,
                                                         unsigned long long* keys) {
    constexpr int ND = HAM::ND;
    const HamTables<T> P = tables_of<T>((const T* const*)tab.coord, (const T* const*)tab.aux, par + (long long)blockIdx.y * HJB_PAR_SLOTS);
    double m[ND];
    T one[ND], p[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) { m[d] = -1e300; one[d] = T(1); p[d] = T(0); }
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < G.total; t += (long long)gridDim.x * blockDim.x) {
        int idx[ND];
        decode<T, ND>(G, t, idx);
        T H, a[ND];
        HAM::eval(P, HAM::cell(P, idx, one), HAM::plane(P, idx[0], one), one, p, H, a);
#pragma unroll
        for (int d = 0; d < ND; ++d) m[d] = fmax(m[d], (double)a[d]);
    }
    fold_bound<ND>(m, keys + (long long)blockIdx.y * HJ_MAX_DIM);
}

template <typename T>
__global__ __launch_bounds__(256) void batch_nan_kernel(const hjb_entry* tab, long long n, int* flags) {
    const hjb_entry* e = tab + blockIdx.y;
    if (e->active == 0) return;
    const T* __restrict__ y = (const T*)e->src;
    bool bad = false;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const T a = y[t];
        bad = bad || (a != a);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags + blockIdx.y, 1);
}

// ---------------------------------------------------------------------------------------------- host side
// the checks every entry point makes on (grid, tables, system); total = the number of cells
static int check_setup(const hjq_grid* g, const hjb_tables* tab, int ham, long long& total) {
    if (!g || !tab) return fail(HJ_EINVAL, "null grid descriptor or tables");
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", (int)g->dtype);
    const int nd = ham_ndim(ham);
    if (nd == 0) return fail(HJ_EUNSUPPORTED, "Hamiltonian %d has no batched kernel (the three built-in systems only)", ham);
    if (g->ndim != nd) return fail(HJ_EINVAL, "Hamiltonian %d lives on %d-D grids, the grid has %d dimensions", ham, nd, (int)g->ndim);
    const int rc = check_axes(g, nd, tab->coord, total);
    return rc ? rc : check_aux(tab->aux, builtin_naux(ham), ham);
}

template <typename T, typename HAM, int SCHEME>
static int launch_substep(const hjq_grid* g, const hjb_tables* tab, int stage, int restrict_sign, const double* params,
                          const hjb_entry* entries, int64_t B, hipStream_t stream, const char* name) {
    constexpr int ND = HAM::ND;
    BatchArgs<T, ND> A;
    memset(&A, 0, sizeof(A));
    fill_grid<T, ND>(g, A.G);
    for (int d = 0; d < ND; ++d) A.sc[d] = scheme_scale<T>(SCHEME, g->dx[d]);
    for (int d = 0; d < HJ_MAX_DIM; ++d) A.coord[d] = (const T*)tab->coord[d];
    for (int s = 0; s < 4; ++s) A.aux[s] = (const T*)tab->aux[s];
    A.stage = stage;
    A.restrict_sign = restrict_sign;
    unsigned bx;
    int rc = blocks_for(A.G.total, "grid too large for one thread per cell", bx);
    if (rc) return rc;
    for (int64_t off = 0; off < B; off += MAX_Y) {
        const int64_t nb = std::min<int64_t>(MAX_Y, B - off);
        A.par = params + off * HJB_PAR_SLOTS;
        A.tab = entries + off;
        hipLaunchKernelGGL((batch_substep_kernel<T, HAM, SCHEME>), dim3(bx, (unsigned)nb), dim3(256), 0, stream, A);
        HIP_TRY(hipGetLastError());
    }
    launched(name);
    return HJ_OK;
}

static int dispatch_substep(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int stage, int restrict_sign,
                            const double* params, const hjb_entry* entries, int64_t B, hipStream_t stream) {
#define HJB_GO(T, HAM, SCH) \
    return launch_substep<T, HAM<T>, SCH>(g, tab, stage, restrict_sign, params, entries, B, stream, "batch_substep_kernel<" #T ", " #HAM ", " #SCH ">")
#define HJB_HAMS(T, SCH)                                                \
    do {                                                                \
        if (ham == HJ_HAM_DUBINS_REL) HJB_GO(T, HamDubinsRel, SCH);     \
        if (ham == HJ_HAM_DOUBLE_INTEGRATOR) HJB_GO(T, HamDoubleIntegrator, SCH); \
        HJB_GO(T, HamDoublePendulum, SCH);                              \
    } while (0)
    static_assert(HJ_ENO2 == 0 && HJ_ENO3 == 1 && HJ_WENO5_ASSHIPPED == 3, "scheme ids name the kernels");
    if (g->dtype == HJ_F64) {
        if (scheme == HJ_ENO2) HJB_HAMS(double, 0);
        if (scheme == HJ_ENO3) HJB_HAMS(double, 1);
        HJB_HAMS(double, 3);
    }
    if (scheme == HJ_ENO2) HJB_HAMS(float, 0);
    if (scheme == HJ_ENO3) HJB_HAMS(float, 1);
    HJB_HAMS(float, 3);
#undef HJB_HAMS
#undef HJB_GO
}

template <typename T, typename HAM>
static int launch_bound(const hjq_grid* g, const hjb_tables* tab, const double* params, int64_t B, unsigned long long* keys,
                        hipStream_t stream) {
    constexpr int ND = HAM::ND;
    GridArgs<T, ND> G;
    memset(&G, 0, sizeof(G));
    fill_grid<T, ND>(g, G);
    const unsigned bx = (unsigned)std::min<long long>((G.total + 255) / 256, 64);
    for (int64_t off = 0; off < B; off += MAX_Y) {
        const int64_t nb = std::min<int64_t>(MAX_Y, B - off);
        hipLaunchKernelGGL((batch_bound_kernel<T, HAM>), dim3(bx, (unsigned)nb), dim3(256), 0, stream, G, *tab,
                           params + off * HJB_PAR_SLOTS, keys + off * HJ_MAX_DIM);
        HIP_TRY(hipGetLastError());
    }
    launched("batch_bound_kernel");
    return HJ_OK;
}

}  // namespace hjb

using namespace hjb;

extern "C" {

int hjb_step_bounds(const hjq_grid* g, const hjb_tables* tab, int ham, const double* params, int64_t B, void* keys,
                    double* sb_host, double* amax_host, void* stream) {
    long long total;
    int rc = check_setup(g, tab, ham, total);
    if (rc) return rc;
    if (B < 0) return fail(HJ_EINVAL, "B must not be negative");
    if (B == 0) return HJ_OK;
    if (!params || !keys || !sb_host) return fail(HJ_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* k = (unsigned long long*)keys;
    HIP_TRY(hipMemsetAsync(k, 0, sizeof(unsigned long long) * HJ_MAX_DIM * (size_t)B, s));
#define HJB_B(T)                                                                                                   \
    rc = ham == HJ_HAM_DUBINS_REL ? launch_bound<T, HamDubinsRel<T>>(g, tab, params, B, k, s)                       \
       : ham == HJ_HAM_DOUBLE_INTEGRATOR ? launch_bound<T, HamDoubleIntegrator<T>>(g, tab, params, B, k, s)         \
                                         : launch_bound<T, HamDoublePendulum<T>>(g, tab, params, B, k, s)
    if (g->dtype == HJ_F64) HJB_B(double);
    else HJB_B(float);
#undef HJB_B
    if (rc) return rc;
    std::vector<unsigned long long> h((size_t)B * HJ_MAX_DIM);
    HIP_TRY(hipMemcpyAsync(h.data(), k, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t b = 0; b < B; ++b)
        sb_host[b] = step_bound_of_keys(&h[(size_t)b * HJ_MAX_DIM], g->dx, g->ndim, amax_host ? amax_host + b * HJ_MAX_DIM : nullptr, HJ_MAX_DIM);
    return HJ_OK;
}

int hjb_substep(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int stage, int restrict_sign,
                const double* params, const hjb_entry* entries, int64_t B, void* stream) {
    long long total;
    int rc = check_setup(g, tab, ham, total);
    if (rc) return rc;
    if ((rc = check_point_scheme(scheme, "batched"))) return rc;
    if ((rc = check_stage_id(stage))) return rc;
    if (B < 0) return fail(HJ_EINVAL, "B must not be negative");
    if (B == 0) return HJ_OK;
    if (!params || !entries) return fail(HJ_EINVAL, "null argument");
    return dispatch_substep(g, tab, scheme, ham, stage, restrict_sign, params, entries, B, (hipStream_t)stream);
}

int hjb_plan(int order, const double* sb_host, int64_t B, double t0, double tf, double factor_cfl, double max_step,
             double stop_tol, double* t_host, int64_t* steps_host) {
    int rc = check_order(order);
    if (rc) return rc;
    if (B < 0 || (B > 0 && !sb_host)) return fail(HJ_EINVAL, "null argument");
    for (int64_t b = 0; b < B; ++b) {
        std::vector<double> dts;
        double t;
        rc = plan_problem(order, sb_host[b], t0, tf, factor_cfl, max_step, stop_tol, &dts, t, b);
        if (rc) return rc;
        if (t_host) t_host[b] = t;
        if (steps_host) steps_host[b] = (int64_t)dts.size();
    }
    return HJ_OK;
}

int hjb_integrate(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int order, int restrict_sign, int post_prev,
                  const double* params, const double* sb_host, const hjb_problem* problems_host, int64_t B, double t0,
                  double tf, double factor_cfl, double max_step, double stop_tol, void* table, int64_t table_bytes,
                  double* t_host, int64_t* steps_host, int32_t* result_in_host, void* stream) {
    long long total;
    int rc = check_setup(g, tab, ham, total);
    if (rc) return rc;
    if ((rc = check_point_scheme(scheme, "batched"))) return rc;
    if ((rc = check_order(order))) return rc;
    if ((rc = check_post_prev(post_prev))) return rc;
    if (B < 0) return fail(HJ_EINVAL, "B must not be negative");
    if (B == 0) return HJ_OK;
    if (!params || !sb_host || !problems_host) return fail(HJ_EINVAL, "null argument");
    std::vector<std::vector<double>> dts((size_t)B);
    std::vector<double> tend((size_t)B);
    int64_t nmax = 0;
    for (int64_t b = 0; b < B; ++b) {
        const hjb_problem& p = problems_host[b];
        if ((rc = check_buffers(order, p.y_in, p.buf_a, p.buf_b, p.work, b))) return rc;
        if ((rc = check_array_ops(p.op_a, p.post_a, p.op_b, p.post_b, b))) return rc;
        if ((rc = plan_problem(order, sb_host[b], t0, tf, factor_cfl, max_step, stop_tol, &dts[(size_t)b], tend[(size_t)b], b))) return rc;
        nmax = std::max<int64_t>(nmax, (int64_t)dts[(size_t)b].size());
    }
    const int64_t launches = nmax * order;
    const int64_t need = launches * B * (int64_t)sizeof(hjb_entry);
    if (launches > 0 && (!table || table_bytes < need))
        return fail(HJ_EINVAL, "the schedule needs %lld bytes of table (%lld launches x %lld problems), got %lld", (long long)need,
                    (long long)launches, (long long)B, (long long)table_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (launches > 0) {
        // entry (step k, stage j, problem b) -- stage k*order + j of the problem's schedule -- at [(k*order + j)*B + b]; zero = inactive
        std::vector<hjb_entry> sched((size_t)(launches * B));
        memset(sched.data(), 0, sched.size() * sizeof(hjb_entry));
        std::vector<Stage> st;
        for (int64_t b = 0; b < B; ++b) {
            const hjb_problem& p = problems_host[b];
            rk_schedule(order, p.y_in, p.buf_a, p.buf_b, p.work, dts[(size_t)b], post_prev, p.op_a, p.post_a, p.op_b, p.post_b, st);
            for (size_t i = 0; i < st.size(); ++i) {
                const Stage& q = st[i];
                sched[i * (size_t)B + (size_t)b] = hjb_entry{q.src, q.y0, q.dst, q.post_a, q.post_b, q.dt, 1, q.post_prev, q.op_a, q.op_b};
            }
        }
        // ONE copy for the whole interval; the wait keeps `sched` alive until the copy has read it
        HIP_TRY(hipMemcpyAsync(table, sched.data(), sched.size() * sizeof(hjb_entry), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int64_t l = 0; l < launches; ++l) {
            rc = dispatch_substep(g, tab, scheme, ham, rk_stage_id(order, (int)(l % order)), restrict_sign, params,
                                  (const hjb_entry*)table + l * B, B, s);
            if (rc) return rc;
        }
    }
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = (int64_t)dts[(size_t)b].size();
        if (t_host) t_host[b] = tend[(size_t)b];
        if (steps_host) steps_host[b] = n;
        if (result_in_host) result_in_host[b] = result_in(n);
    }
    return HJ_OK;
}

int hjb_nan_flags(int dtype, const hjb_entry* entries, int64_t B, int64_t n, int32_t* flags, void* stream) {
    if (dtype != HJ_F64 && dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", dtype);
    if (B < 0 || n < 0) return fail(HJ_EINVAL, "B and n must not be negative");
    if (B == 0) return HJ_OK;
    if (!entries || !flags) return fail(HJ_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)B, s));
    if (n == 0) return HJ_OK;
    const unsigned bx = (unsigned)std::min<long long>((n + 255) / 256, 64);
    for (int64_t off = 0; off < B; off += MAX_Y) {
        const int64_t nb = std::min<int64_t>(MAX_Y, B - off);
        if (dtype == HJ_F64)
            hipLaunchKernelGGL((batch_nan_kernel<double>), dim3(bx, (unsigned)nb), dim3(256), 0, s, entries + off, (long long)n, (int*)flags + off);
        else
            hipLaunchKernelGGL((batch_nan_kernel<float>), dim3(bx, (unsigned)nb), dim3(256), 0, s, entries + off, (long long)n, (int*)flags + off);
        HIP_TRY(hipGetLastError());
    }
    launched(dtype == HJ_F64 ? "batch_nan_kernel<double>" : "batch_nan_kernel<float>");
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjb)

}  // extern "C"
