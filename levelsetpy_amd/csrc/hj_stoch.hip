// libhj_stoch.so (include/hj_stoch.h): phi_t + H(x, grad phi) = trace(sigma^T D^2phi sigma) for a built-in system and a constant sigma,
// every RK stage ONE launch, for gfx950 -- what termSum(termLaxFriedrichs | termRestrictUpdate, termTraceHessian) computes with two
// full-grid kernels, a full-grid add and a stage expression per stage.
//   stoch_substep_kernel<T, HAM, SCHEME, DIAG>  batch_substep_kernel (hj_batch.hip) for one problem, with the diffusion term: one thread per
//                                               cell, every stencil load issued unconditionally.  The Lax-Friedrichs ydot and its clamp are
//                                               formed as there; the Hessian of hessianSecond comes from the face neighbours the upwind stencil
//                                               already holds (v[d][2], v[d][4]: the width-1 ghost of addGhostAllDims is the stencil's first
//                                               ghost, ghost_value(edge, inner, km), bit for bit) and, unless DIAG, from 2 ND (ND - 1) diagonal
//                                               neighbours more; padded_value / nb_offset / trace_triple are hj_curv.h's.  sigma, the system's
//                                               parameters, dt, the arrays and the post-step operators ride in the kernel arguments.
//   stoch_bound_kernel<T, HAM>                  the per-dimension maxima of alpha at zero costate (batch_bound_kernel's evaluation)
// The per-cell functions are the solver's own source, compiled with the solver's flags.  The library links nothing of libhj_mi355x.so.
// What this library shares with libhj_batch.so and libhj_hidim.so is in two headers.  hj_stage_dev.h: tables_of, what a stage stores
// (stage_result, array_op), the fold that ends the bound kernel.  hj_stage_host.h: the descriptor as GridArgs (fill_grid) and its checks,
// the Lax-Friedrichs step bound from the keys, struct Stage and its checks, and the RK schedule (rk_schedule) whose stages hjw_integrate
// dispatches one by one.  Here: sigma and its checks, the stage's alias checks, the interval's check against the post-step arrays.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "hj_tool_host.h"
#include "hj_curv.h"
#include "hj_stage_host.h"
#include "hj_stage_dev.h"
#include "../../include/hj_stoch.h"

namespace hjw {

using namespace hj;
using namespace hj_tool;

template <typename T, int ND> struct StochArgs {
    GridArgs<T, ND> G;
    T sc[ND];                          // costate scale of the scheme (hj_device.h)
    const T* coord[HJ_MAX_DIM];
    const T* aux[4];
    double par[HJB_PAR_SLOTS];
    T sig[ND * ND];                    // sigma, row-major: L = sigma^T, R = sigma
    T hdx_inv[ND];                     // 0.5 / dx_i and 1 / dx_i^2, as curv_kernel takes them (hessian.py:71, :85)
    T dx_inv2[ND];
    const T* src;
    const T* y0;
    T* dst;
    const T* post_a;
    const T* post_b;
    T dt;
    int stage, restrict_sign, post_prev, op_a, op_b;
};

static_assert(HJB_ARR_NONE == 0 && HJB_ARR_MIN == 1 && HJB_ARR_MAX == 2 && HJB_ARR_MAX_NEG == 3, "array_op and check_array_ops take the numbers");

template <typename T, typename HAM, int SCHEME, bool DIAG>
__global__ __launch_bounds__(256) void stoch_substep_kernel(const StochArgs<T, HAM::ND> A) {
    constexpr int ND = HAM::ND;
    constexpr bool NP = np_order(SCHEME);
    constexpr int NPAIR = CurvStencil<ND>::NPAIR;
    static_assert(SCHEME != HJ_WENO5, "the intended WENO5 needs an epsilon reduction over the grid");
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= A.G.total) return;
    const HamTables<T> P = tables_of<T>(A.coord, A.aux, A.par);
    const T* __restrict__ y = A.src;
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
    const T centre = pc0[0];
    const T y0v = use_y0 ? A.y0[t] : T(0);
    // the diagonal neighbours g[pair][k], k = 2 (sign along q) + (sign along p), pairs (p < q) in the order (0,1), (0,2), ..., (1,2), ...
    // (curv_kernel's layout): issued before the upwind stencils so that every load of the cell is in flight together
    T g[NPAIR][4];
    bool ghost = false;
    if constexpr (!DIAG) {
        long long of[ND][2];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            of[d][0] = nb_offset<T, ND>(A.G, idx, d, -1, ghost);
            of[d][1] = nb_offset<T, ND>(A.G, idx, d, 1, ghost);
        }
        int k = 0;
#pragma unroll
        for (int p = 0; p < ND; ++p)
#pragma unroll
            for (int q = p + 1; q < ND; ++q, ++k)
#pragma unroll
                for (int s = 0; s < 4; ++s) g[k][s] = pc0[of[p][s & 1] + of[q][s >> 1]];
    }
    T v[ND][7];
    const typename HAM::Cell hc = HAM::cell(P, idx, A.sc);
    const typename HAM::Plane hp = HAM::plane(P, idx[0], A.sc);
    gather_stencils<T, ND>(A.G, pc0, idx, centre, v);
    if constexpr (!DIAG) {
        if (__any(ghost ? 1 : 0)) {
            // the waves at an extrapolated edge: the corner ghosts of addGhostAllDims in its order (padded_value)
            int k = 0;
#pragma unroll
            for (int p = 0; p < ND; ++p)
#pragma unroll
                for (int q = p + 1; q < ND; ++q, ++k) {
                    const bool ep = A.G.bc[p] != HJ_BC_PERIODIC && (idx[p] == 0 || idx[p] == A.G.n[p] - 1);
                    const bool eq = A.G.bc[q] != HJ_BC_PERIODIC && (idx[q] == 0 || idx[q] == A.G.n[q] - 1);
                    if (!ep && !eq) continue;
#pragma unroll
                    for (int s = 0; s < 4; ++s) g[k][s] = padded_value<T, ND>(A.G, pc0, idx, p, (s & 1) ? 1 : -1, q, (s >> 1) ? 1 : -1);
                }
        }
    }
    T pc[ND], hd[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) upwind_cd<SCHEME, T>(v[d], A.G.K[d], eps[d], wk[d], pc[d], hd[d]);
    T alpha[ND];
    T ydot = lf_ydot<NP, HAM>(P, hc, hp, A.sc, pc, hd, alpha);
    // termRestrictUpdate clamp on the Lax-Friedrichs term, written like direct_substep_kernel's (a NaN stays a NaN).  Written out, not
    // restrict_clamp (hj_stage_dev.h): with the trace added behind it the inlined helper turns a branch of the ENO3 kernels around
    if (A.restrict_sign > 0) ydot = (ydot < T(0)) ? T(0) : ydot;
    else if (A.restrict_sign < 0) ydot = (ydot > T(0)) ? T(0) : ydot;
    {
#pragma clang fp contract(off)
        // hessianSecond (hessian.py:85, :88-99) in curv_kernel's operation order; the face neighbours are the stencil's
        T sii[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const T two_c = T(2) * centre;
            const T up = v[d][4] - two_c;
            const T sum = up + v[d][2];
            sii[d] = A.dx_inv2[d] * sum;
        }
        T tr;
        if constexpr (DIAG) {
            tr = T(0);
#pragma unroll
            for (int i = 0; i < ND; ++i) {
                const T lp = A.sig[i * ND + i] * sii[i];
                const T a = lp * A.sig[i * ND + i];
                tr = i == 0 ? a : tr + a;
            }
        } else {
            T sij[NPAIR];
            int k = 0;
#pragma unroll
            for (int p = 0; p < ND; ++p)
#pragma unroll
                for (int q = p + 1; q < ND; ++q, ++k) {
                    const T dq_p = g[k][3] - g[k][1];
                    const T dq_m = g[k][2] - g[k][0];
                    const T fq_p = A.hdx_inv[q] * dq_p;                    // first[q] at +e_p
                    const T fq_m = A.hdx_inv[q] * dq_m;                    // first[q] at -e_p
                    const T df = fq_p - fq_m;
                    sij[k] = A.hdx_inv[p] * df;
                }
            auto Pm = [&](int m, int kk) -> T {
                if (m == kk) return sii[m];
                const int j = m < kk ? m : kk, i = m < kk ? kk : m;
                return sij[j * ND - j * (j + 1) / 2 + (i - j - 1)];
            };
            // trace(L P R), L = sigma^T, R = sigma (term_trace_hess.py:115-116)
            tr = trace_triple<T, ND>([&](int i, int m) { return A.sig[m * ND + i]; }, Pm,
                                     [&](int kk, int i) { return A.sig[kk * ND + i]; });
        }
        ydot = ydot + tr;                                                  // termSum (term_sum.py:97)
    }
    A.dst[t] = stage_result<NP>(A, stage, ca, cb, use_y0, A.dt, y0v, centre, ydot, t);
}

// max over the grid of alpha_d at zero costate: the evaluation of alpha_bound_kernel (hj_split.h) / batch_bound_kernel, one workgroup
// maximum per dimension folded into keys[d] (order-preserving keys, zero at launch)
template <typename T, int ND> struct BoundArgs {
    GridArgs<T, ND> G;
    const T* coord[HJ_MAX_DIM];
    const T* aux[4];
    double par[HJB_PAR_SLOTS];
};
template <typename T, typename HAM>
__global__ __launch_bounds__(256) void stoch_bound_kernel(const BoundArgs<T, HAM::ND> A, unsigned long long* keys) {
    constexpr int ND = HAM::ND;
    const HamTables<T> P = tables_of<T>(A.coord, A.aux, A.par);
    double m[ND];
    T one[ND], p[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) { m[d] = -1e300; one[d] = T(1); p[d] = T(0); }
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < A.G.total; t += (long long)gridDim.x * blockDim.x) {
        int idx[ND];
        decode<T, ND>(A.G, t, idx);
        T H, a[ND];
        HAM::eval(P, HAM::cell(P, idx, one), HAM::plane(P, idx[0], one), one, p, H, a);
#pragma unroll
        for (int d = 0; d < ND; ++d) m[d] = fmax(m[d], (double)a[d]);
    }
    fold_bound<ND>(m, keys);
}

// ---------------------------------------------------------------------------------------------- host side
// the checks every entry point makes on (grid, tables, system)
static int check_setup(const hjq_grid* g, const hjb_tables* tab, int ham) {
    if (!g || !tab) return fail(HJ_EINVAL, "null grid descriptor or tables");
    if (g->dtype == HJ_F32) return fail(HJ_EUNSUPPORTED, "HJ_F32 has no stochastic kernel (HJ_F64 only)");
    if (g->dtype != HJ_F64) return fail(HJ_EINVAL, "unknown dtype %d", (int)g->dtype);
    const int nd = ham_ndim(ham);
    if (nd == 0) return fail(HJ_EUNSUPPORTED, "Hamiltonian %d has no stochastic kernel (the three built-in systems only)", ham);
    if (g->ndim != nd) return fail(HJ_EINVAL, "Hamiltonian %d lives on %d-D grids, the grid has %d dimensions", ham, nd, (int)g->ndim);
    long long total;
    const int rc = check_axes(g, nd, tab->coord, total);
    return rc ? rc : check_aux(tab->aux, builtin_naux(ham), ham);
}

static int check_scheme(int scheme) {
    if (scheme == HJ_WENO5) return fail(HJ_EUNSUPPORTED, "the intended WENO5 (HJ_WENO5) has no stochastic kernel: its epsilon is a reduction over the grid");
    return check_point_scheme(scheme, "stochastic");
}

// sigma: nd x nd finite numbers; diag = whether the diagonal instantiation runs
static int check_sigma(const double* sigma, int nd, int form, bool& diag) {
    if (!sigma) return fail(HJ_EINVAL, "null sigma");
    if (form < HJW_FORM_AUTO || form > HJW_FORM_DIAGONAL) return fail(HJ_EINVAL, "unknown form %d", form);
    bool off = false;
    for (int i = 0; i < nd; ++i)
        for (int j = 0; j < nd; ++j) {
            if (!std::isfinite(sigma[i * nd + j])) return fail(HJ_EINVAL, "sigma[%d][%d] is not finite", i, j);
            if (i != j && sigma[i * nd + j] != 0.0) off = true;
        }
    if (form == HJW_FORM_DIAGONAL && off) return fail(HJ_EINVAL, "HJW_FORM_DIAGONAL with a sigma that has a non-zero off-diagonal entry");
    diag = form == HJW_FORM_DIAGONAL || (form == HJW_FORM_AUTO && !off);
    return HJ_OK;
}

// the checks on a stage's arrays: nothing read may be null, the output aliases none of them
static int check_stage(const Stage& s) {
    if (!s.src || !s.dst) return fail(HJ_EINVAL, "null src or dst");
    int rc = check_y0(s.stage, s.y0);
    if (rc) return rc;
    if ((rc = check_post_prev(s.post_prev))) return rc;
    if ((rc = check_array_ops(s.op_a, s.post_a, s.op_b, s.post_b))) return rc;
    const bool use_y0 = s.stage >= HJ_STAGE_RK3_HALF;
    if (s.dst == s.src || (use_y0 && s.dst == s.y0) || (s.op_a && s.dst == s.post_a) || (s.op_b && s.dst == s.post_b))
        return fail(HJ_EINVAL, "dst must not alias an array the stage reads");
    return HJ_OK;
}

template <typename T, typename HAM, int SCHEME, bool DIAG>
static int launch_substep(const hjq_grid* g, const hjb_tables* tab, int restrict_sign, const double* params, const double* sigma,
                          const Stage& s, hipStream_t stream, const char* name) {
    constexpr int ND = HAM::ND;
    StochArgs<T, ND> A;
    memset(&A, 0, sizeof(A));
    fill_grid<T, ND>(g, A.G);
    for (int d = 0; d < ND; ++d) {
        A.sc[d] = scheme_scale<T>(SCHEME, g->dx[d]);
        const double di = 1.0 / g->dx[d];              // as curv_launch_nd (hj_api.hip)
        A.hdx_inv[d] = (T)(0.5 * di);
        A.dx_inv2[d] = (T)(di * di);
    }
    for (int d = 0; d < HJ_MAX_DIM; ++d) A.coord[d] = (const T*)tab->coord[d];
    for (int k = 0; k < 4; ++k) A.aux[k] = (const T*)tab->aux[k];
    for (int k = 0; k < HJB_PAR_SLOTS; ++k) A.par[k] = params[k];
    for (int e = 0; e < ND * ND; ++e) A.sig[e] = (T)sigma[e];
    A.src = (const T*)s.src;
    A.y0 = (const T*)s.y0;
    A.dst = (T*)s.dst;
    A.post_a = s.op_a ? (const T*)s.post_a : nullptr;
    A.post_b = s.op_b ? (const T*)s.post_b : nullptr;
    A.dt = (T)s.dt;
    A.stage = s.stage;
    A.restrict_sign = restrict_sign;
    A.post_prev = s.post_prev;
    A.op_a = s.op_a;
    A.op_b = s.op_b;
    unsigned bx;
    int rc = blocks_for(A.G.total, "grid too large for one thread per cell", bx);
    if (rc) return rc;
    hipLaunchKernelGGL((stoch_substep_kernel<T, HAM, SCHEME, DIAG>), dim3(bx), dim3(256), 0, stream, A);
    return launch_done(name);
}

static int dispatch_substep(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int restrict_sign, const double* params,
                            const double* sigma, bool diag, const Stage& s, hipStream_t stream) {
#define HJW_GO(HAM, SCH, DG) \
    return launch_substep<double, HAM<double>, SCH, DG>(g, tab, restrict_sign, params, sigma, s, stream, \
                                                        "stoch_substep_kernel<double, " #HAM ", " #SCH ", " #DG ">")
#define HJW_HAMS(SCH, DG)                                               \
    do {                                                                \
        if (ham == HJ_HAM_DUBINS_REL) HJW_GO(HamDubinsRel, SCH, DG);     \
        if (ham == HJ_HAM_DOUBLE_INTEGRATOR) HJW_GO(HamDoubleIntegrator, SCH, DG); \
        HJW_GO(HamDoublePendulum, SCH, DG);                              \
    } while (0)
    static_assert(HJ_ENO2 == 0 && HJ_ENO3 == 1 && HJ_WENO5_ASSHIPPED == 3, "scheme ids name the kernels");
    if (diag) {
        if (scheme == HJ_ENO2) HJW_HAMS(0, 1);
        if (scheme == HJ_ENO3) HJW_HAMS(1, 1);
        HJW_HAMS(3, 1);
    }
    if (scheme == HJ_ENO2) HJW_HAMS(0, 0);
    if (scheme == HJ_ENO3) HJW_HAMS(1, 0);
    HJW_HAMS(3, 0);
#undef HJW_HAMS
#undef HJW_GO
}

template <typename T, typename HAM>
static int launch_bound(const hjq_grid* g, const hjb_tables* tab, const double* params, unsigned long long* keys, hipStream_t stream) {
    constexpr int ND = HAM::ND;
    BoundArgs<T, ND> A;
    memset(&A, 0, sizeof(A));
    fill_grid<T, ND>(g, A.G);
    for (int d = 0; d < HJ_MAX_DIM; ++d) A.coord[d] = (const T*)tab->coord[d];
    for (int k = 0; k < 4; ++k) A.aux[k] = (const T*)tab->aux[k];
    for (int k = 0; k < HJB_PAR_SLOTS; ++k) A.par[k] = params[k];
    const unsigned bx = (unsigned)std::min<long long>((A.G.total + 255) / 256, 64);
    hipLaunchKernelGGL((stoch_bound_kernel<T, HAM>), dim3(bx), dim3(256), 0, stream, A, keys);
    return launch_done("stoch_bound_kernel");
}

// trace((L D) R) for L = sigma^T, R = sigma, D[m][k] = 1 / (dx_m dx_k): the expression order of trace_ldr (hj_api.hip), which is
// trace_triple's (term_trace_hess.py:119-122)
static double trace_ldr(const hjq_grid* g, const double* sigma) {
#pragma clang fp contract(off)
    const int n = g->ndim;
    double tr = 0.0;
    for (int i = 0; i < n; ++i) {
        double a = 0.0;
        for (int k = 0; k < n; ++k) {
            double lp = sigma[i] * (1.0 / (g->dx[0] * g->dx[k]));                                  // L[i][0] = sigma[0][i]
            for (int m = 1; m < n; ++m) lp = lp + sigma[m * n + i] * (1.0 / (g->dx[m] * g->dx[k]));
            a = k == 0 ? lp * sigma[i] : a + lp * sigma[k * n + i];
        }
        tr = i == 0 ? a : tr + a;
    }
    return tr;
}

}  // namespace hjw

using namespace hjw;

extern "C" {

int hjw_step_bound(const hjq_grid* g, const hjb_tables* tab, int ham, const double* params_host, const double* sigma_host,
                   void* keys, double* sb_host, void* stream) {
    int rc = check_setup(g, tab, ham);
    if (rc) return rc;
    bool diag;
    if ((rc = check_sigma(sigma_host, g->ndim, HJW_FORM_AUTO, diag))) return rc;
    if (!params_host || !keys || !sb_host) return fail(HJ_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* k = (unsigned long long*)keys;
    HIP_TRY(hipMemsetAsync(k, 0, sizeof(unsigned long long) * HJ_MAX_DIM, s));
    rc = ham == HJ_HAM_DUBINS_REL ? launch_bound<double, HamDubinsRel<double>>(g, tab, params_host, k, s)
       : ham == HJ_HAM_DOUBLE_INTEGRATOR ? launch_bound<double, HamDoubleIntegrator<double>>(g, tab, params_host, k, s)
                                         : launch_bound<double, HamDoublePendulum<double>>(g, tab, params_host, k, s);
    if (rc) return rc;
    unsigned long long h[HJ_MAX_DIM];
    HIP_TRY(hipMemcpyAsync(h, k, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double sb_lf = step_bound_of_keys(h, g->dx, g->ndim, nullptr, 0);
    // sb_TH = 1 / (2 max |trace((L D) R)|), inf when nothing diffuses (hj_term_trace_hessian)
    const double mt = std::fabs(trace_ldr(g, sigma_host));
    const double sb_th = mt == 0.0 ? std::numeric_limits<double>::infinity() : 1.0 / (2.0 * mt);
    // termSum (term_sum.py:98, :107-110)
    double inv = 0.0;
    inv += 1.0 / sb_lf;
    inv += 1.0 / sb_th;
    sb_host[0] = inv == 0.0 ? std::numeric_limits<double>::infinity() : 1.0 / inv;
    sb_host[1] = sb_lf;
    sb_host[2] = sb_th;
    return HJ_OK;
}

int hjw_substep(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int stage, int restrict_sign,
                const double* params_host, const double* sigma_host, int form, const hjb_entry* entry_host, void* stream) {
    int rc = check_setup(g, tab, ham);
    if (rc) return rc;
    if ((rc = check_scheme(scheme))) return rc;
    if ((rc = check_stage_id(stage))) return rc;
    bool diag;
    if ((rc = check_sigma(sigma_host, g->ndim, form, diag))) return rc;
    if (!params_host || !entry_host) return fail(HJ_EINVAL, "null argument");
    const hjb_entry& e = *entry_host;
    const bool ops = stage != HJ_STAGE_YDOT;
    Stage s{stage, e.src, e.y0, e.dst, e.dt, ops ? e.post_prev : 0, ops ? e.op_a : 0, ops ? e.op_b : 0, ops ? e.post_a : nullptr,
            ops ? e.post_b : nullptr};
    if ((rc = check_stage(s))) return rc;
    return dispatch_substep(g, tab, scheme, ham, restrict_sign, params_host, sigma_host, diag, s, (hipStream_t)stream);
}

int hjw_plan(int order, double sb, double t0, double tf, double factor_cfl, double max_step, double stop_tol, double* t_host,
             int64_t* steps_host) {
    int rc = check_order(order);
    if (rc) return rc;
    std::vector<double> dts;
    double t;
    rc = plan_problem(order, sb, t0, tf, factor_cfl, max_step, stop_tol, &dts, t, 0);
    if (rc) return rc;
    if (t_host) *t_host = t;
    if (steps_host) *steps_host = (int64_t)dts.size();
    return HJ_OK;
}

int hjw_integrate(const hjq_grid* g, const hjb_tables* tab, int scheme, int ham, int order, int restrict_sign, int post_prev,
                  const double* params_host, const double* sigma_host, int form, double sb, const hjb_problem* problem_host,
                  double t0, double tf, double factor_cfl, double max_step, double stop_tol, double* t_host,
                  int64_t* steps_host, int32_t* result_in_host, void* stream) {
    int rc = check_setup(g, tab, ham);
    if (rc) return rc;
    if ((rc = check_scheme(scheme))) return rc;
    if ((rc = check_order(order))) return rc;
    if ((rc = check_post_prev(post_prev))) return rc;
    bool diag;
    if ((rc = check_sigma(sigma_host, g->ndim, form, diag))) return rc;
    if (!params_host || !problem_host) return fail(HJ_EINVAL, "null argument");
    const hjb_problem& p = *problem_host;
    if ((rc = check_buffers(order, p.y_in, p.buf_a, p.buf_b, p.work))) return rc;
    if ((rc = check_array_ops(p.op_a, p.post_a, p.op_b, p.post_b))) return rc;
    for (const void* w : {(const void*)p.buf_a, (const void*)p.buf_b, (const void*)p.work})
        if (w && ((p.op_a && w == p.post_a) || (p.op_b && w == p.post_b)))
            return fail(HJ_EINVAL, "a buffer the interval writes aliases a post-step array");
    std::vector<double> dts;
    double tend;
    if ((rc = plan_problem(order, sb, t0, tf, factor_cfl, max_step, stop_tol, &dts, tend, 0))) return rc;
    const int64_t n = (int64_t)dts.size();
    hipStream_t s = (hipStream_t)stream;
    launched_none();
    std::vector<Stage> st;
    rk_schedule(order, p.y_in, p.buf_a, p.buf_b, p.work, dts, post_prev, p.op_a, p.post_a, p.op_b, p.post_b, st);
    for (const Stage& q : st)
        if ((rc = dispatch_substep(g, tab, scheme, ham, restrict_sign, params_host, sigma_host, diag, q, s))) return rc;
    if (t_host) *t_host = tend;
    if (steps_host) *steps_host = n;
    if (result_in_host) *result_in_host = result_in(n);
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjw)

}  // extern "C"
