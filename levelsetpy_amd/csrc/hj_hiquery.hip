// libhj_hiquery.so (include/hj_hiquery.h): value-function queries and rollouts on 5-D and 6-D grids, for gfx950.
//   hi_interp_points_kernel<T>              V at states: one thread per (field, state)
//   hi_costate_points_kernel<T, ND, SCHEME> grad V at states: 2^ND lanes per (field, state), one corner node each -- 32 lanes
//                                           at 5-D (two states per wavefront), the whole wavefront at 6-D
//   hi_project_minmax_kernel<T, WAVE>       min / max over a subset of axes, a thread or a wavefront per output node
//   hi_rollout_kernel<T, SCHEME, PLANT>     a trajectory per 2^ND lanes, from its first state to its last
// The arithmetic is not restated here: locate, corner, interp_value, gather_axis and group_sum are hj_query_dev.h's, compiled
// at six axes (HJ_QUERY_MAXD), and the trajectory is hj_rollout_dev.h's rollout_body -- the sources libhj_query.so and
// libhj_rollout.so compile.  What is this file's own: the kernels' frames at a compile-time number of axes, the projection's
// loops over up to five removed axes, and the two plants.
// The kernels take the grid with `ndim` overwritten by the template's constant (at<ND>), so every loop over axes of the
// shared functions unrolls and lo / w / cC / cL / cR stay in registers.
#include <hip/hip_runtime.h>
#include <cmath>
#define HJ_QUERY_MAXD 6
#define HJ_QUERY_MIND 5
#include "hj_tool_host.h"
#include "../../include/hj_hidim.h"
#include "hj_query_dev.h"
#include "hj_rollout_dev.h"
#include "../../include/hj_hiquery.h"

static_assert(HJ_QUERY_MAXD == HJH_MAX_DIM && HJ_QUERY_MIND == HJH_MIN_DIM, "the header's range is hj_hidim.h's");

namespace hjx {

using hjq::MAXD;
using hjq::QGrid;
using hjq::QStencil;
using hjq::ProjArgs;
using hjq::Red;
using hjq::make_grid;
using hjq::check_points;
using hjq::TOO_MANY;
using hjr::Plant;
using hjr::RolloutOut;
using namespace hj_tool;

// the grid with a compile-time number of axes
template <int ND> __device__ __forceinline__ QGrid at(const QGrid& G) {
    QGrid g = G;
    g.ndim = ND;
    return g;
}

// the one-sided derivatives of a corner's stencil at 5-D / 6-D: hj_rollout_dev.h's, which libhj_plant.so's run-time kernels share
using hjr::UpwindHidim;

template <typename T>
__device__ __forceinline__ void put(void* out, long long i, double v, int out_f64) {
    if (out_f64) ((double*)out)[i] = v;
    else ((T*)out)[i] = (T)v;
}

// ---- (a) V at states: thread t -> field t / M, state t % M
template <typename T>
__global__ __launch_bounds__(256) void hi_interp_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                               const double* __restrict__ xs, long long M, QGrid G,
                                                               void* __restrict__ out, int out_f64) {
#pragma clang fp contract(off)
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= nfields * M) return;
    const long long f = t / M, m = t - f * M;
    double v;
    if (G.ndim == 5) v = hjq::interp_value<T>(at<5>(G), data + f * field_stride, xs + m * 5);
    else v = hjq::interp_value<T>(at<6>(G), data + f * field_stride, xs + m * 6);
    put<T>(out, t, v, out_f64);
}

// ---- (b) grad V at states: costate_points_kernel (hj_query.hip) at a compile-time number of axes
struct CostateOut {
    void* costate;
    void* derivL;
    void* derivR;
    void* value;
    int out_f64;
};

template <typename T, int ND, int SCHEME>
__global__ __launch_bounds__(256) void hi_costate_points_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                                const double* __restrict__ xs, long long M, QGrid G0, QStencil<T> S,
                                                                CostateOut O) {
    constexpr int lanes = 1 << ND;                 // 32 or 64: divides the wavefront, groups never straddle one
    const QGrid G = at<ND>(G0);
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long grp = t / lanes;
    const int c = (int)(t - grp * lanes);
    if (grp >= nfields * M) return;                // whole groups leave together
    const long long f = grp / M, m = grp - f * M;
    int lo[MAXD];
    double w[MAXD];
    const bool inside = hjq::locate(G, xs + m * ND, lo, w);
    long long off;
    const double wt = hjq::corner(G, lo, w, c, off);
    const int used = wt != 0.0;
    T cC[ND], cL[ND], cR[ND];
    T raw = T(0);
#pragma unroll
    for (int d = 0; d < ND; ++d) cC[d] = cL[d] = cR[d] = T(0);
    if (inside && used) {
        const T* pc0 = data + f * field_stride + off;
        raw = *pc0;
        if (!hjq::finite(raw)) {
            // the node's own NaN / inf is put back after the differences (computeGradients: NaN stays NaN, +-inf becomes +inf)
            const T back = raw != raw ? raw : T(__builtin_inf());
#pragma unroll
            for (int d = 0; d < ND; ++d) cC[d] = cL[d] = cR[d] = back;
        } else {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                int j = lo[d] + ((c >> d) & 1);
                if (G.per[d] && j >= G.n[d]) j -= G.n[d];
                T v[7];
                hjq::gather_axis<T>(pc0, G.stride[d], j, G.n[d], G.per[d] != 0, S.km[d], raw, v);
                T L, R;
                UpwindHidim::lr<SCHEME, T>(v, S.K[d], L, R);
                cL[d] = L;
                cR[d] = R;
                cC[d] = T(0.5) * (L + R);
            }
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        double p, q, r;
        {
#pragma clang fp contract(off)
            p = wt * (double)cC[d];
            q = wt * (double)cL[d];
            r = wt * (double)cR[d];
        }
        const double sC = hjq::group_sum(p, used, lanes);
        if (c == 0) put<T>(O.costate, grp * ND + d, inside ? sC : nan, O.out_f64);
        if (O.derivL) {
            const double sL = hjq::group_sum(q, used, lanes);
            if (c == 0) put<T>(O.derivL, grp * ND + d, inside ? sL : nan, O.out_f64);
        }
        if (O.derivR) {
            const double sR = hjq::group_sum(r, used, lanes);
            if (c == 0) put<T>(O.derivR, grp * ND + d, inside ? sR : nan, O.out_f64);
        }
    }
    if (O.value) {
        double p;
        {
#pragma clang fp contract(off)
            p = wt * (double)raw;
        }
        const double sV = hjq::group_sum(p, used, lanes);
        if (c == 0) put<T>(O.value, grp, inside ? sV : nan, O.out_f64);
    }
}

// ---- (c) min / max over a subset of axes: the one streaming kernel
// WAVE = false: the last axis is kept -- one thread per output node, neighbouring threads read neighbouring elements.
// WAVE = true:  the last axis is removed -- one wavefront per output node; its lanes stride the last axis (neighbouring
//               lanes read neighbouring elements) inside loops over the other removed axes.
// The removed axes sit at the END of rem_n / rem_s (unused leading slots have n = 1), so the loops need no index division: the
// only divisions are proj_base's, once per output node.
template <typename T, bool WAVE>
__global__ __launch_bounds__(256) void hi_project_minmax_kernel(const T* __restrict__ data, T* __restrict__ out, ProjArgs A) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long node = WAVE ? t / 64 : t;
    const int lane = WAVE ? (int)(t & 63) : 0;
    if (node >= A.nfields * A.nout) return;         // WAVE: whole wavefronts leave together
    const long long f = node / A.nout, o = node - f * A.nout;
    const T* __restrict__ p = data + f * A.field_stride + hjq::proj_base<T>(A, o);
    const T start = A.op == HJQ_MIN ? T(__builtin_inf()) : -T(__builtin_inf());
    Red<T> acc{start, 0};
    static_assert(MAXD == 6, "five loops: at most MAXD - 1 removed axes");
    for (int i0 = 0; i0 < A.rem_n[1]; ++i0)
        for (int i1 = 0; i1 < A.rem_n[2]; ++i1) {
            const T* __restrict__ p2 = p + i0 * A.rem_s[1] + i1 * A.rem_s[2];
            for (int i2 = 0; i2 < A.rem_n[3]; ++i2)
                for (int i3 = 0; i3 < A.rem_n[4]; ++i3) {
                    const T* __restrict__ row = p2 + i2 * A.rem_s[3] + i3 * A.rem_s[4];
                    for (int i4 = lane; i4 < A.rem_n[5]; i4 += WAVE ? 64 : 1) acc.take(row[i4 * A.rem_s[5]], A.op);
                }
        }
    if (WAVE) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const T ov = __shfl_xor(acc.v, s, 64);
            const int on = __shfl_xor(acc.nan, s, 64);
            acc.nan |= on;
            acc.take(ov, A.op);
        }
        if (lane != 0) return;
    }
    out[node] = acc.nan ? T(__builtin_nan("")) : acc.v;
}

}  // namespace hjx

// ---- (d) the plants of hjx_rollout: controls(costate p, state x) -> (c0, c1), f(x; c0, c1) -> xdot, as dynamics.py's
// get_opt_u / get_opt_v / dynamics.  One operation per statement.
namespace hjr {

template <> struct Plant<HJH_HAM_PLANE5D> {
    static constexpr int ND = 5;
    // c0 = a, the acceleration; c1 = al, the angular acceleration: both are the control
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& a, double& al) {
#pragma clang fp contract(off)
        a = P.params[0] * sgn(p[3]);
        al = P.params[1] * sgn(p[4]);
        if (P.u_mode == HJR_MODE_MIN) { a = -a; al = -al; }
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double a, double al, double* k) {
#pragma clang fp contract(off)
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        k[0] = x[3] * c;
        k[1] = x[3] * s;
        k[2] = x[4];
        k[3] = a;
        k[4] = al;
    }
};

template <> struct Plant<HJH_HAM_DUBINS_PAIR6D> {
    static constexpr int ND = 6;
    // c0 = u, the evader's turn rate (the control); c1 = d, the pursuer's (the disturbance)
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& u, double& d) {
#pragma clang fp contract(off)
        u = P.params[2] * sgn(p[2]);
        if (P.u_mode == HJR_MODE_MIN) u = -u;
        d = P.params[3] * sgn(p[5]);
        if (P.d_mode == HJR_MODE_MIN) d = -d;
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double u, double d, double* k) {
#pragma clang fp contract(off)
        const double ve = P.params[0], vp = P.params[1];
        const double c2 = cos(x[2]);
        const double s2 = sin(x[2]);
        const double c5 = cos(x[5]);
        const double s5 = sin(x[5]);
        k[0] = ve * c2;
        k[1] = ve * s2;
        k[2] = u;
        k[3] = vp * c5;
        k[4] = vp * s5;
        k[5] = d;
    }
};

}  // namespace hjr

namespace hjx {

// A finished trajectory idles in its wavefront (rollout_body never returns early), so every __shfl of group_sum runs with all
// lanes of its group active.
template <typename T, int SCHEME, int PLANT>
__global__ __launch_bounds__(256) void hi_rollout_kernel(const T* __restrict__ data, long long field_stride, int ntimes,
                                                         const double* __restrict__ x0, long long M, QGrid G0, QStencil<T> S,
                                                         int sub_samples, double dt_small, hjr_plant P, RolloutOut O) {
    const QGrid G = at<Plant<PLANT>::ND>(G0);
    hjr::rollout_body<T, SCHEME, Plant<PLANT>, UpwindHidim>(data, field_stride, ntimes, x0, M, G, S, sub_samples, dt_small, P, O);
}

// ---------------------------------------------------------------------------------------------- host side
template <typename T>
static void fill_stencil(const hjh_grid* g, const QGrid& G, QStencil<T>& S) {
    for (int d = 0; d < MAXD; ++d) {
        S.km[d] = (d < G.ndim && g->toward_zero[d]) ? T(-1) : T(1);
        hj::fill_stencil_constants<T>(G.dx[d], S.K[d]);
    }
}

template <typename T>
static int interp_launch(const QGrid& G, const void* data, int64_t nfields, int64_t field_stride, const double* xs, int64_t M,
                         void* out, int out_f64, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M, TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_interp_points_kernel<T>), dim3(blocks), dim3(256), 0, stream, (const T*)data, (long long)field_stride,
                       (long long)nfields, xs, (long long)M, G, out, out_f64);
    return launch_done(name);
}

template <typename T, int ND, int SCHEME>
static int costate_launch(const hjh_grid* g, const QGrid& G, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                          int64_t M, const CostateOut& O, hipStream_t stream, const char* name) {
    QStencil<T> S;
    fill_stencil<T>(g, G, S);
    unsigned blocks;
    int rc = blocks_for((long long)nfields * M * (1ll << ND), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_costate_points_kernel<T, ND, SCHEME>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (long long)nfields, xs, (long long)M, G, S, O);
    return launch_done(name);
}

template <typename T, bool WAVE>
static int project_launch(const void* data, void* out, const ProjArgs& A, hipStream_t stream, const char* name) {
    unsigned blocks;
    int rc = blocks_for(A.nfields * A.nout * (WAVE ? 64 : 1), TOO_MANY, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_project_minmax_kernel<T, WAVE>), dim3(blocks), dim3(256), 0, stream, (const T*)data, (T*)out, A);
    return launch_done(name);
}

template <typename T, int SCHEME, int PLANT>
static int rollout_launch(const hjh_grid* g, const QGrid& G, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                          int64_t M, int sub_samples, double dt_small, const hjr_plant& P, const RolloutOut& O, hipStream_t stream,
                          const char* name) {
    QStencil<T> S;
    fill_stencil<T>(g, G, S);
    unsigned blocks;
    int rc = blocks_for((long long)M * (1ll << G.ndim), "too many trajectories for one launch", blocks);
    if (rc) return rc;
    hipLaunchKernelGGL((hi_rollout_kernel<T, SCHEME, PLANT>), dim3(blocks), dim3(256), 0, stream, (const T*)data,
                       (long long)field_stride, (int)ntimes, x0, (long long)M, G, S, sub_samples, dt_small, P, O);
    return launch_done(name);
}

// state dimension of a plant of this library, 0 for any other id
static int plant_ndim(int id) { return id == HJH_HAM_PLANE5D ? 5 : (id == HJH_HAM_DUBINS_PAIR6D ? 6 : 0); }

}  // namespace hjx

using namespace hjx;

extern "C" {

int hjx_interp_points(const hjh_grid* g, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                      int64_t nstates, void* out, int out_f64, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!out) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_points(g, G, total, data, nfields, field_stride, xs, nstates, false))) return rc;
    if (g->dtype == HJ_F64)
        return interp_launch<double>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "hi_interp_points_kernel<double>");
    return interp_launch<float>(G, data, nfields, field_stride, xs, nstates, out, out_f64, (hipStream_t)stream, "hi_interp_points_kernel<float>");
}

int hjx_costate_points(const hjh_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                       int64_t nstates, void* costate, void* derivL, void* derivR, void* value, int out_f64, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!costate) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_point_scheme(scheme, "point"))) return rc;
    if ((rc = check_points(g, G, total, data, nfields, field_stride, xs, nstates, true))) return rc;
    const CostateOut O{costate, derivL, derivR, value, out_f64};
    hipStream_t s = (hipStream_t)stream;
#define HJX_COSTATE(T, ND, SCH) \
    return costate_launch<T, ND, SCH>(g, G, data, nfields, field_stride, xs, nstates, O, s, "hi_costate_points_kernel<" #T ", " #ND ", " #SCH ">")
#define HJX_DIMS(T, SCH)                          \
    do {                                          \
        if (G.ndim == 5) HJX_COSTATE(T, 5, SCH);  \
        HJX_COSTATE(T, 6, SCH);                   \
    } while (0)
    if (g->dtype == HJ_F64) {
        if (scheme == HJ_ENO2) HJX_DIMS(double, 0);
        if (scheme == HJ_ENO3) HJX_DIMS(double, 1);
        HJX_DIMS(double, 3);
    }
    if (scheme == HJ_ENO2) HJX_DIMS(float, 0);
    if (scheme == HJ_ENO3) HJX_DIMS(float, 1);
    HJX_DIMS(float, 3);
#undef HJX_DIMS
#undef HJX_COSTATE
}

int hjx_project_minmax(const hjh_grid* g, const void* data, int64_t nfields, int64_t field_stride, unsigned remove_mask, int op,
                       void* out, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!data || !out) return fail(HJ_EINVAL, "null argument");
    if (nfields < 1) return fail(HJ_EINVAL, "nfields must be positive");
    if (nfields > 1 && field_stride < total) return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, total);
    if (op != HJQ_MIN && op != HJQ_MAX) return fail(HJ_EINVAL, "unknown projection %d", op);
    const unsigned all = (1u << G.ndim) - 1u;
    if ((remove_mask & ~all) || remove_mask == 0 || remove_mask == all)
        return fail(HJ_EINVAL, "remove_mask %#x must name a non-empty proper subset of the %d axes", remove_mask, G.ndim);
    ProjArgs A;
    A.nkeep = A.nrem = 0;
    A.nout = 1;
    for (int d = 0; d < MAXD; ++d) { A.keep_n[d] = A.rem_n[d] = 1; A.keep_s[d] = A.rem_s[d] = 0; }
    for (int d = 0; d < G.ndim; ++d) {
        if (remove_mask >> d & 1u) {
            ++A.nrem;
        } else {
            A.keep_n[A.nkeep] = G.n[d]; A.keep_s[A.nkeep] = G.stride[d]; ++A.nkeep; A.nout *= G.n[d];
        }
    }
    for (int d = G.ndim - 1, k = MAXD - 1; d >= 0; --d)          // removed axes right-aligned: the last one is the innermost loop
        if (remove_mask >> d & 1u) { A.rem_n[k] = G.n[d]; A.rem_s[k] = G.stride[d]; --k; }
    A.field_stride = field_stride;
    A.nfields = nfields;
    A.op = op;
    const bool wave = remove_mask >> (G.ndim - 1) & 1u;
    hipStream_t s = (hipStream_t)stream;
    if (g->dtype == HJ_F64)
        return wave ? project_launch<double, true>(data, out, A, s, "hi_project_minmax_kernel<double, true>")
                    : project_launch<double, false>(data, out, A, s, "hi_project_minmax_kernel<double, false>");
    return wave ? project_launch<float, true>(data, out, A, s, "hi_project_minmax_kernel<float, true>")
                : project_launch<float, false>(data, out, A, s, "hi_project_minmax_kernel<float, false>");
}

int hjx_rollout(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int sub_samples, double dt_small, const hjr_plant* plant, double* traj, int32_t* length,
                int32_t* t_earliest, int32_t* status, void* stream) {
    QGrid G;
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!plant) return fail(HJ_EINVAL, "null plant descriptor");
    if (nstates < 0) return fail(HJ_EINVAL, "nstates must not be negative");
    if (ntimes < 2 || ntimes > 0x7fffffffll) return fail(HJ_EINVAL, "ntimes %lld: a rollout needs at least two stored sets", (long long)ntimes);
    if (sub_samples < 1) return fail(HJ_EINVAL, "sub_samples must be positive");
    if (!std::isfinite(dt_small)) return fail(HJ_EINVAL, "dt_small must be finite");
    if (field_stride < total) return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, total);
    if ((rc = check_point_scheme(scheme, "rollout"))) return rc;
    const int nd = plant_ndim(plant->id);
    if (nd == 0) return fail(HJ_EUNSUPPORTED, "plant %d has no rollout kernel on 5-D / 6-D grids", (int)plant->id);
    if (nd != G.ndim) return fail(HJ_EINVAL, "plant %d has %d states, the grid %d dimensions", (int)plant->id, nd, G.ndim);
    if ((plant->u_mode != HJR_MODE_MIN && plant->u_mode != HJR_MODE_MAX) || (plant->d_mode != HJR_MODE_MIN && plant->d_mode != HJR_MODE_MAX))
        return fail(HJ_EINVAL, "u_mode / d_mode must be HJR_MODE_MIN or HJR_MODE_MAX");
    for (int d = 0; d < G.ndim; ++d)
        if (G.n[d] < HJ_STENCIL) return fail(HJ_EINVAL, "grid too small along dim %d (N=%d, need %d)", d, G.n[d], HJ_STENCIL);
    if (nstates == 0) return HJ_OK;
    if (!data || !x0 || !traj || !length || !status) return fail(HJ_EINVAL, "null argument");
    const RolloutOut O{traj, length, t_earliest, status};
    hipStream_t s = (hipStream_t)stream;
#define HJX_GO(T, SCH, PL) \
    return rollout_launch<T, SCH, PL>(g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, O, s, "hi_rollout_kernel<" #T ", " #SCH ", " #PL ">")
#define HJX_PLANTS(T, SCH)                                     \
    do {                                                       \
        if (plant->id == HJH_HAM_PLANE5D) HJX_GO(T, SCH, 50);  \
        HJX_GO(T, SCH, 51);                                    \
    } while (0)
    static_assert(HJH_HAM_PLANE5D == 50 && HJH_HAM_DUBINS_PAIR6D == 51, "plant ids name the kernels");
    if (g->dtype == HJ_F64) {
        if (scheme == HJ_ENO2) HJX_PLANTS(double, 0);
        if (scheme == HJ_ENO3) HJX_PLANTS(double, 1);
        HJX_PLANTS(double, 3);
    }
    if (scheme == HJ_ENO2) HJX_PLANTS(float, 0);
    if (scheme == HJ_ENO3) HJX_PLANTS(float, 1);
    HJX_PLANTS(float, 3);
#undef HJX_PLANTS
#undef HJX_GO
}

HJ_TOOL_LAST_SYMBOLS(hjx)

}  // extern "C"
