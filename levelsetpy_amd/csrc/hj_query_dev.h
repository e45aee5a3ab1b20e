// Device code shared by the point kernels of libhj_query.so (hj_query.hip), libhj_rollout.so (hj_rollout.hip) and
// libhj_decomp.so (hj_decomp.hip), at six axes by those of libhj_hiquery.so (hj_hiquery.hip), and at either width by the kernels
// libhj_plant.so has hipRTC compile (hj_plant.hip): the grid as a kernel sees it, the cell search, the corner weights, the stencil
// gather, a corner's one-sided derivatives, the ordered sum over a state's corner lanes, and the bodies of the costate and
// projection kernels (costate_body, project_body).  One source, so a value or a costate interpolated inside a rollout has the bits
// interp_points_kernel and costate_points_kernel give for the same state, and a 5-D / 6-D costate is a 2-D .. 4-D one's statements.
// At the end, the host side the four libraries share: the descriptor's checks (make_grid), the stencil constants (fill_stencil)
// and the entry points' checks (interp_points, costate_points, project_minmax).
#ifndef HJ_QUERY_DEV_H
#define HJ_QUERY_DEV_H
#ifndef __HIPCC_RTC__      // hipRTC (libhj_plant.so's run-time kernels, hj_plant.hip) brings the HIP device declarations itself
#include <hip/hip_runtime.h>
#include <cmath>
#endif
#include "hj_device.h"
#include "../../include/hj_query.h"

namespace hjq {

// The axes the structs below have room for, and the dimensions make_grid accepts.  hj_hiquery.hip defines both before it includes
// this header (6, and 5..6); every other library compiles the defaults.
#ifndef HJ_QUERY_MAXD
#define HJ_QUERY_MAXD HJ_MAX_DIM
#endif
#ifndef HJ_QUERY_MIND
#define HJ_QUERY_MIND 1
#endif
constexpr int MAXD = HJ_QUERY_MAXD;
constexpr int MIND = HJ_QUERY_MIND;

// grid as the kernels see it (kernel argument: lives in SGPRs), with room for MD axes.  A translation unit's device code has one
// width, MAXD; hj_plant.hip's host code fills both.
template <int MD> struct QGridT {
    int ndim;
    int n[MD];
    int per[MD];
    long long stride[MD];
    double xmin[MD], xlast[MD], dx[MD];
};
using QGrid = QGridT<MAXD>;

template <typename T, int MD> struct QStencilT {
    T km[MD];
    T K[MD][hj::HJ_NK];
};
template <typename T> using QStencil = QStencilT<T, MAXD>;

// the grid with a compile-time number of axes: every loop over axes of the functions below unrolls, lo / w stay in registers
template <int ND> __device__ __forceinline__ QGrid at(const QGrid& G) {
    QGrid g = G;
    g.ndim = ND;
    return g;
}

// cell index and weight of every axis; false when the state is outside an extrapolated axis (or not finite)
__device__ __forceinline__ bool locate(const QGrid& G, const double* __restrict__ x, int* lo, double* w) {
#pragma clang fp contract(off)
    bool inside = true;
    for (int d = 0; d < G.ndim; ++d) {
        double xd = x[d];
        const double vs0 = G.xmin[d], dx = G.dx[d];
        const int n = G.n[d];
        int i;
        if (!(xd - xd == 0.0)) {          // NaN / inf state
            inside = false;
            xd = vs0;
        }
        if (G.per[d]) {
            const double period = (double)n * dx;
            double mod = fmod(xd - vs0, period);          // Python's %: the sign of the divisor
            if (mod != 0.0) {
                if (mod < 0.0) mod += period;
            } else {
                mod = 0.0;
            }
            xd = vs0 + mod;
            i = (int)floor((xd - vs0) / dx);
            if (i > n - 1) i = n - 1;
        } else {
            if (xd < vs0 || xd > G.xlast[d]) {
                inside = false;
                xd = vs0;
            }
            i = (int)floor((xd - vs0) / dx);
            if (i > n - 2) i = n - 2;
        }
        if (i < 0) i = 0;
        lo[d] = i;
        w[d] = (xd - (vs0 + (double)i * dx)) / dx;
    }
    return inside;
}

// element offset and weight of corner `c`
__device__ __forceinline__ double corner(const QGrid& G, const int* lo, const double* w, int c, long long& off) {
#pragma clang fp contract(off)
    double wt = 1.0;
    off = 0;
    for (int d = 0; d < G.ndim; ++d) {
        const int up = (c >> d) & 1;
        int j = lo[d] + up;
        if (G.per[d] && j >= G.n[d]) j -= G.n[d];
        off += (long long)j * G.stride[d];
        wt *= up ? w[d] : (1.0 - w[d]);
    }
    return wt;
}

// V(x) of one field, the interpolant of include/hj_query.h in fp64: corners in ascending number, those of weight exactly 0
// skipped, a multiply and an add per corner; NaN outside an extrapolated axis.  interp_points_kernel and the kernels of
// libhj_decomp.so call this one function.
template <typename T>
__device__ __forceinline__ double interp_value(const QGrid& G, const T* __restrict__ field, const double* __restrict__ x) {
#pragma clang fp contract(off)
    int lo[MAXD];
    double w[MAXD];
    if (!locate(G, x, lo, w)) return __builtin_nan("");
    double v = 0.0;
    for (int c = 0; c < (1 << G.ndim); ++c) {
        long long off;
        const double wt = corner(G, lo, w, c, off);
        if (wt != 0.0) {
            const double val = (double)field[off];
            const double p = wt * val;
            v = v + p;
        }
    }
    return v;
}

template <typename T> __device__ __forceinline__ bool finite(T v) { return v - v == T(0); }
// computeGradients' replacement of NaN / +-inf by a large number before the differences
template <typename T> __device__ __forceinline__ T ld_work(const T* p) {
    const T v = *p;
    return finite(v) ? v : T(1e6);
}

// the seven values phi[i-3 .. i+3] along one axis of the node at `pc0` (index i on that axis), ghosts as the solver's
// gather_stencils (hj_split.h): wrap on a periodic axis, ghost_value from the edge node and its inner neighbour otherwise
template <typename T>
__device__ __forceinline__ void gather_axis(const T* pc0, long long s, int i, int n, bool per, T km, T centre, T* v) {
    bool ghost = false;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (k == 3) { v[k] = centre; continue; }
        int j = i + k - 3;
        if (j < 0) {
            if (per) j += n; else { j = 0; ghost = true; }
        } else if (j >= n) {
            if (per) j -= n; else { j = n - 1; ghost = true; }
        }
        v[k] = ld_work(pc0 + (long long)(j - i) * s);
    }
    if (ghost) {
        const T* line = pc0 - (long long)i * s;
        if (i < HJ_STENCIL) {
            const T e = ld_work(line), in = ld_work(line + s);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (i + k - 3 < 0) v[k] = hj::ghost_value(e, in, T(3 - k - i) * km);
        }
        if (i + HJ_STENCIL >= n) {
            const T e = ld_work(line + (long long)(n - 1) * s), in = ld_work(line + (long long)(n - 2) * s);
#pragma unroll
            for (int k = 4; k < 7; ++k)
                if (i + k - 3 >= n) v[k] = hj::ghost_value(e, in, T(i + k - 3 - n + 1) * km);
        }
    }
}

// the group's first lane adds the corners' terms in ascending corner number (the order of interp_points_kernel)
__device__ __forceinline__ double group_sum(double term, int used, int lanes) {
#pragma clang fp contract(off)
    double v = 0.0;
    for (int c = 0; c < lanes; ++c) {
        const double p = __shfl(term, c, lanes);
        const int u = __shfl(used, c, lanes);
        if (u) v = v + p;
    }
    return v;
}

// The one-sided derivatives of a corner's stencil.  UpwindSolver: hj_device.h's upwind<>, what computeGradients runs up to 4-D.
struct UpwindSolver {
    template <int SCHEME, typename T>
    __device__ static __forceinline__ void lr(const T* v, const T* K, T& L, T& R) { hj::upwind<SCHEME, T>(v, K, T(0), L, R); }
};
// UpwindHidim: computeGradients' at 5-D / 6-D (hidim_upwind_kernel), so that a corner costate has the bits it gives that node --
// ENO2 / ENO3 with every operation rounded on its own, the as-shipped WENO5 by upwind<>.
struct UpwindHidim {
    template <int SCHEME, typename T>
    __device__ static __forceinline__ void lr(const T* v, const T* K, T& L, T& R) { hj::upwind_lr_hidim<SCHEME, T>(v, K, L, R); }
};

// NDC, of corner_derivs and costate_body: the number of axes where the kernel knows it at compile time, 0 where it is G.ndim at
// run time (up to MAXD).  It sizes the per-axis arrays only.  With NDC the loops over axes still run to nd = G.ndim, which the
// kernel has set to NDC (at<NDC>): they unroll once the body is inlined there.  With a constant bound they would unroll before
// that, and the compiler would then fetch every constant of the stencil argument at the kernel's start (SGPRs: 86 -> 106 at six
// axes, VGPRs 55 -> 72).  The kernels' `__restrict__` is not repeated on the bodies: the kernels' own arguments carry it already.
template <int NDC> __device__ __forceinline__ int axes_bound(int nd) { return NDC ? nd : MAXD; }

// The node at `pc0`, corner `c` of the cell `lo`: its value, and along every axis its left and right derivative and their mean,
// through the solver's own ghost_value and upwind rule (UP) -- so a corner costate has the bits computeGradients gives that node.
// nd: the number of axes (G.ndim).  The caller zeroes cC / cL / cR.
template <typename T, int SCHEME, int NDC, typename UP>
__device__ __forceinline__ T corner_derivs(const QGrid& G, int nd, const QStencil<T>& S, const T* pc0, const int* lo, int c, T* cC, T* cL,
                                           T* cR) {
    const T raw = *pc0;
    if (!finite(raw)) {
        // the node's own NaN / inf is put back after the differences (computeGradients: NaN stays NaN, +-inf becomes +inf)
        const T back = raw != raw ? raw : T(__builtin_inf());
#pragma unroll
        for (int d = 0; d < (NDC ? NDC : MAXD); ++d) cC[d] = cL[d] = cR[d] = back;
    } else {
#pragma unroll
        for (int d = 0; d < axes_bound<NDC>(nd); ++d) {
            if (d >= nd) break;
            int j = lo[d] + ((c >> d) & 1);
            if (G.per[d] && j >= G.n[d]) j -= G.n[d];
            T v[7];
            gather_axis<T>(pc0, G.stride[d], j, G.n[d], G.per[d] != 0, S.km[d], raw, v);
            T L, R;
            UP::template lr<SCHEME, T>(v, S.K[d], L, R);
            cL[d] = L;
            cR[d] = R;
            cC[d] = T(0.5) * (L + R);
        }
    }
    return raw;
}

template <typename T>
__device__ __forceinline__ void put(void* out, long long i, double v, int out_f64) {
    if (out_f64) ((double*)out)[i] = v;
    else ((T*)out)[i] = (T)v;
}

// ---- grad V at states: the body of costate_points_kernel (hj_query.hip; NDC = 0: 2^ndim = 2 .. 16 lanes per state) and of
// hi_costate_points_kernel (hj_hiquery.hip; NDC = 5 or 6: 32 lanes, or the whole wavefront).  Lane c of a (field, state) group owns
// corner c of the state's cell.
struct CostateOut {
    void* costate;
    void* derivL;
    void* derivR;
    void* value;
    int out_f64;
};

template <typename T, int SCHEME, int NDC, typename UP>
__device__ __forceinline__ void costate_body(const T* data, long long field_stride, long long nfields, const double* xs, long long M,
                                             const QGrid& G, const QStencil<T>& S, const CostateOut& O) {
    constexpr int NA = NDC ? NDC : MAXD;
    const int nd = G.ndim;
    const int lanes = 1 << (NDC ? NDC : nd);       // divides the wavefront, groups never straddle one
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long grp = t / lanes;
    const int c = (int)(t - grp * lanes);
    if (grp >= nfields * M) return;                // whole groups leave together
    const long long f = grp / M, m = grp - f * M;
    int lo[MAXD];
    double w[MAXD];
    const bool inside = locate(G, xs + m * nd, lo, w);
    long long off;
    const double wt = corner(G, lo, w, c, off);
    const int used = wt != 0.0;
    T cC[NA], cL[NA], cR[NA];
    T raw = T(0);
#pragma unroll
    for (int d = 0; d < NA; ++d) cC[d] = cL[d] = cR[d] = T(0);
    if (inside && used) raw = corner_derivs<T, SCHEME, NDC, UP>(G, nd, S, data + f * field_stride + off, lo, c, cC, cL, cR);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int d = 0; d < axes_bound<NDC>(nd); ++d) {
        if (d >= nd) break;
        double p, q, r;
        {
#pragma clang fp contract(off)
            p = wt * (double)cC[d];
            q = wt * (double)cL[d];
            r = wt * (double)cR[d];
        }
        const double sC = group_sum(p, used, lanes);
        if (c == 0) put<T>(O.costate, grp * nd + d, inside ? sC : nan, O.out_f64);
        if (O.derivL) {
            const double sL = group_sum(q, used, lanes);
            if (c == 0) put<T>(O.derivL, grp * nd + d, inside ? sL : nan, O.out_f64);
        }
        if (O.derivR) {
            const double sR = group_sum(r, used, lanes);
            if (c == 0) put<T>(O.derivR, grp * nd + d, inside ? sR : nan, O.out_f64);
        }
    }
    if (O.value) {
        double p;
        {
#pragma clang fp contract(off)
            p = wt * (double)raw;
        }
        const double sV = group_sum(p, used, lanes);
        if (c == 0) put<T>(O.value, grp, inside ? sV : nan, O.out_f64);
    }
}

// ---- min / max over a subset of axes: the arguments, the reduction, the decode and the body of project_minmax_kernel
// (hj_query.hip) and hi_project_minmax_kernel (hj_hiquery.hip)
struct ProjArgs {
    int nkeep, nrem;
    int keep_n[MAXD], rem_n[MAXD];                  // sizes, in axis order (removed axes right-aligned, see the kernel)
    long long keep_s[MAXD], rem_s[MAXD];            // strides in the input
    long long nout;                                 // product of keep_n
    long long field_stride, nfields;
    int op;
};

// running min / max that remembers a NaN (np.amin / np.amax: any NaN in the set gives NaN)
template <typename T> struct Red {
    T v;
    int nan;
    __device__ __forceinline__ void take(T x, int op) {
        if (x != x) nan = 1;
        else if (op == HJQ_MIN ? x < v : x > v) v = x;
    }
};

template <typename T>
__device__ __forceinline__ long long proj_base(const ProjArgs& A, long long o) {
    long long base = 0;
    for (int k = A.nkeep - 1; k >= 0; --k) {
        const long long q = o / A.keep_n[k];
        base += (o - q * A.keep_n[k]) * A.keep_s[k];
        o = q;
    }
    return base;
}

// the loops over the removed axes K .. MAXD - 1 (at most MAXD - 1 axes are removed: slot 0 is never one).  The last is the
// innermost: with WAVE the lanes stride it.
template <typename T, bool WAVE, int K = 1>
__device__ __forceinline__ void proj_loops(const ProjArgs& A, const T* __restrict__ p, int lane, Red<T>& acc) {
    if constexpr (K == MAXD - 1) {
        for (int i = lane; i < A.rem_n[K]; i += WAVE ? 64 : 1) acc.take(p[i * A.rem_s[K]], A.op);
    } else {
        for (int i = 0; i < A.rem_n[K]; ++i) proj_loops<T, WAVE, K + 1>(A, p + i * A.rem_s[K], lane, acc);
    }
}

// WAVE = false: the last axis is kept -- one thread per output node, neighbouring threads read neighbouring elements.
// WAVE = true:  the last axis is removed -- one wavefront per output node; its lanes stride the last axis (neighbouring
//               lanes read neighbouring elements) inside loops over the other removed axes.
// The removed axes sit at the END of rem_n / rem_s (unused leading slots have n = 1), so the loops need no index division: the
// only divisions are proj_base's, once per output node.
template <typename T, bool WAVE>
__device__ __forceinline__ void project_body(const T* __restrict__ data, T* __restrict__ out, const ProjArgs& A) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long node = WAVE ? t / 64 : t;
    const int lane = WAVE ? (int)(t & 63) : 0;
    if (node >= A.nfields * A.nout) return;         // WAVE: whole wavefronts leave together
    const long long f = node / A.nout, o = node - f * A.nout;
    const T* __restrict__ p = data + f * A.field_stride + proj_base<T>(A, o);
    const T start = A.op == HJQ_MIN ? T(__builtin_inf()) : -T(__builtin_inf());
    Red<T> acc{start, 0};
    proj_loops<T, WAVE>(A, p, lane, acc);
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

// ---------------------------------------------------------------------------------------------- host side
// The descriptor as the kernels see it, with the checks every library makes on it; total = the number of nodes.  Refusals go to
// the including library's own error record: hj_tool_host.h comes before this header.  A translation unit generated for hipRTC
// (HJ_RTC) is device code only and has no host side.
#ifndef HJ_RTC
#ifndef HJ_TOOL_HOST_H
#error "include hj_tool_host.h before hj_query_dev.h"
#endif
using hj_tool::fail;

// GD: hjq_grid, or hjh_grid (include/hj_hidim.h) where MD is 6 -- the same fields with room for six axes.  mind: the fewest axes
// the caller takes.  A grid of more than 2^40 nodes is refused before the product is formed: N[d] <= 2^30 alone lets it overflow.
template <int MD, typename GD>
static int make_grid(const GD* g, QGridT<MD>& G, long long& total, int mind = MIND) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->ndim < mind || g->ndim > MD) return fail(HJ_EINVAL, "ndim %d outside %d..%d", (int)g->ndim, mind, MD);
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", (int)g->dtype);
    G.ndim = g->ndim;
    total = 1;
    for (int d = 0; d < MD; ++d) {
        G.n[d] = 1; G.per[d] = 0; G.stride[d] = 0; G.xmin[d] = 0; G.xlast[d] = 0; G.dx[d] = 1;
    }
    for (int d = g->ndim - 1; d >= 0; --d) {
        if (g->N[d] < 1 || g->N[d] > (1ll << 30)) return fail(HJ_EINVAL, "N[%d] = %lld out of range", d, (long long)g->N[d]);
        if (g->bc[d] != HJ_BC_EXTRAPOLATE && g->bc[d] != HJ_BC_PERIODIC) return fail(HJ_EINVAL, "unknown boundary kind %d on axis %d", (int)g->bc[d], d);
        if (!(g->dx[d] > 0.0) || !std::isfinite(g->dx[d]) || !std::isfinite(g->xmin[d]) || !std::isfinite(g->xlast[d]))
            return fail(HJ_EINVAL, "axis %d: dx must be positive, xmin / xlast finite", d);
        if (total > (1ll << 40) / g->N[d]) return fail(HJ_EINVAL, "grid too large");
        G.n[d] = (int)g->N[d];
        G.per[d] = g->bc[d] == HJ_BC_PERIODIC;
        G.stride[d] = total;
        G.xmin[d] = g->xmin[d];
        G.xlast[d] = g->xlast[d];
        G.dx[d] = g->dx[d];
        total *= g->N[d];
    }
    return HJ_OK;
}

// the constants of the corner stencils: the ghost slope's sign per axis, hj_device.h's K per spacing
template <typename T, int MD, typename GD>
static void fill_stencil(const GD* g, const QGridT<MD>& G, QStencilT<T, MD>& S) {
    for (int d = 0; d < MD; ++d) {
        S.km[d] = (d < G.ndim && g->toward_zero[d]) ? T(-1) : T(1);
        hj::fill_stencil_constants<T>(G.dx[d], S.K[d]);
    }
}

// the checks of the point entry points on their arrays
static int check_points(const QGrid& G, long long total, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                        int64_t nstates, bool costate) {
    if (!data || !xs) return fail(HJ_EINVAL, "null argument");
    if (nfields < 1 || nstates < 1) return fail(HJ_EINVAL, "nfields and nstates must be positive");
    if (nfields > 1 && field_stride < total) return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, total);
    for (int d = 0; d < G.ndim; ++d) {
        // an extrapolated axis interpolates between nodes i and i+1 <= N-1; the stencils reach HJ_STENCIL nodes (hj_upwind's limit)
        const int need = costate ? HJ_STENCIL : (G.per[d] ? 1 : 2);
        if (G.n[d] < need) return fail(HJ_EINVAL, "grid too small along dim %d (N=%d, need %d)", d, G.n[d], need);
    }
    return HJ_OK;
}

static const char TOO_MANY[] = "too many (field, state) pairs for one launch";

// ---- the entry points of libhj_query.so (hjq_*) and libhj_hiquery.so (hjx_*) up to their launch: every check, in the order the
// refusals are documented in, and what the kernels take.  GD as make_grid's.
template <typename GD>
static int interp_points(const GD* g, const void* data, int64_t nfields, int64_t field_stride, const double* xs, int64_t nstates,
                         const void* out, QGrid& G) {
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!out) return fail(HJ_EINVAL, "null argument");
    return check_points(G, total, data, nfields, field_stride, xs, nstates, false);
}

template <typename GD>
static int costate_points(const GD* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, const double* xs,
                          int64_t nstates, const void* costate, QGrid& G) {
    long long total;
    int rc = make_grid(g, G, total);
    if (rc) return rc;
    if (!costate) return fail(HJ_EINVAL, "null argument");
    if ((rc = hj_tool::check_point_scheme(scheme, "point"))) return rc;
    return check_points(G, total, data, nfields, field_stride, xs, nstates, true);
}

// wave: whether the last axis is removed (the kernels' WAVE)
template <typename GD>
static int project_minmax(const GD* g, const void* data, int64_t nfields, int64_t field_stride, unsigned remove_mask, int op,
                          const void* out, ProjArgs& A, bool& wave) {
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
    wave = remove_mask >> (G.ndim - 1) & 1u;
    return HJ_OK;
}
#endif  // HJ_RTC

}  // namespace hjq
#endif
