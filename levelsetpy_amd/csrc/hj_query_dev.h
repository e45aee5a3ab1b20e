// Device code shared by the point kernels of libhj_query.so (hj_query.hip), libhj_rollout.so (hj_rollout.hip) and
// libhj_decomp.so (hj_decomp.hip), and at six axes by those of libhj_hiquery.so (hj_hiquery.hip): the grid as a
// kernel sees it, the cell search, the corner weights, the stencil gather and the ordered sum over a state's corner lanes.
// One source, so a value or a costate interpolated inside a rollout has the bits interp_points_kernel and
// costate_points_kernel give for the same state.  At the end, the host function that fills the grid from the descriptor.
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

// grid as the kernels see it (kernel argument: lives in SGPRs)
struct QGrid {
    int ndim;
    int n[MAXD];
    int per[MAXD];
    long long stride[MAXD];
    double xmin[MAXD], xlast[MAXD], dx[MAXD];
};

template <typename T> struct QStencil {
    T km[MAXD];
    T K[MAXD][hj::HJ_NK];
};

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

// ---- min / max over a subset of axes: the arguments, the reduction and the decode of project_minmax_kernel (hj_query.hip) and
// hi_project_minmax_kernel (hj_hiquery.hip)
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

// ---------------------------------------------------------------------------------------------- host side
// The descriptor as the kernels see it, with the checks both libraries make on it; total = the number of nodes.  Refusals go to
// the including library's own error record: hj_tool_host.h comes before this header.  A translation unit generated for hipRTC
// (HJ_RTC) is device code only and has no host side.
#ifndef HJ_RTC
#ifndef HJ_TOOL_HOST_H
#error "include hj_tool_host.h before hj_query_dev.h"
#endif
using hj_tool::fail;

// GD: hjq_grid, or hjh_grid (include/hj_hidim.h) where MAXD is 6 -- the same fields with room for six axes.
template <typename GD>
static int make_grid(const GD* g, QGrid& G, long long& total) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->ndim < MIND || g->ndim > MAXD) return fail(HJ_EINVAL, "ndim %d outside %d..%d", (int)g->ndim, MIND, MAXD);
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", (int)g->dtype);
    G.ndim = g->ndim;
    total = 1;
    for (int d = 0; d < MAXD; ++d) {
        G.n[d] = 1; G.per[d] = 0; G.stride[d] = 0; G.xmin[d] = 0; G.xlast[d] = 0; G.dx[d] = 1;
    }
    for (int d = g->ndim - 1; d >= 0; --d) {
        if (g->N[d] < 1 || g->N[d] > (1ll << 30)) return fail(HJ_EINVAL, "N[%d] = %lld out of range", d, (long long)g->N[d]);
        if (g->bc[d] != HJ_BC_EXTRAPOLATE && g->bc[d] != HJ_BC_PERIODIC) return fail(HJ_EINVAL, "unknown boundary kind %d on axis %d", (int)g->bc[d], d);
        if (!(g->dx[d] > 0.0) || !std::isfinite(g->dx[d]) || !std::isfinite(g->xmin[d]) || !std::isfinite(g->xlast[d]))
            return fail(HJ_EINVAL, "axis %d: dx must be positive, xmin / xlast finite", d);
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

// the checks of the point entry points on their arrays
template <typename GD>
static int check_points(const GD* g, const QGrid& G, long long total, const void* data, int64_t nfields, int64_t field_stride,
                 const double* xs, int64_t nstates, bool costate) {
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
#endif  // HJ_RTC

}  // namespace hjq
#endif
