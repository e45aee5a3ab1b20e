// libhj_decomp.so (include/hj_decomp.h): decomposed value functions put back together, for gfx950.
//   backproject_nodes_kernel<T>   conforming grids: a pure index gather, op over the subsystems, one store per node
//   backproject_coords_kernel<T>  any target grid: every subsystem interpolated at the node's coordinates
//   decomp_points_kernel<T>       V and the active subsystem at states: a thread per (field, state)
// The two back-projections are one-pass streaming writers.  A workgroup owns BLOCK * items consecutive output elements,
// each of its waves items * 64 consecutive ones, 64 per step and one element per lane along the last axis: a
// wave-instruction stores 256 or 512 contiguous bytes whatever the alignment of the caller's view.  Indexing:
//   * a wave's first multi-index is decoded ONCE, by divisions of wave-uniform values (scalar registers);
//   * from there it moves by add-and-carry: `split` divides by an extent with the reciprocal the host prepared (one
//     multiply-high) or, for a long axis, by one compare -- never by a run-time division;
//   * when the last axis has 64 nodes or more a wave lies in at most two rows, and the nodes kernel keeps each subsystem's
//     offset over the leading axes for both rows in scalar registers (long_rows): a lane only selects one of them and adds
//     its own step along the last axis: stride 1 is a coalesced read, stride 0 one value for the whole wave;
//   * a shorter last axis puts more rows into a wave: each lane then carries its own row index (the same `split`).
// The kernels see every full grid as FD = 8 axes (leading axes of one node are added by the host), so every loop over axes
// unrolls and every index array stays in registers.  The descriptor rides in the kernel arguments (about 2 KB of the 4 KB
// there are): subsystems are indexed by a wave-uniform loop counter, so their fields arrive by scalar loads.
// Kernels are instantiated on the output type only; a subsystem's element type is a wave-uniform branch at its load.
// Interpolation is hj_query_dev.h's interp_value, the function interp_points_kernel calls: the same bits as eval_u.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "hj_tool_host.h"
#include "hj_query_dev.h"
#include "../../include/hj_decomp.h"

namespace hjd {

using hjq::MAXD;
using hjq::QGrid;
using hjq::make_grid;
using namespace hj_tool;

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int FD = HJD_MAX_DIM;                  // axes of a full grid as the kernels see it
constexpr unsigned LONG_AXIS = 32768;            // from here on `split` compares instead of multiplying
constexpr long long MAX_X = 1ll << 22;           // workgroups of one launch along x
constexpr long long MAX_Y = 65535;               // fields of one launch

struct KSub {
    QGrid G;                                     // the subsystem's grid
    const void* data;
    long long field_step;                        // elements from field f to f + 1; 0 when the subsystem holds one field
    unsigned fstride[FD];                        // elements per node along full axis a, 0 where the subsystem has no such axis
    int axis[MAXD];                              // full axis (of FD) of subsystem axis k
    int f64;                                     // element type of data
};

struct KArgs {
    KSub sub[HJD_MAX_SUBS];
    const double* coord[FD];                     // coords kernel: node coordinates per full axis (null on an added axis)
    unsigned n[FD];                              // nodes per full axis
    unsigned magic[FD];                          // floor(2^32 / n) + 1 for 1 < n < LONG_AXIS
    long long total;                             // nodes of the full grid
    long long block0;                            // first workgroup (along x) of this launch
    long long f0;                                // first field of this launch
    int nsubs, op, items, pad;                   // pad = FD - ndim: the first real axis
};
static_assert(sizeof(KArgs) <= 4096, "the descriptor must fit the kernel-argument segment");

// NaN on either side gives NaN, as np.minimum / np.maximum (and hj_shapes.hip)
__device__ __forceinline__ double fold(double a, double b, int op) {
    double r;
    if (a != a) r = a;
    else if (b != b) r = b;
    else if (op == HJQ_MAX) r = a > b ? a : b;
    else r = a < b ? a : b;
    return r;
}

// one more subsystem value into the running result; `act` follows the lowest subsystem that holds the result
__device__ __forceinline__ void take(double& acc, int& act, double val, int s, int op) {
    if (s == 0) {
        acc = val;
    } else {
        const double next = fold(acc, val, op);
        if (next != acc && next == next) act = s;          // the result moved, and only val can have moved it
        acc = next;
    }
}

// v / n and v % n for v < n + 257 without a division: n = 1 is trivial, a long axis is passed at most once, and otherwise
// floor(v * magic / 2^32) is exact because v * (magic * n - 2^32) <= v * n < 2^32
__device__ __forceinline__ unsigned split(unsigned v, unsigned n, unsigned magic, unsigned& rem) {
    unsigned q;
    if (n == 1u) {
        q = v;
        rem = 0u;
    } else if (n >= LONG_AXIS) {
        q = v >= n ? 1u : 0u;
        rem = q ? v - n : v;
    } else {
        q = __umulhi(v, magic);
        rem = v - q * n;
    }
    return q;
}

// r (the index over the leading axes) moves q <= 257 rows on: add with carry from the last leading axis up
__device__ __forceinline__ void add_rows(unsigned (&r)[FD - 1], unsigned q, const KArgs& A) {
#pragma unroll
    for (int d = FD - 2; d >= 0; --d)
        if (A.n[d] > 1u) q = split(r[d] + q, A.n[d], A.magic[d], r[d]);
}

// the multi-index of flat node `at`: the one place that divides, on wave-uniform values
__device__ __forceinline__ void decode(const KArgs& A, unsigned long long at, unsigned (&r)[FD - 1], unsigned& last) {
    unsigned idx[FD];
    if (A.total <= 0xffffffffll) {
        unsigned rem = (unsigned)at;
#pragma unroll
        for (int d = FD - 1; d >= 0; --d) {
            idx[d] = 0u;
            if (A.n[d] > 1u) {
                const unsigned q = rem / A.n[d];
                idx[d] = rem - q * A.n[d];
                rem = q;
            }
        }
    } else {
        unsigned long long rem = at;
#pragma unroll
        for (int d = FD - 1; d >= 0; --d) {
            idx[d] = 0u;
            if (A.n[d] > 1u) {
                const unsigned long long q = rem / A.n[d];
                idx[d] = (unsigned)(rem - q * A.n[d]);
                rem = q;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < FD - 1; ++d) r[d] = idx[d];
    last = idx[FD - 1];
}

// where a wave stands: 64 consecutive nodes from flat index w0, the first of them at leading index r and last-axis index l0
struct Cursor {
    long long w0;
    unsigned r[FD - 1];
    unsigned l0;
};

__device__ __forceinline__ void advance(const KArgs& A, Cursor& c) {                       // one wave on
    c.w0 += WAVE;
    const unsigned q = split(c.l0 + WAVE, A.n[FD - 1], A.magic[FD - 1], c.l0);
    add_rows(c.r, q, A);
}

// a wave owns items * 64 consecutive nodes of its workgroup's BLOCK * items
__device__ __forceinline__ Cursor first_chunk(const KArgs& A) {
    Cursor c;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const unsigned long long at = ((unsigned long long)(A.block0 + blockIdx.x) * (BLOCK / WAVE) + wave) * (unsigned long long)(WAVE * A.items);
    c.w0 = (long long)at;
    c.l0 = 0u;
#pragma unroll
    for (int d = 0; d < FD - 1; ++d) c.r[d] = 0u;
    if (c.w0 < A.total) decode(A, at, c.r, c.l0);
    return c;
}

// the lane's own index: (leading index, last-axis index) of node w0 + lane
__device__ __forceinline__ void lane_index(const KArgs& A, const Cursor& c, unsigned lane, unsigned (&ri)[FD - 1], unsigned& l) {
    const unsigned q = split(c.l0 + lane, A.n[FD - 1], A.magic[FD - 1], l);
#pragma unroll
    for (int d = 0; d < FD - 1; ++d) ri[d] = c.r[d];
    add_rows(ri, q, A);
}

__device__ __forceinline__ const void* field_of(const KSub& U, long long f) {
    const long long at = f * U.field_step;
    return U.f64 ? (const void*)((const double*)U.data + at) : (const void*)((const float*)U.data + at);
}

__device__ __forceinline__ double load_at(const KSub& U, const void* field, unsigned off) {
    return U.f64 ? ((const double*)field)[off] : (double)((const float*)field)[off];
}

template <typename T>
__device__ __forceinline__ void put(T* __restrict__ out, int* __restrict__ active, long long at, double acc, int act) {
    out[at] = (T)acc;
    if (active) active[at] = acc != acc ? -1 : act;
}

// ---- (a) conforming grids
// A last axis of 64 nodes or more: the wave lies in at most two rows, and everything a subsystem contributes to a node's
// offset but the lane's own step along the last axis is wave-uniform.  The offsets of the wave's row and of the next one
// (base0, base1) live in scalar registers for the wave's whole run; passing into the next row is base0 = base1 and
// base1 += the subsystem's stride along the last leading axis, and only a carry out of that axis recomputes them.
template <typename T>
__device__ __forceinline__ void long_rows(const KArgs& A, Cursor c, long long f, unsigned lane, T* __restrict__ out, int* __restrict__ active) {
    constexpr int S = HJD_MAX_SUBS;
    const unsigned L = A.n[FD - 1];
    unsigned base0[S], base1[S], row_step[S], lane_step[S];
    const void* field[S];
    unsigned r1[FD - 1];
#pragma unroll
    for (int d = 0; d < FD - 1; ++d) r1[d] = c.r[d];
    add_rows(r1, 1u, A);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        base0[s] = base1[s] = row_step[s] = lane_step[s] = 0u;
        field[s] = nullptr;
        if (s < A.nsubs) {
            const KSub& U = A.sub[s];
#pragma unroll
            for (int d = 0; d < FD - 1; ++d) {
                base0[s] += c.r[d] * U.fstride[d];
                base1[s] += r1[d] * U.fstride[d];
            }
            row_step[s] = U.fstride[FD - 2];
            lane_step[s] = U.fstride[FD - 1];
            field[s] = field_of(U, f);
        }
    }
    for (int j = 0; j < A.items && c.w0 < A.total; ++j) {
        const long long node = c.w0 + lane;
        const unsigned v = c.l0 + lane;
        const bool over = v >= L;
        const unsigned l = over ? v - L : v;
        if (node < A.total) {
            double acc = 0.0;
            int act = 0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (s < A.nsubs) {
                    const unsigned sl = lane_step[s];
                    const unsigned step = sl == 1u ? l : (sl == 0u ? 0u : l * sl);
                    take(acc, act, load_at(A.sub[s], field[s], (over ? base1[s] : base0[s]) + step), s, A.op);
                }
            }
            put<T>(out, active, f * A.total + node, acc, act);
        }
        c.w0 += WAVE;
        c.l0 += WAVE;
        if (c.l0 >= L) {                                       // into the next row: at most one, the axis is that long
            c.l0 -= L;
            const bool carry = r1[FD - 2] + 1u >= A.n[FD - 2];
            if (carry) add_rows(r1, 1u, A);
            else r1[FD - 2] += 1u;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (s < A.nsubs) {
                    base0[s] = base1[s];
                    if (carry) {
                        base1[s] = 0u;
#pragma unroll
                        for (int d = 0; d < FD - 1; ++d) base1[s] += r1[d] * A.sub[s].fstride[d];
                    } else {
                        base1[s] += row_step[s];
                    }
                }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void backproject_nodes_kernel(const KArgs A, T* __restrict__ out, int* __restrict__ active) {
    const unsigned lane = threadIdx.x % WAVE;
    const long long f = A.f0 + blockIdx.y;
    Cursor c = first_chunk(A);
    if (A.n[FD - 1] >= (unsigned)WAVE) {
        long_rows<T>(A, c, f, lane, out, active);
        return;
    }
    // a short last axis: several rows in the wave, every lane carries its own
    for (int j = 0; j < A.items && c.w0 < A.total; ++j) {
        const long long node = c.w0 + lane;
        if (node < A.total) {
            unsigned ri[FD - 1], l;
            lane_index(A, c, lane, ri, l);
            double acc = 0.0;
            int act = 0;
            for (int s = 0; s < A.nsubs; ++s) {
                const KSub& U = A.sub[s];
                unsigned off = l * U.fstride[FD - 1];
#pragma unroll
                for (int d = 0; d < FD - 1; ++d)
                    if (U.fstride[d]) off += ri[d] * U.fstride[d];
                take(acc, act, load_at(U, field_of(U, f), off), s, A.op);
            }
            put<T>(out, active, f * A.total + node, acc, act);
        }
        advance(A, c);
    }
}

// the subsystem's value at the state whose full coordinates are x[0 .. FD-1]
__device__ __forceinline__ double sub_value(const KSub& U, long long f, const double (&x)[FD]) {
    double xs[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        double xv = 0.0;
#pragma unroll
        for (int d = 0; d < FD; ++d)
            if (U.axis[k] == d) xv = x[d];
        xs[k] = xv;
    }
    const void* field = field_of(U, f);
    return U.f64 ? hjq::interp_value<double>(U.G, (const double*)field, xs) : hjq::interp_value<float>(U.G, (const float*)field, xs);
}

// ---- (b) any target grid
template <typename T>
__global__ __launch_bounds__(BLOCK) void backproject_coords_kernel(const KArgs A, T* __restrict__ out, int* __restrict__ active) {
    const unsigned lane = threadIdx.x % WAVE;
    const long long f = A.f0 + blockIdx.y;
    Cursor c = first_chunk(A);
    for (int j = 0; j < A.items && c.w0 < A.total; ++j) {
        const long long node = c.w0 + lane;
        if (node < A.total) {
            unsigned ri[FD - 1], l;
            lane_index(A, c, lane, ri, l);
            double x[FD];
#pragma unroll
            for (int d = 0; d < FD - 1; ++d) x[d] = A.coord[d] ? A.coord[d][ri[d]] : 0.0;
            x[FD - 1] = A.coord[FD - 1][l];
            double acc = 0.0;
            int act = 0;
            for (int s = 0; s < A.nsubs; ++s) take(acc, act, sub_value(A.sub[s], f, x), s, A.op);
            put<T>(out, active, f * A.total + node, acc, act);
        }
        advance(A, c);
    }
}

// ---- (c) states: thread t -> field t / M, state t % M
template <typename T>
__global__ __launch_bounds__(BLOCK) void decomp_points_kernel(const KArgs A, const double* __restrict__ xs, long long M, long long nfields,
                                                              T* __restrict__ out, int* __restrict__ active) {
    const long long t = (A.block0 + blockIdx.x) * (long long)BLOCK + threadIdx.x;
    if (t >= nfields * M) return;
    const long long f = t / M, m = t - f * M;
    const int ndim = FD - A.pad;
    double x[FD];
#pragma unroll
    for (int d = 0; d < FD; ++d) x[d] = d >= A.pad ? xs[m * ndim + (d - A.pad)] : 0.0;
    double acc = 0.0;
    int act = 0;
    for (int s = 0; s < A.nsubs; ++s) take(acc, act, sub_value(A.sub[s], f, x), s, A.op);
    put<T>(out, active, t, acc, act);
}

// ---------------------------------------------------------------------------------------------- host side
// everything the kernels would trust about the descriptor; fills the subsystems of A
static int check_decomp(const hjd_decomp* D, int64_t nfields, KArgs& A) {
    if (!D) return fail(HJ_EINVAL, "null decomposition descriptor");
    if (D->ndim < 1 || D->ndim > HJD_MAX_DIM) return fail(HJ_EINVAL, "ndim %d: a full space of 1 .. %d axes", (int)D->ndim, (int)HJD_MAX_DIM);
    if (D->nsubs < 1 || D->nsubs > HJD_MAX_SUBS) return fail(HJ_EINVAL, "nsubs %d: 1 .. %d subsystems", (int)D->nsubs, (int)HJD_MAX_SUBS);
    if (D->op != HJQ_MIN && D->op != HJQ_MAX) return fail(HJ_EINVAL, "op %d: HJQ_MIN (%d, union) or HJQ_MAX (%d, intersection)", (int)D->op, (int)HJQ_MIN, (int)HJQ_MAX);
    if (nfields < 1) return fail(HJ_EINVAL, "nfields = %lld: at least one field", (long long)nfields);
    std::memset(&A, 0, sizeof(A));
    A.nsubs = D->nsubs;
    A.op = D->op;
    A.pad = FD - D->ndim;
    for (int s = 0; s < D->nsubs; ++s) {
        const hjd_sub& u = D->sub[s];
        KSub& U = A.sub[s];
        if (u.grid.ndim < 1 || u.grid.ndim > HJ_MAX_DIM)
            return fail(HJ_EINVAL, "subsystem %d: ndim %d: a subsystem grid has 1 .. %d dimensions", s, (int)u.grid.ndim, (int)HJ_MAX_DIM);
        long long total = 0;
        if (int rc = make_grid(&u.grid, U.G, total)) {
            const std::string why = g_err;
            return fail(rc, "subsystem %d: %s", s, why.c_str());
        }
        if (total > 0x7fffffffll) return fail(HJ_EUNSUPPORTED, "subsystem %d: %lld nodes: at most 2^31 - 1 per field", s, total);
        unsigned seen = 0;
        for (int k = 0; k < u.grid.ndim; ++k) {
            const int a = u.axis[k];
            if (a < 0 || a >= D->ndim) return fail(HJ_EINVAL, "subsystem %d: axis[%d] = %d is outside the %d axes of the full space", s, k, a, (int)D->ndim);
            if (seen >> a & 1u) return fail(HJ_EINVAL, "subsystem %d: axis[%d] = %d repeats an axis of the same subsystem", s, k, a);
            seen |= 1u << a;
            U.axis[k] = A.pad + a;
            U.fstride[A.pad + a] = (unsigned)U.G.stride[k];
        }
        for (int k = u.grid.ndim; k < MAXD; ++k) U.axis[k] = -1;
        if (u.nfields != 1 && u.nfields != nfields)
            return fail(HJ_EINVAL, "subsystem %d: nfields %lld: 1 or the %lld of the call", s, (long long)u.nfields, (long long)nfields);
        if (u.nfields > 1 && u.field_stride < total)
            return fail(HJ_EINVAL, "subsystem %d: field_stride %lld is less than its %lld nodes", s, (long long)u.field_stride, total);
        if (!u.data) return fail(HJ_EINVAL, "subsystem %d: null data", s);
        U.data = u.data;
        U.field_step = u.nfields > 1 ? u.field_stride : 0;
        U.f64 = u.grid.dtype == HJ_F64;
    }
    return HJ_OK;
}

static int check_out_dtype(int out_dtype) {
    if (out_dtype != HJ_F64 && out_dtype != HJ_F32)
        return fail(HJ_EUNSUPPORTED, "out_dtype %d: the output must be fp64 (%d) or fp32 (%d)", out_dtype, (int)HJ_F64, (int)HJ_F32);
    return HJ_OK;
}

// the full grid into A: FD axes, the real ones last
static int check_full_grid(const hjd_decomp* D, const int64_t* N, int64_t nfields, KArgs& A) {
    if (!N) return fail(HJ_EINVAL, "null N");
    for (int d = 0; d < FD; ++d) {
        A.n[d] = 1u;
        A.magic[d] = 0u;
    }
    A.total = 1;
    for (int a = 0; a < D->ndim; ++a) {
        if (N[a] < 0 || N[a] > 0x7fffffffll) return fail(HJ_EINVAL, "N[%d] = %lld: 0 .. 2^31 - 1 nodes per axis", a, (long long)N[a]);
        if (A.total && N[a] > 0x7fffffffffffffffll / A.total) return fail(HJ_EINVAL, "the full grid has more than 2^63 - 1 nodes");
        A.total *= N[a];
        const unsigned n = (unsigned)N[a];
        A.n[A.pad + a] = n;
        if (n > 1u && n < LONG_AXIS) A.magic[A.pad + a] = (unsigned)(0x100000000ull / n) + 1u;
    }
    if (A.total && nfields > 0x7fffffffffffffffll / A.total) return fail(HJ_EINVAL, "nfields x nodes exceeds 2^63 - 1");
    return HJ_OK;
}

template <typename T, typename K>
static int stream_launch(K kernel, KArgs& A, int64_t nfields, void* out, int32_t* active, hipStream_t stream, const char* name) {
    A.items = A.total >= (1ll << 24) ? 16 : 4;                  // 4096 nodes per workgroup on a large grid, 1024 on a small one
    const long long per = (long long)BLOCK * A.items;
    const long long blocks = (A.total + per - 1) / per;
    for (long long f0 = 0; f0 < nfields; f0 += MAX_Y) {         // gridDim.y ends at 65535: further fields take further launches
        const long long nf = nfields - f0 < MAX_Y ? nfields - f0 : MAX_Y;
        for (long long b0 = 0; b0 < blocks; b0 += MAX_X) {
            const long long nb = blocks - b0 < MAX_X ? blocks - b0 : MAX_X;
            A.f0 = f0;
            A.block0 = b0;
            hipLaunchKernelGGL(kernel, dim3((unsigned)nb, (unsigned)nf), dim3(BLOCK), 0, stream, A, (T*)out, active);
            HIP_TRY(hipGetLastError());
        }
    }
    launched(name);
    return HJ_OK;
}

}  // namespace hjd

using namespace hjd;

extern "C" {

int hjd_backproject_nodes(const hjd_decomp* decomp, const int64_t* N, int64_t nfields, void* out, int out_dtype, int32_t* active,
                          void* stream) {
    KArgs A;
    int rc = check_decomp(decomp, nfields, A);
    if (rc) return rc;
    if ((rc = check_out_dtype(out_dtype))) return rc;
    if ((rc = check_full_grid(decomp, N, nfields, A))) return rc;
    for (int s = 0; s < decomp->nsubs; ++s)
        for (int k = 0; k < decomp->sub[s].grid.ndim; ++k) {
            const int a = decomp->sub[s].axis[k];
            if (N[a] != decomp->sub[s].grid.N[k])
                return fail(HJ_EINVAL, "subsystem %d: axis %d has %lld nodes, full axis %d has %lld: the grids do not conform (hjd_backproject_coords interpolates)",
                            s, k, (long long)decomp->sub[s].grid.N[k], a, (long long)N[a]);
        }
    if (A.total == 0) return HJ_OK;
    if (!out) return fail(HJ_EINVAL, "null output");
    if (out_dtype == HJ_F64)
        return stream_launch<double>(backproject_nodes_kernel<double>, A, nfields, out, active, (hipStream_t)stream, "backproject_nodes_kernel<double>");
    return stream_launch<float>(backproject_nodes_kernel<float>, A, nfields, out, active, (hipStream_t)stream, "backproject_nodes_kernel<float>");
}

int hjd_backproject_coords(const hjd_decomp* decomp, const int64_t* N, const double* const* coord, int64_t nfields, void* out, int out_dtype,
                           int32_t* active, void* stream) {
    KArgs A;
    int rc = check_decomp(decomp, nfields, A);
    if (rc) return rc;
    if ((rc = check_out_dtype(out_dtype))) return rc;
    if ((rc = check_full_grid(decomp, N, nfields, A))) return rc;
    if (!coord) return fail(HJ_EINVAL, "null coordinate tables");
    for (int a = 0; a < decomp->ndim; ++a) {
        if (!coord[a]) return fail(HJ_EINVAL, "null coordinate table of axis %d", a);
        A.coord[A.pad + a] = coord[a];
    }
    if (A.total == 0) return HJ_OK;
    if (!out) return fail(HJ_EINVAL, "null output");
    if (out_dtype == HJ_F64)
        return stream_launch<double>(backproject_coords_kernel<double>, A, nfields, out, active, (hipStream_t)stream, "backproject_coords_kernel<double>");
    return stream_launch<float>(backproject_coords_kernel<float>, A, nfields, out, active, (hipStream_t)stream, "backproject_coords_kernel<float>");
}

int hjd_points(const hjd_decomp* decomp, const double* xs, int64_t nstates, int64_t nfields, void* out, int out_f64, int32_t* active,
               void* stream) {
    KArgs A;
    int rc = check_decomp(decomp, nfields, A);
    if (rc) return rc;
    if (nstates < 0) return fail(HJ_EINVAL, "nstates = %lld is negative", (long long)nstates);
    if (nstates && nfields > 0x7fffffffffffffffll / nstates) return fail(HJ_EINVAL, "nfields x nstates exceeds 2^63 - 1");
    if (nstates == 0) return HJ_OK;
    if (!xs) return fail(HJ_EINVAL, "null states");
    if (!out) return fail(HJ_EINVAL, "null output");
    const long long blocks = (nfields * nstates + BLOCK - 1) / BLOCK;
    for (long long b0 = 0; b0 < blocks; b0 += MAX_X) {
        const unsigned nb = (unsigned)(blocks - b0 < MAX_X ? blocks - b0 : MAX_X);
        A.block0 = b0;
        if (out_f64)
            hipLaunchKernelGGL((decomp_points_kernel<double>), dim3(nb), dim3(BLOCK), 0, (hipStream_t)stream, A, xs, (long long)nstates,
                               (long long)nfields, (double*)out, active);
        else
            hipLaunchKernelGGL((decomp_points_kernel<float>), dim3(nb), dim3(BLOCK), 0, (hipStream_t)stream, A, xs, (long long)nstates,
                               (long long)nfields, (float*)out, active);
        HIP_TRY(hipGetLastError());
    }
    launched(out_f64 ? "decomp_points_kernel<double>" : "decomp_points_kernel<float>");
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjd)

}  // extern "C"
