// libhj_ttr.so (include/hj_ttr.h): time-to-reach functions for gfx950.
//   ttr_init_kernel        ttr = (y <= level) ? t : +inf, last_y = y
//   ttr_update_kernel      one step of the recurrence, in place on ttr and last_y
//   ttr_from_stack_kernel  the whole recurrence over a time-first stack in one pass: a node's previous value and its running
//                          ttr stay in registers, every value of the stack is read once, ttr is written once
// All three are streams.  Every access is ONE element per lane, neighbouring lanes on neighbouring elements: a wave-instruction
// covers 512 contiguous bytes of fp64 (256 of fp32) whatever the alignment of the array -- callers pass views at any element
// offset, and with an odd field_stride the slices of a stack alternate between 16-byte and 8-byte alignment, so no access here
// is wider than an element and no head or tail needs peeling.  Bytes in flight come from depth instead: a thread owns NODES
// nodes BLOCK apart and issues the loads of DEPTH slices before it consumes the first (NODES * DEPTH loads outstanding).
// The recurrence is written one operation per statement with contraction off: the results are NumPy's, bit for bit.
#include <hip/hip_runtime.h>
#include "hj_tool_host.h"
#include "../../include/hj_ttr.h"

namespace hjt {

using namespace hj_tool;

constexpr int BLOCK = 256;
constexpr int NODES = 2;              // nodes per thread and pass of the grid-stride loop, BLOCK apart
constexpr int DEPTH = 4;              // slices of the stack whose loads are issued before the first is consumed
constexpr long long MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups: larger arrays take further passes of the grid-stride loop

// one step of the recurrence for one node (hj_ttr.h); `last` and `ttr` are the node's state.  Returns `changed`.
__device__ __forceinline__ bool step(double y, double t, double t_last, double level, int mode, double& last, double& ttr) {
#pragma clang fp contract(off)
    bool changed = (y <= level) && (last > level);
    if (mode & HJT_FIRST) changed = changed && (ttr == __builtin_inf());
    if (changed) {
        double tc = t;
        if (!(mode & HJT_NO_INTERP)) {
            const double a = last - level;
            const double b = y - level;
            const double dt = t - t_last;
            const double num = dt * a;
            const double den = b - a;
            const double q = num / den;
            tc = t_last - q;
        }
        ttr = tc;
    }
    last = y;
    return changed;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ttr_init_kernel(const T* __restrict__ y, long long n, double t, double level,
                                                         double* __restrict__ ttr, T* __restrict__ last_y) {
    const long long stride = (long long)gridDim.x * (BLOCK * NODES);
    for (long long base = (long long)blockIdx.x * (BLOCK * NODES) + threadIdx.x; base < n; base += stride) {
        T v[NODES];
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            const long long i = base + (long long)j * BLOCK;
            v[j] = y[i < n ? i : n - 1];
        }
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            const long long i = base + (long long)j * BLOCK;
            if (i < n) {
                ttr[i] = ((double)v[j] <= level) ? t : __builtin_inf();
                last_y[i] = v[j];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ttr_update_kernel(const T* __restrict__ y, long long n, double t, double t_last, double level,
                                                           int mode, double* __restrict__ ttr, T* __restrict__ last_y) {
    const long long stride = (long long)gridDim.x * (BLOCK * NODES);
    for (long long base = (long long)blockIdx.x * (BLOCK * NODES) + threadIdx.x; base < n; base += stride) {
        T v[NODES], l[NODES];
        double r[NODES];
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            const long long i = base + (long long)j * BLOCK;
            const long long c = i < n ? i : n - 1;
            v[j] = y[c];
            l[j] = last_y[c];
            r[j] = (mode & HJT_FIRST) ? ttr[c] : 0.0;         // only the earliest-crossing rule looks at the old ttr
        }
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            const long long i = base + (long long)j * BLOCK;
            if (i < n) {
                double last = (double)l[j];
                if (step((double)v[j], t, t_last, level, mode, last, r[j])) ttr[i] = r[j];
                last_y[i] = v[j];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ttr_from_stack_kernel(const T* __restrict__ data, long long T_, long long field_stride,
                                                               long long n, const double* __restrict__ tau, double level, int mode,
                                                               double* __restrict__ ttr) {
    const long long stride = (long long)gridDim.x * (BLOCK * NODES);
    for (long long base = (long long)blockIdx.x * (BLOCK * NODES) + threadIdx.x; base < n; base += stride) {
        long long c[NODES];                   // a node past the end reads node n - 1 and stores nothing
        double last[NODES], r[NODES];
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            const long long i = base + (long long)j * BLOCK;
            c[j] = i < n ? i : n - 1;
        }
        const double t0 = tau[0];
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            last[j] = (double)data[c[j]];
            r[j] = (last[j] <= level) ? t0 : __builtin_inf();
        }
        double t_last = t0;
        long long k = 1;
        for (; k + DEPTH <= T_; k += DEPTH) {
            T v[DEPTH][NODES];
            double tk[DEPTH];
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                const T* __restrict__ slice = data + (k + u) * field_stride;
                tk[u] = tau[k + u];
#pragma unroll
                for (int j = 0; j < NODES; ++j) v[u][j] = slice[c[j]];
            }
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
#pragma unroll
                for (int j = 0; j < NODES; ++j) step((double)v[u][j], tk[u], t_last, level, mode, last[j], r[j]);
                t_last = tk[u];
            }
        }
        for (; k < T_; ++k) {
            const T* __restrict__ slice = data + k * field_stride;
            const double t = tau[k];
            T v[NODES];
#pragma unroll
            for (int j = 0; j < NODES; ++j) v[j] = slice[c[j]];
#pragma unroll
            for (int j = 0; j < NODES; ++j) step((double)v[j], t, t_last, level, mode, last[j], r[j]);
            t_last = t;
        }
#pragma unroll
        for (int j = 0; j < NODES; ++j) {
            const long long i = base + (long long)j * BLOCK;
            if (i < n) ttr[i] = r[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side
// capped, unlike hj_tool::blocks_for: the kernels walk larger arrays in a grid-stride loop
static unsigned stream_blocks(long long n) {
    const long long per = (long long)BLOCK * NODES;
    const long long b = (n + per - 1) / per;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

static int check_common(int dtype, int64_t n, int mode) {
    if (dtype != HJ_F64 && dtype != HJ_F32) return fail(HJ_EUNSUPPORTED, "dtype %d: the data must be fp64 (%d) or fp32 (%d)", dtype, (int)HJ_F64, (int)HJ_F32);
    if (mode & ~(HJT_FIRST | HJT_NO_INTERP)) return fail(HJ_EINVAL, "unknown mode %d (HJT_FIRST | HJT_NO_INTERP)", mode);
    if (n < 0) return fail(HJ_EINVAL, "n = %lld is negative", (long long)n);
    return HJ_OK;
}

template <typename T>
static int init_launch(const void* y, int64_t n, double t, double level, double* ttr, void* last_y, hipStream_t stream, const char* name) {
    hipLaunchKernelGGL((ttr_init_kernel<T>), dim3(stream_blocks(n)), dim3(BLOCK), 0, stream, (const T*)y, (long long)n, t, level, ttr, (T*)last_y);
    return launch_done(name);
}

template <typename T>
static int update_launch(const void* y, int64_t n, double t, double t_last, double level, int mode, double* ttr, void* last_y,
                         hipStream_t stream, const char* name) {
    hipLaunchKernelGGL((ttr_update_kernel<T>), dim3(stream_blocks(n)), dim3(BLOCK), 0, stream, (const T*)y, (long long)n, t, t_last, level,
                       mode, ttr, (T*)last_y);
    return launch_done(name);
}

template <typename T>
static int stack_launch(const void* data, int64_t T_, int64_t field_stride, int64_t n, const double* tau, double level, int mode,
                        double* ttr, hipStream_t stream, const char* name) {
    hipLaunchKernelGGL((ttr_from_stack_kernel<T>), dim3(stream_blocks(n)), dim3(BLOCK), 0, stream, (const T*)data, (long long)T_,
                       (long long)field_stride, (long long)n, tau, level, mode, ttr);
    return launch_done(name);
}

}  // namespace hjt

using namespace hjt;

extern "C" {

int hjt_ttr_init(int dtype, const void* y, int64_t n, double t, double level, double* ttr, void* last_y, void* stream) {
    int rc = check_common(dtype, n, 0);
    if (rc) return rc;
    if (n == 0) return HJ_OK;
    if (!y || !ttr || !last_y) return fail(HJ_EINVAL, "null argument");
    if (dtype == HJ_F64) return init_launch<double>(y, n, t, level, ttr, last_y, (hipStream_t)stream, "ttr_init_kernel<double>");
    return init_launch<float>(y, n, t, level, ttr, last_y, (hipStream_t)stream, "ttr_init_kernel<float>");
}

int hjt_ttr_update(int dtype, const void* y, int64_t n, double t, double t_last, double level, int mode, double* ttr, void* last_y,
                   void* stream) {
    int rc = check_common(dtype, n, mode);
    if (rc) return rc;
    if (n == 0) return HJ_OK;
    if (!y || !ttr || !last_y) return fail(HJ_EINVAL, "null argument");
    if (y == last_y) return fail(HJ_EINVAL, "y and last_y are the same array: last_y is updated in place");
    if (dtype == HJ_F64)
        return update_launch<double>(y, n, t, t_last, level, mode, ttr, last_y, (hipStream_t)stream, "ttr_update_kernel<double>");
    return update_launch<float>(y, n, t, t_last, level, mode, ttr, last_y, (hipStream_t)stream, "ttr_update_kernel<float>");
}

int hjt_ttr_from_stack(int dtype, const void* data, int64_t T, int64_t field_stride, int64_t n, const double* tau_dev, double level,
                       int mode, double* ttr, void* stream) {
    int rc = check_common(dtype, n, mode);
    if (rc) return rc;
    if (T < 1) return fail(HJ_EINVAL, "T = %lld: a stack has at least one slice", (long long)T);
    if (field_stride < n) return fail(HJ_EINVAL, "field_stride %lld is smaller than a slice (%lld)", (long long)field_stride, (long long)n);
    if (n == 0) return HJ_OK;
    if (!data || !tau_dev || !ttr) return fail(HJ_EINVAL, "null argument");
    if (dtype == HJ_F64)
        return stack_launch<double>(data, T, field_stride, n, tau_dev, level, mode, ttr, (hipStream_t)stream, "ttr_from_stack_kernel<double>");
    return stack_launch<float>(data, T, field_stride, n, tau_dev, level, mode, ttr, (hipStream_t)stream, "ttr_from_stack_kernel<float>");
}

HJ_TOOL_LAST_SYMBOLS(hjt)

}  // extern "C"
