// libhj_resample.so (include/hj_resample.h): value functions resampled across grids and frames, on grids of 1 to 6 dimensions, for gfx950.
//   resample_kernel<T, ND, REDUCE>  a thread owns one node of one output array (blockIdx.y the array): it reads its coordinates from
//                                   the destination's vectors, applies the member's affine map, interpolates the source field there
//                                   and stores once; with REDUCE it folds over the K members in registers
//   resample_counts_kernel          adds an output array's partial counts of filled nodes into inside_counts
//   resample_fill_kernel<ND, FOLD>  HJM_FILL_MAX only: finds the unfilled nodes again from the geometry alone (of one member, or
//                                   of all K with FOLD) and stores the array's maximum there
// The interpolant is not restated: it is hj_query_dev.h's locate / interp_value, compiled at six axes (HJ_QUERY_MAXD) the way
// hj_hiquery.hip compiles them, on the grid with `ndim` overwritten by the template's constant (at<ND>), so lo / w and the 2^ND
// corner loop stay in registers.  The fold is hj_shapes_dev.h's nmin / nmax.  The node decode is hj_index_dev.h's walk (tail /
// head split, host-prepared reciprocals, blockIdx.x split in 32 bits: nothing divides) at a compile-time number of axes.
// The map row and the field are read through blockIdx.y and the loop over members is the same in every lane: scalar loads and
// wave-uniform branches.
// Registers (make resource-usage-resample): no instantiation uses scratch or spills a register.  That takes three measures, each
// explained where it stands: the fold reads the source grid again per member (member_grid) and the map one line at a time
// (image<ND, true>), and the unfolded 6-D kernel carries the grid's bounds in vector registers under a bound of six waves per SIMD.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#define HJ_QUERY_MAXD 6
#include "hj_tool_host.h"
#include "../../include/hj_hidim.h"
#include "hj_query_dev.h"
#include "hj_shapes_dev.h"
#include "hj_index_dev.h"
#include "../../include/hj_resample.h"

static_assert(HJ_QUERY_MAXD == HJM_MAX_DIM, "the interpolant is compiled at the header's width");

namespace hjm {

using namespace hj_tool;
using namespace hj_index;
using hjq::QGrid;
using hjq::at;
using hjg_dev::nmin;
using hjg_dev::nmax;
using hjg_dev::MAX_Y;

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int MD = HJM_MAX_DIM;
constexpr int SLOTS = HJM_COUNT_SLOTS;       // partial counts per output array

struct RsArgs {
    QGrid G;                                // the source
    Index X;                                // the destination's extents and the split of blockIdx.x
    const double* coord[MD];                // the destination's coordinate vectors
    const double* maps;                     // K rows of ndim * ndim + ndim, or null: the identity
    long long total;                        // nodes of the destination
    long long node0;                        // flat node of this launch's first head index at tail node 0
    long long field_stride;
    long long K;
    long long a0;                           // first output array of this launch
    long long k0;                           // HJM_REDUCE_NONE: member of array a0 ...
    unsigned f0;                            // ... and its field
    unsigned nfields;
    unsigned long long field_recip;         // recip64(nfields)
    unsigned long long* keys;               // one key of the running maximum per output array (HJM_FILL_MAX)
    unsigned long long* counts;             // filled nodes per output array, in SLOTS partial counts (resample_counts_kernel adds them)
    double fill_value;
    int fill_mode;
    int out_f64;
};

// what a lane of either kernel starts from: whether it owns a node, the node's coordinates and its flat index
template <int ND> struct Node {
    double x[ND];
    long long node;
    bool mine;
};

// false: the whole wave is past the tail's end (wave-uniform).  A lane past the end takes the last node and stores nothing.
template <int ND>
__device__ __forceinline__ bool own_node(const RsArgs& A, Node<ND>& P) {
    const int tid = threadIdx.x;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid / WAVE);
    unsigned hl, chunk;
    split_block(A.X, blockIdx.x, hl, chunk);
    if (chunk * (unsigned)BLOCK + wave * WAVE >= A.X.tail) return false;
    const unsigned own = chunk * (unsigned)BLOCK + (unsigned)tid;
    P.mine = own < A.X.tail;
    const unsigned t = P.mine ? own : A.X.tail - 1u;
    unsigned idx[ND];
    node_index<ND>(A.X, hl, t, idx);
#pragma unroll
    for (int d = 0; d < ND; ++d) P.x[d] = A.coord[d][idx[d]];
    P.node = A.node0 + (long long)hl * (long long)A.X.tail + (long long)t;
    return true;
}

// the members an output array reads, [kb, ke), and its field; wave-uniform
template <int REDUCE>
__device__ __forceinline__ void members_of(const RsArgs& A, long long& kb, long long& ke, unsigned& f) {
    if (REDUCE == HJM_REDUCE_NONE) {
        const unsigned v = A.f0 + blockIdx.y;                    // below 2^31 + 2^16
        unsigned q = v;
        f = 0u;
        if (A.nfields > 1u) {
            q = quotient(v, A.field_recip);
            f = v - q * A.nfields;
        }
        kb = A.k0 + (long long)q;
        ke = kb + 1;
    } else {
        f = A.f0 + blockIdx.y;
        kb = 0;
        ke = A.K;
    }
}

// y = A x + b of member k, every product taken, left to right; null maps: y = x
// LINES: read one line of A at a time (the fold: read as a whole, the row of a 6-D map is 84 scalar registers beside the grid's 60)
template <int ND, bool LINES>
__device__ __forceinline__ void image(const double* __restrict__ maps, long long k, const double (&x)[ND], double* y) {
#pragma clang fp contract(off)
    if (!maps) {
#pragma unroll
        for (int i = 0; i < ND; ++i) y[i] = x[i];
        return;
    }
    const double* __restrict__ row = maps + k * (ND * ND + ND);
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        if (LINES) asm volatile("" : "+s"(row));
        double e = row[i * ND] * x[0];
#pragma unroll
        for (int d = 1; d < ND; ++d) {
            const double q = row[i * ND + d] * x[d];
            e = e + q;
        }
        y[i] = e + row[ND * ND + i];
    }
}

// The source grid as one member's iteration of the fold reads it: again from the kernel-argument segment, through a pointer the
// compiler cannot see through, its bounds and spacings moved to vector registers.  Read once before the loop, the grid and
// everything locate derives from it alone (n - 1, n - 2, the period, fmod's reciprocal and its special-case masks, two scalar
// registers per boolean) is held across the loop over members: 90 to 115 scalar registers spilled to vector lanes at six axes.
// Read per member it costs a few scalar loads that hit the cache; the 36 doubles of six axes have room in the vector file (the
// fold kernels keep 4 waves per SIMD at 5-D and 6-D either way) and none beside the map's line in the scalar file.
static_assert(offsetof(RsArgs, G) == 0, "member_grid reads the grid at the start of the first kernel argument");
template <int ND>
__device__ __forceinline__ QGrid member_grid() {
    const __attribute__((address_space(4))) QGrid* p = (const __attribute__((address_space(4))) QGrid*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    QGrid g;
    g.ndim = ND;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        g.n[d] = p->n[d]; g.per[d] = p->per[d]; g.stride[d] = p->stride[d];
        g.xmin[d] = p->xmin[d]; g.xlast[d] = p->xlast[d]; g.dx[d] = p->dx[d];
        asm volatile("" : "+v"(g.xmin[d]), "+v"(g.xlast[d]), "+v"(g.dx[d]));
    }
    return g;
}

__device__ __forceinline__ void put(void* out, long long i, double v, int out_f64) {
    if (out_f64) ((double*)out)[i] = v;
    else ((float*)out)[i] = (float)v;
}

template <typename T, int ND, int REDUCE>
__global__ __launch_bounds__(BLOCK, REDUCE == HJM_REDUCE_NONE ? 6 : 1) void resample_kernel(const RsArgs A, const T* __restrict__ data, void* __restrict__ out) {
    Node<ND> P;
    if (!own_node<ND>(A, P)) return;
    long long kb, ke;
    unsigned f;
    members_of<REDUCE>(A, kb, ke, f);
    const T* __restrict__ field = data + (long long)f * A.field_stride;
    bool filled = false;
    double acc = __builtin_nan("");
    auto member = [&](const QGrid& G, long long k) {
        double y[hjq::MAXD];
        image<ND, REDUCE != HJM_REDUCE_NONE>(A.maps, k, P.x, y);
        int lo[hjq::MAXD];
        double w[hjq::MAXD];
        if (hjq::locate(G, y, lo, w)) {                          // interp_value locates again: the same expressions, computed once
            const double v = hjq::interp_value<T>(G, field, y);
            if (REDUCE == HJM_REDUCE_MIN) acc = filled ? nmin(acc, v) : v;
            else if (REDUCE == HJM_REDUCE_MAX) acc = filled ? nmax(acc, v) : v;
            else acc = v;
            filled = true;
        }
    };
    if constexpr (REDUCE == HJM_REDUCE_NONE) {
        QGrid G = at<ND>(A.G);
        if (ND == 6) {                                           // the grid's bounds in vector registers: without, 28 scalar registers spill
#pragma unroll
            for (int d = 0; d < ND; ++d) asm volatile("" : "+v"(G.xmin[d]), "+v"(G.xlast[d]));
        }
        member(G, kb);
    } else {
        for (long long k = kb; k < ke; ++k) member(member_grid<ND>(), k);
    }

    const long long arr = A.a0 + blockIdx.y;
    const bool counted = P.mine && filled;
    // an unfilled node of HJM_FILL_MAX is stored by resample_fill_kernel: every element is stored once
    if (counted || (P.mine && A.fill_mode != HJM_FILL_MAX))
        put(out, arr * A.total + P.node, filled ? acc : (A.fill_mode == HJM_FILL_VALUE ? A.fill_value : __builtin_nan("")), A.out_f64);

    // the array's filled count and maximum: reduced over the wave, one lane issues the atomics, and only those that change something.
    // The count goes to one of SLOTS partial counts, chosen by the wave's place in the launch: every wave adds, and adds to ONE address
    // queue behind each other (measured: 7 to 10 ns each, which at one address per array was the whole kernel's time at 201^3 and 25^6)
    const unsigned long long votes = __ballot(counted);
    const bool first = (threadIdx.x & (WAVE - 1)) == 0;
    const unsigned slot = (blockIdx.x * (unsigned)(BLOCK / WAVE) + threadIdx.x / WAVE) & (unsigned)(SLOTS - 1);
    if (first && votes) atomicAdd(A.counts + arr * SLOTS + slot, (unsigned long long)__popcll(votes));
    if (A.fill_mode == HJM_FILL_MAX) {
        const bool has = counted && acc == acc;
        const double top = hj::wave_max(has ? acc : -__builtin_huge_val());
        if (__any(has) && first) hj::key_max(A.keys + arr, top);
    }
}

// the value a key stands for; key 0: no filled non-NaN node
__device__ __forceinline__ double key_value(unsigned long long k) {
    if (k == 0ull) return __builtin_nan("");
    const unsigned long long b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

template <int ND, int REDUCE>
__global__ __launch_bounds__(BLOCK) void resample_fill_kernel(const RsArgs A, void* __restrict__ out) {
    Node<ND> P;
    if (!own_node<ND>(A, P)) return;
    long long kb, ke;
    unsigned f;
    members_of<REDUCE>(A, kb, ke, f);
    bool filled = false;
    for (long long k = kb; k < ke && !__all(filled); ++k) {
        const QGrid G = REDUCE == HJM_REDUCE_NONE ? at<ND>(A.G) : member_grid<ND>();
        double y[hjq::MAXD];
        image<ND, REDUCE != HJM_REDUCE_NONE>(A.maps, k, P.x, y);
        int lo[hjq::MAXD];
        double w[hjq::MAXD];
        filled |= hjq::locate(G, y, lo, w);
    }
    const long long arr = A.a0 + blockIdx.y;
    if (P.mine && !filled) put(out, arr * A.total + P.node, key_value(A.keys[arr]), A.out_f64);
}

// inside_counts[array] = the sum of the array's partial counts
__global__ __launch_bounds__(BLOCK) void resample_counts_kernel(const unsigned long long* __restrict__ slots, long long* __restrict__ counts,
                                                                long long arrays) {
    const long long a = blockIdx.x * (long long)BLOCK + threadIdx.x;
    if (a >= arrays) return;
    unsigned long long sum = 0ull;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) sum += slots[a * SLOTS + s];
    counts[a] = (long long)sum;
}

// ---------------------------------------------------------------------------------------------- host side
static long long arrays_of(int64_t nfields, int64_t K, int reduce) { return reduce == HJM_REDUCE_NONE ? K * nfields : nfields; }

// the destination: ndim as the source's, 1 .. 2^31 - 1 nodes per axis, at most 2^63 - 1 in all
static int check_dst(const hjh_grid* dst, int ndim, long long& total) {
    if (int rc = hjg_dev::check_extents<MD>(dst, total)) return rc;
    if (ndim && dst->ndim != ndim) return fail(HJ_EINVAL, "the source grid has %d dimensions, the destination %d", ndim, (int)dst->ndim);
    for (int d = 0; d < dst->ndim; ++d)
        if (dst->N[d] < 1) return fail(HJ_EINVAL, "N[%d] = %lld: a destination axis has at least one node", d, (long long)dst->N[d]);
    return HJ_OK;
}

static int check_batch(int64_t nfields, int64_t K, int reduce, long long total) {
    if (K < 1) return fail(HJ_EINVAL, "K = %lld: at least one map", (long long)K);
    if (nfields < 1 || nfields > 0x7fffffffll) return fail(HJ_EINVAL, "nfields = %lld: 1 .. 2^31 - 1 fields", (long long)nfields);
    if (reduce != HJM_REDUCE_NONE && reduce != HJM_REDUCE_MIN && reduce != HJM_REDUCE_MAX) return fail(HJ_EINVAL, "unknown reduce %d", reduce);
    if (reduce == HJM_REDUCE_NONE && K > 0x7fffffffffffffffll / nfields) return fail(HJ_EINVAL, "K x nfields exceeds 2^63 - 1");
    if (arrays_of(nfields, K, reduce) > 0x7fffffffffffffffll / total) return fail(HJ_EINVAL, "output arrays x nodes exceeds 2^63 - 1");
    return HJ_OK;
}

// every launch of one kernel: along the head, and per head launch along the output arrays.  launch(blocks, ny)
template <typename F>
static int all_launches(RsArgs& A, const Plan& L, long long arrays, int reduce, F&& launch) {
    return head_launches(L, A.X, A.node0, [&](unsigned blocks) {
        for (long long a0 = 0; a0 < arrays; a0 += MAX_Y) {
            A.a0 = a0;
            A.k0 = reduce == HJM_REDUCE_NONE ? a0 / A.nfields : 0;
            A.f0 = (unsigned)(reduce == HJM_REDUCE_NONE ? a0 % A.nfields : a0);
            launch(blocks, (unsigned)(arrays - a0 < MAX_Y ? arrays - a0 : MAX_Y));
            HIP_TRY(hipGetLastError());
        }
        return (int)HJ_OK;
    });
}

template <typename T, int ND, int REDUCE>
static int run(RsArgs& A, const Plan& L, long long arrays, long long* inside_counts, const void* data, void* out, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(A.keys, 0, (size_t)hjm_workspace_size(arrays), stream));              // the keys and the partial counts
    int rc = all_launches(A, L, arrays, REDUCE, [&](unsigned blocks, unsigned ny) {
        hipLaunchKernelGGL((resample_kernel<T, ND, REDUCE>), dim3(blocks, ny), dim3(BLOCK), 0, stream, A, (const T*)data, out);
    });
    if (rc) return rc;
    launched(kernel_name("resample_kernel", type_tag<T>::name(), {ND, REDUCE}).c_str());
    hipLaunchKernelGGL(resample_counts_kernel, dim3((unsigned)((arrays + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, A.counts, inside_counts, arrays);
    HIP_TRY(hipGetLastError());
    launched_also("resample_counts_kernel");
    if (A.fill_mode != HJM_FILL_MAX) return HJ_OK;
    constexpr int FOLD = REDUCE == HJM_REDUCE_NONE ? HJM_REDUCE_NONE : HJM_REDUCE_MIN;       // the geometry of min and max is one
    rc = all_launches(A, L, arrays, REDUCE, [&](unsigned blocks, unsigned ny) {
        hipLaunchKernelGGL((resample_fill_kernel<ND, FOLD>), dim3(blocks, ny), dim3(BLOCK), 0, stream, A, out);
    });
    if (rc) return rc;
    launched_also(("resample_fill_kernel<" + std::to_string(ND) + ", " + std::to_string(FOLD) + ">").c_str());
    return HJ_OK;
}

template <typename T, int ND>
static int run_reduce(int reduce, RsArgs& A, const Plan& L, long long arrays, long long* counts, const void* data, void* out, hipStream_t stream) {
    if (reduce == HJM_REDUCE_NONE) return run<T, ND, HJM_REDUCE_NONE>(A, L, arrays, counts, data, out, stream);
    if (reduce == HJM_REDUCE_MIN) return run<T, ND, HJM_REDUCE_MIN>(A, L, arrays, counts, data, out, stream);
    return run<T, ND, HJM_REDUCE_MAX>(A, L, arrays, counts, data, out, stream);
}

template <typename T>
static int run_ndim(int reduce, RsArgs& A, const Plan& L, long long arrays, long long* counts, const void* data, void* out, hipStream_t stream) {
    return dispatch_ndim(A.G.ndim, [&](auto nd) { return run_reduce<T, decltype(nd)::value>(reduce, A, L, arrays, counts, data, out, stream); });
}

}  // namespace hjm

using namespace hjm;

extern "C" {

int hjm_resample(const hjh_grid* src, const hjh_grid* dst, const double* const* coord, const void* data, int64_t nfields,
                 int64_t field_stride, const double* maps, int64_t K, int reduce, int fill_mode, double fill_value, void* out,
                 int out_dtype, int64_t* inside_counts, void* workspace, void* stream) {
    RsArgs A{};
    long long src_total = 0, total = 0;
    if (int rc = hjq::make_grid(src, A.G, src_total)) return rc;
    if (int rc = check_dst(dst, src->ndim, total)) return rc;
    if (out_dtype != HJ_F64 && out_dtype != HJ_F32)
        return fail(HJ_EUNSUPPORTED, "out_dtype %d: the output must be fp64 (%d) or fp32 (%d)", out_dtype, (int)HJ_F64, (int)HJ_F32);
    if (int rc = check_batch(nfields, K, reduce, total)) return rc;
    if (fill_mode != HJM_FILL_NAN && fill_mode != HJM_FILL_VALUE && fill_mode != HJM_FILL_MAX) return fail(HJ_EINVAL, "unknown fill_mode %d", fill_mode);
    if (fill_mode == HJM_FILL_VALUE && fill_value != fill_value) return fail(HJ_EINVAL, "fill_value is NaN: HJM_FILL_NAN says that");
    if (nfields > 1 && field_stride < src_total)
        return fail(HJ_EINVAL, "field_stride %lld is smaller than the source grid (%lld)", (long long)field_stride, src_total);
    if (!maps && K > 1) return fail(HJ_EINVAL, "null maps with K = %lld: only one map can be the identity", (long long)K);
    for (int d = 0; d < A.G.ndim; ++d) {
        const int need = A.G.per[d] ? 1 : 2;                     // an extrapolated axis interpolates between nodes i and i + 1
        if (A.G.n[d] < need) return fail(HJ_EINVAL, "source grid too small along dim %d (N=%d, need %d)", d, A.G.n[d], need);
    }
    if (!coord || !data || !out || !inside_counts || !workspace) return fail(HJ_EINVAL, "null argument");
    for (int d = 0; d < A.G.ndim; ++d)
        if (!coord[d]) return fail(HJ_EINVAL, "null coordinate table of axis %d", d);

    Limits lim;
    if (int rc = read_limits(lim, BLOCK)) return rc;
    const Plan L = make_plan(dst, total, BLOCK, A.X, lim);
    const long long arrays = arrays_of(nfields, K, reduce);
    for (int d = 0; d < A.G.ndim; ++d) A.coord[d] = coord[d];
    A.maps = maps;
    A.total = total;
    A.field_stride = field_stride;
    A.K = K;
    A.nfields = (unsigned)nfields;
    A.field_recip = recip64(A.nfields);
    A.keys = (unsigned long long*)workspace;
    A.counts = A.keys + arrays;
    A.fill_value = fill_value;
    A.fill_mode = fill_mode;
    A.out_f64 = out_dtype == HJ_F64;
    if (src->dtype == HJ_F64) return run_ndim<double>(reduce, A, L, arrays, (long long*)inside_counts, data, out, (hipStream_t)stream);
    return run_ndim<float>(reduce, A, L, arrays, (long long*)inside_counts, data, out, (hipStream_t)stream);
}

int64_t hjm_workspace_size(int64_t arrays) { return arrays > 0 ? arrays * (int64_t)((1 + SLOTS) * sizeof(unsigned long long)) : 0; }

int hjm_plan(const hjh_grid* dst, int64_t nfields, int64_t K, int reduce, hjm_launch_plan* plan) {
    long long total = 0;
    if (int rc = check_dst(dst, 0, total)) return rc;
    if (int rc = check_batch(nfields, K, reduce, total)) return rc;
    if (!plan) return fail(HJ_EINVAL, "null argument");
    Limits lim;
    if (int rc = read_limits(lim, BLOCK)) return rc;
    Index X;
    publish(make_plan(dst, total, BLOCK, X, lim), *plan);
    plan->arrays = arrays_of(nfields, K, reduce);
    plan->array_launches = (int32_t)((plan->arrays + MAX_Y - 1) / MAX_Y);
    return HJ_OK;
}

int hjm_decode(const hjh_grid* dst, int64_t node, int32_t idx[6]) {
    long long total = 0;
    if (int rc = check_dst(dst, 0, total)) return rc;
    if (!idx) return fail(HJ_EINVAL, "null argument");
    if (int rc = check_node(node, total)) return rc;
    Limits lim;
    if (int rc = read_limits(lim, BLOCK)) return rc;
    Index X;
    const Plan L = make_plan(dst, total, BLOCK, X, lim);
    decode(L, X, dst->ndim, node, idx);
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjm)

}  // extern "C"
