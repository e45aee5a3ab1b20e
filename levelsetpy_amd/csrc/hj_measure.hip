// libhj_measure.so (include/hj_measure.h): volumes, overlaps and bounds of sublevel sets on grids of 1 to 6 dimensions, for gfx950.
//   measure_kernel<TA, TB, ND, CMP>  a thread owns one node of one field (blockIdx.y the field): the node statistics, and, where the
//                                    node is a cell's base, the cell's class from its 2^ND corners.  The workgroup's cut cells are
//                                    compacted by wave ballots into a list in LDS; CAP of them at a time have their corner values
//                                    gathered into LDS, and the (cell, simplex) pairs are spread over the 256 lanes.  With CMP every
//                                    cell is classified four times (a, b, nmin, nmax) from the same loads and a list entry is a
//                                    (cell, set) pair
//   measure_fold_kernel              a thread owns one record: adds its slots, with the carry of Q_cut, and turns the bounds round
// The per-simplex rule is hj_measure_dev.h's simplex_q / simplex_chain, which hjv_simplex_q_host runs on the host.  The minimum and
// maximum are hj_shapes_dev.h's nmin / nmax.  The node decode is hj_index_dev.h's walk (tail / head split, host-prepared reciprocals,
// blockIdx.x split in 32 bits: nothing divides) at a compile-time number of axes.
// Nothing a lane indexes at run time is a register array: the corner values live in LDS, the recursion's row is indexed by vertex in
// loops of compile-time bounds, the per-set accumulators are selected by predicates (make resource-usage-measure: no scratch).
// Every sum is an integer sum -- ballots and shuffles in the wave, LDS across the waves, one atomic add per workgroup and counter
// into one of `slots` partial records (one address per record would queue every workgroup of a field behind each other) -- so the
// totals do not depend on the order of arrival.  Q_cut is 128 bits: the low word is added first and the carry, read off the value
// the atomic returns, goes into the high word with the workgroup's own high word.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include "hj_tool_host.h"
#include "../../include/hj_hidim.h"
#include "hj_shapes_dev.h"
#include "hj_index_dev.h"
#include "hj_measure_dev.h"
#include "../../include/hj_measure.h"

namespace hjv {

using namespace hj_tool;
using namespace hj_index;
using hjg_dev::nmin;
using hjg_dev::nmax;
using hjg_dev::MAX_Y;
using hjv_dev::factorial;
using hjv_dev::simplex_chain;
using hjv_dev::simplex_q;

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int WAVES = BLOCK / WAVE;
constexpr int MD = HJV_MAX_DIM;
constexpr int WORDS = HJV_RECORD_WORDS;
constexpr int SUMS = 7;                      // per-wave partial sums: full, cut, invalid, inside, nan, Q_cut low, Q_cut high
static_assert(HJV_LO == 8 && HJV_HI == HJV_LO + MD && WORDS == HJV_HI + MD, "the record ends with the two rows of bounds");

struct MvArgs {
    Index X;                                // the grid's extents and the split of blockIdx.x
    long long stride[MD];                   // nodes between neighbours along axis d
    long long node0;                        // flat node of this launch's first head index at tail node 0
    long long stride_a, stride_b;           // elements between fields (stride_b 0: one field of b for all)
    unsigned long long* slots;              // records x nslots partial records of WORDS words
    double level;
    unsigned periodic;                      // bit d: axis d is periodic
    unsigned f0;                            // first field of this launch
    unsigned nslots;                        // a power of two
};

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

template <typename TA, typename TB, int ND, bool CMP>
__global__ __launch_bounds__(BLOCK) void measure_kernel(const MvArgs A, const TA* __restrict__ a, const TB* __restrict__ b) {
    constexpr int NS = CMP ? 4 : 1;                              // the sets a cell is classified for
    constexpr int NC = 1 << ND;                                  // corners of a cell
    constexpr int CAP = ND <= 3 ? BLOCK : (2048 >> ND);          // list entries whose corners LDS holds at a time: 16 KiB at most
    constexpr unsigned FACT = (unsigned)factorial(ND);
    constexpr int UNROLL = CMP ? 2 : 8;                          // of the corner loop
    __shared__ double corners[CAP * NC];
    __shared__ long long base_node[BLOCK];                       // of the thread's cell, where it has one
    __shared__ unsigned char wraps[BLOCK];                       // bit d: the cell's upper node of axis d is node 0
    __shared__ unsigned short list[BLOCK * NS];                  // cut (cell, set) pairs: thread | set << 8
    __shared__ unsigned n_list;
    __shared__ unsigned long long wsum[WAVES][NS][SUMS];
    __shared__ unsigned bounds[NS][2 * MD];                      // max of n[d] - index, max of index + 1, over the inside nodes

    const unsigned tid = threadIdx.x;
    const unsigned lane = tid & (WAVE - 1);
    const unsigned wave = tid / WAVE;
    if (tid == 0) n_list = 0u;
    if (tid < NS * 2 * MD) (&bounds[0][0])[tid] = 0u;
    __syncthreads();

    unsigned hl, chunk;
    split_block(A.X, blockIdx.x, hl, chunk);
    const unsigned own = chunk * (unsigned)BLOCK + tid;
    const bool mine = own < A.X.tail;                            // a lane past the tail's end takes the last node and counts nothing
    const unsigned t = mine ? own : A.X.tail - 1u;
    unsigned idx[ND];
    node_index<ND>(A.X, hl, t, idx);
    const long long node = A.node0 + (long long)hl * (long long)A.X.tail + (long long)t;
    const unsigned field = A.f0 + blockIdx.y;
    const TA* __restrict__ fa = a + (long long)field * A.stride_a;
    const TB* __restrict__ fb = CMP ? b + (long long)field * A.stride_b : nullptr;
    const double level = A.level;

    // f of every set at one node
    auto values = [&](long long n, double (&f)[NS]) {
        const double va = (double)fa[n];
        if constexpr (CMP) {
            const double vb = (double)fb[n];
            f[HJV_SET_A] = va - level;
            f[HJV_SET_B] = vb - level;
            f[HJV_SET_UNION] = nmin(va, vb) - level;
            f[HJV_SET_INTERSECTION] = nmax(va, vb) - level;
        } else {
            f[0] = va - level;
        }
    };

    // ---- the node
    double f0[NS];
    values(node, f0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const bool inside = mine && f0[s] <= 0.0;
        const unsigned long long bi = __ballot(inside);
        const unsigned long long bn = __ballot(mine && f0[s] != f0[s]);
        if (lane == 0) {
            wsum[wave][s][3] = (unsigned long long)__popcll(bi);
            wsum[wave][s][4] = (unsigned long long)__popcll(bn);
        }
        if (bi) {                                                // wave-uniform
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const unsigned lo = wave_max_u32(inside ? A.X.n[d] - idx[d] : 0u);
                const unsigned hi = wave_max_u32(inside ? idx[d] + 1u : 0u);
                if (lane == 0) {
                    atomicMax(&bounds[s][d], lo);
                    atomicMax(&bounds[s][MD + d], hi);
                }
            }
        }
    }

    // ---- the cell whose base the node is
    bool base = mine;
    unsigned wrap = 0u;
    long long up[ND];                                            // from the lower to the upper node of axis d
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const bool last = idx[d] + 1u == A.X.n[d];
        if (last) {
            base = base && ((A.periodic >> d) & 1u);
            wrap |= 1u << d;
        }
        up[d] = last ? -(long long)(A.X.n[d] - 1u) * A.stride[d] : A.stride[d];
    }
    bool bad[NS], pos[NS], neg[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        bad[s] = !__builtin_isfinite(f0[s]);
        pos[s] = f0[s] > 0.0;
        neg[s] = f0[s] < 0.0;
    }
    if (base) {
        base_node[tid] = node;
        wraps[tid] = (unsigned char)wrap;
        // a few corners at a time: unrolled as a whole, the 2^ND loads of both inputs are all in flight at once and the 5-D and
        // 6-D comparisons spill
#pragma unroll UNROLL
        for (int c = 1; c < NC; ++c) {
            long long o = node;
#pragma unroll
            for (int d = 0; d < ND; ++d)
                if ((c >> d) & 1) o += up[d];
            double fc[NS];
            values(o, fc);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                bad[s] = bad[s] || !__builtin_isfinite(fc[s]);
                pos[s] = pos[s] || fc[s] > 0.0;
                neg[s] = neg[s] || fc[s] < 0.0;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const bool ok = base && !bad[s];
        const bool cut = ok && pos[s] && neg[s];
        const unsigned long long bf = __ballot(ok && !pos[s]);
        const unsigned long long bc = __ballot(cut);
        const unsigned long long bv = __ballot(base && bad[s]);
        if (lane == 0) {
            wsum[wave][s][0] = (unsigned long long)__popcll(bf);
            wsum[wave][s][1] = (unsigned long long)__popcll(bc);
            wsum[wave][s][2] = (unsigned long long)__popcll(bv);
        }
        if (bc) {                                                // wave-uniform: the wave's cut cells take consecutive entries
            unsigned start = 0u;
            if (lane == 0) start = atomicAdd(&n_list, (unsigned)__popcll(bc));
            start = (unsigned)__shfl((int)start, 0);
            if (cut) list[start + (unsigned)__popcll(bc & ((1ull << lane) - 1ull))] = (unsigned short)(tid | ((unsigned)s << 8));
        }
    }
    __syncthreads();

    // ---- the cut cells: CAP entries at a time, corners into LDS, then (entry, simplex) pairs over the lanes
    const unsigned entries = n_list;                             // at most BLOCK * NS
    unsigned long long acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0ull;
    for (unsigned r0 = 0u; r0 < entries; r0 += (unsigned)CAP) {  // workgroup-uniform
        const unsigned nc = entries - r0 < (unsigned)CAP ? entries - r0 : (unsigned)CAP;
        for (unsigned e = tid; e < nc * (unsigned)NC; e += (unsigned)BLOCK) {
            const unsigned cell = e >> ND, c = e & (unsigned)(NC - 1);
            const unsigned entry = list[r0 + cell];
            const unsigned owner = entry & 255u, set = entry >> 8;
            const unsigned w = wraps[owner];
            long long o = base_node[owner];
#pragma unroll
            for (int d = 0; d < ND; ++d)
                if ((c >> d) & 1u) o += ((w >> d) & 1u) ? -(long long)(A.X.n[d] - 1u) * A.stride[d] : A.stride[d];
            double fc[NS];
            values(o, fc);
            double v = fc[0];
#pragma unroll
            for (int s = 1; s < NS; ++s) v = set == (unsigned)s ? fc[s] : v;
            corners[cell * NC + c] = v;
        }
        __syncthreads();
        for (unsigned p = tid; p < nc * FACT; p += (unsigned)BLOCK) {
            const unsigned cell = p / FACT, sx = p - cell * FACT;
            unsigned chain[ND + 1];
            simplex_chain<ND>(sx, chain);
            double f[ND + 1];
#pragma unroll
            for (int k = 0; k <= ND; ++k) f[k] = corners[cell * NC + chain[k]];
            const unsigned long long q = simplex_q<ND>(f);
            const unsigned set = list[r0 + cell] >> 8;
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] += set == (unsigned)s ? q : 0ull;
        }
        __syncthreads();
    }
    // a lane's sum is below 2^64 (at most BLOCK * NS * 720 / BLOCK terms of 2^52); the wave's is not: the halves are summed apart
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const unsigned long long lows = wave_sum_u64(acc[s] & 0xffffffffull);
        const unsigned long long highs = wave_sum_u64(acc[s] >> 32);
        if (lane == 0) {
            const unsigned long long lo = lows + (highs << 32);
            wsum[wave][s][5] = lo;
            wsum[wave][s][6] = (highs >> 32) + (lo < lows ? 1ull : 0ull);
        }
    }
    __syncthreads();

    // ---- one add per workgroup and counter, into the slot of this workgroup
    unsigned long long* __restrict__ slot0 = A.slots + ((unsigned long long)field * NS * A.nslots + (blockIdx.x & (A.nslots - 1u))) * WORDS;
    if (tid < NS * 6) {
        const unsigned s = tid / 6u, k = tid - s * 6u;
        unsigned long long* __restrict__ slot = slot0 + (unsigned long long)s * A.nslots * WORDS;
        if (k < 5u) {
            unsigned long long v = 0ull;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) v += wsum[w][s][k];
            const int word = k == 0u ? HJV_FULL : (k == 1u ? HJV_CUT : (k == 2u ? HJV_INVALID : (k == 3u ? HJV_INSIDE : HJV_NAN)));
            if (v) atomicAdd(slot + word, v);
        } else {
            unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const unsigned long long l = wsum[w][s][5];
                lo += l;
                hi += wsum[w][s][6] + (lo < l ? 1ull : 0ull);
            }
            if (lo | hi) {
                unsigned long long carry = 0ull;
                if (lo) {
                    const unsigned long long old = atomicAdd(slot + HJV_QLO, lo);
                    carry = old + lo < old ? 1ull : 0ull;
                }
                if (hi + carry) atomicAdd(slot + HJV_QHI, hi + carry);
            }
        }
    } else if (tid >= WAVE && tid < WAVE + NS * 2 * MD) {
        const unsigned j = tid - WAVE, s = j / (2u * MD), k = j - s * (2u * MD);
        const unsigned long long v = bounds[s][k];
        unsigned long long* p = slot0 + (unsigned long long)s * A.nslots * WORDS + HJV_LO + k;
        // a maximum only grows: a stale smaller value read here costs an atomic, never a result
        if (v && v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
    }
}

struct FoldArgs {
    long long records;
    long long cells;
    unsigned n[MD];
    unsigned nslots;
};

__global__ __launch_bounds__(BLOCK) void measure_fold_kernel(const FoldArgs F, const unsigned long long* __restrict__ slots,
                                                             unsigned long long* __restrict__ records) {
    const long long r = blockIdx.x * (long long)BLOCK + threadIdx.x;
    if (r >= F.records) return;
    const unsigned long long* __restrict__ p = slots + (unsigned long long)r * F.nslots * WORDS;
    unsigned long long out[WORDS];
#pragma unroll
    for (int k = 0; k < WORDS; ++k) out[k] = 0ull;
    for (unsigned s = 0; s < F.nslots; ++s) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) {
            const unsigned long long v = p[s * WORDS + k];
            if (k >= HJV_LO) {
                out[k] = v > out[k] ? v : out[k];
            } else if (k == HJV_QLO) {
                out[k] += v;
                out[HJV_QHI] += out[k] < v ? 1ull : 0ull;
            } else {
                out[k] += v;
            }
        }
    }
    out[HJV_CELLS] = (unsigned long long)F.cells;
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        out[HJV_LO + d] = (unsigned long long)((long long)F.n[d] - (long long)out[HJV_LO + d]);
        out[HJV_HI + d] = (unsigned long long)((long long)out[HJV_HI + d] - 1ll);
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k) records[r * WORDS + k] = out[k];
}

// ---------------------------------------------------------------------------------------------- host side
// partial records per field and set: a power of two, no more than the grid has workgroups
static long long slots_of(const Plan& L) {
    long long slots = 1;
    while (slots < HJV_MAX_SLOTS && slots < L.head * L.chunks) slots *= 2;           // head * chunks <= total
    return slots;
}

// the grid: 1 .. 6 axes of 2 .. 2^31 - 1 nodes, at most 2^63 - 1 in all, every boundary kind known
static int check_grid(const hjh_grid* g, long long& total) {
    if (int rc = hjg_dev::check_extents<MD>(g, total)) return rc;
    for (int d = 0; d < g->ndim; ++d) {
        if (g->N[d] < 2) return fail(HJ_EINVAL, "N[%d] = %lld: an axis has at least two nodes", d, (long long)g->N[d]);
        if (g->bc[d] != HJ_BC_EXTRAPOLATE && g->bc[d] != HJ_BC_PERIODIC) return fail(HJ_EINVAL, "unknown boundary kind %d along dim %d", (int)g->bc[d], d);
    }
    return HJ_OK;
}

static int check_fields(int64_t nfields) {
    if (nfields < 1 || nfields > 0x7fffffffll) return fail(HJ_EINVAL, "nfields = %lld: 1 .. 2^31 - 1 fields", (long long)nfields);
    return HJ_OK;
}

template <typename TA, typename TB, int ND, bool CMP>
static int run(MvArgs& A, const Plan& L, long long nfields, const FoldArgs& F, const void* a, const void* b, void* records, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(A.slots, 0, (size_t)(F.records * F.nslots * WORDS * 8), stream));
    int rc = head_launches(L, A.X, A.node0, [&](unsigned blocks) {
        for (long long f0 = 0; f0 < nfields; f0 += MAX_Y) {
            A.f0 = (unsigned)f0;
            const unsigned ny = (unsigned)(nfields - f0 < MAX_Y ? nfields - f0 : MAX_Y);
            hipLaunchKernelGGL((measure_kernel<TA, TB, ND, CMP>), dim3(blocks, ny), dim3(BLOCK), 0, stream, A, (const TA*)a, (const TB*)b);
            HIP_TRY(hipGetLastError());
        }
        return (int)HJ_OK;
    });
    if (rc) return rc;
    launched((std::string("measure_kernel<") + type_tag<TA>::name() + ", " + type_tag<TB>::name() + ", " + std::to_string(ND) + ", " +
              (CMP ? "1>" : "0>")).c_str());
    unsigned blocks = 0;
    if (int rc = blocks_for(F.records, "more than 2^32 - 1 records", blocks)) return rc;
    hipLaunchKernelGGL(measure_fold_kernel, dim3(blocks), dim3(BLOCK), 0, stream, F, (const unsigned long long*)A.slots, (unsigned long long*)records);
    HIP_TRY(hipGetLastError());
    launched_also("measure_fold_kernel");
    return HJ_OK;
}

template <typename TA, typename TB, bool CMP>
static int run_ndim(int ndim, MvArgs& A, const Plan& L, long long nfields, const FoldArgs& F, const void* a, const void* b, void* records, hipStream_t stream) {
    return dispatch_ndim(ndim, [&](auto nd) { return run<TA, TB, decltype(nd)::value, CMP>(A, L, nfields, F, a, b, records, stream); });
}

template <int D>
static unsigned long long simplex_host(const double* f) {
    double v[D + 1];
    for (int k = 0; k <= D; ++k) v[k] = f[k];
    return simplex_q<D>(v);
}

}  // namespace hjv

using namespace hjv;

extern "C" {

int hjv_measure(const hjh_grid* g, const void* a, int64_t nfields, int64_t stride_a, const void* b, int b_dtype, int64_t nfields_b,
                int64_t stride_b, double level, void* records, void* workspace, void* stream) {
    long long total = 0;
    if (int rc = check_grid(g, total)) return rc;
    if (int rc = check_fields(nfields)) return rc;
    Limits lim;                                                  // before the workspace is looked at: hjv_workspace_size gave 0 for a limit it refused
    if (int rc = read_limits(lim, BLOCK)) return rc;
    if (!std::isfinite(level)) return fail(HJ_EINVAL, "level is not finite");
    if (nfields > 1 && stride_a < total) return fail(HJ_EINVAL, "stride_a %lld is smaller than the grid (%lld)", (long long)stride_a, total);
    if (b) {
        if (b_dtype != HJ_F64 && b_dtype != HJ_F32)
            return fail(HJ_EUNSUPPORTED, "b_dtype %d: the second input must be fp64 (%d) or fp32 (%d)", b_dtype, (int)HJ_F64, (int)HJ_F32);
        if (nfields_b != 1 && nfields_b != nfields)
            return fail(HJ_EINVAL, "nfields_b = %lld: one field, or as many as a (%lld)", (long long)nfields_b, (long long)nfields);
        if (nfields_b > 1 && stride_b < total) return fail(HJ_EINVAL, "stride_b %lld is smaller than the grid (%lld)", (long long)stride_b, total);
    }
    if (!a || !records || !workspace) return fail(HJ_EINVAL, "null argument");

    MvArgs A{};
    const Plan L = make_plan(g, total, BLOCK, A.X, lim);
    FoldArgs F{};
    F.records = nfields * (b ? 4 : 1);
    F.cells = 1;
    F.nslots = (unsigned)slots_of(L);
    long long stride = 1;
    for (int d = MD - 1; d >= 0; --d) {
        F.n[d] = A.X.n[d];
        A.stride[d] = stride;
        stride *= (long long)A.X.n[d];
        if (d < g->ndim) {
            const bool periodic = g->bc[d] == HJ_BC_PERIODIC;
            if (periodic) A.periodic |= 1u << d;
            F.cells *= (long long)A.X.n[d] - (periodic ? 0 : 1);
        }
    }
    A.stride_a = nfields > 1 ? stride_a : 0;
    A.stride_b = b && nfields_b > 1 ? stride_b : 0;
    A.slots = (unsigned long long*)workspace;
    A.level = level;
    A.nslots = F.nslots;
    hipStream_t st = (hipStream_t)stream;
    const bool a64 = g->dtype == HJ_F64;
    if (!b) return a64 ? run_ndim<double, double, false>(g->ndim, A, L, nfields, F, a, nullptr, records, st) : run_ndim<float, float, false>(g->ndim, A, L, nfields, F, a, nullptr, records, st);
    const bool b64 = b_dtype == HJ_F64;
    if (a64) return b64 ? run_ndim<double, double, true>(g->ndim, A, L, nfields, F, a, b, records, st) : run_ndim<double, float, true>(g->ndim, A, L, nfields, F, a, b, records, st);
    return b64 ? run_ndim<float, double, true>(g->ndim, A, L, nfields, F, a, b, records, st) : run_ndim<float, float, true>(g->ndim, A, L, nfields, F, a, b, records, st);
}

int64_t hjv_workspace_size(const hjh_grid* g, int64_t nfields, int compare) {
    long long total = 0;
    Limits lim;
    if (check_grid(g, total) || check_fields(nfields) || read_limits(lim, BLOCK)) return 0;
    Index X;
    return nfields * (compare ? 4 : 1) * slots_of(make_plan(g, total, BLOCK, X, lim)) * (int64_t)(WORDS * sizeof(unsigned long long));
}

int hjv_plan(const hjh_grid* g, int64_t nfields, hjv_launch_plan* plan) {
    long long total = 0;
    if (int rc = check_grid(g, total)) return rc;
    if (int rc = check_fields(nfields)) return rc;
    if (!plan) return fail(HJ_EINVAL, "null argument");
    Limits lim;
    if (int rc = read_limits(lim, BLOCK)) return rc;
    Index X;
    const Plan L = make_plan(g, total, BLOCK, X, lim);
    publish(L, *plan);
    plan->nfields = nfields;
    plan->field_launches = (int32_t)((nfields + MAX_Y - 1) / MAX_Y);
    plan->slots = slots_of(L);
    return HJ_OK;
}

int hjv_decode(const hjh_grid* g, int64_t node, int32_t idx[6]) {
    long long total = 0;
    if (int rc = check_grid(g, total)) return rc;
    if (!idx) return fail(HJ_EINVAL, "null argument");
    if (int rc = check_node(node, total)) return rc;
    Limits lim;
    if (int rc = read_limits(lim, BLOCK)) return rc;
    Index X;
    const Plan L = make_plan(g, total, BLOCK, X, lim);
    decode(L, X, g->ndim, node, idx);
    return HJ_OK;
}

int hjv_simplex_q_host(int D, const double* f, uint64_t* q) {
    if (D < 1 || D > MD) return fail(HJ_EINVAL, "D = %d: simplices of 1 .. %d dimensions", D, MD);
    if (!f || !q) return fail(HJ_EINVAL, "null argument");
    for (int k = 0; k <= D; ++k)
        if (!std::isfinite(f[k])) return fail(HJ_EINVAL, "f[%d] is not finite: such a cell is invalid and has no simplex", k);
    *q = dispatch_ndim(D, [&](auto d) { return simplex_host<decltype(d)::value>(f); });
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjv)

}  // extern "C"
