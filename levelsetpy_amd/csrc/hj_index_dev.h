// The node walk of the libraries on grids of 1 to 6 dimensions (hj_hishapes.hip, hj_resample.hip, hj_measure.hip), written once:
// NOTHING here divides or takes a remainder by a run-time extent on the device, in 32 or in 64 bits.
//   * the host splits the axes into a tail (the longest suffix with fewer than 2^31 nodes) and a head; a workgroup owns `block`
//     consecutive tail nodes of ONE head index, so blockIdx.x = head' * chunks + chunk and every linear index is below 2^32;
//   * a launch has fewer than 2^32 THREADS: the runtime takes gridDim.x * blockDim.x modulo 2^32 and says nothing, so a launch
//     of 2^24 workgroups of 256 or more runs only the first (gridDim.x * 256) mod 2^32 threads.  (Measured on a grid of
//     4 305 300 000 nodes: one launch of 16 817 580 workgroups stored 10 333 184 nodes, profiles/node_walk_head.txt.)  A head
//     index is at most 2^23 workgroups, so whole head indices always fit and a grid past 2^32 nodes takes several launches;
//   * `quotient` divides a 32-bit value by an extent with the 64-bit reciprocal the host prepared: one multiply-high, exact for
//     every 32-bit dividend;
//   * blockIdx.x is split, and the head index decoded, ONCE per wave from wave-uniform values (scalar registers): the head index
//     of a launch's first workgroup arrives decoded (the host divides) and head' is added to it with carry;
//   * every lane divides its OWN tail node through the tail axes, on the vector unit.  Decoding the wave's first node on the
//     scalar unit and moving the lanes on by add-and-carry was built first and measured slower (profiles/hishapes_timing.txt).
// `split_block` and `node_index` are __host__ __device__: `decode` runs them on the host for any node of any grid, which is what
// hjk_decode, hjm_decode and hjv_decode return.
#ifndef HJ_INDEX_DEV_H
#define HJ_INDEX_DEV_H
#include <hip/hip_runtime.h>
#include <cerrno>
#include <cstdlib>
#include "../../include/hj_hidim.h"

namespace hj_index {

constexpr int AXES = HJH_MAX_DIM;

// what the decode reads: the extents (1 past ndim), their reciprocals and the split of blockIdx.x; a kernel argument
struct Index {
    unsigned long long recip[AXES];         // floor(2^64 / n) + 1 for n > 1 (2^64 / n for a power of two): quotient
    unsigned long long chunk_recip;         // the same of `chunks`
    unsigned n[AXES];                       // nodes per axis
    unsigned h0[AXES];                      // multi-index of this launch's first head index (tail axes: 0)
    unsigned chunks;                        // workgroups per head index
    unsigned tail;                          // nodes of the tail, below 2^31
    int first_tail;                         // axes first_tail .. AXES - 1 are the tail
};

// floor(v / n) for any 32-bit v by the reciprocal r = floor(2^64 / n) + 1 of n > 1: the high 64 bits of v * r, exact because
// v * (r * n - 2^64) <= v * n < 2^64
__host__ __device__ __forceinline__ unsigned quotient(unsigned v, unsigned long long r) {
    const unsigned long long lo = (unsigned long long)v * (unsigned)r;
    const unsigned long long hi = (unsigned long long)v * (unsigned)(r >> 32);
    return (unsigned)((hi + (lo >> 32)) >> 32);
}

// blockIdx.x = head' * chunks + chunk -> head' (the head index counted from this launch's first) and the chunk; wave-uniform
__host__ __device__ __forceinline__ void split_block(const Index& X, unsigned block, unsigned& hl, unsigned& chunk) {
    hl = block;
    chunk = 0u;
    if (X.chunks > 1u) {
        hl = quotient(block, X.chunk_recip);
        chunk = block - hl * X.chunks;
    }
}

// The multi-index of tail node t of head index h0 + hl on a grid of ND axes.  The tail axes divide t, a lane's own value: vector
// arithmetic, one multiply-high per axis.  The head axes add hl to the launch's first head index with carry: wave-uniform, scalar
// arithmetic.
template <int ND>
__host__ __device__ __forceinline__ void node_index(const Index& X, unsigned hl, unsigned t, unsigned (&idx)[ND]) {
    unsigned up = hl;
#pragma unroll
    for (int d = ND - 1; d >= 0; --d) {
        if (d > X.first_tail) {                                  // a tail axis below the tail's first: divide the tail node
            idx[d] = 0u;
            if (X.n[d] > 1u) {
                const unsigned q = quotient(t, X.recip[d]);
                idx[d] = t - q * X.n[d];
                t = q;
            }
        } else if (d == X.first_tail) {
            idx[d] = t;
        } else if (d > 0) {                                      // a head axis: the launch's first head index plus head', with carry
            const unsigned v = X.h0[d] + up;                     // both below 2^31
            idx[d] = 0u;
            up = v;                                              // an axis of one node passes the carry on
            if (X.n[d] > 1u) {
                up = quotient(v, X.recip[d]);
                idx[d] = v - up * X.n[d];
            }
        } else {
            idx[0] = X.h0[0] + up;
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side
// Refusals go to the including library's own error record: hj_tool_host.h comes before this header.
#ifndef HJ_TOOL_HOST_H
#error "include hj_tool_host.h before hj_index_dev.h"
#endif

// the split of the axes and the launches along the head; an empty grid's plan is all zeros
struct Plan {
    int first_tail;
    int block;                              // threads of a workgroup
    long long total, tail, head;            // nodes of the grid; of the tail; head indices: total = head * tail
    long long chunks;                       // workgroups per head index
    long long heads_per_launch, launches;   // a launch ends below 2^32 threads (LAUNCH_THREADS)
    long long blocks_full, blocks_last;     // gridDim.x of every launch but the last, and of the last
};

static unsigned long long recip64(unsigned n) { return n > 1u ? 0xffffffffffffffffull / n + 1ull : 0ull; }

// The plan's two limits: the tail has fewer than `tail_below` nodes and a launch at most `launch_blocks` workgroups.  A test
// facility lowers them through the environment, so that small grids take the head axes' carry, the 64-bit node and the walk
// over several launches; unset they are the constants below.
constexpr long long LAUNCH_THREADS = 0xffffffffll;           // threads of one launch at most: see the head of this file
struct Limits {
    long long tail_below = 0x80000000ll;
    long long launch_blocks = LAUNCH_THREADS / 256;
};

static int read_limit(const char* name, long long& limit) {
    const char* text = std::getenv(name);
    if (!text) return HJ_OK;
    char* end = nullptr;
    errno = 0;
    const long long v = std::strtoll(text, &end, 10);
    if (end == text || *end || errno || v < 1 || v > limit)
        return hj_tool::fail(HJ_EINVAL, "%s = '%s': a whole number from 1 to %lld", name, text, limit);
    limit = v;
    return HJ_OK;
}

// the limits of one entry call, read once: its plan, its decode and its launches see the same
static int read_limits(Limits& lim, int block) {
    lim = Limits{};
    lim.launch_blocks = LAUNCH_THREADS / block;
    if (int rc = read_limit("HJ_INDEX_TAIL_BELOW", lim.tail_below)) return rc;
    return read_limit("HJ_INDEX_LAUNCH_BLOCKS", lim.launch_blocks);
}

// the plan of a grid of `total` nodes for workgroups of `block` threads, and what the decode reads of it (X.h0 is set per launch)
static Plan make_plan(const hjh_grid* g, long long total, int block, Index& X, const Limits& lim) {
    Plan L{};
    X = Index{};
    for (int d = 0; d < AXES; ++d) {
        X.n[d] = d < g->ndim ? (unsigned)g->N[d] : 1u;
        X.recip[d] = recip64(X.n[d]);
    }
    L.block = block;
    L.total = total;
    if (total == 0) return L;
    long long tail = 1;
    int ft = AXES;
    // the grid's last axis is the tail's whatever the limit: it always fits the constant, and a lowered limit at or below its
    // extent counts as just above it
    while (ft > 0 && (ft >= g->ndim || tail * (long long)X.n[ft - 1] < lim.tail_below)) tail *= (long long)X.n[--ft];
    L.first_tail = ft;
    L.tail = tail;
    L.head = total / tail;
    L.chunks = (tail + block - 1) / block;
    L.heads_per_launch = std::min<long long>(L.head, std::max<long long>(1, lim.launch_blocks / L.chunks));   // a launch holds a whole head index
    L.launches = (L.head + L.heads_per_launch - 1) / L.heads_per_launch;
    L.blocks_full = L.heads_per_launch * L.chunks;
    L.blocks_last = (L.head - (L.launches - 1) * L.heads_per_launch) * L.chunks;
    if (L.launches == 1) L.blocks_full = L.blocks_last;
    X.chunks = (unsigned)L.chunks;
    X.chunk_recip = recip64(X.chunks);
    X.tail = (unsigned)tail;
    X.first_tail = ft;
    return L;
}

// the plan's fields as a library's public plan struct (hjk_ / hjm_ / hjv_launch_plan) names them; the library adds its own
template <typename PUBLIC>
static void publish(const Plan& L, PUBLIC& out) {
    out = PUBLIC{};
    out.first_tail = L.first_tail;
    out.total = L.total;
    out.tail = L.tail;
    out.head = L.head;
    out.chunks = L.chunks;
    out.heads_per_launch = L.heads_per_launch;
    out.launches = L.launches;
    out.blocks_full = L.blocks_full;
    out.blocks_last = L.blocks_last;
}

// the multi-index of head index `head` into X.h0: the one place that divides, on the host
static void set_head(Index& X, long long head) {
    for (int d = AXES - 1; d >= 0; --d) {
        X.h0[d] = 0u;
        if (d < X.first_tail) {
            X.h0[d] = (unsigned)(head % (long long)X.n[d]);
            head /= (long long)X.n[d];
        }
    }
}

// every launch along the head: X.h0 and node0 (the flat node of the launch's first head index at tail node 0) are set, then
// launch(blocks) runs with the launch's gridDim.x; its first non-zero return ends the walk
template <typename F>
static int head_launches(const Plan& L, Index& X, long long& node0, F&& launch) {
    for (long long l = 0; l < L.launches; ++l) {
        const long long head = l * L.heads_per_launch;
        set_head(X, head);
        node0 = head * L.tail;
        if (int rc = launch((unsigned)(l + 1 < L.launches ? L.blocks_full : L.blocks_last))) return rc;
    }
    return HJ_OK;
}

static int check_node(long long node, long long total) {
    if (node < 0 || node >= total) return hj_tool::fail(HJ_EINVAL, "node %lld: the grid has nodes 0 .. %lld", node, total - 1);
    return HJ_OK;
}

// The multi-index of flat node `node` by the launch, workgroup and thread that own it, as head_launches and the kernels lay them
// out, decoded at `ndim` axes (the kernel's own number); idx past ndim is 0.
static void decode(const Plan& L, Index& X, int ndim, long long node, int32_t idx[AXES]) {
    const long long head = node / L.tail, t = node % L.tail;
    const long long launch = head / L.heads_per_launch;
    set_head(X, launch * L.heads_per_launch);
    const unsigned block = (unsigned)((head - launch * L.heads_per_launch) * L.chunks + t / L.block);
    const unsigned lane = (unsigned)(t % L.block);
    for (int d = 0; d < AXES; ++d) idx[d] = 0;
    hj_tool::dispatch_ndim(ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        unsigned own[ND], hl = 0u, chunk = 0u;
        split_block(X, block, hl, chunk);
        node_index<ND>(X, hl, chunk * (unsigned)L.block + lane, own);
        for (int d = 0; d < ND; ++d) idx[d] = (int32_t)own[d];
    });
}

}  // namespace hj_index
#endif
