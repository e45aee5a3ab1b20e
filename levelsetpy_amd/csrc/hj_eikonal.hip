// libhj_eikonal.so (include/hj_eikonal.h): signed distance and first-arrival time from a level set, for gfx950.
//   eikonal_init_kernel<T>    rule 1 of the header: a thread owns one node of one member (blockIdx.y the member), writes the
//                             fp64 work array, marks the tiles a near node can reach and votes the member's sign flags.
//   eikonal_tile_kernel<D>    rule 2, the hot path: one workgroup per tile, one thread per node.  A tile that is not marked
//                             returns at once; a marked one stages itself and a one-node halo in LDS and relaxes all its nodes
//                             between barriers until none changes, then writes what changed and marks the tiles across the
//                             faces its changed nodes lie on.  The host launches it once per pass over all tiles.
//   eikonal_finish_kernel<T>  rule 3: sign, band, walls, one rounding; one element per lane, so views at any offset work.
// The work array holds, per node: NaN a wall; -u (sign bit set, -0.0 included) a near node, frozen; otherwise the current
// value, +inf at first.  No mask array exists.
// Tiles of one pass read each other's halo from global memory while those values are being written.  That is allowed because
// values only decrease and a tile that wrote a face value marks the tile behind that face for the NEXT pass (another launch,
// so the reader then sees it): a stale read costs a pass, never a result.  It REQUIRES every access to the work array to be
// one aligned 8-byte load or store, never two halves: the array is addressed as double only, from an 8-byte aligned base,
// and nothing here reads or writes it through a narrower or a wider type.
// A tile does not mark itself unless it left its loop at the trip-count cap: having converged against the halo it staged, it
// has nothing to do until a neighbour marks it.
// Every branch on tile, member or pass is wave-uniform (blockIdx and kernel arguments only); rule 2 itself is branch-free.
// Every device function is one operation per statement with contraction off: the results are the restatement's.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hj_tool_host.h"
#include "../../include/hj_eikonal.h"

namespace hje {

using namespace hj_tool;

constexpr int BLOCK = 256;              // the flat kernels
constexpr long long MAX_Y = 65535;      // gridDim.y of one launch
constexpr int GROUP = 8;                // passes between two reads of the counters
#define HJE_INF __builtin_inf()

// tiles: 256 | 16 x 32 | 4 x 8 x 16 | 4 x 4 x 4 x 8, the last axis longest so that global rows coalesce
__host__ __device__ constexpr int tile_dim(int D, int d) {
    return d >= D ? 1 : D == 1 ? 256 : D == 2 ? (d == 0 ? 16 : 32) : D == 3 ? (d == 0 ? 4 : d == 1 ? 8 : 16) : (d == 3 ? 8 : 4);
}
__host__ __device__ constexpr int tile_nodes(int D) { return tile_dim(D, 0) * tile_dim(D, 1) * tile_dim(D, 2) * tile_dim(D, 3); }
__host__ __device__ constexpr int halo_cells(int D) {
    return (tile_dim(D, 0) + 2) * (D > 1 ? tile_dim(D, 1) + 2 : 1) * (D > 2 ? tile_dim(D, 2) + 2 : 1) * (D > 3 ? tile_dim(D, 3) + 2 : 1);
}

struct Args {
    double* work;                       // K x total
    int* cur;                           // K x ntiles: the tiles of this pass
    int* next;                          // K x ntiles: the tiles of the next one
    unsigned long long* counters;
    int* signs;                         // K
    const void* data;
    const double* speed;                // total, or null
    void* out;
    double speed_scalar, s_scalar;      // s_scalar = 1 / speed_scalar
    double level, band;
    double h[HJ_MAX_DIM], w[HJ_MAX_DIM];        // dx and 1 / (dx * dx)
    long long stride[HJ_MAX_DIM];       // elements between neighbours along an axis
    long long total, field_stride, k0;
    int n[HJ_MAX_DIM], nt[HJ_MAX_DIM], td[HJ_MAX_DIM], periodic[HJ_MAX_DIM];
    int ndim, ntiles, pass;
};

// the node's index per axis, last axis fastest; 32-bit divisions whenever the grid allows them
__device__ __forceinline__ void node_index(const Args& A, long long node, int (&idx)[HJ_MAX_DIM]) {
    if (A.total <= 0xffffffffll) {
        unsigned r = (unsigned)node;
#pragma unroll
        for (int d = HJ_MAX_DIM - 1; d >= 1; --d) {
            if (d < A.ndim) {
                const unsigned q = r / (unsigned)A.n[d];
                idx[d] = (int)(r - q * (unsigned)A.n[d]);
                r = q;
            }
        }
        idx[0] = (int)r;
    } else {
        long long r = node;
#pragma unroll
        for (int d = HJ_MAX_DIM - 1; d >= 1; --d) {
            if (d < A.ndim) {
                const long long q = r / A.n[d];
                idx[d] = (int)(r - q * A.n[d]);
                r = q;
            }
        }
        idx[0] = (int)r;
    }
}

// ---------------------------------------------------------------------------------------------- rule 1
template <typename T>
__global__ __launch_bounds__(BLOCK) void eikonal_init_kernel(const Args A) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const long long member = A.k0 + blockIdx.y;
    const long long t = blockIdx.x * (long long)BLOCK + tid;
    const bool inside = t < A.total;
    const long long node = inside ? t : A.total - 1;             // a thread past the end looks at the last node and stores nothing
    int idx[HJ_MAX_DIM] = {0, 0, 0, 0};
    node_index(A, node, idx);

    const T* __restrict__ data = (const T*)A.data + member * A.field_stride;
    const double phi = (double)data[node] - A.level;
    const double sp = A.speed ? A.speed[node] : A.speed_scalar;
    const bool wall = (phi != phi) || !(sp > 0.0);
    const bool pos = phi > 0.0;

    double S = 0.0;
    bool crossing = false;
#pragma unroll
    for (int d = 0; d < HJ_MAX_DIM; ++d) {
        if (d < A.ndim) {
            double td = HJE_INF;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                long long j = -1;
                if (side == 0) {
                    if (idx[d] > 0) j = node - A.stride[d];
                    else if (A.periodic[d]) j = node + (A.n[d] - 1) * A.stride[d];
                } else {
                    if (idx[d] < A.n[d] - 1) j = node + A.stride[d];
                    else if (A.periodic[d]) j = node - (A.n[d] - 1) * A.stride[d];
                }
                if (j >= 0) {
                    const double pj = (double)data[j] - A.level;
                    const double sj = A.speed ? A.speed[j] : A.speed_scalar;
                    const bool wall_j = (pj != pj) || !(sj > 0.0);
                    if (!wall && !wall_j && pos != (pj > 0.0)) {
                        const double ai = __builtin_fabs(phi);
                        const double num = A.h[d] * ai;
                        const double diff = phi - pj;
                        const double den = __builtin_fabs(diff);
                        double tt = num / den;
                        if (ai == HJE_INF || __builtin_fabs(pj) == HJE_INF) tt = A.h[d] / 2.0;
                        td = tt < td ? tt : td;
                    }
                }
            }
            if (td < HJE_INF) {
                const double q = td * td;
                const double r = 1.0 / q;
                S = crossing ? S + r : r;
                crossing = true;
            }
        }
    }
    const double s = 1.0 / sp;
    const double root = __builtin_sqrt(S);
    double u = s / root;
    const bool zero = phi == 0.0;
    if (zero) u = 0.0;
    const bool near = !wall && (zero || crossing);
    const double stored = wall ? __builtin_nan("") : (near ? -u : HJE_INF);
    if (inside) A.work[member * A.total + t] = stored;

    // the tiles this near node can change: its own, and the one behind every tile face it lies on
    if (inside && near && u < A.band) {
        int* next = A.next + member * A.ntiles;
        int tile = 0, tc[HJ_MAX_DIM] = {0, 0, 0, 0}, ts[HJ_MAX_DIM] = {0, 0, 0, 0};
#pragma unroll
        for (int d = 0; d < HJ_MAX_DIM; ++d) {
            if (d < A.ndim) {
                tc[d] = idx[d] / A.td[d];
                tile = tile * A.nt[d] + tc[d];
            }
        }
        int run = 1;
#pragma unroll
        for (int d = HJ_MAX_DIM - 1; d >= 0; --d) {
            if (d < A.ndim) {
                ts[d] = run;
                run *= A.nt[d];
            }
        }
        next[tile] = 1;
#pragma unroll
        for (int d = 0; d < HJ_MAX_DIM; ++d) {
            if (d < A.ndim) {
                const int l = idx[d] - tc[d] * A.td[d];
                if (l == 0) {
                    if (tc[d] > 0) next[tile - ts[d]] = 1;
                    else if (A.periodic[d]) next[tile + (A.nt[d] - 1) * ts[d]] = 1;
                }
                if (l == A.td[d] - 1 || idx[d] == A.n[d] - 1) {
                    if (tc[d] < A.nt[d] - 1) next[tile + ts[d]] = 1;
                    else if (A.periodic[d]) next[tile - (A.nt[d] - 1) * ts[d]] = 1;
                }
            }
        }
    }

    // the signs the member's nodes showed: one vote per wave, and an atomic only when it would add a bit
    const int mine = (inside && !wall) ? (phi < 0.0 ? HJE_NEG : (pos ? HJE_POS : HJE_ZERO)) : 0;
    const int seen = (__any(mine & HJE_NEG) ? HJE_NEG : 0) | (__any(mine & HJE_POS) ? HJE_POS : 0) | (__any(mine & HJE_ZERO) ? HJE_ZERO : 0);
    if ((tid & 63) == 0 && seen) {
        int* f = A.signs + member;
        if (seen & ~__atomic_load_n(f, __ATOMIC_RELAXED)) atomicOr(f, seen);
    }
}

// ---------------------------------------------------------------------------------------------- rule 2
// (a, h, w) sorted ascending by a, ties in axis order: adjacent exchanges on strict > only, so the sort is stable
template <int D>
__device__ __forceinline__ void sort_axes(double (&a)[D], double (&h)[D], double (&w)[D]) {
#pragma unroll
    for (int end = D - 1; end >= 1; --end) {
#pragma unroll
        for (int i = 0; i < end; ++i) {
            const bool swap = a[i] > a[i + 1];
            const double a0 = swap ? a[i + 1] : a[i], a1 = swap ? a[i] : a[i + 1];
            const double h0 = swap ? h[i + 1] : h[i], h1 = swap ? h[i] : h[i + 1];
            const double w0 = swap ? w[i + 1] : w[i], w1 = swap ? w[i] : w[i + 1];
            a[i] = a0, a[i + 1] = a1, h[i] = h0, h[i + 1] = h1, w[i] = w0, w[i + 1] = w1;
        }
    }
}

// the new value of a node with sorted neighbour minima a, its old value and s = 1 / speed
template <int D>
__device__ __forceinline__ double relax(const double (&a)[D], const double (&h)[D], const double (&w)[D], double s, double band, double old) {
#pragma clang fp contract(off)
    const double step = h[0] * s;
    double cand = a[0] + step;
    bool done = D == 1 ? true : cand <= a[1];
    double Asum = w[0], B = 0.0, Q = 0.0;
    const double ss = s * s;
#pragma unroll
    for (int k = 1; k < D; ++k) {                       // candidate_{k+1} of the header
        const double b = a[k] - a[0];
        const double p = w[k] * b;
        Asum = Asum + w[k];
        B = B + p;
        const double pb = p * b;
        Q = Q + pb;
        const double C = Q - ss;
        const double BB = B * B;
        const double AC = Asum * C;
        const double disc = BB - AC;
        const double root = __builtin_sqrt(disc);
        const double num = B + root;
        const double quot = num / Asum;
        const double c = a[0] + quot;
        cand = done ? cand : c;
        done = done || (k == D - 1 ? true : c <= a[k + 1]);
    }
    const bool take = a[0] < HJE_INF && cand <= band && cand < old;       // a NaN candidate fails both comparisons
    return take ? cand : old;
}

template <int D>
__global__ __launch_bounds__(tile_nodes(D)) void eikonal_tile_kernel(const Args A) {
    constexpr int NT = tile_nodes(D), CELLS = halo_cells(D);
    __shared__ double lds[CELLS];
    const int tid = threadIdx.x;
    const long long member = A.k0 + blockIdx.y;
    const int tile = blockIdx.x;
    int* cur = A.cur + member * A.ntiles;
    if (cur[tile] == 0) return;                          // not marked for this pass: the whole workgroup leaves

    int tc[D], o[D], ts[D];
    {
        int r = tile, run = 1;
#pragma unroll
        for (int d = D - 1; d >= 0; --d) {
            const int q = r / A.nt[d];
            tc[d] = r - q * A.nt[d];
            r = q;
            o[d] = tc[d] * tile_dim(D, d);
            ts[d] = run;
            run *= A.nt[d];
        }
    }
    double* work = A.work + member * A.total;

    // the tile and a one-node halo: periodic wrap applied here, nodes off the grid and walls staged as +inf, frozen values as u.
    // Cells in the halo of two axes at once are no node's neighbour and are not loaded.
    for (int c = tid; c < CELLS; c += NT) {
        int r = c, l[D];
#pragma unroll
        for (int d = D - 1; d >= 0; --d) {
            const int L = tile_dim(D, d) + 2;
            l[d] = r % L;
            r /= L;
        }
        long long gi = 0;
        bool ok = true;
        int halos = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            int g = o[d] + l[d] - 1;
            halos += (l[d] == 0 || l[d] == tile_dim(D, d) + 1) ? 1 : 0;
            if (g < 0) {
                ok = ok && A.periodic[d];
                g = A.n[d] - 1;
            } else if (g >= A.n[d]) {
                ok = ok && A.periodic[d] && g == A.n[d];
                g = 0;
            }
            gi = gi * A.n[d] + g;
        }
        double v = HJE_INF;
        if (ok && halos <= 1) {
            const double raw = work[gi];
            v = raw != raw ? HJE_INF : __builtin_fabs(raw);
        }
        lds[c] = v;
    }

    // this thread's node
    int ld[D], me = 0, nb[D];
    long long gi = 0;
    bool in_grid = true;
    {
        int r = tid, run = 1;
#pragma unroll
        for (int d = D - 1; d >= 0; --d) {
            ld[d] = r % tile_dim(D, d);
            r /= tile_dim(D, d);
            nb[d] = run;                                  // LDS cells between neighbours along axis d
            me += (ld[d] + 1) * run;
            run *= tile_dim(D, d) + 2;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int g = o[d] + ld[d];
            in_grid = in_grid && g < A.n[d];
            gi = gi * A.n[d] + g;
        }
    }
    const double orig = in_grid ? work[gi] : __builtin_nan("");
    const bool live = orig > 0.0;                        // not frozen (sign bit), not a wall (NaN), on the grid
    double s = 1.0;
    if (live) s = A.speed ? 1.0 / A.speed[gi] : A.s_scalar;
    double val = orig;

    __syncthreads();
    if (tid == 0) cur[tile] = 0;                         // every wave has read the mark: clear it for the pass after next

    // relax all nodes against the values of the last barrier until none changes.  A value moves one node per trip, and no
    // path inside the tile is longer than its node count: the cap below bounds the loop whatever the data.
    bool more = true;
    for (int trip = 0; trip < NT && more; ++trip) {
        bool changed = false;
        if (live) {
            double a[D], h[D], w[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double lo = lds[me - nb[d]], hi = lds[me + nb[d]];
                a[d] = lo < hi ? lo : hi;
                h[d] = A.h[d];
                w[d] = A.w[d];
            }
            sort_axes<D>(a, h, w);
            const double nv = relax<D>(a, h, w, s, A.band, val);
            changed = nv < val;
            val = nv;
        }
        __syncthreads();                                 // every read of this trip is done
        if (changed) lds[me] = val;
        more = __syncthreads_or(changed) != 0;
    }

    const bool wrote = live && val < orig;
    if (wrote) {
        work[gi] = val;                                  // one aligned 8-byte store
        if (val < A.band) {                              // a neighbour of this node can still improve: mark the tiles that stage it
            int* next = A.next + member * A.ntiles;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (ld[d] == 0) {
                    if (tc[d] > 0) next[tile - ts[d]] = 1;
                    else if (A.periodic[d]) next[tile + (A.nt[d] - 1) * ts[d]] = 1;
                }
                if (ld[d] == tile_dim(D, d) - 1 || o[d] + ld[d] == A.n[d] - 1) {
                    if (tc[d] < A.nt[d] - 1) next[tile + ts[d]] = 1;
                    else if (A.periodic[d]) next[tile - (A.nt[d] - 1) * ts[d]] = 1;
                }
            }
        }
    }
    const int any = __syncthreads_or(wrote);
    if (tid == 0) {
        atomicAdd(A.counters + 0, 1ull);
        if (any) {
            atomicAdd(A.counters + 1, 1ull);
            atomicMax(A.counters + 2, (unsigned long long)(A.pass + 1));
        }
        if (more) (A.next + member * A.ntiles)[tile] = 1;            // left at the cap, still changing: go on next pass
    }
}

// ---------------------------------------------------------------------------------------------- rule 3
template <typename T>
__global__ __launch_bounds__(BLOCK) void eikonal_finish_kernel(const Args A) {
    const long long member = A.k0 + blockIdx.y;
    const long long t = blockIdx.x * (long long)BLOCK + threadIdx.x;
    if (t >= A.total) return;
    const double raw = A.work[member * A.total + t];
    const double phi = (double)((const T*)A.data)[member * A.field_stride + t] - A.level;
    const double u = __builtin_fabs(raw);
    const double v = u < A.band ? u : A.band;
    double r = phi > 0.0 ? v : (phi < 0.0 ? -v : 0.0);
    if (raw != raw) r = raw;
    ((T*)A.out)[member * A.total + t] = (T)r;
}

// ---------------------------------------------------------------------------------------------- host side
struct Layout {
    long long total, ntiles, header, work_at, flags_at, bytes;
    int nt[HJ_MAX_DIM];
};

static int check_grid(const hjq_grid* g, int64_t K, Layout& L) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->ndim < 1 || g->ndim > HJ_MAX_DIM) return fail(HJ_EINVAL, "ndim %d: grids of 1 .. %d dimensions", g->ndim, HJ_MAX_DIM);
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "dtype %d: fp64 (%d) or fp32 (%d)", g->dtype, (int)HJ_F64, (int)HJ_F32);
    if (K < 1) return fail(HJ_EINVAL, "K = %lld: at least one member", (long long)K);
    L.total = 1;
    L.ntiles = 1;
    for (int d = 0; d < HJ_MAX_DIM; ++d) L.nt[d] = 1;
    for (int d = 0; d < g->ndim; ++d) {
        if (g->N[d] < 0 || g->N[d] > 0x7fffffffll) return fail(HJ_EINVAL, "N[%d] = %lld: 0 .. 2^31 - 1 nodes per axis", d, (long long)g->N[d]);
        if (!(g->dx[d] > 0.0) || g->dx[d] == HJE_INF) return fail(HJ_EINVAL, "dx[%d] = %g: a positive finite spacing", d, g->dx[d]);
        if (g->bc[d] != HJ_BC_EXTRAPOLATE && g->bc[d] != HJ_BC_PERIODIC) return fail(HJ_EINVAL, "bc[%d] = %d: extrapolate (%d) or periodic (%d)", d, g->bc[d], (int)HJ_BC_EXTRAPOLATE, (int)HJ_BC_PERIODIC);
        if (L.total && g->N[d] > 0x7fffffffffffffffll / L.total) return fail(HJ_EINVAL, "the grid has more than 2^63 - 1 nodes");
        L.total *= g->N[d];
        const int td = tile_dim(g->ndim, d);
        const long long nt = (g->N[d] + td - 1) / td;
        L.nt[d] = (int)nt;
        L.ntiles *= nt;
        if (L.ntiles > 0x7fffffffll) return fail(HJ_EINVAL, "the grid has more than 2^31 - 1 tiles");
    }
    if (L.total && K > 0x0fffffffffffffffll / L.total) return fail(HJ_EINVAL, "K x nodes exceeds 2^60");
    if (L.total > 0x7fffffffll * (long long)BLOCK) return fail(HJ_EINVAL, "too many nodes for one launch");
    L.header = (HJE_FLAGS_OFFSET + 4 * K + 255) / 256 * 256;
    L.work_at = L.header;
    L.flags_at = (L.work_at + 8 * K * L.total + 255) / 256 * 256;
    L.bytes = L.flags_at + (2 * 4 * K * L.ntiles + 255) / 256 * 256;
    return HJ_OK;
}

template <typename Kernel>
static int launch_members(Kernel kernel, Args& A, int64_t K, unsigned blocks, unsigned threads, hipStream_t stream) {
    for (long long k0 = 0; k0 < K; k0 += MAX_Y) {               // gridDim.y ends at 65535: further members take further launches
        const long long nk = K - k0 < MAX_Y ? K - k0 : MAX_Y;
        A.k0 = k0;
        hipLaunchKernelGGL(kernel, dim3(blocks, (unsigned)nk), dim3(threads), 0, stream, A);
        HIP_TRY(hipGetLastError());
    }
    return HJ_OK;
}

template <int D>
static int tile_pass(Args& A, int64_t K, hipStream_t stream) {
    return launch_members(eikonal_tile_kernel<D>, A, K, (unsigned)A.ntiles, (unsigned)tile_nodes(D), stream);
}

// The counters' landing place on the host: 64 bytes of pinned memory per calling thread, allocated at its first call and
// kept (a call must not pay an allocation and hipHostFree's device-wide wait for a 24-byte read-back).  It holds nothing
// between calls.
static int pinned_counters(unsigned long long*& p) {
    static thread_local unsigned long long* mine = nullptr;
    if (!mine) HIP_TRY(hipHostMalloc((void**)&mine, 64, hipHostMallocPortable));
    p = mine;
    return HJ_OK;
}

template <typename T>
static int solve(Args& A, int64_t K, int64_t max_passes, int64_t* passes_host, hipStream_t stream) {
    unsigned blocks;
    int rc = blocks_for(A.total, "too many nodes for one launch", blocks);
    if (rc) return rc;
    unsigned long long* host = nullptr;
    rc = pinned_counters(host);
    if (rc) return rc;
    const bool f64 = sizeof(T) == 8;
    rc = launch_members(eikonal_init_kernel<T>, A, K, blocks, BLOCK, stream);     // marks A.next: the tiles of pass 0
    if (rc) return rc;
    static const char* const TILE_NAMES[] = {"", "eikonal_tile_kernel<1>", "eikonal_tile_kernel<2>", "eikonal_tile_kernel<3>", "eikonal_tile_kernel<4>"};
    long long launched_passes = 0, last = 0;
    for (;;) {
        const long long group = max_passes - launched_passes < GROUP ? max_passes - launched_passes : GROUP;
        for (long long p = 0; p < group; ++p) {
            int* t = A.cur;                                       // the flag arrays take turns
            A.cur = A.next;
            A.next = t;
            A.pass = (int)(launched_passes + p);
            rc = A.ndim == 1 ? tile_pass<1>(A, K, stream) : A.ndim == 2 ? tile_pass<2>(A, K, stream) : A.ndim == 3 ? tile_pass<3>(A, K, stream) : tile_pass<4>(A, K, stream);
            if (rc) return rc;
        }
        launched_passes += group;
        HIP_TRY(hipMemcpyAsync(host, A.counters, 24, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        last = (long long)host[2];
        if (last < launched_passes) break;                        // the last pass launched changed nothing: the fixed point
        if (launched_passes >= max_passes)
            return fail(HJ_ESTATE, "not converged after max_passes = %lld passes (the last one still changed values): walls that make a maze need a larger max_passes",
                        (long long)max_passes);
    }
    if (passes_host) *passes_host = last + 1;
    rc = launch_members(eikonal_finish_kernel<T>, A, K, blocks, BLOCK, stream);
    if (rc) return rc;
    launched(f64 ? "eikonal_init_kernel<double>" : "eikonal_init_kernel<float>");
    launched_also(TILE_NAMES[A.ndim]);
    launched_also(f64 ? "eikonal_finish_kernel<double>" : "eikonal_finish_kernel<float>");
    return HJ_OK;
}

}  // namespace hje

using namespace hje;

extern "C" {

int hje_workspace_size(const hjq_grid* g, int64_t K, int64_t* bytes) {
    Layout L;
    int rc = check_grid(g, K, L);
    if (rc) return rc;
    if (!bytes) return fail(HJ_EINVAL, "null argument");
    *bytes = L.bytes;
    return HJ_OK;
}

int hje_signed_distance(const hjq_grid* g, const void* data, int64_t K, int64_t field_stride, double level, double band,
                        const double* speed, double speed_scalar, void* out, void* workspace, int64_t workspace_bytes,
                        int64_t max_passes, int64_t* passes_host, void* stream) {
    Layout L;
    int rc = check_grid(g, K, L);
    if (rc) return rc;
    if (field_stride < L.total) return fail(HJ_EINVAL, "field_stride %lld is less than the %lld nodes of the grid", (long long)field_stride, L.total);
    if (level != level) return fail(HJ_EINVAL, "level is NaN");
    if (!(band > 0.0)) return fail(HJ_EINVAL, "band = %g: a positive width, +inf for none", band);
    if (max_passes < 1 || max_passes > 0x7ffffff0ll) return fail(HJ_EINVAL, "max_passes = %lld: 1 .. 2^31 - 16", (long long)max_passes);
    if (workspace_bytes < L.bytes) return fail(HJ_EINVAL, "workspace of %lld bytes: hje_workspace_size asks for %lld", (long long)workspace_bytes, L.bytes);
    if (passes_host) *passes_host = 0;
    if (L.total == 0) return HJ_OK;
    if (!data || !out || !workspace) return fail(HJ_EINVAL, "null argument");
    if ((uintptr_t)workspace % 8) return fail(HJ_EINVAL, "the workspace must be 8-byte aligned: the work array is read and written 8 bytes at a time");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    HIP_TRY(hipMemsetAsync(ws, 0, (size_t)L.header, st));
    HIP_TRY(hipMemsetAsync(ws + L.flags_at, 0, (size_t)(L.bytes - L.flags_at), st));
    Args A;
    A.counters = (unsigned long long*)ws;
    A.signs = (int*)(ws + HJE_FLAGS_OFFSET);
    A.work = (double*)(ws + L.work_at);
    A.cur = (int*)(ws + L.flags_at) + K * L.ntiles;              // swapped before pass 0: the init kernel marks A.next
    A.next = (int*)(ws + L.flags_at);
    A.data = data;
    A.speed = speed;
    A.out = out;
    A.speed_scalar = speed_scalar;
    A.s_scalar = 1.0 / speed_scalar;
    A.level = level;
    A.band = band;
    A.total = L.total;
    A.field_stride = field_stride;
    A.k0 = 0;
    A.ndim = g->ndim;
    A.ntiles = (int)L.ntiles;
    A.pass = 0;
    long long run = 1;
    for (int d = HJ_MAX_DIM - 1; d >= 0; --d) {
        const bool in = d < g->ndim;
        A.n[d] = in ? (int)g->N[d] : 1;
        A.nt[d] = L.nt[d];
        A.td[d] = tile_dim(g->ndim, d);
        A.periodic[d] = in && g->bc[d] == HJ_BC_PERIODIC;
        A.h[d] = in ? g->dx[d] : 1.0;
        const double hh = A.h[d] * A.h[d];
        A.w[d] = 1.0 / hh;
        A.stride[d] = run;
        if (in) run *= g->N[d];
    }
    if (g->dtype == HJ_F64) return solve<double>(A, K, max_passes, passes_host, st);
    return solve<float>(A, K, max_passes, passes_host, st);
}

HJ_TOOL_LAST_SYMBOLS(hje)

}  // extern "C"
