// libhj_surface.so (include/hj_surface.h): level sets of a value function as indexed meshes for gfx950.
// Marching simplices on the Kuhn subdivision: D! simplices per cell, one per permutation of the axes; phi is linear in a
// simplex, so the only table is the list of permutations, generated below at compile time.
//   classify_kernel<T, D>  per node: the mask of its active edges (2^D - 1 bits, the edges whose LOWER end it is) and
//                          the face count of the cell it is the lowest corner of; an exclusive scan of both inside the
//                          tile of 1024 nodes; the tile totals.  A tile where nothing crosses writes its two totals
//                          and nothing else.
//   scan_blocks_kernel     one workgroup per field: exclusive scan of the tile totals (int64), nv and nf
//   emit_kernel<T, D>      per node: its vertices at tile base + in-tile offset, the faces of its cell; a vertex index
//                          is base(lower node) + popcount(mask(lower node) & below(edge class))
// Coordinates keep the product and the sum apart (contraction off), as tests/surface_ref.py computes them.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hj_tool_host.h"
#include "../../include/hj_surface.h"

namespace hjs {

using namespace hj_tool;

constexpr int TPB = 256;                 // threads per workgroup
constexpr int ITEMS = 4;                 // nodes per thread in classify_kernel
constexpr int TILE = TPB * ITEMS;        // nodes per scan tile: 7 * 1024 vertices and 12 * 1024 faces fit 16 bits each
constexpr int SCAN_TPB = 1024;

// grid as the kernels see it (kernel argument: lives in SGPRs)
struct SGrid {
    int n[3];
    long long stride[3];
    double xmin[3], dx[3];
    long long nodes, ntiles;
};

// per-field workspace (all offsets in elements of the array's own type)
struct Work {
    long long* exclv;          // [ntiles + 1] tile totals, then their exclusive scan; [ntiles] = nv
    long long* exclf;          // [ntiles + 1] likewise for faces
    unsigned short* vloc;      // [nodes] vertices of the tile before this node
    unsigned short* floc;      // [nodes] faces of the tile before this node's cell
    unsigned char* mask;       // [nodes] active edges whose lower end is this node: bit (b & ~a) - 1
    unsigned char* fcnt;       // [nodes] faces of the cell whose corner 0 is this node
};

__host__ __device__ inline Work field_work(void* ws, long long nfields, long long f, long long nodes, long long ntiles) {
    Work W;
    long long* p = (long long*)ws;
    W.exclv = p + f * (ntiles + 1);
    W.exclf = p + (nfields + f) * (ntiles + 1);
    unsigned short* q = (unsigned short*)(p + 2 * nfields * (ntiles + 1));
    W.vloc = q + f * nodes;
    W.floc = q + (nfields + f) * nodes;
    unsigned char* r = (unsigned char*)(q + 2 * nfields * nodes);
    W.mask = r + f * nodes;
    W.fcnt = r + (nfields + f) * nodes;
    return W;
}

static size_t work_bytes(long long nfields, long long nodes, long long ntiles) {
    return (size_t)nfields * ((size_t)(ntiles + 1) * 16 + (size_t)nodes * 6);
}

// ---- the Kuhn subdivision: simplex s is the s-th permutation p of (0..D-1) in lexicographic order
template <int D> struct Kuhn {
    static constexpr int NS = D == 2 ? 2 : 6;
    unsigned chain[NS];        // corner numbers v0 .. vD, 3 bits each: v0 = 0, v_k = v_{k-1} | 1 << p[k-1]
    unsigned par;              // bit s: parity of p's inversion count
};

template <int D> __host__ __device__ constexpr Kuhn<D> make_kuhn() {
    Kuhn<D> K{};
    for (int s = 0; s < Kuhn<D>::NS; ++s) {
        int avail[D] = {};
        for (int d = 0; d < D; ++d) avail[d] = d;
        int left = D, r = s, f = 1, inv = 0;
        for (int d = 2; d < D; ++d) f *= d;                  // (D - 1)!
        unsigned v = 0, packed = 0;
        for (int k = 1; k <= D; ++k) {
            const int q = r / f;                             // the q-th of the axes still available
            r -= q * f;
            inv += q;
            v |= 1u << avail[q];
            packed |= v << (3 * k);
            for (int m = q; m + 1 < left; ++m) avail[m] = avail[m + 1];
            --left;
            if (left > 1) f /= left;
        }
        K.chain[s] = packed;
        K.par |= (unsigned)(inv & 1) << s;
    }
    return K;
}

static_assert(make_kuhn<2>().chain[0] == (1u << 3 | 3u << 6) && make_kuhn<2>().chain[1] == (2u << 3 | 3u << 6), "2-D simplices");
static_assert(make_kuhn<2>().par == 0b10u && make_kuhn<3>().par == 0b100110u, "permutation parities");
static_assert(make_kuhn<3>().chain[3] == (2u << 3 | 6u << 6 | 7u << 9), "simplex 3 is p = (1, 2, 0)");

__host__ __device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }

template <int D> __host__ __device__ __forceinline__ long long corner_offset(const SGrid& G, int c) {
    long long off = 0;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (c >> d & 1) off += G.stride[d];
    return off;
}

// The node's own value and those of the corners above it that exist: bit c of `valid` says corner c is a node of the grid,
// bit c of `in` that it is inside (phi <= level), bit c of `fin` that it is finite.
template <typename T, int D>
__host__ __device__ __forceinline__ void load_corners(const T* __restrict__ field, const SGrid& G, long long node, int* idx, double* p,
                                             unsigned& valid, unsigned& in, unsigned& fin, double level) {
    long long q = node;
#pragma unroll
    for (int d = D - 1; d > 0; --d) {
        const long long nq = q / G.n[d];
        idx[d] = (int)(q - nq * G.n[d]);
        q = nq;
    }
    idx[0] = (int)q;
    unsigned up = 0;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (idx[d] < G.n[d] - 1) up |= 1u << d;
    valid = in = fin = 0;
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
        p[c] = 0.0;
        if ((c & ~up) == 0) {
            const double v = (double)field[node + corner_offset<D>(G, c)];
            p[c] = v;
            valid |= 1u << c;
            if (v <= level) in |= 1u << c;
            if (finite(v)) fin |= 1u << c;
        }
    }
}

template <int D>
__host__ __device__ __forceinline__ void classify_node(unsigned valid, unsigned in, unsigned fin, unsigned& mask, unsigned& faces) {
    constexpr int NC = 1 << D;
    constexpr unsigned ALL = (1u << NC) - 1u;
    mask = faces = 0;
    const unsigned mixed = (in ^ (0u - (in & 1u))) & valid;          // corners on the other side than corner 0
    if (mixed == 0 && (fin & valid) == valid) return;               // nothing crosses here
    if (fin & 1u) mask = (mixed & fin) >> 1;                         // edge 0 - c: bit c - 1
    if (valid != ALL) return;                                        // no cell has this node as its corner 0
    constexpr Kuhn<D> K = make_kuhn<D>();
#pragma unroll
    for (int s = 0; s < Kuhn<D>::NS; ++s) {
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k <= D; ++k) bits |= 1u << (K.chain[s] >> (3 * k) & 7u);
        if ((fin & bits) != bits) continue;
        const int k = __builtin_popcount(in & bits);
        if (D == 3) faces += (k == 1 || k == 3) ? 1 : (k == 2 ? 2 : 0);
        else faces += (k == 1 || k == 2) ? 1 : 0;
    }
}

__device__ __forceinline__ unsigned wave_inclusive(unsigned x, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned y = __shfl_up(x, s, 64);
        if (lane >= s) x += y;
    }
    return x;
}

__device__ __forceinline__ long long wave_inclusive(long long x, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const long long y = __shfl_up(x, s, 64);
        if (lane >= s) x += y;
    }
    return x;
}

// ---- (a) classify: workgroup b of field blockIdx.y owns nodes [b * TILE, (b + 1) * TILE); thread t takes t, t + 256, ...
template <typename T, int D>
__global__ __launch_bounds__(TPB) void classify_kernel(const T* __restrict__ data, long long field_stride, long long nfields,
                                                       SGrid G, double level, void* __restrict__ ws) {
    const long long f = blockIdx.y;
    const T* __restrict__ field = data + f * field_stride;
    const Work W = field_work(ws, nfields, f, G.nodes, G.ntiles);
    const long long base = (long long)blockIdx.x * TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned packed[ITEMS], masks[ITEMS];
    unsigned any = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const long long node = base + k * TPB + tid;
        packed[k] = masks[k] = 0;
        if (node < G.nodes) {
            int idx[D];
            double p[1 << D];
            unsigned valid, in, fin, m, nfaces;
            load_corners<T, D>(field, G, node, idx, p, valid, in, fin, level);
            classify_node<D>(valid, in, fin, m, nfaces);
            masks[k] = m;
            packed[k] = (unsigned)__builtin_popcount(m) | nfaces << 16;         // vertices low, faces high: no carry between them in a tile
        }
        any |= packed[k];
    }
    if (!__syncthreads_or((int)any)) {                                // the common case: two totals, nothing else
        if (tid == 0) W.exclv[blockIdx.x] = W.exclf[blockIdx.x] = 0;
        return;
    }
    __shared__ unsigned wsum[TPB / 64];
    unsigned carry = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned incl = wave_inclusive(packed[k], lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        const unsigned excl = carry + before + incl - packed[k];
        const long long node = base + k * TPB + tid;
        if (node < G.nodes) {
            W.vloc[node] = (unsigned short)(excl & 0xffffu);
            W.floc[node] = (unsigned short)(excl >> 16);
            W.mask[node] = (unsigned char)masks[k];
            W.fcnt[node] = (unsigned char)(packed[k] >> 16);
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        W.exclv[blockIdx.x] = carry & 0xffffu;
        W.exclf[blockIdx.x] = carry >> 16;
    }
}

// ---- (b) tile totals -> exclusive scan in place, totals to [ntiles] and to counts: one workgroup per field
__global__ __launch_bounds__(SCAN_TPB) void scan_blocks_kernel(void* __restrict__ ws, long long nfields, long long nodes,
                                                               long long ntiles, long long* __restrict__ counts) {
    const long long f = blockIdx.x;
    const Work W = field_work(ws, nfields, f, nodes, ntiles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ long long sv[SCAN_TPB / 64], sf[SCAN_TPB / 64];
    long long cv = 0, cf = 0;
    for (long long b0 = 0; b0 < ntiles; b0 += SCAN_TPB) {
        const long long i = b0 + tid;
        const long long v = i < ntiles ? W.exclv[i] : 0, fc = i < ntiles ? W.exclf[i] : 0;
        const long long iv = wave_inclusive(v, lane), jf = wave_inclusive(fc, lane);
        if (lane == 63) { sv[wave] = iv; sf[wave] = jf; }
        __syncthreads();
        long long bv = 0, bf = 0, tv = 0, tf = 0;
#pragma unroll
        for (int w = 0; w < SCAN_TPB / 64; ++w) {
            if (w < wave) { bv += sv[w]; bf += sf[w]; }
            tv += sv[w];
            tf += sf[w];
        }
        if (i < ntiles) {
            W.exclv[i] = cv + bv + iv - v;
            W.exclf[i] = cf + bf + jf - fc;
        }
        cv += tv;
        cf += tf;
        __syncthreads();
    }
    if (tid == 0) {
        W.exclv[ntiles] = cv;
        W.exclf[ntiles] = cf;
        counts[2 * f] = cv;
        counts[2 * f + 1] = cf;
    }
}

// ---- (c) emit: the vertices of one node's edges and the faces of its cell
template <typename T, int D>
__host__ __device__ __forceinline__ void emit_node(const T* __restrict__ field, const SGrid& G, double level, const Work& W,
                                                   long long node, long long nv, long long nf, double* __restrict__ verts,
                                                   int* __restrict__ faces) {
#pragma clang fp contract(off)
    const unsigned m = W.mask[node], nfaces = W.fcnt[node];
    if ((m | nfaces) == 0) return;
    const long long tile = node / TILE;
    const long long v0 = W.exclv[tile], f0 = W.exclf[tile];
    int idx[D];
    double p[1 << D];
    unsigned valid, in, fin;
    load_corners<T, D>(field, G, node, idx, p, valid, in, fin, level);

    // vertices of the edges 0 - c, ascending c
    long long vi = v0 + W.vloc[node];
#pragma unroll
    for (int c = 1; c < (1 << D); ++c) {
        if (!(m >> (c - 1) & 1u)) continue;
        const double num = level - p[0], den = p[c] - p[0];
        const double t = num / den;
        if (vi < nv) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double step = (double)idx[d] * G.dx[d];
                double x = G.xmin[d] + step;
                if (c >> d & 1) {
                    const double move = t * G.dx[d];
                    x = x + move;
                }
                verts[vi * D + d] = x;
            }
        }
        ++vi;
    }
    if (nfaces == 0) return;

    // faces of the cell, simplex by simplex
    constexpr Kuhn<D> K = make_kuhn<D>();
    long long fi = f0 + W.floc[node];
#pragma unroll
    for (int s = 0; s < Kuhn<D>::NS; ++s) {
        const unsigned chain = K.chain[s];
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k <= D; ++k) bits |= 1u << (chain >> (3 * k) & 7u);
        if ((fin & bits) != bits) continue;
        // simplex vertex numbers that are inside / outside, ascending, 2 bits each
        unsigned ins = 0, outs = 0;
        int ni = 0, no = 0, inv = 0;
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            if (in >> (chain >> (3 * k) & 7u) & 1u) {
                ins |= (unsigned)k << (2 * ni++);
                inv += no;                                           // every outside number before it is a smaller one placed after
            } else {
                outs |= (unsigned)k << (2 * no++);
            }
        }
        if (ni == 0 || no == 0) continue;
        const unsigned par = (K.par >> s & 1u) ^ (unsigned)(inv & 1);
        // index of the vertex on the simplex edge between its inside vertex number I(a) and outside vertex number O(b)
        auto edge = [&](int a, int b) -> int {
            const int i = (int)(ins >> (2 * a) & 3u), o = (int)(outs >> (2 * b) & 3u);
            const int lo = i < o ? i : o, hi = i < o ? o : i;
            const unsigned ca = chain >> (3 * lo) & 7u, cb = chain >> (3 * hi) & 7u;
            const unsigned cls = (cb & ~ca) - 1u;
            const long long low = node + corner_offset<D>(G, (int)ca);
            const unsigned ml = W.mask[low];
            const long long first = W.exclv[low / TILE] + W.vloc[low];
            return (int)(first + __builtin_popcount(ml & ((1u << cls) - 1u)));
        };
        if (D == 2) {
            int a = edge(0, 0);
            int b = ni == 1 ? edge(0, 1) : edge(1, 0);
            if (par ^ (unsigned)(ni == 2)) { const int t = a; a = b; b = t; }
            if (fi < nf) {
                faces[fi * 2] = a;
                faces[fi * 2 + 1] = b;
            }
            ++fi;
        } else if (ni == 2) {
            const int q0 = edge(0, 0), q1 = edge(0, 1), q2 = edge(1, 1), q3 = edge(1, 0);
            if (fi + 1 < nf) {
                faces[fi * 3] = q0;
                faces[fi * 3 + 1] = par ? q2 : q1;
                faces[fi * 3 + 2] = par ? q1 : q2;
                faces[fi * 3 + 3] = q0;
                faces[fi * 3 + 4] = par ? q3 : q2;
                faces[fi * 3 + 5] = par ? q2 : q3;
            }
            fi += 2;
        } else {
            const int a = edge(0, 0);
            const int b = ni == 1 ? edge(0, 1) : edge(1, 0);
            const int c = ni == 1 ? edge(0, 2) : edge(2, 0);
            if (fi < nf) {
                faces[fi * 3] = a;
                faces[fi * 3 + 1] = par ? c : b;
                faces[fi * 3 + 2] = par ? b : c;
            }
            ++fi;
        }
    }
}

// one thread per node of ONE field; a workgroup lies inside one scan tile and leaves at once when that tile is empty
template <typename T, int D>
__global__ __launch_bounds__(TPB) void emit_kernel(const T* __restrict__ field, SGrid G, double level, Work W, long long nv,
                                                   long long nf, double* __restrict__ verts, int* __restrict__ faces) {
    const long long tile = blockIdx.x / ITEMS;
    if (W.exclv[tile + 1] == W.exclv[tile] && W.exclf[tile + 1] == W.exclf[tile]) return;
    const long long node = (long long)blockIdx.x * TPB + threadIdx.x;
    if (node < G.nodes) emit_node<T, D>(field, G, level, W, node, nv, nf, verts, faces);
}

// ---------------------------------------------------------------------------------------------- host side
static int make_grid(const hjq_grid* g, SGrid& G) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->ndim < 1 || g->ndim > HJ_MAX_DIM) return fail(HJ_EINVAL, "ndim %d outside 1..%d", (int)g->ndim, HJ_MAX_DIM);
    if (g->ndim != 2 && g->ndim != 3)
        return fail(HJ_EUNSUPPORTED, "level sets are extracted from 2-D and 3-D grids only (ndim %d): project or slice first", (int)g->ndim);
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", (int)g->dtype);
    long long total = 1;
    for (int d = 0; d < 3; ++d) { G.n[d] = 1; G.stride[d] = 0; G.xmin[d] = 0; G.dx[d] = 1; }
    for (int d = g->ndim - 1; d >= 0; --d) {
        if (g->N[d] < 2 || g->N[d] > (1ll << 30)) return fail(HJ_EINVAL, "N[%d] = %lld: a cell needs 2 nodes per axis", d, (long long)g->N[d]);
        if (!std::isfinite(g->dx[d]) || g->dx[d] == 0.0 || !std::isfinite(g->xmin[d])) return fail(HJ_EINVAL, "axis %d: dx must be finite and not 0, xmin finite", d);
        G.n[d] = (int)g->N[d];
        G.stride[d] = total;
        G.xmin[d] = g->xmin[d];
        G.dx[d] = g->dx[d];
        total *= g->N[d];
        // one thread per node in emit_kernel, whole tiles: a launch holds fewer than 2^32 threads
        if (total > (1ll << 32) - TILE) return fail(HJ_EUNSUPPORTED, "grid of more than 2^32 - %d nodes", TILE);
    }
    G.nodes = total;
    G.ntiles = (total + TILE - 1) / TILE;
    return HJ_OK;
}

static int check_common(const SGrid& G, const void* data, int64_t nfields, int64_t field_stride, double level, const void* ws,
                        size_t ws_bytes) {
    if (!data || !ws) return fail(HJ_EINVAL, "null argument");
    if (nfields < 1 || nfields > 65535) return fail(HJ_EINVAL, "nfields %lld outside 1..65535", (long long)nfields);
    if (nfields > 1 && field_stride < G.nodes) return fail(HJ_EINVAL, "field_stride %lld is smaller than the grid (%lld)", (long long)field_stride, G.nodes);
    if (level != level) return fail(HJ_EINVAL, "level is NaN");
    if ((uintptr_t)ws % 8) return fail(HJ_EINVAL, "workspace must be 8-byte aligned");
    const size_t need = work_bytes(nfields, G.nodes, G.ntiles);
    if (ws_bytes < need) return fail(HJ_EINVAL, "workspace of %zu bytes, %zu needed", ws_bytes, need);
    return HJ_OK;
}

template <typename T, int D>
static int count_launch(const SGrid& G, const void* data, int64_t nfields, int64_t field_stride, double level, void* ws,
                        int64_t* counts, hipStream_t stream, const char* name) {
    hipLaunchKernelGGL((classify_kernel<T, D>), dim3((unsigned)G.ntiles, (unsigned)nfields), dim3(TPB), 0, stream, (const T*)data,
                       (long long)field_stride, (long long)nfields, G, level, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(scan_blocks_kernel, dim3((unsigned)nfields), dim3(SCAN_TPB), 0, stream, ws, (long long)nfields, G.nodes,
                       G.ntiles, (long long*)counts);
    HIP_TRY(hipGetLastError());
    launched(name);
    launched_also("scan_blocks_kernel");
    return HJ_OK;
}

template <typename T, int D>
static int emit_launch(const SGrid& G, const void* data, int64_t nfields, int64_t field_stride, double level, const void* ws,
                       const int64_t* counts, double* verts, int32_t* faces, hipStream_t stream, const char* name) {
    const unsigned blocks = (unsigned)(G.ntiles * ITEMS);
    long long vat = 0, fat = 0;
    launched_none();
    for (int64_t f = 0; f < nfields; ++f) {
        const long long nv = counts[2 * f], nf = counts[2 * f + 1];
        if (nv == 0 && nf == 0) continue;
        const Work W = field_work(const_cast<void*>(ws), nfields, f, G.nodes, G.ntiles);
        hipLaunchKernelGGL((emit_kernel<T, D>), dim3(blocks), dim3(TPB), 0, stream, (const T*)data + f * field_stride, G, level, W, nv,
                           nf, verts + vat * D, faces + fat * D);
        HIP_TRY(hipGetLastError());
        launched_also(name);
        vat += nv;
        fat += nf;
    }
    return HJ_OK;
}

}  // namespace hjs

using namespace hjs;

extern "C" {

int hjs_workspace_size(const hjq_grid* g, int64_t nfields, size_t* bytes) {
    SGrid G;
    int rc = make_grid(g, G);
    if (rc) return rc;
    if (!bytes) return fail(HJ_EINVAL, "null argument");
    if (nfields < 1 || nfields > 65535) return fail(HJ_EINVAL, "nfields %lld outside 1..65535", (long long)nfields);
    *bytes = work_bytes(nfields, G.nodes, G.ntiles);
    return HJ_OK;
}

int hjs_count(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, double level, void* workspace,
              size_t workspace_bytes, int64_t* counts, void* stream) {
    SGrid G;
    int rc = make_grid(g, G);
    if (rc) return rc;
    if (!counts) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_common(G, data, nfields, field_stride, level, workspace, workspace_bytes))) return rc;
    hipStream_t s = (hipStream_t)stream;
#define HJS_COUNT(T, D) return count_launch<T, D>(G, data, nfields, field_stride, level, workspace, counts, s, "classify_kernel<" #T ", " #D ">")
    if (g->dtype == HJ_F64) {
        if (g->ndim == 2) HJS_COUNT(double, 2);
        HJS_COUNT(double, 3);
    }
    if (g->ndim == 2) HJS_COUNT(float, 2);
    HJS_COUNT(float, 3);
#undef HJS_COUNT
}

int hjs_emit(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, double level, const void* workspace,
             size_t workspace_bytes, const int64_t* counts_host, double* verts, int32_t* faces, void* stream) {
    SGrid G;
    int rc = make_grid(g, G);
    if (rc) return rc;
    if (!counts_host) return fail(HJ_EINVAL, "null argument");
    if ((rc = check_common(G, data, nfields, field_stride, level, workspace, workspace_bytes))) return rc;
    long long tv = 0, tf = 0;
    for (int64_t f = 0; f < nfields; ++f) {
        const long long nv = counts_host[2 * f], nf = counts_host[2 * f + 1];
        if (nv < 0 || nf < 0) return fail(HJ_EINVAL, "field %lld: negative count", (long long)f);
        if (nv >= (1ll << 31) || nf >= (1ll << 31))
            return fail(HJ_EUNSUPPORTED, "field %lld: %lld vertices, %lld faces: int32 indices hold fewer than 2^31", (long long)f, nv, nf);
        tv += nv;
        tf += nf;
    }
    if ((tv && !verts) || (tf && !faces)) return fail(HJ_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
#define HJS_EMIT(T, D) return emit_launch<T, D>(G, data, nfields, field_stride, level, workspace, counts_host, verts, faces, s, "emit_kernel<" #T ", " #D ">")
    if (g->dtype == HJ_F64) {
        if (g->ndim == 2) HJS_EMIT(double, 2);
        HJS_EMIT(double, 3);
    }
    if (g->ndim == 2) HJS_EMIT(float, 2);
    HJS_EMIT(float, 3);
#undef HJS_EMIT
}

HJ_TOOL_LAST_SYMBOLS(hjs)

}  // extern "C"
