// Second-order centred derivatives and motion by mean curvature as ONE kernel launch each (gfx950).
//
//   hessianSecond        first partials + lower triangle of the Hessian      SpatialDerivative/Other/hessian.py:4
//   curvatureSecond      kappa (O&F eq. 1.8) and |grad phi|                  SpatialDerivative/Other/curvature.py:4
//   laplacianSecond      sum_i phi_ii                                        SpatialDerivative/Other/laplacian.py:3
//   centeredFirstSecond  the centred first partial of one dimension          SpatialDerivative/Other/centered.py:3
//   termCurvature        ydot = b kappa |grad phi|  (+ max b for the CFL)    ExplicitIntegration/Term/term_curvature.py:7
//   termTraceHessian     ydot = trace(L D^2phi R)  (+ max |trace(L D R)|)    ExplicitIntegration/Term/term_trace_hess.py:8
//
// The shipped hessianSecond raises (hessian.py:61,71), so curvatureSecond / laplacianSecond / termCurvature do too; the
// curvature loop over mixed partials runs j < i - 1 (curvature.py:48 and hessian.py:88, a mistranslation of MATLAB's j = 1:i-1) and drops
// -2 phi_x phi_y phi_xy in 2-D.  Implemented here is what their docstrings and ToolboxLS describe,
// restated in NumPy in tests/curvature_ref.py: parity UNPINNED, checked against that restatement.  The formulas, in the
// order hessian.py / curvature.py evaluate them (contraction off, as in hj_terms.h):
//   phi_i  = (0.5 / dx_i) (phi(+e_i) - phi(-e_i))                                   hessian.py:64-71
//   phi_ii = dx_i^-2 ((phi(+e_i) - 2 phi) + phi(-e_i))                              :85
//   phi_ij = (0.5 / dx_j) (phi_i(+e_j) - phi_i(-e_j))   for j < i                   :88-99
//   kappa  = (sum_i phi_ii (|p|^2 - phi_i^2) - sum_{j<i} 2 phi_i phi_j phi_ij) / |p|^3,  0 where |p| = 0   curvature.py:39-55
// phi_i(+-e_j) is the centred first partial at the diagonal neighbours, so a cell reads the compact stencil: itself, its
// 2 ND face neighbours and the 4 diagonal neighbours (+-1, +-1) of every axis pair -- 9 points in 2-D, 19 in 3-D, 33 in 4-D.
//
// Ghost cells: those of addGhostAllDims(grid, data, 1) (add_ghost_all.py:39-43), made on the fly.  One thread per cell, every
// stencil load issued unconditionally (as gather_stencils of hj_split.h): a neighbour across a periodic edge is the wrapped
// cell, one across an extrapolated edge loads the edge cell first and only waves that touch such an edge rebuild the ghost
// values (padded_value below).  L1/L2 absorb the stencil reuse.
#pragma once
#include "hj_split.h"

namespace hj {

enum { HJ_CURV_TERM = 0, HJ_CURV_CURV = 1, HJ_CURV_LAPL = 2, HJ_CURV_HESS = 3, HJ_CURV_CENTERED = 4, HJ_CURV_TRACE = 5,
       HJ_CURV_TRACE_SC = 6 };   // TRACE_SC: HJ_CURV_TRACE with every matrix entry a scalar (no loads, no reduction)

// number of (face + diagonal) neighbours of the compact second-order stencil
template <int ND> struct CurvStencil {
    static constexpr int NPAIR = ND * (ND - 1) / 2;
    static constexpr int NNB = 2 * ND + 4 * NPAIR;
};

template <typename T, int ND> struct CurvArgs {
    const T* y;
    GridArgs<T, ND> G;
    T hdx_inv[ND];                // 0.5 / dx_i   (0.5 * dxInv[i], hessian.py:71)
    T dx_inv2[ND];                // dxInv[i]^2   (hessian.py:85)
    const T* b;                   // HJ_CURV_TERM: per-node multiplier, or null: b_scalar
    T b_scalar;
    int dim;                      // HJ_CURV_CENTERED: the dimension
    T* out[ND + ND * (ND + 1) / 2];   // TERM: ydot; CURV: kappa, |grad phi|; LAPL: sum; CENTERED: deriv;
                                      // HESS: first[0..ND), then second(i, j), j <= i, row by row
    unsigned long long* key;      // HJ_CURV_TERM with array b: atomicMax key of max b; HJ_CURV_TRACE with reduce: of max |T|
};

// HJ_CURV_TRACE / HJ_CURV_TRACE_SC only (no other mode reads it): the ND x ND matrices L and R, row-major, entry e a grid-shaped
// array (L[e] non-null) or the scalar Ls[e] (likewise R); dd[m * ND + k] = 1 / (dx_m dx_k), the D of the step bound (:119)
template <typename T, int ND> struct TraceArgs {
    const T* L[ND * ND];
    const T* R[ND * ND];
    T Ls[ND * ND];
    T Rs[ND * ND];
    double dd[ND * ND];
    int reduce;                   // some entry is an array: reduce max |trace((L D) R)| into key
};
// the kernel's second argument: TraceArgs for the trace modes, empty for the others.  Chosen by specialisation, not by an
// expression over the (unnamed) mode enum: such an expression is part of the kernel's mangled name, and the host and device
// compilations number unnamed types independently, so the host stub would register a name the code object lacks.
struct NoTraceArgs {};
template <typename T, int ND, int OUT> struct CurvTraceArgsOf { using type = NoTraceArgs; };
template <typename T, int ND> struct CurvTraceArgsOf<T, ND, HJ_CURV_TRACE> { using type = TraceArgs<T, ND>; };
template <typename T, int ND> struct CurvTraceArgsOf<T, ND, HJ_CURV_TRACE_SC> { using type = TraceArgs<T, ND>; };
template <typename T, int ND, int OUT> using CurvTraceArgs = typename CurvTraceArgsOf<T, ND, OUT>::type;

// phi on the ghost-padded array at idx + a e_p + c e_q (p < q; c = 0: a face neighbour, q unused).  addGhostAllDims pads
// dimension 0 first, then dimension 1 of the already padded array, and so on: a corner ghost (outside in p AND in q) is
// dimension q's ghost rule applied to dimension p's ghost values -- extrapolated from the two p-ghosts at the q edge and one
// cell inside it, or the p-ghost of the wrapped q cell on a periodic q axis.  Reproduced in that order here.
template <typename T, int ND>
__device__ __forceinline__ T padded_value(const GridArgs<T, ND>& G, const T* pc0, const int* idx, int p, int a, int q, int c) {
#pragma clang fp contract(off)
    // value after padding dimension p, at p-offset a, with dimension q at the in-range index jq
    auto along_p = [&](int jq) -> T {
        const T* base = c ? pc0 + (long long)(jq - idx[q]) * G.stride[q] : pc0;
        const int n = G.n[p], i = idx[p], j = i + a;
        const long long s = G.stride[p];
        if (j >= 0 && j < n) return base[(long long)a * s];
        if (G.bc[p] == HJ_BC_PERIODIC) return base[(long long)((j < 0 ? j + n : j - n) - i) * s];
        const int e = j < 0 ? 0 : n - 1, in = j < 0 ? 1 : n - 2;
        return ghost_value(base[(long long)(e - i) * s], base[(long long)(in - i) * s], G.km[p]);
    };
    if (!c) return along_p(0);
    const int n = G.n[q], jq = idx[q] + c;
    if (jq >= 0 && jq < n) return along_p(jq);
    if (G.bc[q] == HJ_BC_PERIODIC) return along_p(jq < 0 ? jq + n : jq - n);
    const int e = jq < 0 ? 0 : n - 1, in = jq < 0 ? 1 : n - 2;
    return ghost_value(along_p(e), along_p(in), G.km[q]);
}

// offset of the in-range cell a load at idx +- 1 along d goes to (periodic: the wrapped cell; extrapolated: the edge cell,
// flagged for the fix-up)
template <typename T, int ND>
__device__ __forceinline__ long long nb_offset(const GridArgs<T, ND>& G, const int* idx, int d, int a, bool& ghost) {
    const int n = G.n[d], j = idx[d] + a;
    int k = j;
    if (j < 0) { if (G.bc[d] == HJ_BC_PERIODIC) k = j + n; else { k = 0; ghost = true; } }
    else if (j >= n) { if (G.bc[d] == HJ_BC_PERIODIC) k = j - n; else { k = n - 1; ghost = true; } }
    return (long long)(k - idx[d]) * G.stride[d];
}

// trace(M1 P M2) for ND x ND matrices as cellMatrixMultiply / cellMatrixTrace evaluate it (term_trace_hess.py:115-116): the
// products over ascending k starting from the k = 0 product, then the diagonal summed over ascending i; only the diagonal of
// (M1 P) M2 is formed.  U is the arithmetic type.
template <typename U, int ND, typename F1, typename FP, typename F2>
__device__ __forceinline__ U trace_triple(F1 m1, FP p, F2 m2) {
#pragma clang fp contract(off)
    U tr = U(0);
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        U a = U(0);
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            U lp = m1(i, 0) * p(0, k);
#pragma unroll
            for (int m = 1; m < ND; ++m) lp = lp + m1(i, m) * p(m, k);
            a = k == 0 ? lp * m2(0, i) : a + lp * m2(k, i);
        }
        tr = i == 0 ? a : tr + a;
    }
    return tr;
}

template <typename T, int ND, int OUT>
__global__ __launch_bounds__(256) void curv_kernel(const CurvArgs<T, ND> A, const CurvTraceArgs<T, ND, OUT> TR) {
#pragma clang fp contract(off)
    constexpr int NP = CurvStencil<ND>::NPAIR;
    double mb = -1e300;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < A.G.total; t += (long long)gridDim.x * blockDim.x) {
        int idx[ND];
        decode<T, ND>(A.G, t, idx);
        const T* pc0 = A.y + t;
        const T ctr = pc0[0];
        if constexpr (OUT == HJ_CURV_CENTERED) {
            const int d = A.dim;
            bool ghost = false;
            const long long om = nb_offset<T, ND>(A.G, idx, d, -1, ghost), op = nb_offset<T, ND>(A.G, idx, d, 1, ghost);
            T vm = pc0[om], vp = pc0[op];
            if (__any(ghost ? 1 : 0)) {
                if (A.G.bc[d] != HJ_BC_PERIODIC && idx[d] == 0) vm = padded_value<T, ND>(A.G, pc0, idx, d, -1, 0, 0);
                if (A.G.bc[d] != HJ_BC_PERIODIC && idx[d] == A.G.n[d] - 1) vp = padded_value<T, ND>(A.G, pc0, idx, d, 1, 0, 0);
            }
            A.out[0][t] = A.hdx_inv[d] * (vp - vm);
            continue;
        }
        // face neighbours f[d][0] = phi(-e_d), f[d][1] = phi(+e_d); diagonal ones g[pair][k], k = 2 (sign along q) + (sign along p),
        // for the pairs (p < q) in the order (0,1), (0,2), ..., (1,2), ...  Every load goes out before any is used.
        constexpr bool DIAG = OUT != HJ_CURV_LAPL;
        T f[ND][2];
        T g[NP > 0 ? NP : 1][4];
        bool ghost = false;
        long long of[ND][2];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            of[d][0] = nb_offset<T, ND>(A.G, idx, d, -1, ghost);
            of[d][1] = nb_offset<T, ND>(A.G, idx, d, 1, ghost);
            f[d][0] = pc0[of[d][0]];
            f[d][1] = pc0[of[d][1]];
        }
        if constexpr (DIAG) {
            int k = 0;
#pragma unroll
            for (int p = 0; p < ND; ++p)
#pragma unroll
                for (int q = p + 1; q < ND; ++q, ++k)
#pragma unroll
                    for (int s = 0; s < 4; ++s) g[k][s] = pc0[of[p][s & 1] + of[q][s >> 1]];
        }
        // the trace modes: the entries of L and R at this node, loaded with the stencil (an array entry's pointer is uniform)
        constexpr bool TRACE = OUT == HJ_CURV_TRACE || OUT == HJ_CURV_TRACE_SC;
        constexpr int NM = TRACE ? ND * ND : 1;
        T Lm[NM], Rm[NM];
        if constexpr (TRACE) {
#pragma unroll
            for (int e = 0; e < ND * ND; ++e) {
                if constexpr (OUT == HJ_CURV_TRACE_SC) {
                    Lm[e] = TR.Ls[e];
                    Rm[e] = TR.Rs[e];
                } else {
                    Lm[e] = TR.L[e] ? TR.L[e][t] : TR.Ls[e];
                    Rm[e] = TR.R[e] ? TR.R[e][t] : TR.Rs[e];
                }
            }
        }
        if (__any(ghost ? 1 : 0)) {
            // the waves at an extrapolated edge: the ghost values of addGhostAllDims in its order (padded_value)
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (A.G.bc[d] == HJ_BC_PERIODIC) continue;
                if (idx[d] == 0) f[d][0] = padded_value<T, ND>(A.G, pc0, idx, d, -1, 0, 0);
                if (idx[d] == A.G.n[d] - 1) f[d][1] = padded_value<T, ND>(A.G, pc0, idx, d, 1, 0, 0);
            }
            if constexpr (DIAG) {
                int k = 0;
#pragma unroll
                for (int p = 0; p < ND; ++p)
#pragma unroll
                    for (int q = p + 1; q < ND; ++q, ++k) {
                        const bool ep = A.G.bc[p] != HJ_BC_PERIODIC && (idx[p] == 0 || idx[p] == A.G.n[p] - 1);
                        const bool eq = A.G.bc[q] != HJ_BC_PERIODIC && (idx[q] == 0 || idx[q] == A.G.n[q] - 1);
                        if (!ep && !eq) continue;
#pragma unroll
                        for (int s = 0; s < 4; ++s) g[k][s] = padded_value<T, ND>(A.G, pc0, idx, p, (s & 1) ? 1 : -1, q, (s >> 1) ? 1 : -1);
                    }
            }
        }
        // second(i, i) and, for HESS / CURV / TERM, the first partials and second(i, j), j < i
        T sii[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) sii[d] = A.dx_inv2[d] * ((f[d][1] - T(2) * ctr) + f[d][0]);
        if constexpr (OUT == HJ_CURV_LAPL) {
            T lap = sii[0];
#pragma unroll
            for (int d = 1; d < ND; ++d) lap = lap + sii[d];                              // laplacian.py:38-40
            A.out[0][t] = lap;
            continue;
        }
        T fi[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) fi[d] = A.hdx_inv[d] * (f[d][1] - f[d][0]);
        // second(i, j), j < i: the centred difference along j of first[i] at the diagonal neighbours; pair (p=j, q=i)
        T sij[NP > 0 ? NP : 1];
        {
            int k = 0;
#pragma unroll
            for (int p = 0; p < ND; ++p)
#pragma unroll
                for (int q = p + 1; q < ND; ++q, ++k) {
                    const T fq_p = A.hdx_inv[q] * (g[k][3] - g[k][1]);     // first[q] at +e_p: phi(+e_q + e_p) - phi(-e_q + e_p)
                    const T fq_m = A.hdx_inv[q] * (g[k][2] - g[k][0]);     // first[q] at -e_p
                    sij[k] = A.hdx_inv[p] * (fq_p - fq_m);
                }
        }
        if constexpr (TRACE) {
            // term_trace_hess.py:103-127: P the full symmetric Hessian (:110-112), ydot = trace(L P R) unnegated (:115-116, :127)
            auto P = [&](int m, int k) -> T {
                if (m == k) return sii[m];
                const int j = m < k ? m : k, i = m < k ? k : m;
                return sij[j * ND - j * (j + 1) / 2 + (i - j - 1)];
            };
            A.out[0][t] = trace_triple<T, ND>([&](int i, int k) { return Lm[i * ND + k]; }, P,
                                              [&](int k, int i) { return Rm[k * ND + i]; });
            if (OUT == HJ_CURV_TRACE && TR.reduce) {
                // the step bound's T(x) = trace((L D) R) (:119-122) in double, whatever T is
                const double tx = trace_triple<double, ND>([&](int i, int k) { return (double)Lm[i * ND + k]; },
                                                           [&](int m, int k) { return TR.dd[m * ND + k]; },
                                                           [&](int k, int i) { return (double)Rm[k * ND + i]; });
                mb = fmax(mb, fabs(tx));
            }
            continue;
        }
        if constexpr (OUT == HJ_CURV_HESS) {
#pragma unroll
            for (int d = 0; d < ND; ++d) A.out[d][t] = fi[d];
            // second(i, j), j <= i, row by row
            int o = ND;
#pragma unroll
            for (int i = 0; i < ND; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j, ++o) {
                    if (j == i) A.out[o][t] = sii[i];
                    else A.out[o][t] = sij[j * ND - j * (j + 1) / 2 + (i - j - 1)];
                }
            continue;
        }
        // curvature.py:39-55 with j < i
        T g2 = fi[0] * fi[0];
#pragma unroll
        for (int d = 1; d < ND; ++d) g2 = g2 + fi[d] * fi[d];
        const T gm = sqrt(g2);
        T kap = T(0);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            kap = kap + sii[i] * (g2 - fi[i] * fi[i]);
#pragma unroll
            for (int j = 0; j < i; ++j) kap = kap - ((T(2) * fi[i]) * fi[j]) * sij[j * ND - j * (j + 1) / 2 + (i - j - 1)];
        }
        if (gm > T(0)) kap = kap / ((gm * gm) * gm);
        if constexpr (OUT == HJ_CURV_CURV) {
            A.out[0][t] = kap;
            A.out[1][t] = gm;
        } else {
            // term_curvature.py:141,147: delta = -b kappa |p|, ydot = -delta
            const T bb = A.b ? A.b[t] : A.b_scalar;
            A.out[0][t] = (bb * kap) * gm;
            if (A.b) mb = fmax(mb, (double)bb);
        }
    }
    if constexpr (OUT == HJ_CURV_TERM || OUT == HJ_CURV_TRACE) {
        // uniform across the launch: no thread reaches the barrier
        if constexpr (OUT == HJ_CURV_TERM) { if (!A.b) return; }
        else { if (!TR.reduce) return; }
        __shared__ double red[4];
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const double w = wave_max(mb);
        if (lane == 0) red[wv] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
            if (m > -1e299) key_max(A.key, m);
        }
    }
}

}  // namespace hj
