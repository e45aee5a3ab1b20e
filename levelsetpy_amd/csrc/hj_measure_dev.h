// The per-simplex rule of libhj_measure.so (include/hj_measure.h), written once: measure_kernel runs it on the device and
// hjv_simplex_q_host on the host, so the two cannot drift apart.  Every operation is rounded on its own (contraction off), in the
// order the header states; tests/measure_ref.py restates it with Python floats and integers.
#ifndef HJ_MEASURE_DEV_H
#define HJ_MEASURE_DEV_H
#include <hip/hip_runtime.h>
#include <math.h>

namespace hjv_dev {

constexpr unsigned long long Q_ONE = 1ull << 52;         // the whole simplex

constexpr int factorial(int n) { return n <= 1 ? 1 : n * factorial(n - 1); }

// q of the simplex with vertex values f[0 .. D] in path order: 2^52 times the fraction of it where the linear interpolant is <= 0.
// The row of the recursion is indexed by VERTEX (row[j] is F(i, .) at positive vertex j, 0 elsewhere) and every loop has
// compile-time bounds, so that the row and f stay in registers: a row compacted to the positives would be indexed at run time.
// `next` walks the positives of one row from the last to the first: F(i, j + 1), 1 past the last positive.
template <int D>
__host__ __device__ __forceinline__ unsigned long long simplex_q(const double (&f)[D + 1]) {
#pragma clang fp contract(off)
    bool any_pos = false, any_neg = false;
#pragma unroll
    for (int v = 0; v <= D; ++v) {
        any_pos |= f[v] > 0.0;
        any_neg |= f[v] < 0.0;
    }
    if (!any_pos) return Q_ONE;
    if (!any_neg) return 0ull;
    double row[D + 1];
#pragma unroll
    for (int v = 0; v <= D; ++v) row[v] = 0.0;           // F(k, j) = 0
    double top = 0.0;
#pragma unroll
    for (int i = D; i >= 0; --i) {                       // the negatives, last to first
        if (f[i] < 0.0) {
            const double na = -f[i];
            double next = 1.0;                           // F(i, m) = 1
#pragma unroll
            for (int j = D; j >= 0; --j) {               // the positives, last to first
                if (f[j] > 0.0) {
                    const double den = f[j] - f[i];
                    const double theta = na / den;
                    const double one_less = 1.0 - theta;
                    const double left = theta * next;
                    const double right = one_less * row[j];
                    next = left + right;
                    row[j] = next;
                }
            }
            top = next;                                  // F(i, 0)
        }
    }
    const double scaled = top * 4503599627370496.0;      // 2^52
    const unsigned long long q = (unsigned long long)rint(scaled);
    return q < Q_ONE ? q : Q_ONE;
}

// simplex s of a D-cell: the s-th permutation p of (0 .. D-1) in lexicographic order; chain[k] is corner v_k (v_0 = 0,
// v_k = v_{k-1} | 1 << p[k-1]).  The factorial digits divide by constants; "the c-th unused axis" is a scan over D bits.
template <int D>
__host__ __device__ __forceinline__ void simplex_chain(unsigned s, unsigned (&chain)[D + 1]) {
    unsigned used = 0u;
    chain[0] = 0u;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const unsigned radix = (unsigned)factorial(D - 1 - i);
        const unsigned c = s / radix;
        s -= c * radix;
        unsigned seen = 0u, pick = 0u;
#pragma unroll
        for (int b = 0; b < D; ++b) {
            const bool unused = !((used >> b) & 1u);
            if (unused && seen == c) pick = (unsigned)b;
            seen += unused ? 1u : 0u;
        }
        used |= 1u << pick;
        chain[i + 1] = used;
    }
}

}  // namespace hjv_dev
#endif
