// The leaves and the two folds of a scene (include/hj_shapes.h, include/hj_hishapes.h): device source of hj_shapes.hip, compiled at
// MD = 4 axes, and of hj_hishapes.hip, compiled at MD = 6.  ONE source, so a program gives the same bits in either library.
// Every function is written one operation per statement with contraction off: the results are NumPy's, bit for bit.
#ifndef HJ_SHAPES_DEV_H
#define HJ_SHAPES_DEV_H
#include <hip/hip_runtime.h>

namespace hjg_dev {

// NaN on either side gives NaN, as np.minimum / np.maximum (and array_op of hj_batch.hip)
__device__ __forceinline__ double nmin(double a, double b) {
    double r;
    if (a != a) r = a;
    else if (b != b) r = b;
    else r = a < b ? a : b;
    return r;
}

__device__ __forceinline__ double nmax(double a, double b) {
    double r;
    if (a != a) r = a;
    else if (b != b) r = b;
    else r = a > b ? a : b;
    return r;
}

// sqrt(sum over the axes not in `ignore` of (x_d - c_d)(x_d - c_d)) - r;  p = c[ndim], r
template <int MD>
__device__ __forceinline__ double ball(const double (&x)[MD], int ndim, int ignore, const double* __restrict__ p) {
#pragma clang fp contract(off)
    double s = 0.0;                     // 0 + first term is the first term: the terms are squares
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        if (d < ndim && !((ignore >> d) & 1)) {
            const double e = x[d] - p[d];
            const double q = e * e;
            s = s + q;
        }
    }
    const double root = __builtin_sqrt(s);
    return root - p[ndim];
}

// p = l[ndim], u[ndim]
template <int MD>
__device__ __forceinline__ double rect(const double (&x)[MD], int ndim, const double* __restrict__ p) {
#pragma clang fp contract(off)
    const double a0 = x[0] - p[ndim];
    const double b0 = p[0] - x[0];
    double m = nmax(a0, b0);
#pragma unroll
    for (int d = 1; d < MD; ++d) {
        if (d < ndim) {
            const double a = x[d] - p[ndim + d];
            m = nmax(m, a);
            const double b = p[d] - x[d];
            m = nmax(m, b);
        }
    }
    return m;
}

// p = n[ndim], point[ndim]
template <int MD>
__device__ __forceinline__ double halfspace(const double (&x)[MD], int ndim, const double* __restrict__ p) {
#pragma clang fp contract(off)
    const double e0 = x[0] - p[ndim];
    double s = p[0] * e0;
#pragma unroll
    for (int d = 1; d < MD; ++d) {
        if (d < ndim) {
            const double e = x[d] - p[ndim + d];
            const double q = p[d] * e;
            s = s + q;
        }
    }
    return s;
}

// a sphere in J linear images of the coordinates;  p = A[J][ndim] row-major, c[J], r.  Every image takes all ndim terms, left to
// right from the first; the squares are summed from the first image on
template <int MD>
__device__ __forceinline__ double ball_of(const double (&x)[MD], int ndim, int J, const double* __restrict__ p) {
#pragma clang fp contract(off)
    const double* __restrict__ c = p + J * ndim;
    double s = 0.0;
    for (int j = 0; j < J; ++j) {
        const double* __restrict__ a = p + j * ndim;
        double e = a[0] * x[0];
#pragma unroll
        for (int d = 1; d < MD; ++d) {
            if (d < ndim) {
                const double q = a[d] * x[d];
                e = e + q;
            }
        }
        e = e - c[j];
        const double q = e * e;
        s = j == 0 ? q : s + q;
    }
    const double root = __builtin_sqrt(s);
    return root - c[J];
}

}  // namespace hjg_dev
#endif
