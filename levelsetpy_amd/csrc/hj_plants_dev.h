// The three built-in plants of the rollout kernels (include/hj_rollout.h's table): specialisations of hj_rollout_dev.h's Plant<ID>, shared by
// libhj_rollout.so (hj_rollout.hip) and libhj_mc.so (hj_mc.hip).  controls(costate p, state x) -> (c0, c1), f(x; c0, c1) -> xdot, one operation
// per statement.  Not part of what hipRTC compiles (hj_plant.hip brings its own plant).  Include after hj_rollout_dev.h.
#ifndef HJ_PLANTS_DEV_H
#define HJ_PLANTS_DEV_H
#include "hj_rollout_dev.h"

namespace hjr {

template <> struct Plant<HJ_HAM_DUBINS_REL> {
    static constexpr int ND = 3;
    // c0 = a, the evader's turn rate (the control); c1 = b, the pursuer's (the disturbance)
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& a, double& b) {
#pragma clang fp contract(off)
        const double w = P.params[2];
        const double s1 = p[0] * x[1];
        const double s2 = p[1] * x[0];
        double s = s1 - s2;
        s = s - p[2];
        a = w * sgn(s);
        if (P.u_mode == HJR_MODE_MIN) a = -a;
        b = w * sgn(p[2]);
        if (P.d_mode == HJR_MODE_MIN) b = -b;
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double a, double b, double* k) {
#pragma clang fp contract(off)
        const double ve = P.params[0], vp = P.params[1];
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        const double vc = vp * c;
        const double drift = -ve + vc;
        const double ax2 = a * x[1];
        k[0] = drift + ax2;
        const double vs = vp * s;
        const double ax1 = a * x[0];
        k[1] = vs - ax1;
        k[2] = b - a;
    }
};

template <> struct Plant<HJ_HAM_DOUBLE_INTEGRATOR> {
    static constexpr int ND = 2;
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& u, double& unused) {
#pragma clang fp contract(off)
        u = P.params[0] * sgn(p[1]);
        if (P.u_mode == HJR_MODE_MIN) u = -u;
        unused = 0.0;
    }
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double u, double, double* k) {
        k[0] = x[1];
        k[1] = u;
    }
};

template <> struct Plant<HJ_HAM_DOUBLE_PENDULUM> {
    static constexpr int ND = 4;
    __device__ static __forceinline__ void controls(const hjr_plant& P, const double* p, const double* x, double& u1, double& u2) {
#pragma clang fp contract(off)
        u1 = P.params[0] * sgn(p[1]);
        u2 = P.params[0] * sgn(p[3]);
        if (P.u_mode == HJR_MODE_MIN) { u1 = -u1; u2 = -u2; }
    }
    // the drift in the expression order of DoublePendulum4D._drift (every product and sum left to right)
    __device__ static __forceinline__ void f(const hjr_plant& P, const double* x, double u1, double u2, double* k) {
#pragma clang fp contract(off)
        constexpr double G = 9.8, L1 = 1.0, L2 = 1.0, M1 = 1.0, M2 = 1.0;
        const double w1 = x[1], w2 = x[3];
        const double s1 = sin(x[0]), c1 = cos(x[0]), s2 = sin(x[2]), c2 = cos(x[2]);
        const double a0 = s2 * c1, a1 = c2 * s1;
        const double sd = a0 - a1;
        const double b0 = c2 * c1, b1 = s2 * s1;
        const double cd = b0 + b1;
        const double m12 = M1 + M2;
        double t = M2 * L1; t = t * cd; t = t * cd;
        const double den1 = m12 * L1 - t;
        double q1 = M2 * L1; q1 = q1 * w1; q1 = q1 * w1; q1 = q1 * sd; q1 = q1 * cd;
        double q2 = M2 * G; q2 = q2 * s2; q2 = q2 * cd;
        double q3 = M2 * L2; q3 = q3 * w2; q3 = q3 * w2; q3 = q3 * sd;
        double q4 = m12 * G; q4 = q4 * s1;
        double n1 = q1 + q2; n1 = n1 + q3; n1 = n1 - q4;
        const double f1 = n1 / den1;
        const double den2 = (L2 / L1) * den1;
        double r1 = -M2 * L2; r1 = r1 * w2; r1 = r1 * w2; r1 = r1 * sd; r1 = r1 * cd;
        double r2 = m12 * G; r2 = r2 * s1; r2 = r2 * cd;
        double r3 = m12 * L1; r3 = r3 * w1; r3 = r3 * w1; r3 = r3 * sd;
        double r4 = m12 * G; r4 = r4 * s2;
        double n3 = r1 + r2; n3 = n3 - r3; n3 = n3 - r4;
        const double f3 = n3 / den2;
        k[0] = w1;
        k[1] = f1 + u1;
        k[2] = w2;
        k[3] = f3 + u2;
    }
};

}  // namespace hjr
#endif
