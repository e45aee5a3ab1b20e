// Host layer of the stateless libraries (every library the Makefile builds beside libhj_mi355x.so): the error text, the record of
// the kernels the last successful call launched, the argument checks more than one of them makes, the (dtype, scheme) dispatch of
// the point and rollout kernels and the ndim dispatch of the 1-D to 6-D kernels.
// Host code only.  Every one of these libraries is ONE translation unit that includes this header once, so the `static
// thread_local` records below are that library's own: a refusal in libhj_query.so leaves hjt_last_error() as it was.
// (libhj_mi355x.so has a record of its own, shared by its objects: hj_host.h.)
#ifndef HJ_TOOL_HOST_H
#define HJ_TOOL_HOST_H
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/hj_mi355x.h"

namespace hj_tool {

// ---- error record: what <prefix>_last_error() returns
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return ::hj_tool::fail(HJ_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// ---- last-kernel record: what <prefix>_last_kernel() returns, the names joined by ';' in launch order
static thread_local std::string g_kernels;

static void launched(const char* name) { g_kernels = name; }
static void launched_none() { g_kernels.clear(); }
static void launched_also(const char* name) {
    if (!g_kernels.empty()) g_kernels += ';';
    g_kernels += name;
}

// the end of a launcher: the launch's own error, then the record
static int launch_done(const char* name) {
    HIP_TRY(hipGetLastError());
    launched(name);
    return HJ_OK;
}

// the two ABI symbols every library ends with (inside its extern "C" block)
#define HJ_TOOL_LAST_SYMBOLS(prefix)                                                \
    const char* prefix##_last_error(void) { return ::hj_tool::g_err; }              \
    const char* prefix##_last_kernel(void) { return ::hj_tool::g_kernels.c_str(); }

// ---- checks
// workgroups of 256 threads for `threads` threads; `refusal` is the caller's message for a launch of 2^32 threads or more: the
// runtime takes gridDim.x * blockDim.x modulo 2^32 without an error, and such a launch would run only a part of its threads
static int blocks_for(long long threads, const char* refusal, unsigned& blocks) {
    const long long b = (threads + 255) / 256;
    if (b > 0xffffffffll / 256) return fail(HJ_EINVAL, "%s", refusal);
    blocks = (unsigned)b;
    return HJ_OK;
}

// the schemes the point, rollout and batched kernels are instantiated for; `kind` names the kernel in the message
static int check_point_scheme(int scheme, const char* kind) {
    if (scheme != HJ_ENO2 && scheme != HJ_ENO3 && scheme != HJ_WENO5_ASSHIPPED)
        return fail(HJ_EUNSUPPORTED, "scheme %d has no %s kernel (ENO2, ENO3, as-shipped WENO5 only)", scheme, kind);
    return HJ_OK;
}

// ---- (dtype, scheme) -> the template arguments of a point or rollout kernel.  `f` is a generic lambda: f(type_tag<T>,
// std::integral_constant<int, SCHEME>) for the element type of a checked dtype and a scheme check_point_scheme let through.
template <typename T> struct type_tag {
    using type = T;
    static const char* name() { return sizeof(T) == 8 ? "double" : "float"; }
};
template <int V> using int_c = std::integral_constant<int, V>;

template <typename F> static int dispatch(int dtype, int scheme, F&& f) {
    auto schemes = [&](auto t) {
        if (scheme == HJ_ENO2) return f(t, int_c<HJ_ENO2>{});
        if (scheme == HJ_ENO3) return f(t, int_c<HJ_ENO3>{});
        return f(t, int_c<HJ_WENO5_ASSHIPPED>{});
    };
    return dtype == HJ_F64 ? schemes(type_tag<double>{}) : schemes(type_tag<float>{});
}

// ndim -> a compile-time constant: f(int_c<1>) .. f(int_c<6>) for a checked number of axes (or of a simplex's dimensions)
template <typename F> static auto dispatch_ndim(int ndim, F&& f) {
    switch (ndim) {
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        case 3: return f(int_c<3>{});
        case 4: return f(int_c<4>{});
        case 5: return f(int_c<5>{});
        default: return f(int_c<6>{});
    }
}

// what launch_done records: "kernel<double, 0, 2>" from the kernel's name, its element type and its integer arguments
static std::string kernel_name(const char* kernel, const char* type, std::initializer_list<int> ints, const char* tail = "") {
    std::string s = std::string(kernel) + "<" + type;
    for (int v : ints) s += ", " + std::to_string(v);
    return s + tail + ">";
}

// state dimension of a built-in system, 0 for any other id
static int ham_ndim(int id) {
    return id == HJ_HAM_DUBINS_REL ? 3 : (id == HJ_HAM_DOUBLE_INTEGRATOR ? 2 : (id == HJ_HAM_DOUBLE_PENDULUM ? 4 : 0));
}

// ---- the schedule of one interval (hjb_plan, hjb_integrate, hjh_integrate): ONE statement of the time arithmetic
// the time a step of `order` from t with deltaT = dt reaches: the expressions of hj_rk_step (ode_cfl_1/2/3.py)
static double step_time(int order, double t0, double dt) {
    if (order == 1) return t0 + dt;
    const double t1 = t0 + dt, t2 = t1 + dt;
    if (order == 2) return 0.5 * (t0 + t2);
    const double tHalf = 0.25 * (3 * t0 + t2);
    const double tThreeHalf = tHalf + dt;
    return (1.0 / 3.0) * (t0 + 2 * tThreeHalf);
}

// one problem's steps over [t0, tf]: dts gets deltaT of every step (may be null), t the time reached
static int plan_problem(int order, double sb, double t0, double tf, double factor_cfl, double max_step, double stop_tol,
                        std::vector<double>* dts, double& t, int64_t b) {
    // the loop of odeCFLn (ode_cfl_3.py:125): while tf - t >= small*|tf|, small = 100*eps (:81); stop_tol >= 0: HJIPDE_solve's
    const double small = 100.0 * 2.220446049250313e-16;
    t = t0;
    int64_t steps = 0;
    auto more = [&]() { return stop_tol < 0 ? (tf - t >= small * std::fabs(tf)) : (t < tf - stop_tol); };
    if (!(sb > 0.0)) return fail(HJ_EINVAL, "problem %lld: the step bound must be positive (got %g)", (long long)b, sb);
    while (more()) {
        // deltaT = min(factorCFL*stepBound, tspan[1]-t, maxStep)  (ode_cfl_3.py:142)
        const double dt = std::min(std::min(factor_cfl * sb, tf - t), max_step);
        const double tn = step_time(order, t, dt);
        if (!(tn > t)) return fail(HJ_ESTATE, "problem %lld: time step underflow at t=%g (dt=%g)", (long long)b, t, dt);
        if (++steps > (1ll << 24)) return fail(HJ_ESTATE, "problem %lld: more than 2^24 steps in one interval", (long long)b);
        if (dts) dts->push_back(dt);
        t = tn;
    }
    return HJ_OK;
}

}  // namespace hj_tool
#endif
