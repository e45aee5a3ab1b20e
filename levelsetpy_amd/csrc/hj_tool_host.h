// Host layer of the stateless libraries (libhj_query.so, libhj_surface.so, libhj_ttr.so, libhj_rollout.so, libhj_batch.so, libhj_shapes.so, libhj_decomp.so, libhj_eikonal.so): the
// error text, the record of the kernels the last successful call launched, and the argument checks more than one of them makes.
// Host code only.  Every one of these libraries is ONE translation unit that includes this header once, so the `static
// thread_local` records below are that library's own: a refusal in libhj_query.so leaves hjt_last_error() as it was.
// (libhj_mi355x.so has a record of its own, shared by its objects: hj_host.h.)
#ifndef HJ_TOOL_HOST_H
#define HJ_TOOL_HOST_H
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <string>
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
// workgroups of 256 threads for `threads` threads; `refusal` is the caller's message for more than 2^31 - 1 of them
static int blocks_for(long long threads, const char* refusal, unsigned& blocks) {
    const long long b = (threads + 255) / 256;
    if (b > 0x7fffffffll) return fail(HJ_EINVAL, "%s", refusal);
    blocks = (unsigned)b;
    return HJ_OK;
}

// the schemes the point, rollout and batched kernels are instantiated for; `kind` names the kernel in the message
static int check_point_scheme(int scheme, const char* kind) {
    if (scheme != HJ_ENO2 && scheme != HJ_ENO3 && scheme != HJ_WENO5_ASSHIPPED)
        return fail(HJ_EUNSUPPORTED, "scheme %d has no %s kernel (ENO2, ENO3, as-shipped WENO5 only)", scheme, kind);
    return HJ_OK;
}

// state dimension of a built-in system, 0 for any other id
static int ham_ndim(int id) {
    return id == HJ_HAM_DUBINS_REL ? 3 : (id == HJ_HAM_DOUBLE_INTEGRATOR ? 2 : (id == HJ_HAM_DOUBLE_PENDULUM ? 4 : 0));
}

}  // namespace hj_tool
#endif
