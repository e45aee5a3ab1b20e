// libhj_hidim.so (include/hj_hidim.h): Hamilton-Jacobi substeps on 5-D and 6-D grids, for gfx950.
//   hidim_substep_kernel<T, HAM, SCHEME>  batch_substep_kernel (hj_batch.hip) without the problem axis: one thread per cell, every stencil load
//                                         issued unconditionally, 256 threads per workgroup.  Everything rides in the kernel arguments.
//   hidim_upwind_kernel<T, ND, SCHEME>    derivL / derivR of the axes of a mask from one gather per cell, and their 4 reductions per axis
//   hidim_bound_kernel<T, HAM>            the per-axis maxima of alpha at zero costate
// The per-cell functions (decode, gather_stencils, upwind_cd, upwind, rk_stage_out, post_step) are the solver's own source (hj_device.h,
// hj_split.h), instantiated at ND = 5 and 6 and compiled with the solver's flags.  HJ_MAX_DIM stays 4: HamTables cannot hold the coordinates
// of axes 4 and 5, so the two systems here read a table struct of their own (HiTables), and the one solver function that takes a HamTables,
// lf_ydot, has its dissipation sum restated (hidim_ydot).  The library links nothing of libhj_mi355x.so.
// The substep and bound kernels, HiTables, hidim_ydot and SubstepArgs live in hj_hidim_dev.h (array_op, the clamp, what a stage stores and
// the bound kernel's fold: hj_stage_dev.h, which it includes and libhj_batch.so / libhj_stoch.so share): this file instantiates them for the two
// built-in systems, and hipRTC compiles them around an expression registered with hjh_ham_register (HamUser<T>, generated below; ids from
// HJH_HAM_USER_BASE).  Such a kernel is built lazily at its first launch, per device, under the lock of hj_rtc_host.h, kept in the on-disk
// code-object cache that libhj_mi355x.so's registrations use, and launched through the module API with the very SubstepArgs block the
// built-in instantiations get: 256 threads, one thread per cell, 64-bit indexing.
// Host side, hj_stage_host.h holds what the three libraries share: the descriptor as GridArgs (fill_grid) and its checks, the step bound from
// the keys, struct Stage, a stage's and an interval's checks, and the RK schedule (rk_schedule) that hjh_integrate hands to ONE dispatch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>
#include <sstream>
#include <vector>
#include "hj_tool_host.h"
#include "hj_hidim_dev.h"
#include "hj_stage_host.h"
#define HJ_RTC_FAIL ::hj_tool::fail
#include "hj_rtc_host.h"

namespace hjh {

using namespace hj;
using namespace hj_tool;

// ---- the systems.  Interface and scaling as hj_device.h's: cell() folds the costate scales sc[d] into the cell's coefficients, eval() takes
// the UNSCALED costates q (p_d = sc[d] q_d), returns H(x, p) and alpha_s[d] = sc[d] alpha_d.  NP (ENO2 / ENO3, sc = 1): the expression of
// include/hj_hidim.h operation by operation, each a statement of its own, contraction off.
template <typename T> struct HamPlane5D {
    static constexpr int ND = 5;
    static constexpr int ID = HJH_HAM_PLANE5D;
    struct Cell { T vc, vs, om, am, al, s; };      // sc0 (x3 cos x2), sc1 (x3 sin x2), sc2 x4, sc3 a_max, sc4 alpha_max, the sign
    __device__ static __forceinline__ Cell cell(const HiTables<T>& P, const int* idx, const T* sc) {
#pragma clang fp contract(off)
        const T c = P.aux[0][idx[2]], s = P.aux[1][idx[2]];
        const T v = P.coord[3][idx[3]], om = P.coord[4][idx[4]];
        const T vc = v * c;
        const T vs = v * s;
        Cell k;
        k.vc = sc[0] * vc;
        k.vs = sc[1] * vs;
        k.om = sc[2] * om;
        k.am = sc[3] * P.par[0];
        k.al = sc[4] * P.par[1];
        k.s = P.par[2];
        return k;
    }
    template <bool NP>
    __device__ static __forceinline__ void eval(const Cell& k, const T* q, T& H, T* alpha) {
        if constexpr (NP) {
#pragma clang fp contract(off)
            const T t0 = q[0] * k.vc;
            const T t1 = q[1] * k.vs;
            const T t2 = q[2] * k.om;
            const T a3 = k.am * t_abs(q[3]);
            const T t3 = k.s * a3;
            const T a4 = k.al * t_abs(q[4]);
            const T t4 = k.s * a4;
            T h = t0 + t1;
            h = h + t2;
            h = h + t3;
            h = h + t4;
            H = h;
        } else {
            H = q[0] * k.vc + q[1] * k.vs + q[2] * k.om + k.s * (k.am * t_abs(q[3])) + k.s * (k.al * t_abs(q[4]));
        }
        alpha[0] = t_abs(k.vc);
        alpha[1] = t_abs(k.vs);
        alpha[2] = t_abs(k.om);
        alpha[3] = k.am;
        alpha[4] = k.al;
    }
};

template <typename T> struct HamDubinsPair6D {
    static constexpr int ND = 6;
    static constexpr int ID = HJH_HAM_DUBINS_PAIR6D;
    struct Cell { T a0, a1, we, a3, a4, wp; };     // sc0 v_e cos x2, sc1 v_e sin x2, sc2 w_e, sc3 v_p cos x5, sc4 v_p sin x5, sc5 w_p
    __device__ static __forceinline__ Cell cell(const HiTables<T>& P, const int* idx, const T* sc) {
#pragma clang fp contract(off)
        const T ce = P.aux[0][idx[2]], se = P.aux[1][idx[2]];
        const T cp = P.aux[2][idx[5]], sp = P.aux[3][idx[5]];
        const T a0 = P.par[0] * ce;
        const T a1 = P.par[0] * se;
        const T a3 = P.par[1] * cp;
        const T a4 = P.par[1] * sp;
        Cell k;
        k.a0 = sc[0] * a0;
        k.a1 = sc[1] * a1;
        k.we = sc[2] * P.par[2];
        k.a3 = sc[3] * a3;
        k.a4 = sc[4] * a4;
        k.wp = sc[5] * P.par[3];
        return k;
    }
    template <bool NP>
    __device__ static __forceinline__ void eval(const Cell& k, const T* q, T& H, T* alpha) {
        if constexpr (NP) {
#pragma clang fp contract(off)
            const T t0 = q[0] * k.a0;
            const T t1 = q[1] * k.a1;
            const T t3 = q[3] * k.a3;
            const T t4 = q[4] * k.a4;
            const T t2 = k.we * t_abs(q[2]);
            const T t5 = k.wp * t_abs(q[5]);
            T h = t0 + t1;
            h = h + t3;
            h = h + t4;
            h = h + t2;
            h = h - t5;
            H = -h;
        } else {
            H = -(q[0] * k.a0 + q[1] * k.a1 + q[3] * k.a3 + q[4] * k.a4 + k.we * t_abs(q[2]) - k.wp * t_abs(q[5]));
        }
        alpha[0] = t_abs(k.a0);
        alpha[1] = t_abs(k.a1);
        alpha[2] = k.we;
        alpha[3] = t_abs(k.a3);
        alpha[4] = t_abs(k.a4);
        alpha[5] = k.wp;
    }
};

// (the one-sided derivatives of hidim_upwind_kernel: hj_device.h's upwind_lr_hidim -- the exact form for ENO2 / ENO3 -- shared with hj_hiquery.hip)
template <typename T, int ND> struct UpwindArgs {
    GridArgs<T, ND> G;
    const T* src;
    T* dL[ND];
    T* dR[ND];
    unsigned long long* keys;          // 4 * HJH_MAX_DIM keys, or null
    unsigned mask;
};

template <typename T, int ND, int SCHEME>
__global__ __launch_bounds__(256) void hidim_upwind_kernel(const UpwindArgs<T, ND> A) {
    static_assert(SCHEME != HJ_WENO5, "the intended WENO5 needs an epsilon reduction over the grid");
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const bool live = t < A.G.total;
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T v[ND][7];
    if (live) {
        int idx[ND];
        decode<T, ND>(A.G, t, idx);
        const T* pc0 = A.src + t;
        gather_stencils<T, ND>(A.G, pc0, idx, pc0[0], v);
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if (!((A.mask >> d) & 1u)) continue;           // uniform
        double m[4] = {-1e300, -1e300, -1e300, -1e300};
        if (live) {
            T L, R;
            upwind_lr_hidim<SCHEME, T>(v[d], A.G.K[d], L, R);
            A.dL[d][t] = L;
            A.dR[d][t] = R;
            m[0] = -(double)L; m[1] = (double)L; m[2] = -(double)R; m[3] = (double)R;
        }
        if (A.keys) {                                  // uniform
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double w = wave_max(m[k]);
                if (lane == 0) red[wv][k] = w;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                const int k = threadIdx.x;
                const double w = fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]));
                if (w > -1e299) key_max(A.keys + 4 * d + k, w);
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side
static int hidim_ham_ndim(int ham) { return ham == HJH_HAM_PLANE5D ? 5 : (ham == HJH_HAM_DUBINS_PAIR6D ? 6 : 0); }

// ---- systems registered at run time (hjh_ham_register).  They live in a deque (registration never moves an element another thread may be
// launching); every look at it and at the kernel tables takes HJ_RTC_LOCK.
struct HiKernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
};
struct HiUserHam {
    std::string name, body, include_dir, rtc_path;
    int ndim = 0, nparams = 0, naux = 0;
    int aux_axes[4] = {0, 0, 0, 0};
    std::map<long long, HiKernel> substep;      // key: ((device * 2 + fp32) * 4 + scheme)
    std::map<long long, HiKernel> bound;        // key: device * 2 + fp32
};
static std::deque<HiUserHam> g_user;

static HiUserHam* user_of(int ham) {
    const long long i = (long long)ham - HJH_HAM_USER_BASE;
    return (i >= 0 && i < (long long)g_user.size()) ? &g_user[(size_t)i] : nullptr;
}

// The translation unit hipRTC compiles: the kernel header and the system type around the caller's expression.  cell() reads the node's
// coordinates and the naux table values once; eval() forms p[d] = sc[d] q[d], runs the expression -- under contraction off where NP holds
// (ENO2 / ENO3), so that a C++ expression written like a NumPy callback rounds every operation where NumPy does -- and scales alpha[d] by
// sc[d].  Every array of Cell is indexed by constants once cell() and eval() are inlined and unrolled: the values stay in registers.
static std::string user_source(const HiUserHam& u, int id) {
    std::ostringstream o;
    o << "#include \"hj_hidim_dev.h\"\nnamespace hjh {\n"
         "template <typename T> struct HamUser {\n"
         "    static constexpr int ND = " << u.ndim << ";\n"
         "    static constexpr int ID = " << id << ";\n"
         "    static constexpr int NAUX = " << u.naux << ";\n"
         "    struct Cell { T x[ND]; T sc[ND]; T aux[NAUX > 0 ? NAUX : 1]; T par[HJH_PAR_SLOTS]; };\n"
         "    __device__ static __forceinline__ Cell cell(const HiTables<T>& P, const int* idx, const T* sc) {\n"
         "        Cell c;\n"
         "#pragma unroll\n"
         "        for (int d = 0; d < ND; ++d) { c.x[d] = P.coord[d][idx[d]]; c.sc[d] = sc[d]; }\n"
         "        c.aux[0] = T(0);\n";
    for (int k = 0; k < u.naux; ++k) o << "        c.aux[" << k << "] = P.aux[" << k << "][idx[" << u.aux_axes[k] << "]];\n";
    o << "#pragma unroll\n"
         "        for (int k = 0; k < HJH_PAR_SLOTS; ++k) c.par[k] = P.par[k];\n"
         "        return c;\n    }\n"
         "    template <bool NP>\n"
         "    __device__ static __forceinline__ void eval(const Cell& c, const T* q, T& H, T* alpha) {\n"
         "        T p[ND];\n"
         "#pragma unroll\n"
         "        for (int d = 0; d < ND; ++d) { p[d] = c.sc[d] * q[d]; alpha[d] = T(0); }\n"
         "        const T* x = c.x;\n        const T* aux = c.aux;\n        const T* par = c.par;\n"
         "        (void)x; (void)aux; (void)par;\n        H = T(0);\n"
         "        if constexpr (NP) {\n"
         "#pragma clang fp contract(off)\n"
         "            {\n#line 1 \"" << u.name << "\"\n" << u.body << "\n            }\n"
         "        } else {\n"
         "            {\n#line 1 \"" << u.name << "\"\n" << u.body << "\n            }\n"
         "        }\n"
         "#pragma unroll\n"
         "        for (int d = 0; d < ND; ++d) alpha[d] = c.sc[d] * alpha[d];     // the kernel carries alpha in the stencil's scale\n"
         "    }\n};\n}\n";
    return o.str();
}

// what the disk cache's key covers besides the generated source (hj_rtc_host.h)
static const hj_rtc::Unit& hidim_unit() {
    static const hj_rtc::Unit u = {{"/hj_hidim_dev.h", "/hj_stage_dev.h", "/hj_split.h", "/hj_device.h", "/../../include/hj_hidim.h", "/../../include/hj_mi355x.h"},
                                   {sizeof(SubstepArgs<double, 5>), sizeof(SubstepArgs<double, 6>), sizeof(SubstepArgs<float, 5>),
                                    sizeof(SubstepArgs<float, 6>), sizeof(HiTables<double>), sizeof(HiTables<float>)}};
    return u;
}

static std::string substep_expr(const char* tn, int scheme) {
    return std::string("hjh::hidim_substep_kernel<") + tn + ", hjh::HamUser<" + tn + ">, " + std::to_string(scheme) + ">";
}
static std::string bound_expr(const char* tn) { return std::string("hjh::hidim_bound_kernel<") + tn + ", hjh::HamUser<" + tn + ">>"; }

// the kernel of (system, current device, type[, scheme]): built at its first use.  Call with HJ_RTC_LOCK held.
static int user_kernel(HiUserHam& u, int ham, bool f32, int scheme, bool bound, hipFunction_t& fn) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const long long key = bound ? (long long)dev * 2 + (f32 ? 1 : 0) : (((long long)dev * 2 + (f32 ? 1 : 0)) * 4 + scheme);
    HiKernel& k = (bound ? u.bound : u.substep)[key];
    if (!k.fn) {
        const char* tn = f32 ? "float" : "double";
        int rc = hj_rtc::rtc_build(hidim_unit(), user_source(u, ham), bound ? bound_expr(tn) : substep_expr(tn, scheme), u.name, u.include_dir,
                                   u.rtc_path, k.mod, k.fn);
        if (rc) { k.mod = nullptr; k.fn = nullptr; return rc; }
    }
    fn = k.fn;
    return HJ_OK;
}

static int check_grid(const hjh_grid* g, long long& total) {
    if (!g) return fail(HJ_EINVAL, "null grid descriptor");
    if (g->dtype != HJ_F64 && g->dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", (int)g->dtype);
    if (g->ndim < HJH_MIN_DIM || g->ndim > HJH_MAX_DIM)
        return fail(HJ_EINVAL, "grid.ndim must be %d..%d here (got %d; 1..%d: the solver of hj_mi355x.h)", (int)HJH_MIN_DIM, (int)HJH_MAX_DIM,
                    (int)g->ndim, HJ_MAX_DIM);
    return check_axes(g, g->ndim, nullptr, total);
}

// the checks every entry point that evaluates a system makes on (grid, tables, system, parameters)
static int check_setup(const hjh_grid* g, const hjh_tables* tab, int ham, const double* params_host, long long& total) {
    int rc = check_grid(g, total);
    if (rc) return rc;
    if (!tab) return fail(HJ_EINVAL, "null tables");
    int nd = hidim_ham_ndim(ham), naux = ham == HJH_HAM_PLANE5D ? 2 : 4;
    if (ham >= HJH_HAM_USER_BASE) {
        HJ_RTC_LOCK;
        const HiUserHam* u = user_of(ham);
        if (!u) return fail(HJ_EINVAL, "unknown Hamiltonian id %d: nothing is registered under it (hjh_ham_register)", ham);
        nd = u->ndim;
        naux = u->naux;
    }
    if (nd == 0) return fail(HJ_EUNSUPPORTED, "Hamiltonian %d has no kernel here (HJH_HAM_PLANE5D, HJH_HAM_DUBINS_PAIR6D)", ham);
    if (g->ndim != nd) return fail(HJ_EINVAL, "Hamiltonian %d lives on %d-D grids, the grid has %d dimensions", ham, nd, (int)g->ndim);
    if ((rc = check_coord(tab->coord, nd))) return rc;
    if ((rc = check_aux(tab->aux, naux, ham))) return rc;
    if (!params_host) return fail(HJ_EINVAL, "null parameters");
    return HJ_OK;
}

// what a stage needs besides the setup; shared by hjh_substep and hjh_integrate
static int check_ops(int restrict_sign, int post_prev, int op_a, const void* post_a, int op_b, const void* post_b) {
    const int rc = check_post_prev(post_prev);
    return rc ? rc : check_array_ops(op_a, post_a, op_b, post_b);
}

template <typename T> static void fill_tables(const hjh_tables* tab, const double* params_host, HiTables<T>& P) {
    for (int d = 0; d < HJH_MAX_DIM; ++d) P.coord[d] = (const T*)tab->coord[d];
    for (int s = 0; s < 4; ++s) P.aux[s] = (const T*)tab->aux[s];
    for (int s = 0; s < HJH_PAR_SLOTS; ++s) P.par[s] = (T)params_host[s];
}

// the argument block of one call's stages (every stage of a call shares it but for set_stage's fields), and its workgroup count
template <typename T, int ND>
static int fill_substep(const hjh_grid* g, const hjh_tables* tab, int scheme, int restrict_sign, const double* params_host, SubstepArgs<T, ND>& A,
                        unsigned& bx) {
    memset(&A, 0, sizeof(A));
    fill_grid<T, ND>(g, A.G);
    for (int d = 0; d < ND; ++d) A.sc[d] = scheme_scale<T>(scheme, g->dx[d]);
    fill_tables<T>(tab, params_host, A.P);
    A.restrict_sign = restrict_sign;
    return blocks_for(A.G.total, "grid too large for one thread per cell", bx);
}
template <typename T, int ND> static void set_stage(const Stage& s, SubstepArgs<T, ND>& A) {
    A.src = (const T*)s.src; A.y0 = (const T*)s.y0; A.dst = (T*)s.dst;
    A.post_a = (const T*)s.post_a; A.post_b = (const T*)s.post_b;
    A.dt = (T)s.dt;
    A.stage = s.stage; A.post_prev = s.post_prev; A.op_a = s.op_a; A.op_b = s.op_b;
}

template <typename T, typename HAM, int SCHEME>
static int launch_substep(const hjh_grid* g, const hjh_tables* tab, int restrict_sign, const double* params_host, const Stage* st, int nst,
                          hipStream_t stream, const char* name) {
    constexpr int ND = HAM::ND;
    SubstepArgs<T, ND> A;
    unsigned bx;
    int rc = fill_substep<T, ND>(g, tab, SCHEME, restrict_sign, params_host, A, bx);
    if (rc) return rc;
    for (int k = 0; k < nst; ++k) {
        set_stage<T, ND>(st[k], A);
        hipLaunchKernelGGL((hidim_substep_kernel<T, HAM, SCHEME>), dim3(bx), dim3(256), 0, stream, A);
        HIP_TRY(hipGetLastError());
    }
    launched(name);
    return HJ_OK;
}

// the same for a registered system: its kernel is built (or found in the disk cache) before the first launch, so a call that fails to
// compile has launched nothing
template <typename T, int ND>
static int launch_user_substep(const hjh_grid* g, const hjh_tables* tab, int scheme, int ham, int restrict_sign, const double* params_host,
                               const Stage* st, int nst, hipStream_t stream) {
    HJ_RTC_LOCK;
    HiUserHam* u = user_of(ham);
    if (!u || u->ndim != ND) return fail(HJ_EINVAL, "unknown Hamiltonian id %d", ham);
    SubstepArgs<T, ND> A;
    unsigned bx;
    int rc = fill_substep<T, ND>(g, tab, scheme, restrict_sign, params_host, A, bx);
    if (rc) return rc;
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(*u, ham, sizeof(T) == 4, scheme, false, fn))) return rc;
    for (int k = 0; k < nst; ++k) {
        set_stage<T, ND>(st[k], A);
        if ((rc = hj_rtc::module_launch(fn, bx, 256, 0, stream, &A, sizeof(A)))) return rc;
    }
    const std::string name = std::string("hidim_substep_kernel<") + (sizeof(T) == 4 ? "float" : "double") + ", HamUser:" + u->name + ", " +
                             std::to_string(scheme) + ">";
    launched(name.c_str());
    return HJ_OK;
}

static int dispatch_substep(const hjh_grid* g, const hjh_tables* tab, int scheme, int ham, int restrict_sign, const double* params_host,
                            const Stage* st, int nst, hipStream_t stream) {
    if (ham >= HJH_HAM_USER_BASE) {
        if (g->dtype == HJ_F64)
            return g->ndim == 5 ? launch_user_substep<double, 5>(g, tab, scheme, ham, restrict_sign, params_host, st, nst, stream)
                                : launch_user_substep<double, 6>(g, tab, scheme, ham, restrict_sign, params_host, st, nst, stream);
        return g->ndim == 5 ? launch_user_substep<float, 5>(g, tab, scheme, ham, restrict_sign, params_host, st, nst, stream)
                            : launch_user_substep<float, 6>(g, tab, scheme, ham, restrict_sign, params_host, st, nst, stream);
    }
#define HJH_GO(T, HAM, SCH) \
    return launch_substep<T, HAM<T>, SCH>(g, tab, restrict_sign, params_host, st, nst, stream, "hidim_substep_kernel<" #T ", " #HAM ", " #SCH ">")
#define HJH_HAMS(T, SCH)                                              \
    do {                                                              \
        if (ham == HJH_HAM_PLANE5D) HJH_GO(T, HamPlane5D, SCH);       \
        HJH_GO(T, HamDubinsPair6D, SCH);                              \
    } while (0)
    static_assert(HJ_ENO2 == 0 && HJ_ENO3 == 1 && HJ_WENO5_ASSHIPPED == 3, "scheme ids name the kernels");
    if (g->dtype == HJ_F64) {
        if (scheme == HJ_ENO2) HJH_HAMS(double, 0);
        if (scheme == HJ_ENO3) HJH_HAMS(double, 1);
        HJH_HAMS(double, 3);
    }
    if (scheme == HJ_ENO2) HJH_HAMS(float, 0);
    if (scheme == HJ_ENO3) HJH_HAMS(float, 1);
    HJH_HAMS(float, 3);
#undef HJH_HAMS
#undef HJH_GO
}

template <typename T, int ND, int SCHEME>
static int launch_upwind(const hjh_grid* g, const void* src, unsigned mask, void* const* dL, void* const* dR, unsigned long long* keys,
                         hipStream_t stream, const char* name) {
    UpwindArgs<T, ND> A;
    memset(&A, 0, sizeof(A));
    fill_grid<T, ND>(g, A.G);
    A.src = (const T*)src;
    for (int d = 0; d < ND; ++d)
        if ((mask >> d) & 1u) { A.dL[d] = (T*)dL[d]; A.dR[d] = (T*)dR[d]; }
    A.keys = keys;
    A.mask = mask;
    unsigned bx;
    int rc = blocks_for(A.G.total, "grid too large for one thread per cell", bx);
    if (rc) return rc;
    if (keys) HIP_TRY(hipMemsetAsync(keys, 0, sizeof(unsigned long long) * 4 * HJH_MAX_DIM, stream));
    hipLaunchKernelGGL((hidim_upwind_kernel<T, ND, SCHEME>), dim3(bx), dim3(256), 0, stream, A);
    return launch_done(name);
}

// hidim_bound_kernel's argument block as the module API takes it
template <typename T, int ND> struct BoundKernArgs {
    GridArgs<T, ND> G;
    HiTables<T> P;
    unsigned long long* keys;
};
template <typename T, int ND>
static int launch_user_bound(const hjh_grid* g, const hjh_tables* tab, int ham, const double* params_host, unsigned long long* keys, unsigned bx,
                             hipStream_t stream) {
    HJ_RTC_LOCK;
    HiUserHam* u = user_of(ham);
    if (!u || u->ndim != ND) return fail(HJ_EINVAL, "unknown Hamiltonian id %d", ham);
    hipFunction_t fn = nullptr;
    int rc = user_kernel(*u, ham, sizeof(T) == 4, 0, true, fn);
    if (rc) return rc;
    BoundKernArgs<T, ND> K;
    memset(&K, 0, sizeof(K));
    fill_grid<T, ND>(g, K.G);
    fill_tables<T>(tab, params_host, K.P);
    K.keys = keys;
    HIP_TRY(hipMemsetAsync(keys, 0, sizeof(unsigned long long) * HJH_MAX_DIM, stream));
    if ((rc = hj_rtc::module_launch(fn, bx, 256, 0, stream, &K, sizeof(K)))) return rc;
    const std::string name = std::string("hidim_bound_kernel<") + (sizeof(T) == 4 ? "float" : "double") + ", HamUser:" + u->name + ">";
    launched(name.c_str());
    return HJ_OK;
}

static int launch_builtin_bound(const hjh_grid* g, const hjh_tables* tab, int ham, const double* params_host, unsigned long long* k, unsigned bx,
                                hipStream_t s) {
    HIP_TRY(hipMemsetAsync(k, 0, sizeof(unsigned long long) * HJH_MAX_DIM, s));
#define HJH_B(T, HAM)                                                                                          \
    do {                                                                                                       \
        GridArgs<T, HAM<T>::ND> G;                                                                             \
        memset(&G, 0, sizeof(G));                                                                              \
        fill_grid<T, HAM<T>::ND>(g, G);                                                                        \
        HiTables<T> P;                                                                                         \
        fill_tables<T>(tab, params_host, P);                                                                   \
        hipLaunchKernelGGL((hidim_bound_kernel<T, HAM<T>>), dim3(bx), dim3(256), 0, s, G, P, k);               \
        HIP_TRY(hipGetLastError());                                                                            \
        launched("hidim_bound_kernel<" #T ", " #HAM ">");                                                      \
    } while (0)
    if (g->dtype == HJ_F64) { if (ham == HJH_HAM_PLANE5D) HJH_B(double, HamPlane5D); else HJH_B(double, HamDubinsPair6D); }
    else { if (ham == HJH_HAM_PLANE5D) HJH_B(float, HamPlane5D); else HJH_B(float, HamDubinsPair6D); }
#undef HJH_B
    return HJ_OK;
}

}  // namespace hjh

using namespace hjh;

extern "C" {

int hjh_substep(const hjh_grid* g, const hjh_tables* tab, int scheme, int ham, int stage, int restrict_sign, const double* params_host,
                const void* src, const void* y0, void* dst, double dt, int post_prev, int op_a, const void* post_a, int op_b,
                const void* post_b, void* stream) {
    long long total;
    int rc = check_setup(g, tab, ham, params_host, total);
    if (rc) return rc;
    if ((rc = check_point_scheme(scheme, "5-D / 6-D substep"))) return rc;
    if ((rc = check_stage_id(stage))) return rc;
    if ((rc = check_ops(restrict_sign, post_prev, op_a, post_a, op_b, post_b))) return rc;
    if (!src || !dst) return fail(HJ_EINVAL, "null argument");
    if (src == dst) return fail(HJ_EINVAL, "dst must not alias src");
    if ((rc = check_y0(stage, y0))) return rc;
    const Stage st = {stage, src, y0, dst, dt, post_prev, op_a, op_b, post_a, post_b};
    return dispatch_substep(g, tab, scheme, ham, restrict_sign, params_host, &st, 1, (hipStream_t)stream);
}

int hjh_step_bound(const hjh_grid* g, const hjh_tables* tab, int ham, const double* params_host, void* keys, double* sb_host,
                   double* amax_host, void* stream) {
    long long total;
    int rc = check_setup(g, tab, ham, params_host, total);
    if (rc) return rc;
    if (!keys || !sb_host) return fail(HJ_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* k = (unsigned long long*)keys;
    const unsigned bx = (unsigned)std::min<long long>((total + 255) / 256, 1024);
    if (ham >= HJH_HAM_USER_BASE) {
        if (g->dtype == HJ_F64) rc = g->ndim == 5 ? launch_user_bound<double, 5>(g, tab, ham, params_host, k, bx, s) : launch_user_bound<double, 6>(g, tab, ham, params_host, k, bx, s);
        else rc = g->ndim == 5 ? launch_user_bound<float, 5>(g, tab, ham, params_host, k, bx, s) : launch_user_bound<float, 6>(g, tab, ham, params_host, k, bx, s);
    } else rc = launch_builtin_bound(g, tab, ham, params_host, k, bx, s);
    if (rc) return rc;
    unsigned long long h[HJH_MAX_DIM];
    HIP_TRY(hipMemcpyAsync(h, k, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *sb_host = step_bound_of_keys(h, g->dx, g->ndim, amax_host, HJH_MAX_DIM);
    return HJ_OK;
}

int hjh_integrate(const hjh_grid* g, const hjh_tables* tab, int scheme, int ham, int order, int restrict_sign, int post_prev,
                  const double* params_host, double sb, const void* y_in, void* buf_a, void* buf_b, void* work, int op_a,
                  const void* post_a, int op_b, const void* post_b, double t0, double tf, double factor_cfl, double max_step,
                  double stop_tol, double* t_host, int64_t* steps_host, int32_t* result_in_host, void* stream) {
    long long total;
    int rc = check_setup(g, tab, ham, params_host, total);
    if (rc) return rc;
    if ((rc = check_point_scheme(scheme, "5-D / 6-D substep"))) return rc;
    if ((rc = check_order(order))) return rc;
    if ((rc = check_ops(restrict_sign, post_prev, op_a, post_a, op_b, post_b))) return rc;
    if ((rc = check_buffers(order, y_in, buf_a, buf_b, work))) return rc;
    // the schedule: the time arithmetic of hjb_plan (hj_tool_host.h), known before the first launch because alpha ignores the data
    std::vector<double> dts;
    double tend;
    if ((rc = plan_problem(order, sb, t0, tf, factor_cfl, max_step, stop_tol, &dts, tend, 0))) return rc;
    const int64_t n = (int64_t)dts.size();
    std::vector<Stage> st;
    rk_schedule(order, y_in, buf_a, buf_b, work, dts, post_prev, op_a, post_a, op_b, post_b, st);
    if (n > 0 && (rc = dispatch_substep(g, tab, scheme, ham, restrict_sign, params_host, st.data(), (int)st.size(), (hipStream_t)stream))) return rc;
    if (t_host) *t_host = tend;
    if (steps_host) *steps_host = n;
    if (result_in_host) *result_in_host = result_in(n);
    return HJ_OK;
}

int hjh_upwind(const hjh_grid* g, int scheme, const void* src, unsigned axis_mask, void* const* derivL_host, void* const* derivR_host,
               void* keys, void* stream) {
    long long total;
    int rc = check_grid(g, total);
    if (rc) return rc;
    if ((rc = check_point_scheme(scheme, "5-D / 6-D derivative"))) return rc;
    if (axis_mask == 0 || (axis_mask >> g->ndim)) return fail(HJ_EINVAL, "axis_mask 0x%x names no axis or one beyond the grid's %d", axis_mask, (int)g->ndim);
    if (!src || !derivL_host || !derivR_host) return fail(HJ_EINVAL, "null argument");
    for (int d = 0; d < g->ndim; ++d)
        if (((axis_mask >> d) & 1u) && (!derivL_host[d] || !derivR_host[d])) return fail(HJ_EINVAL, "null output array of axis %d", d);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* k = (unsigned long long*)keys;
#define HJH_U(T, ND, SCH) \
    return launch_upwind<T, ND, SCH>(g, src, axis_mask, derivL_host, derivR_host, k, s, "hidim_upwind_kernel<" #T ", " #ND ", " #SCH ">")
#define HJH_DIMS(T, SCH)                        \
    do {                                        \
        if (g->ndim == 5) HJH_U(T, 5, SCH);     \
        HJH_U(T, 6, SCH);                       \
    } while (0)
    if (g->dtype == HJ_F64) {
        if (scheme == HJ_ENO2) HJH_DIMS(double, 0);
        if (scheme == HJ_ENO3) HJH_DIMS(double, 1);
        HJH_DIMS(double, 3);
    }
    if (scheme == HJ_ENO2) HJH_DIMS(float, 0);
    if (scheme == HJ_ENO3) HJH_DIMS(float, 1);
    HJH_DIMS(float, 3);
#undef HJH_DIMS
#undef HJH_U
}

int hjh_ham_register(const char* name, int ndim, int nparams, const char* body, int naux, const int32_t* aux_axes, const char* include_dir,
                     const char* hiprtc_path, int* ham_id) {
    if (!name || !body || !include_dir || !ham_id) return fail(HJ_EINVAL, "null argument");
    // the name goes into #line directives of the generated source (compiler messages then point into the caller's text)
    for (const char* ch = name; *ch; ++ch)
        if (*ch == '"' || *ch == '\\' || (unsigned char)*ch < 32) return fail(HJ_EINVAL, "the name of a Hamiltonian must not contain quotes, backslashes or control characters");
    if (ndim < HJH_MIN_DIM || ndim > HJH_MAX_DIM)
        return fail(HJ_EUNSUPPORTED, "hjh_ham_register: grid.dim must be %d or %d, got %d (2..%d: hj_ham_register of hj_mi355x.h)", (int)HJH_MIN_DIM, (int)HJH_MAX_DIM, ndim, HJ_MAX_DIM);
    if (nparams < 0 || nparams > HJH_PAR_SLOTS) return fail(HJ_EINVAL, "a Hamiltonian takes 0..%d parameters (HJH_PAR_SLOTS), got %d", HJH_PAR_SLOTS, nparams);
    if (naux < 0 || naux > 4) return fail(HJ_EINVAL, "a Hamiltonian reads 0..4 tables (the aux slots of hjh_tables), got %d", naux);
    if (naux > 0 && !aux_axes) return fail(HJ_EINVAL, "naux > 0 needs the tables' axes");
    for (int k = 0; k < naux; ++k)
        if (aux_axes[k] < 0 || aux_axes[k] >= ndim) return fail(HJ_EINVAL, "table %d runs along axis %d, outside the grid's 0..%d", k, (int)aux_axes[k], ndim - 1);
    HJ_RTC_LOCK;
    for (size_t i = 0; i < g_user.size(); ++i) {
        const HiUserHam& v = g_user[i];
        bool same = v.name == name && v.ndim == ndim && v.nparams == nparams && v.body == body && v.naux == naux;
        for (int k = 0; same && k < naux; ++k) same = v.aux_axes[k] == aux_axes[k];
        if (same) {
            *ham_id = HJH_HAM_USER_BASE + (int)i;       // registering the same expression again: the same id, nothing recompiled
            return HJ_OK;
        }
    }
    HiUserHam u;
    u.name = name;
    u.body = body;
    u.include_dir = include_dir;
    u.rtc_path = hiprtc_path ? hiprtc_path : "";
    u.ndim = ndim;
    u.nparams = nparams;
    u.naux = naux;
    for (int k = 0; k < naux; ++k) u.aux_axes[k] = aux_axes[k];
    g_user.push_back(u);
    *ham_id = HJH_HAM_USER_BASE + (int)g_user.size() - 1;
    return HJ_OK;
}

int hjh_ham_info(int ham_id, int* ndim, int* nparams, int* naux, int32_t* aux_axes, int* kernels_built) {
    HJ_RTC_LOCK;
    const HiUserHam* u = user_of(ham_id);
    if (!u) return fail(HJ_EINVAL, "unknown Hamiltonian id %d", ham_id);
    if (ndim) *ndim = u->ndim;
    if (nparams) *nparams = u->nparams;
    if (naux) *naux = u->naux;
    for (int k = 0; k < 4 && aux_axes; ++k) aux_axes[k] = k < u->naux ? u->aux_axes[k] : -1;
    if (kernels_built) {
        int n = 0;
        for (const auto& kv : u->bound) n += kv.second.fn ? 1 : 0;
        for (const auto& kv : u->substep) n += kv.second.fn ? 1 : 0;
        *kernels_built = n;
    }
    return HJ_OK;
}

int hjh_ham_compile_check(int ham_id, int scheme, int dtype) {
    HJ_RTC_LOCK;
    const HiUserHam* u = user_of(ham_id);
    if (!u) return fail(HJ_EINVAL, "unknown Hamiltonian id %d", ham_id);
    int rc = check_point_scheme(scheme, "5-D / 6-D substep");
    if (rc) return rc;
    if (dtype != HJ_F64 && dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", dtype);
    const char* tn = dtype == HJ_F32 ? "float" : "double";
    return hj_rtc::rtc_compile_check(user_source(*u, ham_id), {substep_expr(tn, scheme), bound_expr(tn)}, u->name, u->include_dir, u->rtc_path);
}

int hjh_ham_source(int ham_id, char* buf, int64_t n) {
    HJ_RTC_LOCK;
    const HiUserHam* u = user_of(ham_id);
    if (!u) return fail(HJ_EINVAL, "unknown Hamiltonian id %d", ham_id);
    const std::string src = user_source(*u, ham_id);
    if (!buf || n < (int64_t)src.size() + 1) return fail(HJ_EINVAL, "the generated source needs a buffer of %zu bytes", src.size() + 1);
    memcpy(buf, src.c_str(), src.size() + 1);
    return HJ_OK;
}

int hjh_ham_cache_stats(int* compiled, int* loaded_from_cache) {
    HJ_RTC_LOCK;
    if (compiled) *compiled = hj_rtc::g_rtc_compiles;
    if (loaded_from_cache) *loaded_from_cache = hj_rtc::g_rtc_cache_hits;
    return HJ_OK;
}

HJ_TOOL_LAST_SYMBOLS(hjh)

}  // extern "C"
