// libhj_plant.so (include/hj_plant.h): trajectory rollouts of a plant the caller writes, for gfx950.
//   user_rollout_kernel<T, SCHEME>   rollout_kernel / hi_rollout_kernel around PlantUser, the two registered bodies: 2^ND lanes per
//                                    trajectory, 256 threads per workgroup, the trajectory hj_rollout_dev.h's rollout_body
//   user_noisy_rollout_kernel<T, SCHEME>      the same body with hj_mc_dev.h's NoisyHooks: libhj_mc.so's noisy_rollout_kernel around PlantUser
//   user_filtered_rollout_kernel<T, SCHEME>   with hj_filter_dev.h's HooksOf around PlantUser's Control: libhj_filter.so's filtered_rollout_kernel
//   user_decide_points_kernel<T, SCHEME>      and its decide_points_kernel
// This file holds NO kernel.  It keeps the table of registered plants, generates a translation unit per plant (plant_source:
// HJ_QUERY_MAXD for the plant's dimension, hj_query_dev.h, hj_rollout_dev.h, PlantUser, the kernel), has hipRTC compile the
// instantiation a launch needs -- lazily per (plant, element type, scheme, device), under hj_rtc_host.h's lock, through its disk
// cache -- and launches it through the module API with one argument block (hj_plant_dev.h's RolloutArgs, NoisyArgs, FilterArgs).  The
// descriptor's and the call's checks are the other rollout libraries': make_grid and fill_stencil of hj_query_dev.h at either width,
// check_rollout of hj_rollout_dev.h, the noise's of hj_mc_dev.h, the filter's of hj_filter.hip (read from that file with its kernels and
// entry points left out).  The library links nothing of the others.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>
#include <sstream>
#include <vector>
#include "hj_tool_host.h"
#include "hj_plant_dev.h"
#define HJ_FILTER_CHECKS_ONLY
#include "hj_filter.hip"
#define HJ_RTC_FAIL ::hj_tool::fail
#define HJ_RTC_WHAT "plant"
#include "hj_rtc_host.h"

namespace hjp {

using namespace hj_tool;

struct Kernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
};
// registered plants live in a deque (registration never moves an element another thread may be launching); every look at it
// and at the kernel tables takes HJ_RTC_LOCK
struct UserPlant {
    std::string name, controls, dynamics, include_dir, rtc_path;
    int ndim = 0, nu = 0, nd = 0, nparams = 0;
    std::map<long long, Kernel> kernels;        // key: (((device * 2 + fp32) * 4 + scheme) * 4 + kind)
};
static std::deque<UserPlant> g_plants;

static UserPlant* plant_of(int id) {
    const long long i = (long long)id - HJP_PLANT_BASE;
    return (i >= 0 && i < (long long)g_plants.size()) ? &g_plants[(size_t)i] : nullptr;
}

// The translation unit hipRTC compiles.  Both bodies run in fp64 under contraction off, each in a block of its own after a
// #line directive, so that a compiler message reads name:line with the line counted inside that body.  u, dst and dx start at
// zero: a body that leaves one out leaves a number, not a register's last content.
static std::string plant_source(const UserPlant& u) {
    std::ostringstream o;
    const bool hi = u.ndim > HJ_MAX_DIM;
    o << "#define HJ_QUERY_MAXD " << (hi ? HJH_MAX_DIM : HJ_MAX_DIM) << "\n";
    if (hi) o << "#define HJ_QUERY_MIND " << HJH_MIN_DIM << "\n";
    o << "#include \"hj_query_dev.h\"\n#include \"hj_rollout_dev.h\"\n#include \"hj_plant_dev.h\"\n"
         "namespace hjp {\n"
         "struct PlantUser {\n"
         "    static constexpr int ND = " << u.ndim << ", NU = " << u.nu << ", NDST = " << u.nd << ";\n"
         "    struct Control { double u[NU > 0 ? NU : 1]; double dst[NDST > 0 ? NDST : 1]; };\n"
         "    __device__ static __forceinline__ void controls(const hjp_plant& hj_P, const double* p, const double* x, Control& hj_c) {\n"
         "#pragma clang fp contract(off)\n"
         "        using hjr::sgn;\n"
         "        const double* par = hj_P.params;\n"
         "        const bool u_max = hj_P.u_mode == HJR_MODE_MAX, d_max = hj_P.d_mode == HJR_MODE_MAX;\n"
         "        double* u = hj_c.u;\n        double* dst = hj_c.dst;\n"
         "        for (int i = 0; i < (NU > 0 ? NU : 1); ++i) u[i] = 0.0;\n"
         "        for (int j = 0; j < (NDST > 0 ? NDST : 1); ++j) dst[j] = 0.0;\n"
         "        (void)p; (void)x; (void)par; (void)u_max; (void)d_max;\n"
         "        {\n#line 1 \"" << u.name << "\"\n" << u.controls << "\n#line 1 \"PlantUser\"\n        }\n"
         "    }\n"
         "    __device__ static __forceinline__ void f(const hjp_plant& hj_P, const double* x, const Control& hj_c, double* dx) {\n"
         "#pragma clang fp contract(off)\n"
         "        using hjr::sgn;\n"
         "        const double* par = hj_P.params;\n"
         "        const double* u = hj_c.u;\n        const double* dst = hj_c.dst;\n"
         "        for (int d = 0; d < ND; ++d) dx[d] = 0.0;\n"
         "        (void)x; (void)par; (void)u; (void)dst;\n"
         "        {\n#line 1 \"" << u.name << "\"\n" << u.dynamics << "\n#line 1 \"PlantUser\"\n        }\n"
         "    }\n"
         "};\n"
         "// A finished trajectory idles in its wavefront (rollout_body never returns early), so every __shfl of group_sum runs with\n"
         "// all lanes of its group active.\n"
         "template <typename T, int SCHEME>\n"
         "__global__ __launch_bounds__(256) void user_rollout_kernel(RolloutArgs<T, hjq::MAXD> A) { user_rollout<T, SCHEME, PlantUser>(A); }\n"
         "// the same body with the noise's hooks and with the filter's: groups of 2^ND lanes stay whole there too\n"
         "template <typename T, int SCHEME>\n"
         "__global__ __launch_bounds__(256) void user_noisy_rollout_kernel(NoisyArgs<T, hjq::MAXD> A) { user_noisy_rollout<T, SCHEME, PlantUser>(A); }\n"
         "template <typename T, int SCHEME>\n"
         "__global__ __launch_bounds__(256) void user_filtered_rollout_kernel(FilterArgs<T, hjq::MAXD> A) { user_filtered<T, SCHEME, PlantUser, false>(A); }\n"
         "template <typename T, int SCHEME>\n"
         "__global__ __launch_bounds__(256) void user_decide_points_kernel(FilterArgs<T, hjq::MAXD> A) { user_filtered<T, SCHEME, PlantUser, true>(A); }\n"
         "}\n";
    return o.str();
}

// what the disk cache's key covers besides the generated source (hj_rtc_host.h): every header the unit includes, the public ones
// among them, and the sizes of the kernel's argument block
static const hj_rtc::Unit& plant_unit() {
    static const hj_rtc::Unit u = {{"/hj_plant_dev.h", "/hj_query_dev.h", "/hj_rollout_dev.h", "/hj_device.h", "/../../include/hj_plant.h",
                                    "/../../include/hj_rollout.h", "/../../include/hj_query.h", "/../../include/hj_hidim.h",
                                    "/../../include/hj_mi355x.h", "/hj_filter_dev.h", "/hj_mc_dev.h", "/hj_plants_dev.h",
                                    "/../../include/hj_filter.h", "/../../include/hj_mc.h"},
                                   {sizeof(RolloutArgs<double, HJ_MAX_DIM>), sizeof(RolloutArgs<float, HJ_MAX_DIM>),
                                    sizeof(RolloutArgs<double, HJH_MAX_DIM>), sizeof(RolloutArgs<float, HJH_MAX_DIM>), sizeof(hjp_plant),
                                    sizeof(NoisyArgs<double, HJ_MAX_DIM>), sizeof(NoisyArgs<float, HJ_MAX_DIM>),
                                    sizeof(NoisyArgs<double, HJH_MAX_DIM>), sizeof(NoisyArgs<float, HJH_MAX_DIM>),
                                    sizeof(FilterArgs<double, HJ_MAX_DIM>), sizeof(FilterArgs<float, HJ_MAX_DIM>),
                                    sizeof(FilterArgs<double, HJH_MAX_DIM>), sizeof(FilterArgs<float, HJH_MAX_DIM>)}};
    return u;
}

static const char* const KERNEL_NAMES[] = {"user_rollout_kernel", "user_noisy_rollout_kernel", "user_filtered_rollout_kernel",
                                           "user_decide_points_kernel"};            // by HJP_KERNEL_*

static std::string kernel_expr(int kind, const char* tn, int scheme) {
    return std::string("hjp::") + KERNEL_NAMES[kind] + "<" + tn + ", " + std::to_string(scheme) + ">";
}

// the kernel of (plant, current device, type, scheme, kind): built at its first use.  Call with HJ_RTC_LOCK held.
static int user_kernel(UserPlant& u, int kind, bool f32, int scheme, hipFunction_t& fn) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    Kernel& k = u.kernels[(((long long)dev * 2 + (f32 ? 1 : 0)) * 4 + scheme) * 4 + kind];
    if (!k.fn) {
        int rc = hj_rtc::rtc_build(plant_unit(), plant_source(u), kernel_expr(kind, f32 ? "float" : "double", scheme), u.name, u.include_dir,
                                   u.rtc_path, k.mod, k.fn);
        if (rc) { k.mod = nullptr; k.fn = nullptr; return rc; }
    }
    fn = k.fn;
    return HJ_OK;
}

// the part every argument block begins with.  The caller has zeroed the block.
template <typename T, int MD, typename GD>
static void fill_rollout(RolloutArgs<T, MD>& A, const UserPlant& u, const GD* g, const hjq::QGridT<MD>& G, const void* data, int64_t ntimes,
                         int64_t field_stride, const double* x0, int64_t M, int sub_samples, double dt_small, const hjp_plant& P, double* traj,
                         int32_t* length, int32_t* t_earliest, int32_t* status) {
    A.data = (const T*)data;
    A.field_stride = field_stride;
    A.x0 = x0;
    A.M = M;
    A.ntimes = (int)ntimes;
    A.sub_samples = sub_samples;
    A.dt_small = dt_small;
    A.G = G;
    hjq::fill_stencil(g, G, A.S);
    A.P = P;
    for (int k = u.nparams; k < HJP_PAR_SLOTS; ++k) A.P.params[k] = 0.0;
    A.traj = traj;
    A.length = length;
    A.t_earliest = t_earliest;
    A.status = status;
}

// `groups` groups of 2^ndim lanes of kernel `kind` with the block A
template <typename T, typename ARGS>
static int launch_kind(UserPlant& u, int kind, int scheme, long long groups, int ndim, const char* refusal, ARGS& A, hipStream_t stream) {
    unsigned blocks;
    int rc = blocks_for(groups * (1ll << ndim), refusal, blocks);
    if (rc) return rc;
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(u, kind, sizeof(T) == 4, scheme, fn))) return rc;      // a plant that does not compile has launched nothing
    if ((rc = hj_rtc::module_launch(fn, blocks, 256, 0, stream, &A, sizeof(A)))) return rc;
    launched(kernel_name(KERNEL_NAMES[kind], type_tag<T>::name(), {scheme}, (", PlantUser:" + u.name).c_str()).c_str());
    return HJ_OK;
}

// check_rollout with what the library asks of its plants.  Call with HJ_RTC_LOCK held: from the look at the registry to the launch.
// filter: the kernel replaces controls, so the plant must have some.
template <int MD>
static int check_user(const hjq::QGridT<MD>& G, long long total, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                      int64_t nstates, int sub_samples, double dt_small, const hjp_plant* plant, const void* traj, const void* length,
                      const void* status, bool filter, UserPlant*& u, bool& go) {
    return hjr::check_rollout(G, total, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, traj, length, status, [&]() {
        u = plant_of(plant->id);
        if (!u) return fail(HJ_EINVAL, "unknown plant id %d: nothing is registered under it (hjp_plant_register)", (int)plant->id);
        if (u->ndim != G.ndim) return fail(HJ_EINVAL, "plant '%s' has %d states, the grid %d dimensions", u->name.c_str(), u->ndim, G.ndim);
        if (plant->nparams != u->nparams) return fail(HJ_EINVAL, "plant '%s' takes %d parameters, the descriptor has %d", u->name.c_str(), u->nparams, (int)plant->nparams);
        if (filter && u->nu == 0) return fail(HJ_EINVAL, "plant '%s' has no controls: there is nothing to filter", u->name.c_str());
        return (int)HJ_OK;
    }, go);
}

template <int MD, typename GD>
static int rollout(const GD* g, int mind, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                   int sub_samples, double dt_small, const hjp_plant* plant, double* traj, int32_t* length, int32_t* t_earliest, int32_t* status,
                   void* stream) {
    hjq::QGridT<MD> G;
    long long total;
    int rc = hjq::make_grid(g, G, total, mind);
    if (rc) return rc;
    HJ_RTC_LOCK;
    UserPlant* u = nullptr;
    bool go;
    rc = check_user(G, total, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, traj, length, status, false, u, go);
    if (rc || !go) return rc;
    auto run = [&](auto t) {
        using T = typename decltype(t)::type;
        RolloutArgs<T, MD> A;
        memset(&A, 0, sizeof(A));
        fill_rollout(A, *u, g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, traj, length, t_earliest, status);
        return launch_kind<T>(*u, HJP_KERNEL_ROLLOUT, scheme, nstates, G.ndim, hjr::TOO_MANY_TRAJ, A, (hipStream_t)stream);
    };
    return g->dtype == HJ_F64 ? run(type_tag<double>{}) : run(type_tag<float>{});
}

// hjn_rollout (hj_mc.hip) for a registered plant
template <int MD, typename GD>
static int noisy_rollout(const GD* g, int mind, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                         int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals, const double* Gm, double sq, int policy,
                         int sub_samples, double dt_small, const hjp_plant* plant, double* final_state, int32_t* length, int32_t* status,
                         double* value_end, double* value_min, double* traj, int32_t* t_earliest, void* stream) {
    hjq::QGridT<MD> G;
    long long total;
    int rc = hjq::make_grid(g, G, total, mind);
    if (rc) return rc;
    HJ_RTC_LOCK;
    UserPlant* u = nullptr;
    bool go;
    // check_rollout asks for a trajectory array; here it is optional, so the final states stand in for it
    rc = check_user(G, total, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, final_state, length, status, false, u, go);
    if (rc || (rc = hjn::check_noise(G.ndim, ntimes, sub_samples, nreal, policy, sq, Gm)) || !go) return rc;
    if ((rc = hjn::check_realisations(G.ndim, nstates, nreal, value_end, value_min))) return rc;
    auto run = [&](auto t) {
        using T = typename decltype(t)::type;
        NoisyArgs<T, MD> A;
        memset(&A, 0, sizeof(A));
        fill_rollout(A.R, *u, g, G, data, ntimes, field_stride, x0, nstates * nreal, sub_samples, dt_small, *plant, traj, length, t_earliest, status);
        A.nreal = nreal;
        A.normals = normals;
        A.first = first_realisation;
        A.seed = seed;
        A.nsteps = (ntimes - 1) * (long long)sub_samples;
        A.sq = sq;
        for (int k = 0; k < G.ndim * G.ndim; ++k) A.G[k] = Gm[k];          // the rest stays 0.0
        A.policy = policy;
        A.final_state = final_state;
        A.value_end = value_end;
        A.value_min = value_min;
        return launch_kind<T>(*u, HJP_KERNEL_NOISY, scheme, nstates * nreal, G.ndim, hjn::TOO_MANY_REAL, A, (hipStream_t)stream);
    };
    return g->dtype == HJ_F64 ? run(type_tag<double>{}) : run(type_tag<float>{});
}

// hjf_rollout (hj_filter.hip) for a registered plant
template <int MD, typename GD>
static int filtered_rollout(const GD* g, int mind, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                            int64_t nstates, int sub_samples, double dt_small, const hjp_plant* plant, int slice_policy, int64_t slice, int nominal,
                            const double* u_nom, const void* nom_data, int64_t nom_ntimes, int64_t nom_field_stride, int nom_u_mode, double level,
                            double margin, int dstb, double* final_state, double* gap_min, double* value_end, int32_t* interventions,
                            int32_t* first_intervention, int32_t* length, int32_t* status, double* traj, uint8_t* active, double* applied,
                            void* stream) {
    hjq::QGridT<MD> G;
    long long total;
    int rc = hjq::make_grid(g, G, total, mind);
    if (rc) return rc;
    HJ_RTC_LOCK;
    UserPlant* u = nullptr;
    bool go;
    // one converged field for every time stamp (stride 0) is the static policy's alone, and the final states stand in for traj: hjf_rollout
    const bool single = field_stride == 0 && slice_policy == HJF_SLICE_STATIC;
    rc = check_user(G, total, scheme, data, ntimes, single ? (int64_t)total : field_stride, x0, nstates, sub_samples, dt_small, plant, final_state,
                    length, status, true, u, go);
    if (rc) return rc;
    if ((rc = hjf::check_rollout_filter(total, ntimes, sub_samples, single, slice_policy, slice, nominal, nom_ntimes, nom_field_stride, nom_u_mode,
                                        level, margin, dstb)))
        return rc;
    if (!go) {
        launched_none();
        return HJ_OK;
    }
    if (!gap_min || !value_end || !interventions || !first_intervention || (nominal == HJF_NOMINAL_TABLE ? !u_nom : !nom_data))
        return fail(HJ_EINVAL, "null argument");
    if ((rc = hjf::check_states(nstates, G.ndim))) return rc;
    auto run = [&](auto t) {
        using T = typename decltype(t)::type;
        FilterArgs<T, MD> A;
        memset(&A, 0, sizeof(A));
        fill_rollout(A.R, *u, g, G, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, *plant, traj, length, nullptr, status);
        A.F = hjf::Filter{u_nom, nom_data, (long long)nom_field_stride, (int)nom_ntimes, nom_u_mode, level, margin, nominal, slice_policy,
                          (int)slice, dstb, (int)ntimes, sub_samples};
        A.E = hjf::FilterOut{final_state, gap_min, value_end, interventions, first_intervention, status, active, applied, nullptr, nullptr, nullptr};
        return launch_kind<T>(*u, HJP_KERNEL_FILTERED, scheme, nstates, G.ndim, hjf::TOO_MANY_STATES, A, (hipStream_t)stream);
    };
    return g->dtype == HJ_F64 ? run(type_tag<double>{}) : run(type_tag<float>{});
}

// hjf_decide (hj_filter.hip) for a registered plant
template <int MD, typename GD>
static int decide(const GD* g, int mind, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice, const double* xs,
                  int64_t nstates, const hjp_plant* plant, const double* u_nom, double level, double margin, int dstb, double* applied,
                  uint8_t* active, double* value, double* gap, double* costate, void* stream) {
    hjq::QGridT<MD> G;
    long long total;
    int rc = hjq::make_grid(g, G, total, mind);
    if (rc) return rc;
    HJ_RTC_LOCK;
    UserPlant* u = nullptr;
    bool go;
    // check_rollout with what a point does not have held at values it accepts: two sets a grid apart, one sub-step, a zero step
    rc = check_user(G, total, scheme, data, 2, (int64_t)total, xs, nstates, 1, 0.0, plant, applied, active, value, true, u, go);
    if (rc || (rc = hjf::check_decide_filter(total, nfields, field_stride, slice, level, margin, dstb))) return rc;
    if (!go) {
        launched_none();
        return HJ_OK;
    }
    if (!gap || !u_nom) return fail(HJ_EINVAL, "null argument");
    if ((rc = hjf::check_states(nstates, G.ndim))) return rc;
    auto run = [&](auto t) {
        using T = typename decltype(t)::type;
        FilterArgs<T, MD> A;
        memset(&A, 0, sizeof(A));
        fill_rollout(A.R, *u, g, G, data, nfields, nfields > 1 ? field_stride : 0, xs, nstates, 1, 0.0, *plant, nullptr, nullptr, nullptr, nullptr);
        A.F = hjf::Filter{u_nom, nullptr, 0, 1, HJR_MODE_MIN, level, margin, HJF_NOMINAL_TABLE, HJF_SLICE_STATIC, (int)slice, dstb, (int)nfields, 1};
        A.E = hjf::FilterOut{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, active, applied, value, gap, costate};
        return launch_kind<T>(*u, HJP_KERNEL_DECIDE, scheme, nstates, G.ndim, hjf::TOO_MANY_STATES, A, (hipStream_t)stream);
    };
    return g->dtype == HJ_F64 ? run(type_tag<double>{}) : run(type_tag<float>{});
}

}  // namespace hjp

using namespace hjp;

extern "C" {

int hjp_plant_register(const char* name, int ndim, int ncontrols, int ndisturbances, int nparams, const char* controls_src,
                       const char* dynamics_src, const char* include_dir, const char* hiprtc_path, int* plant_id) {
    if (!name || !controls_src || !dynamics_src || !include_dir || !plant_id) return fail(HJ_EINVAL, "null argument");
    // the name goes into #line directives of the generated source (compiler messages then point into the caller's text)
    for (const char* ch = name; *ch; ++ch)
        if (*ch == '"' || *ch == '\'' || *ch == '\\' || (unsigned char)*ch < 32) return fail(HJ_EINVAL, "the name of a plant must not contain quotes, backslashes or control characters");
    if (ndim < HJP_MIN_DIM || ndim > HJP_MAX_DIM) return fail(HJ_EUNSUPPORTED, "hjp_plant_register: a plant has %d..%d states, got %d", HJP_MIN_DIM, HJP_MAX_DIM, ndim);
    if (nparams < 0 || nparams > HJP_PAR_SLOTS) return fail(HJ_EINVAL, "a plant takes 0..%d parameters (HJP_PAR_SLOTS), got %d", HJP_PAR_SLOTS, nparams);
    if (ncontrols < 0 || ndisturbances < 0 || ncontrols + ndisturbances < 1 || ncontrols + ndisturbances > HJP_MAX_CONTROLS)
        return fail(HJ_EINVAL, "a plant has 1..%d controls and disturbances together (HJP_MAX_CONTROLS), got %d + %d", HJP_MAX_CONTROLS, ncontrols, ndisturbances);
    HJ_RTC_LOCK;
    for (size_t i = 0; i < g_plants.size(); ++i) {
        const UserPlant& v = g_plants[i];
        if (v.name == name && v.ndim == ndim && v.nu == ncontrols && v.nd == ndisturbances && v.nparams == nparams && v.controls == controls_src &&
            v.dynamics == dynamics_src) {
            *plant_id = HJP_PLANT_BASE + (int)i;        // registering the same text again: the same id, nothing recompiled
            return HJ_OK;
        }
    }
    UserPlant u;
    u.name = name;
    u.controls = controls_src;
    u.dynamics = dynamics_src;
    u.include_dir = include_dir;
    u.rtc_path = hiprtc_path ? hiprtc_path : "";
    u.ndim = ndim;
    u.nu = ncontrols;
    u.nd = ndisturbances;
    u.nparams = nparams;
    g_plants.push_back(u);
    *plant_id = HJP_PLANT_BASE + (int)g_plants.size() - 1;
    return HJ_OK;
}

int hjp_plant_info(int plant_id, int* ndim, int* ncontrols, int* ndisturbances, int* nparams, int* kernels_built) {
    HJ_RTC_LOCK;
    const UserPlant* u = plant_of(plant_id);
    if (!u) return fail(HJ_EINVAL, "unknown plant id %d", plant_id);
    if (ndim) *ndim = u->ndim;
    if (ncontrols) *ncontrols = u->nu;
    if (ndisturbances) *ndisturbances = u->nd;
    if (nparams) *nparams = u->nparams;
    if (kernels_built) {
        int n = 0;
        for (const auto& kv : u->kernels) n += kv.second.fn ? 1 : 0;
        *kernels_built = n;
    }
    return HJ_OK;
}

int hjp_plant_source(int plant_id, char* buf, int64_t n) {
    HJ_RTC_LOCK;
    const UserPlant* u = plant_of(plant_id);
    if (!u) return fail(HJ_EINVAL, "unknown plant id %d", plant_id);
    const std::string src = plant_source(*u);
    if (!buf || n < (int64_t)src.size() + 1) return fail(HJ_EINVAL, "the generated source needs a buffer of %zu bytes", src.size() + 1);
    memcpy(buf, src.c_str(), src.size() + 1);
    return HJ_OK;
}

int hjp_plant_cache_stats(int* compiled, int* loaded_from_cache) {
    HJ_RTC_LOCK;
    if (compiled) *compiled = hj_rtc::g_rtc_compiles;
    if (loaded_from_cache) *loaded_from_cache = hj_rtc::g_rtc_cache_hits;
    return HJ_OK;
}

int hjp_plant_compile_kind(int plant_id, int kind, int scheme, int dtype) {
    HJ_RTC_LOCK;
    const UserPlant* u = plant_of(plant_id);
    if (!u) return fail(HJ_EINVAL, "unknown plant id %d", plant_id);
    if (kind < HJP_KERNEL_ROLLOUT || kind > HJP_KERNEL_DECIDE) return fail(HJ_EINVAL, "unknown kernel kind %d (HJP_KERNEL_*)", kind);
    int rc = check_point_scheme(scheme, "rollout");
    if (rc) return rc;
    if (dtype != HJ_F64 && dtype != HJ_F32) return fail(HJ_EINVAL, "unknown dtype %d", dtype);
    if ((kind == HJP_KERNEL_FILTERED || kind == HJP_KERNEL_DECIDE) && u->nu == 0)
        return fail(HJ_EINVAL, "plant '%s' has no controls: there is nothing to filter", u->name.c_str());
    return hj_rtc::rtc_compile_check(plant_source(*u), {kernel_expr(kind, dtype == HJ_F32 ? "float" : "double", scheme)}, u->name, u->include_dir,
                                     u->rtc_path);
}

int hjp_plant_compile_check(int plant_id, int scheme, int dtype) { return hjp_plant_compile_kind(plant_id, HJP_KERNEL_ROLLOUT, scheme, dtype); }

int hjp_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                int sub_samples, double dt_small, const hjp_plant* plant, double* traj, int32_t* length, int32_t* t_earliest, int32_t* status,
                void* stream) {
    return rollout<HJ_MAX_DIM>(g, HJP_MIN_DIM, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, traj, length, t_earliest,
                               status, stream);
}

int hjp_rollout_hi(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                   int sub_samples, double dt_small, const hjp_plant* plant, double* traj, int32_t* length, int32_t* t_earliest, int32_t* status,
                   void* stream) {
    return rollout<HJH_MAX_DIM>(g, HJH_MIN_DIM, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, traj, length,
                                t_earliest, status, stream);
}

int hjp_noisy_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                      int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals, const double* G, double sq, int policy,
                      int sub_samples, double dt_small, const hjp_plant* plant, double* final_state, int32_t* length, int32_t* status,
                      double* value_end, double* value_min, double* traj, int32_t* t_earliest, void* stream) {
    return noisy_rollout<HJ_MAX_DIM>(g, HJP_MIN_DIM, scheme, data, ntimes, field_stride, x0, nstates, nreal, first_realisation, seed, normals, G, sq,
                                     policy, sub_samples, dt_small, plant, final_state, length, status, value_end, value_min, traj, t_earliest, stream);
}

int hjp_noisy_rollout_hi(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                         int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals, const double* G, double sq, int policy,
                         int sub_samples, double dt_small, const hjp_plant* plant, double* final_state, int32_t* length, int32_t* status,
                         double* value_end, double* value_min, double* traj, int32_t* t_earliest, void* stream) {
    return noisy_rollout<HJH_MAX_DIM>(g, HJH_MIN_DIM, scheme, data, ntimes, field_stride, x0, nstates, nreal, first_realisation, seed, normals, G, sq,
                                      policy, sub_samples, dt_small, plant, final_state, length, status, value_end, value_min, traj, t_earliest, stream);
}

int hjp_filtered_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                         int sub_samples, double dt_small, const hjp_plant* plant, int slice_policy, int64_t slice, int nominal, const double* u_nom,
                         const void* nom_data, int64_t nom_ntimes, int64_t nom_field_stride, int nom_u_mode, double level, double margin, int dstb,
                         double* final_state, double* gap_min, double* value_end, int32_t* interventions, int32_t* first_intervention,
                         int32_t* length, int32_t* status, double* traj, uint8_t* active, double* applied, void* stream) {
    return filtered_rollout<HJ_MAX_DIM>(g, HJP_MIN_DIM, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, slice_policy, slice,
                                        nominal, u_nom, nom_data, nom_ntimes, nom_field_stride, nom_u_mode, level, margin, dstb, final_state, gap_min,
                                        value_end, interventions, first_intervention, length, status, traj, active, applied, stream);
}

int hjp_filtered_rollout_hi(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0, int64_t nstates,
                            int sub_samples, double dt_small, const hjp_plant* plant, int slice_policy, int64_t slice, int nominal,
                            const double* u_nom, const void* nom_data, int64_t nom_ntimes, int64_t nom_field_stride, int nom_u_mode, double level,
                            double margin, int dstb, double* final_state, double* gap_min, double* value_end, int32_t* interventions,
                            int32_t* first_intervention, int32_t* length, int32_t* status, double* traj, uint8_t* active, double* applied,
                            void* stream) {
    return filtered_rollout<HJH_MAX_DIM>(g, HJH_MIN_DIM, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant, slice_policy,
                                         slice, nominal, u_nom, nom_data, nom_ntimes, nom_field_stride, nom_u_mode, level, margin, dstb, final_state,
                                         gap_min, value_end, interventions, first_intervention, length, status, traj, active, applied, stream);
}

int hjp_decide(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice, const double* xs,
               int64_t nstates, const hjp_plant* plant, const double* u_nom, double level, double margin, int dstb, double* applied,
               uint8_t* active, double* value, double* gap, double* costate, void* stream) {
    return decide<HJ_MAX_DIM>(g, HJP_MIN_DIM, scheme, data, nfields, field_stride, slice, xs, nstates, plant, u_nom, level, margin, dstb, applied, active,
                              value, gap, costate, stream);
}

int hjp_decide_hi(const hjh_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice, const double* xs,
                  int64_t nstates, const hjp_plant* plant, const double* u_nom, double level, double margin, int dstb, double* applied,
                  uint8_t* active, double* value, double* gap, double* costate, void* stream) {
    return decide<HJH_MAX_DIM>(g, HJH_MIN_DIM, scheme, data, nfields, field_stride, slice, xs, nstates, plant, u_nom, level, margin, dstb, applied,
                               active, value, gap, costate, stream);
}

HJ_TOOL_LAST_SYMBOLS(hjp)

}  // extern "C"
