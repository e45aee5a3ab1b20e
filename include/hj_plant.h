/* libhj_plant.so: hjr_rollout / hjx_rollout for a plant the CALLER writes (gfx950).
 *
 * hj_rollout.h and hj_hiquery.h roll out trajectories of five built-in plants.  Here the plant is two pieces of device
 * source registered at run time: how the controls follow from the costate, and the dynamics.  The library ships no kernel:
 * user_rollout_kernel<T, SCHEME> is compiled with hipRTC for gfx950 around a registered plant, lazily per (plant, element
 * type, scheme, device), and kept in the on-disk code-object cache of the registered Hamiltonians (csrc/hj_rtc_host.h).  The
 * trajectory itself -- the bisection over the stored sets, the costate, sgn, RK4 -- is the source the built-in rollout
 * kernels compile (csrc/hj_rollout_dev.h's rollout_body), with the costate's upwind rule of that dimension: computeGradients'
 * up to 4-D, the 5-D / 6-D solver's above.  A plant registered with the text of a built-in one gives that kernel's bits.
 *
 * The entry points are stateless but for the table of registered plants.  Every array pointer is DEVICE memory owned by the
 * caller; inputs are never written.  Calls are asynchronous on `stream` (0: the null stream).  Return value: HJ_OK (0) or a
 * negative HJ_E* code of hj_mi355x.h; hjp_last_error() holds the text.  A call that returns an error has launched nothing
 * and touched no output.
 *
 * The two bodies are C++ statements, compiled in fp64 with contraction off (one operation per statement rounds where NumPy
 * rounds), with device math functions and sgn() (+1 for s >= 0, -1 for s < 0, NaN for NaN) at hand:
 *   controls_src   reads  p[d] (the costate), x[d] (the state), par[k], the booleans u_max / d_max (the caller's u_mode /
 *                  d_mode is HJR_MODE_MAX; uniform over the launch)
 *                  assigns u[i], i < ncontrols, and dst[j], j < ndisturbances
 *   dynamics_src   reads  x[d], u[i], dst[j], par[k];  assigns dx[d], d < ndim
 * The controls are held over an RK4 step, the dynamics are evaluated four times in it.  Neither body sees t, the value or a
 * table: a trajectory's state is not a node.  NaN is the expressions' own business (sgn hands it on): the kernel poisons
 * nothing, as the built-in plants do not.
 */
#ifndef HJ_PLANT_H
#define HJ_PLANT_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else                                  /* hipRTC has no system headers and declares the signed widths alone */
typedef __UINT8_TYPE__ uint8_t;
typedef __UINT64_TYPE__ uint64_t;
#endif
#include "hj_hidim.h"
#include "hj_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HJP_PAR_SLOTS 16
#define HJP_MAX_CONTROLS 8             /* ncontrols + ndisturbances, at least 1 */
#define HJP_MIN_DIM 2
#define HJP_MAX_DIM 6
/* ids of registered plants start here: no HJ_HAM_* / HJH_HAM_* id, built in or registered (100.., 1000..), is one */
enum { HJP_PLANT_BASE = 1000000 };

typedef struct hjp_plant {
    int32_t id;                        /* what hjp_plant_register gave */
    int32_t u_mode;                    /* HJR_MODE_MIN | HJR_MODE_MAX: u_max in controls_src */
    int32_t d_mode;                    /* the same for the disturbances: d_max */
    int32_t nparams;                   /* as registered */
    double params[HJP_PAR_SLOTS];      /* par[k]; unused slots 0 */
} hjp_plant;

/* Register a plant of `ndim` states (HJP_MIN_DIM .. HJP_MAX_DIM).  name: for messages and kernel names, and the file name
 * compiler messages carry (name:line, lines counted inside each body); no quotes, backslashes or control characters.
 * include_dir: the directory of hj_rollout_dev.h (the package's csrc).  hiprtc_path: libhiprtc.so, or null for the loader's.
 * Compiles nothing.  The same (name, numbers, texts) again gives the same id. */
int hjp_plant_register(const char* name, int ndim, int ncontrols, int ndisturbances, int nparams, const char* controls_src,
                       const char* dynamics_src, const char* include_dir, const char* hiprtc_path, int* plant_id);

/* any output may be null.  kernels_built: kernels of this plant loaded in this process */
int hjp_plant_info(int plant_id, int* ndim, int* ncontrols, int* ndisturbances, int* nparams, int* kernels_built);

/* the translation unit hipRTC is given, NUL-terminated, into buf[n] */
int hjp_plant_source(int plant_id, char* buf, int64_t n);

/* kernels compiled / loaded from the disk cache by this library in this process */
int hjp_plant_cache_stats(int* compiled, int* loaded_from_cache);

/* compile user_rollout_kernel<dtype, scheme> now; needs no GPU.  HJ_EINVAL with the compiler's message if a body is wrong */
int hjp_plant_compile_check(int plant_id, int scheme, int dtype);

/* hjr_rollout (hj_rollout.h) for a registered plant of 2 .. 4 states: arguments, outputs and status codes as there.  Every
 * element of every output is written; nstates == 0 returns HJ_OK and launches nothing.  HJ_EINVAL: an id nothing is
 * registered under, a plant on a grid of another dimension, nparams other than registered, a null pointer, ntimes < 2, a
 * grid below the stencil width; HJ_EUNSUPPORTED: a scheme without a point kernel. */
int hjp_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int sub_samples, double dt_small, const hjp_plant* plant, double* traj, int32_t* length,
                int32_t* t_earliest, int32_t* status, void* stream);

/* hjx_rollout (hj_hiquery.h) for a registered plant of 5 or 6 states */
int hjp_rollout_hi(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                   int64_t nstates, int sub_samples, double dt_small, const hjp_plant* plant, double* traj, int32_t* length,
                   int32_t* t_earliest, int32_t* status, void* stream);

/* ---- a registered plant under the Monte Carlo check of hj_mc.h and the safety filter of hj_filter.h.  The kernels are that
 * library's trajectory bodies compiled at run time around the plant, as user_rollout_kernel is: user_noisy_rollout_kernel,
 * user_filtered_rollout_kernel, user_decide_points_kernel<T, SCHEME>.  _hi: a plant of 5 or 6 states on an hjh_grid. */
enum { HJP_KERNEL_ROLLOUT = 0, HJP_KERNEL_NOISY = 1, HJP_KERNEL_FILTERED = 2, HJP_KERNEL_DECIDE = 3 };

/* hjp_plant_compile_check for the kernel of `kind` (HJP_KERNEL_*).  A plant without controls has no FILTERED / DECIDE kernel */
int hjp_plant_compile_kind(int plant_id, int kind, int scheme, int dtype);

/* hjn_rollout (hj_mc.h): its arguments, its contract word for word, its outputs.  The checks are hjp_rollout's, then hjn_rollout's.
 * G is ndim x ndim, row-major, HOST memory. */
int hjp_noisy_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                      int64_t nstates, int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals,
                      const double* G, double sq, int policy, int sub_samples, double dt_small, const hjp_plant* plant,
                      double* final_state, int32_t* length, int32_t* status, double* value_end, double* value_min, double* traj,
                      int32_t* t_earliest, void* stream);
int hjp_noisy_rollout_hi(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                         int64_t nstates, int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals,
                         const double* G, double sq, int policy, int sub_samples, double dt_small, const hjp_plant* plant,
                         double* final_state, int32_t* length, int32_t* status, double* value_end, double* value_min, double* traj,
                         int32_t* t_earliest, void* stream);

/* hjf_rollout (hj_filter.h) with the plant's held values u[0 .. ncontrols) and dst[0 .. ndisturbances): the nominal replaces the
 * controls u[] (a row of u_nom has ncontrols values; the value nominal runs controls_src on grad Vn with u_max from nom_u_mode and
 * takes its u[] only), HJF_DSTB_ZERO sets every dst[j] to 0.0.  applied (may be null): nstates x nsteps x W fp64, W = max(2,
 * ncontrols + ndisturbances): u then dst, padded with 0.0.  Everything else as there; the checks are hjp_rollout's, then
 * hjf_rollout's.  HJ_EINVAL for a plant without controls: there is nothing to filter. */
int hjp_filtered_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                         int64_t nstates, int sub_samples, double dt_small, const hjp_plant* plant, int slice_policy, int64_t slice,
                         int nominal, const double* u_nom, const void* nom_data, int64_t nom_ntimes, int64_t nom_field_stride,
                         int nom_u_mode, double level, double margin, int dstb, double* final_state, double* gap_min,
                         double* value_end, int32_t* interventions, int32_t* first_intervention, int32_t* length, int32_t* status,
                         double* traj, uint8_t* active, double* applied, void* stream);
int hjp_filtered_rollout_hi(const hjh_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                            int64_t nstates, int sub_samples, double dt_small, const hjp_plant* plant, int slice_policy,
                            int64_t slice, int nominal, const double* u_nom, const void* nom_data, int64_t nom_ntimes,
                            int64_t nom_field_stride, int nom_u_mode, double level, double margin, int dstb, double* final_state,
                            double* gap_min, double* value_end, int32_t* interventions, int32_t* first_intervention, int32_t* length,
                            int32_t* status, double* traj, uint8_t* active, double* applied, void* stream);

/* hjf_decide (hj_filter.h): u_nom nstates x ncontrols, applied nstates x W */
int hjp_decide(const hjq_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice, const double* xs,
               int64_t nstates, const hjp_plant* plant, const double* u_nom, double level, double margin, int dstb, double* applied,
               uint8_t* active, double* value, double* gap, double* costate, void* stream);
int hjp_decide_hi(const hjh_grid* g, int scheme, const void* data, int64_t nfields, int64_t field_stride, int64_t slice,
                  const double* xs, int64_t nstates, const hjp_plant* plant, const double* u_nom, double level, double margin, int dstb,
                  double* applied, uint8_t* active, double* value, double* gap, double* costate, void* stream);

const char* hjp_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g.
 * "user_rollout_kernel<double, 3, PlantUser:planar_quad>" or "user_filtered_rollout_kernel<double, 3, PlantUser:planar_quad>"
 * (element type, scheme, plant) */
const char* hjp_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
