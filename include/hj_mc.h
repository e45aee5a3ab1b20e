/* libhj_mc.so: Monte Carlo rollouts of dx = f(x, u*, d*) dt + G dW through a stored value function in one launch (gfx950).
 *
 * computeStochTrajs for M initial states times R realisations at once: every realisation stays on the device from its first
 * state to its last.  The entry points are stateless -- no hj_ctx: the grid descriptor of hj_query.h and a HIP stream per call.
 * Every array pointer of hjn_rollout and hjn_normals is DEVICE memory owned by the caller; inputs are never written.  The calls
 * are asynchronous on `stream` (0: the null stream).  Return value: HJ_OK (0) or a negative HJ_E* code of hj_mi355x.h;
 * hjn_last_error() holds the text.  A call that returns an error has launched nothing and touched no output.
 *
 * A realisation is the trajectory of hj_rollout.h (the same 2^ND lanes, the state in fp64, every operation rounded on its own)
 * with two changes.  With T = ntimes, r = first_realisation + m R + k the global index of realisation k of state m, the state x
 * and tE = 0 at the start:
 *     column 0 = x;  v = V[T-1](x);  value_end = value_min = v
 *     for it = 0 .. T-2:
 *         HJN_POLICY_EARLIEST: tE = the index hj_rollout.h's bisection over [tE, T-1] settles on; if tE == T-1: stop
 *         HJN_POLICY_CLOCK:    tE = it (the time-consistent policy of a solve that stores every slice); it never stops early
 *         for s = 0 .. sub_samples-1:
 *             p = grad V[tE](x);  u, d = the plant's controls for p at x;  x = RK4(x, dt_small; u, d held)     (hj_rollout.h)
 *             step = it sub_samples + s;  xi_0 .. xi_{ND-1} = the normals of (r, step)
 *             for every i:  n_i = ((G_i0 xi_0) + (G_i1 xi_1)) + ...  (all ND products taken, left to right);  t_i = sq n_i
 *             for every i:  x_i = x_i + t_i
 *         column it+1 = x;  v = V[T-1](x);  value_end = v;  value_min = nmin(value_min, v)
 * nmin(a, b) is NaN if either is NaN, else b < a ? b : a.  V[f](x) is hjq_interp_points' value in fp64 (NaN outside an
 * extrapolated axis).  The cell search follows the noise as it follows the RK4 step.
 *
 * The normals of (r, step) are `normals` where the caller supplies them, else the generator's:
 *     Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), key (seed_lo, seed_hi),
 *     counter (r_lo, r_hi, step, j), j the index of the pair of normals (2j, 2j+1), j = 0 .. (ND+1)/2 - 1; words w0 .. w3:
 *     k1 = (w0 >> 5) 2^26 + (w1 >> 6);  u1 = (k1 + 1) 2^-53  in (0, 1];   k2 likewise from w2, w3;  u2 = k2 2^-53  in [0, 1)
 *     rad = sqrt(-2 log(u1));  a = (2 pi) u2  (2 pi the double 6.283185307179586);  xi_2j = rad cos a;  xi_2j+1 = rad sin a
 * every operation rounded on its own (an odd ND drops the last pair's second normal).  Every lane of a realisation's group
 * computes them redundantly.  The words are the same on the host and on the device; log, cos and sin are each side's own.
 */
#ifndef HJ_MC_H
#define HJ_MC_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else                                  /* hipRTC has no system headers and declares the signed widths alone */
typedef __UINT32_TYPE__ uint32_t;
typedef __UINT64_TYPE__ uint64_t;
#endif
#include "hj_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HJN_POLICY_EARLIEST = 0, HJN_POLICY_CLOCK = 1 };

/* g, scheme, data, ntimes, field_stride, x0, nstates, sub_samples, dt_small, plant: as hjr_rollout, with its checks.
 * nreal: R >= 1 realisations of every state.  first_realisation: the global index of realisation 0 of state 0.  seed: the key.
 * normals (may be null: generate): nstates x nreal x (ntimes-1) sub_samples x ndim fp64.  G: ndim x ndim fp64, row-major, HOST
 * memory, finite (it travels in the kernel arguments).  sq: sqrt(dt_small) as the caller formed it, finite.
 * policy: HJN_POLICY_*.  Outputs, every element written:
 *   final nstates x nreal x ndim fp64: the last recorded state;  length, status nstates x nreal int32: as hjr_rollout
 *   (HJN_POLICY_CLOCK: length ntimes, status HJR_EXHAUSTED or HJR_LEFT_GRID);  value_end, value_min nstates x nreal fp64;
 *   traj (may be null) nstates x nreal x ndim x ntimes fp64, NaN past the length;  t_earliest (may be null) nstates x nreal x
 *   ntimes int32, -1 where no slice was chosen.
 * nstates * nreal * 2^ndim must be below 2^32 (HJ_EINVAL otherwise; the caller splits over states: the bits do not depend on
 * the split).  nstates == 0 returns HJ_OK and launches nothing. */
int hjn_rollout(const hjq_grid* g, int scheme, const void* data, int64_t ntimes, int64_t field_stride, const double* x0,
                int64_t nstates, int64_t nreal, uint64_t first_realisation, uint64_t seed, const double* normals, const double* G,
                double sq, int policy, int sub_samples, double dt_small, const hjr_plant* plant, double* final_state,
                int32_t* length, int32_t* status, double* value_end, double* value_min, double* traj, int32_t* t_earliest,
                void* stream);

/* The generator on the device, for realisations first .. first+count-1 and steps step0 .. step0+nsteps-1 (step0 + nsteps at
 * most 2^32), nd = 1 .. 4 normals a step.  out_words (may be null): count x nsteps x (nd+1)/2 x 4 uint32, the Philox words of
 * every pair.  out_normals (may be null): count x nsteps x nd fp64.  count == 0 or nsteps == 0 launches nothing. */
int hjn_normals(uint64_t seed, uint64_t first, int64_t count, int64_t step0, int64_t nsteps, int nd, uint32_t* out_words,
                double* out_normals, void* stream);
/* The same generator on the host, into HOST arrays: no GPU is needed. */
int hjn_normals_host(uint64_t seed, uint64_t first, int64_t count, int64_t step0, int64_t nsteps, int nd, uint32_t* out_words,
                     double* out_normals);

const char* hjn_last_error(void);
/* name of the kernel the calling thread's last successful launch ran, e.g. "noisy_rollout_kernel<double, 1, 0>" (element
 * type, scheme, plant id) or "normals_kernel" */
const char* hjn_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
