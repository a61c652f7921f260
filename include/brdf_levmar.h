/*
 * brdf_levmar.h -- C ABI of libbrdf_hip.so, the MI355X (gfx950) replacement for the Levenberg-
 * Marquardt fitting path of ccalantzis/BRDF.
 *
 * The boundary is the reference's L3->L4 edge: levmar/levmar.h as it is called from
 * brdfdata.cpp:1058 and :1119.  Relinking brdfdata.o against this library instead of
 * levmar/liblevmar.a (BRDF.pro:30) keeps every call site unchanged; see INTEGRATION.md for the one
 * registration line that lets the library recognise the application's BRDFFunc callback.
 *
 * All entry points are plain C: pointers and sizes, no C++/torch types.  Unless a name ends in
 * `_dev`, pointers are HOST pointers.  Errors never call exit(): they return LM_ERROR (-1) after a
 * message on stderr, as the reference does for its own argument errors (lm_core.c:502-505,
 * lmbc_core.c:440-461), and brdf_hip_last_error() returns the text.
 *
 * Host threads.  Every entry point works on the calling thread's current HIP device (brdf_hip_fit_batch_multi
 * excepted: it runs on the devices it is given, from threads of its own) and keeps its buffers per host thread, so
 * threads on different devices are independent.  Threads that share a device get correct results; but two single fits
 * that both take the resident single-launch regime (brdf_hip_fit_dev, the drop-in calls, the fits of a batch with
 * n > 4096; up to #CUs * 4096 samples) can fail to be co-resident, wait out their spin budget and fall back to the
 * launch chain with a warning on stderr: serialise single fits per device.  The brdf_hip_last_* getters report the
 * calling thread's last call.  Model registration (brdf_hip_register_model) is process-wide and locked.
 */
#ifndef BRDF_LEVMAR_H
#define BRDF_LEVMAR_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants, same values as levmar/levmar.h:68-100 -------------------------------------------- */
#define LM_DIF_WORKSZ(npar, nmeas) (4 * (nmeas) + 4 * (npar) + (nmeas) * (npar) + (npar) * (npar))
#define LM_BC_DIF_WORKSZ(npar, nmeas) (2 * (nmeas) + 4 * (npar) + (nmeas) * (npar) + (npar) * (npar))
#define LM_DER_WORKSZ(npar, nmeas) (2 * (nmeas) + 4 * (npar) + (nmeas) * (npar) + (npar) * (npar))    /* levmar.h:68 */
#define LM_BC_DER_WORKSZ(npar, nmeas) (2 * (nmeas) + 4 * (npar) + (nmeas) * (npar) + (npar) * (npar)) /* levmar.h:74 */
#define LM_VERSION "2.6 (November 2011)" /* levmar.h:101: the interface version this library stands in for */
#define LM_OPTS_SZ 5
#define LM_INFO_SZ 10
#define LM_ERROR (-1)
#define LM_INIT_MU 1E-03
#define LM_STOP_THRESH 1E-17
#define LM_DIFF_DELTA 1E-06

/* adata payload of the BRDF callback: replaces `struct extraData`, brdfdata.cpp:962-966 (same layout).
 * angles is SoA: [0,n) cos(L.N), [n,2n) cos(N.H), [2n,3n) cos(R.V) (Phong) or cos(N.V) (Ward). */
struct brdf_extra_data {
  double *angles;
  int modelInfo; /* 0 Phong, 1 Blinn-Phong (brdfdata.h:44); 2 Ward (extension, not in the reference) */
};

enum { BRDF_MODEL_PHONG = 0, BRDF_MODEL_BLINN_PHONG = 1, BRDF_MODEL_WARD = 2 };
enum { BRDF_METHOD_DIF = 0, BRDF_METHOD_BC_DIF = 1,
       BRDF_METHOD_BC_DER = 2, /* device entry points: dlevmar_bc_der with the model's analytic Jacobian (BRDFJac_hip's) */
       BRDF_METHOD_DER = 3     /* device entry points: dlevmar_der with it */ };

/* ---- drop-in solver entry points ----------------------------------------------------------------- */

/* Replaces dlevmar_dif, levmar/levmar.h:112-115 (body lm_core.c:438-842).  Same arguments, return
 * value (#iterations or LM_ERROR) and info[0..9] meaning.  `work` is accepted and ignored (the
 * scratch lives in HBM); nothing is written to it.
 *   - `func` registered with brdf_hip_register_model (or BRDFFunc_hip): the BRDF model is evaluated by the
 *     library's device code, m must be 3 (x == NULL means a zero measurement vector, as in levmar).
 *   - any other `func`, 1 <= m <= 8: `func` is called on the host (it is the caller's code), all n-sized work
 *     around it runs on the device; small problems (n*m <= 65536) are summed in the reference's order and
 *     reproduce levmar bit for bit.
 *   - `covar` (this entry and the three below, for a registered model): where levmar leaves it unwritten or writes memory it
 *     never set -- itmax = 0, a stop before the first Jacobian (info[8] == 0), a singular J^T J ("singular matrix") -- the
 *     nine values returned are 0.0.  A refused call (n < m, a lower bound above its upper one) does not touch it. */
int dlevmar_dif(void (*func)(double *p, double *hx, int m, int n, void *adata), double *p, double *x,
                int m, int n, int itmax, double *opts, double *info, double *work, double *covar,
                void *adata);

/* Replaces dlevmar_bc_dif, levmar/levmar.h:124-127 (body lmbc_core.c:1062-1129 over :369-1022): the
 * call the application actually makes.  lb/ub/dscl may be NULL as in the reference; unlike the
 * reference, lb/ub are never rescaled in place when dscl is given. */
int dlevmar_bc_dif(void (*func)(double *p, double *hx, int m, int n, void *adata), double *p, double *x,
                   int m, int n, double *lb, double *ub, double *dscl, int itmax, double *opts,
                   double *info, double *work, double *covar, void *adata);

/* Replaces dlevmar_der, levmar/levmar.h:106-110 (body lm_core.c:64-432): unconstrained LM with the caller's
 * analytic Jacobian.  Host callbacks on the host, n-sized work on the device (generic path, 1 <= m <= 8). */
int dlevmar_der(void (*func)(double *p, double *hx, int m, int n, void *adata),
                void (*jacf)(double *p, double *j, int m, int n, void *adata), double *p, double *x, int m, int n,
                int itmax, double *opts, double *info, double *work, double *covar, void *adata);

/* Replaces dlevmar_bc_der, levmar/levmar.h:118-122 (body lmbc_core.c:369-1022): box-constrained LM with the
 * caller's analytic Jacobian jacf (row-major n x m, jac[i*m+j]).  func and jacf are host callbacks and are
 * called on the host; the residuals, J^T J, J^T e run on the device (generic path, 1 <= m <= 8). */
int dlevmar_bc_der(void (*func)(double *p, double *hx, int m, int n, void *adata),
                   void (*jacf)(double *p, double *j, int m, int n, void *adata), double *p, double *x, int m, int n,
                   double *lb, double *ub, double *dscl, int itmax, double *opts, double *info, double *work,
                   double *covar, void *adata);

/* levmar/levmar.h:357-361 (misc_core.c:598-611): standard deviation / Pearson correlation of the fitted
 * parameters from the m x m covariance returned through `covar`. */
double dlevmar_stddev(double *covar, int m, int i);
double dlevmar_corcoef(double *covar, int m, int i, int j);

/* levmar/levmar.h:376 (misc_core.c:616-658): coefficient of determination R^2 = 1 - SS_err / SS_tot of the model at p.
 * func is the caller's host callback (evaluated once, on the host); the three n-sized sums run on the device, in the
 * reference's descending order for n <= 65536.  x == NULL is read as a zero vector (the reference dereferences it). */
double dlevmar_R2(void (*func)(double *p, double *hx, int m, int n, void *adata), double *p, double *x, int m, int n,
                  void *adata);

/* levmar/levmar.h:336 (Axb_core.c:1140-1277): solves the m x m system A x = B by Crout LU with implicit row scaling and
 * partial pivoting; returns 1, or 0 if a row of A is zero.  A == NULL (the reference's "release the retained buffer"
 * call) does nothing and returns 1.  A scalar O(m^3) utility on the host for callers that link it (lmdemo-style
 * programs); the fitter itself solves its 3 x 3 systems in device registers.  Re-entrant, unlike the reference's. */
int dAx_eq_b_LU_noLapack(double *A, double *B, double *x, int m);

/* ---- single-precision twins: levmar/levmar.h:208-231 (slevmar_der / _dif / _bc_der / _bc_dif; the reference instantiates
 * them from the same *_core.c sources with LM_REAL = float, lm.c:43-63), :340 (sAx_eq_b_LU_noLapack), :364 (slevmar_chkjac),
 * :381-383 (slevmar_stddev / _corcoef / _R2).  Same semantics as the d-prefixed entry points above, all arithmetic in
 * float.  The callbacks are host code evaluated on the host (generic path, 1 <= m <= 8); the n-sized work -- residuals,
 * FD Jacobian fill, J^T J / J^T e, Broyden update -- runs on the device.  The BRDF application itself is double-only
 * (brdfdata.cpp:1058, :1119), so there is no registered-model shortcut for these. */
int slevmar_der(void (*func)(float *p, float *hx, int m, int n, void *adata), void (*jacf)(float *p, float *j, int m, int n, void *adata),
                float *p, float *x, int m, int n, int itmax, float *opts, float *info, float *work, float *covar, void *adata);
int slevmar_dif(void (*func)(float *p, float *hx, int m, int n, void *adata), float *p, float *x, int m, int n, int itmax, float *opts,
                float *info, float *work, float *covar, void *adata);
int slevmar_bc_der(void (*func)(float *p, float *hx, int m, int n, void *adata), void (*jacf)(float *p, float *j, int m, int n, void *adata),
                   float *p, float *x, int m, int n, float *lb, float *ub, float *dscl, int itmax, float *opts, float *info, float *work,
                   float *covar, void *adata);
int slevmar_bc_dif(void (*func)(float *p, float *hx, int m, int n, void *adata), float *p, float *x, int m, int n, float *lb, float *ub,
                   float *dscl, int itmax, float *opts, float *info, float *work, float *covar, void *adata);
void slevmar_chkjac(void (*func)(float *p, float *hx, int m, int n, void *adata), void (*jacf)(float *p, float *j, int m, int n, void *adata),
                    float *p, int m, int n, void *adata, float *err);
float slevmar_stddev(float *covar, int m, int i);
float slevmar_corcoef(float *covar, int m, int i, int j);
float slevmar_R2(void (*func)(float *p, float *hx, int m, int n, void *adata), float *p, float *x, int m, int n, void *adata);
int sAx_eq_b_LU_noLapack(float *A, float *B, float *x, int m);

/* Declares that `func` has the semantics of the reference's BRDFFunc (brdfdata.cpp:969-989): adata
 * points to a struct laid out like brdf_extra_data and the value depends on modelInfo.  A host
 * function pointer cannot run on the GPU; registration is how the drop-in entry points know they
 * may evaluate the model with the library's own HIP device code instead.  Returns 0, or -1 if the
 * table (16 entries) is full.  Thread-safe. */
int brdf_hip_register_model(void (*func)(double *p, double *hx, int m, int n, void *adata));
int brdf_hip_unregister_model(void (*func)(double *p, double *hx, int m, int n, void *adata));

/* A BRDFFunc-compatible callback evaluated on the GPU (kernel K1 alone): hx[i] = model(p; sample i).
 * Replaces BRDFFunc, brdfdata.cpp:969-989; always treated as registered. */
void BRDFFunc_hip(double *p, double *hx, int m, int n, void *adata);

/* The analytic Jacobian of the built-in models in levmar's jacf form (n x 3, row-major), evaluated on the GPU
 * (the reference only ever differentiates BRDFFunc numerically).  Passing it as `jacf` to
 * dlevmar_bc_der together with a registered `func` keeps the whole fit on the device (RQ_JAC passes then cost one
 * transcendental per sample instead of two and count no function evaluations, lmbc_core.c:1119-1124). */
void BRDFJac_hip(double *p, double *jac, int m, int n, void *adata);

/* Replaces dlevmar_chkjac, levmar/levmar.h:361-364 (body misc_core.c:250-321): err[i] near 1 where row i of jacf's
 * Jacobian agrees with func, near 0 where it does not.  func/jacf run on the host (caller's code), the comparison of
 * the n rows runs on the device. */
void dlevmar_chkjac(void (*func)(double *p, double *hx, int m, int n, void *adata),
                    void (*jacf)(double *p, double *j, int m, int n, void *adata), double *p, int m, int n, void *adata,
                    double *err);

/* ---- device-resident and batched entry points (extensions; the reference has no batched call) ----- */

/* One fit over samples already resident in HBM.  d_angles: 3*n doubles (planes as above), d_x: n
 * doubles, both DEVICE pointers.  p (in/out, 3), lb/ub/dscl (3 or NULL), opts (5 or NULL), info (10 or
 * NULL), covar (9 or NULL) are HOST pointers.  stream: a hipStream_t (NULL = default stream).
 * Returns as dlevmar_dif / dlevmar_bc_dif do. */
int brdf_hip_fit_dev(int method, int model, const double *d_angles, const double *d_x, int n, double *p,
                     const double *lb, const double *ub, const double *dscl, int itmax,
                     const double *opts, double *info, double *covar, void *stream);

/* K fits over ONE set of planes: what the reference's callers do with the three colour channels of a capture -- one
 * dlevmar_bc_dif call after the other over the same phi / thetaDash / theta (brdfdata.cpp:1159-1181, :1202-1219).  Channel c's
 * measurements are d_x + c * x_stride (device); p [channels][3] in/out, info [channels][10], covar [channels][9] (or NULL): HOST.
 * For BRDF_METHOD_BC_DIF / BRDF_METHOD_BC_DER with channels <= 3 and a fit that fits the chip the channels share ONE resident
 * launch (the planes are read and prepared once; while one channel's sums are exchanged and its LM step runs, the others
 * sweep): every channel's p, info and covar are bit-identical to brdf_hip_fit_dev on that channel alone.  Otherwise the
 * channels are fitted one after the other (same results).  Returns 0, or LM_ERROR if any channel's fit failed. */
int brdf_hip_fit_channels_dev(int method, int model, const double *d_angles, const double *d_x, long long x_stride, int n, int channels,
                              double *p, const double *lb, const double *ub, const double *dscl, int itmax, const double *opts,
                              double *info, double *covar, void *stream);
/* counters of channel `channel` of the most recent brdf_hip_fit_channels_dev on this thread; *shared_launch = 1 if it was one launch */
int brdf_hip_last_channels_stats(int channel, int *shared_launch, long long *passes, long long *jac_passes, double *device_us);
/* diagnostic builds (-DBRDF_STAMPS) only: shader cycles per section of that channel's control wave (1 waiting for the sweeping
 * waves, 2 reduction stage 2, 3 exchange, 4 LM step, 5 uniforms), summed over its passes */
int brdf_hip_last_channels_stamps(int channel, long long *out8);

/* S independent fits of n samples each -- the loop of CBRDFdata::CalcBRDFEquation
 * (brdfdata.cpp:1195-1220) as one call.  All array arguments are DEVICE pointers:
 *   d_angles[S][3][n], d_x[S][n], d_p[S][3] (in: starting points, out: fitted), d_info[S][10] (or NULL),
 *   d_ret[S] ints (or NULL; per-fit return value).
 * lb/ub/opts are HOST pointers shared by all fits.  method: any BRDF_METHOD_*.  n <= 4096: one launch (or two), a fit
 * per lane / wavefront / workgroup by size, asynchronous on `stream`.  n > 4096: the fits run one after the other, each
 * spread over the whole chip (the single-fit regimes of brdf_hip_fit_dev), and the call returns when they are done.
 * Returns 0 on success, LM_ERROR on bad arguments / launch failure. */
int brdf_hip_fit_batch_dev(int method, int model, const double *d_angles, const double *d_x, int S, int n,
                           double *d_p, const double *lb, const double *ub, int itmax,
                           const double *opts, double *d_info, int *d_ret, void *stream);

/* Host-pointer convenience over brdf_hip_fit_batch_dev (uploads, fits, downloads, synchronises).
 * Returns the number of fits that ended in LM_ERROR, or LM_ERROR itself on argument/HIP errors. */
int brdf_hip_fit_batch(int method, int model, const double *angles, const double *x, int S, int n,
                       double *p, const double *lb, const double *ub, int itmax, const double *opts,
                       double *info, int *ret);

/* brdf_hip_fit_batch over several GPUs: the S fits are split into ndev contiguous shards, shard k going to device
 * devices[k] (HIP ordinals of this process; a device may be listed more than once, devices == NULL: every visible
 * device once, ndev ignored).  Shard k holds fits [k*ceil(S/ndev), ...) -- the rule of brdf_amd/dist.py shard_range;
 * trailing shards may be short or empty.  Arguments and return value otherwise as brdf_hip_fit_batch: HOST pointers,
 * per-fit p/info/ret land in the caller's arrays, the return value is the number of fits that ended in LM_ERROR, or
 * LM_ERROR itself on bad arguments or a HIP failure (message in brdf_hip_last_error() of the calling thread).  Every
 * fit's p, info and ret are bit-identical to brdf_hip_fit_batch on one device.  The caller's current device is left as
 * it was, and so are the calling thread's brdf_hip_last_fit_* counters.
 *   - Arguments (null angles/x/p, S or n <= 0, an unknown model/method, ndev < 1 or > 64 with a list) are checked
 *     before any HIP call; device ordinals against hipGetDeviceCount before anything is uploaded.
 *   - One host thread per DISTINCT listed device, started by the call and joined before it returns: it creates its
 *     own stream and runs that device's shards one after the other in list order (upload, brdf_hip_fit_batch_dev,
 *     download).  A device listed twice never runs two shards of one call at the same time.  The buffers and the
 *     library's per-thread workspaces of a call are allocated by it and freed before it returns.
 *   - Errors: the first failed shard (in list order) is named as "device D, fits [a, b): <message>".  The other
 *     devices still finish their shards.  Results are downloaded only after a shard's fit succeeded: the rows of
 *     p / info / ret of a shard whose upload or fit failed, and of the later shards of the same device, are left as
 *     the caller passed them.
 *   - Two host threads that call brdf_hip_fit_batch_multi at the same time are serialised (one process-wide lock
 *     around the call). */
int brdf_hip_fit_batch_multi(int method, int model, const double *angles, const double *x, int S, int n, double *p,
                             const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret,
                             const int *devices, int ndev);
/* shard `shard` of this thread's most recent brdf_hip_fit_batch_multi: its device, first fit, fit count, and
 * milliseconds of upload / fit / download as that device's stream saw them (HIP events; 0 for a phase that did not
 * run, e.g. an empty shard); returns 0, or LM_ERROR if `shard` is out of range */
int brdf_hip_last_multi_stats(int shard, int *device, long long *first, long long *count, double *ms3);

/* ---- per-fit statistics at a fitted point (extensions) ------------------------------------------------------ */
/* What a single fit returns through `covar` and levmar's utilities, for S fits at once: one evaluation pass over the
 * samples of every fit at the point d_p[s] (kernels of their own, fit_stats.hip; the fit kernels are not involved).
 *   covar[s] = sumsq / (n - 3) * inverse(J^T J), levmar's LEVMAR_COVAR (misc_core.c:564-591, the same Crout LU), with
 *     J the Jacobian AT d_p[s] as `method` forms it -- BRDF_METHOD_DIF / _BC_DIF: finite differences with levmar's steps
 *     (delta = |opts[4]|, central when opts[4] < 0; opts == NULL: forward, LM_DIFF_DELTA), BRDF_METHOD_BC_DER / _DER: the
 *     analytic rows of BRDFJac_hip -- and sumsq = sum (x - f(p))^2.  For a converged dlevmar_bc_dif / _bc_der / _der fit
 *     this is the covariance levmar itself returns (it inverts the J^T J of its last iteration's point).  For dlevmar_dif
 *     it is the Jacobian at p, NOT levmar's secant (Broyden-updated) one, whose value depends on the path of the fit.
 *   stats[s] = { sumsq, R2, sd[0], sd[1], sd[2], rho01, rho02, rho12 }: R2 = 1 - sumsq / sum (x - mean x)^2 as dlevmar_R2
 *     (misc_core.c:616-658; the IEEE result when x is constant), sd[i] = sqrt(covar[i][i]) and rho_ij = covar[i][j] /
 *     sqrt(covar[i][i] covar[j][j]): dlevmar_stddev / dlevmar_corcoef on the returned covar[s] give the same values.
 *   rank[s] = 3, or 0 where J^T J has a zero row or any input or result is not finite; then covar[s] and the six
 *     values derived from it are 0.0 (what a single fit's covar shows in that case); sumsq and R2 are still written.
 * d_angles[S][3][n], d_x[S][n], d_p[S][3] (read only), d_covar[S][9], d_stats[S][BRDF_STATS_SZ], d_rank[S]: DEVICE
 * pointers, each output may be NULL (not all three); opts (5 or NULL): HOST, only opts[4] is read.  n >= 3.  All sums are
 * fixed-order trees: two calls give the same bits, and a fit's result does not depend on S or on its place in the batch.
 * Asynchronous on `stream`.  Arguments are checked before any HIP call.  Returns 0, or LM_ERROR with a message in
 * brdf_hip_last_error().  Not covered: dscl, a multi-GPU variant (call the host-pointer entry per device); weights only in
 * brdf_hip_fit_stats_batch_weighted_dev below (n <= 16). */
#define BRDF_STATS_SZ 8
int brdf_hip_fit_stats_batch_dev(int method, int model, const double *d_angles, const double *d_x, int S, int n,
                                 const double *d_p, const double *opts, double *d_covar, double *d_stats, int *d_rank,
                                 void *stream);
/* the same with HOST pointers: uploads, runs, downloads, synchronises */
int brdf_hip_fit_stats_batch(int method, int model, const double *angles, const double *x, int S, int n, const double *p,
                             const double *opts, double *covar, double *stats, int *rank);

/* ---- per-fit sample counts ("ragged" batches; extensions) ------------------------------------------------- */
/* brdf_hip_fit_batch_dev / brdf_hip_fit_stats_batch_dev for fits that do not all have n samples: fit s of a ragged batch is levmar
 * on the first counts[s] samples of its rows.  Leaving samples out of a fit (lights behind the surface, clipped pixels; see
 * brdf_amd.compact_samples and brdf_hip_fit_capture_masked_dev) is a fit of fewer samples.
 *   Layout      the uniform call's: d_angles[S][3][n], d_x[S][n]; n is the row stride and the largest count; d_counts[S] is a
 *               DEVICE array of ints (HOST in the two host-pointer entries).
 *   Samples     fit s uses samples [0, counts[s]) of each of its rows.
 *   Padding     entries at or behind counts[s] are never used: they may hold anything, NaN included, and no result depends on them.
 *   No counts   d_counts == NULL behaves exactly as the uniform entry point (it is that call).
 *   Too few     0 <= counts[s] < 3 is levmar's own n < m refusal (lm_core.c:502, lmbc_core.c:440): ret[s] = LM_ERROR, info[s] all
 *               zeros, p[s] as it came -- what the kernels do for any refused start.
 *   Out of range  a count < 0 or > n is treated the same way (the host cannot see it; nothing outside the row is read).
 *   Statistics  degrees of freedom are counts[s] - 3 and all sums run over the fit's own samples.  counts[s] < 3 or outside [0, n]:
 *               rank = 0, zero covar and zeros for the six values derived from it; sumsq and R2 are still written over the samples
 *               there are (both 0 for a count of 0 or out of range).
 *   Kernel      chosen by the stride n, as in the uniform calls: a batch whose counts span several size classes (<= 16, 64, 256,
 *               1024, 4096) runs EVERY fit in the stride's class -- a fit of 5 samples in rows of 4096 occupies a whole workgroup.
 *               Batches with very unequal counts belong in the packed entries below, which bucket by size class.  Within the
 *               stride's own class a fit's p / info / ret (and covar / stats / rank) are bit-identical to the uniform call with
 *               n = counts[s] on that fit alone; below it they agree as two summation orders do.
 *   n > 4096    the fits run one after the other through the single-fit regimes with n = counts[s] (the counts are copied to the
 *               host next to p; a count below 3 is refused there without a launch); the statistics run the uniform pass per fit
 *               with S = 1, n = counts[s].  Both synchronise the stream.
 *   Checks      everything the host can see (null pointers, S or n <= 0, unknown model / method, lb > ub) is checked before any
 *               HIP call.
 * Not covered: dscl, brdf_hip_fit_batch_multi; per-sample weights only as below (n <= 16, dlevmar_bc_dif / dlevmar_bc_der). */
int brdf_hip_fit_batch_ragged_dev(int method, int model, const double *d_angles, const double *d_x, const int *d_counts, int S, int n,
                                  double *d_p, const double *lb, const double *ub, int itmax, const double *opts, double *d_info,
                                  int *d_ret, void *stream);
int brdf_hip_fit_batch_ragged(int method, int model, const double *angles, const double *x, const int *counts, int S, int n, double *p,
                              const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret);
int brdf_hip_fit_stats_batch_ragged_dev(int method, int model, const double *d_angles, const double *d_x, const int *d_counts, int S,
                                        int n, const double *d_p, const double *opts, double *d_covar, double *d_stats, int *d_rank,
                                        void *stream);
int brdf_hip_fit_stats_batch_ragged(int method, int model, const double *angles, const double *x, const int *counts, int S, int n,
                                    const double *p, const double *opts, double *covar, double *stats, int *rank);

/* ---- per-sample weights, n <= 16 (extensions) --------------------------------------------------------------- */
/* The ragged batch above with a weight per sample, in ONE size class: n <= 16 (the application's own: 16 lights per surfel) and
 * BRDF_METHOD_BC_DIF / BRDF_METHOD_BC_DER.
 *   Definition  fit s is levmar (dlevmar_bc_dif, or dlevmar_bc_der with the device Jacobian) on the weighted problem
 *               hx_i = sqrt(w_i) f_i(p), x'_i = sqrt(w_i) x_i over the first counts[s] samples of its rows: what a levmar caller
 *               does today by scaling inside the callback.  info[1] = sum w_i (x_i - f_i(p))^2.
 *   Layout      d_w[S][n] has the layout of d_x; d_counts[S] as in the ragged call, or NULL: every fit has n samples.
 *   Unit weights  w = 1.0 everywhere returns the BYTES of brdf_hip_fit_batch_ragged_dev (the statistics: of
 *               brdf_hip_fit_stats_batch_ragged_dev): every operation the weights add is exact then.
 *   Zero        a weight of 0 is a sample that contributes nothing and still counts in n.
 *   Refused     a fit whose counted samples include a weight that is negative or not finite is refused as n < m is: ret[s] =
 *               LM_ERROR, info[s] all zeros, p[s] as it came.  Nothing at or behind counts[s] is read.
 *   Statistics  at d_p[s], with J the Jacobian of the weighted problem as `method` forms it:  sumsq = sum w e^2 (+ extra_ss[s]);
 *               covar = sumsq / (nobs[s] - 3) * inverse(J^T W J);  R2 = 1 - sumsq / SStot, SStot = sum w (x - mean)^2 (+ extra_ss[s]),
 *               mean = sum w x / sum w;  sd, rho and rank as in brdf_hip_fit_stats_batch_dev.  d_extra_ss[S] (DEVICE, may be NULL)
 *               is a sum of squares that does not depend on p -- for a fit of group means weighted by the groups' sizes, the
 *               spread of the observations inside their groups, which makes sumsq, covar and R2 those of the fit of all
 *               observations.  d_nobs[S] (DEVICE, may be NULL: the fit's count) is the observation count of the degrees of freedom.
 *               A count below 3: rank 0 as in the ragged pass; a negative or non-finite weight: rank 0, sumsq and R2 not finite.
 *   Checks      refused before any HIP call, under the entry's own name: n > 16, a method other than BRDF_METHOD_BC_DIF /
 *               BRDF_METHOD_BC_DER, NULL weights, and everything the ragged entries refuse.
 * The host-pointer twins upload, run, download and synchronise; brdf_hip_fit_batch_weighted returns the number of fits that ended in
 * LM_ERROR.  Not covered: weights above 16 samples per fit, for dlevmar_dif / dlevmar_der, and in the packed, multi-GPU and
 * single-fit calls; dscl. */
int brdf_hip_fit_batch_weighted_dev(int method, int model, const double *d_angles, const double *d_x, const double *d_w, const int *d_counts,
                                    int S, int n, double *d_p, const double *lb, const double *ub, int itmax, const double *opts,
                                    double *d_info, int *d_ret, void *stream);
int brdf_hip_fit_batch_weighted(int method, int model, const double *angles, const double *x, const double *w, const int *counts, int S, int n,
                                double *p, const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret);
int brdf_hip_fit_stats_batch_weighted_dev(int method, int model, const double *d_angles, const double *d_x, const double *d_w,
                                          const int *d_counts, int S, int n, const double *d_p, const double *opts, const double *d_extra_ss,
                                          const int *d_nobs, double *d_covar, double *d_stats, int *d_rank, void *stream);
int brdf_hip_fit_stats_batch_weighted(int method, int model, const double *angles, const double *x, const double *w, const int *counts, int S,
                                      int n, const double *p, const double *opts, const double *extra_ss, const int *nobs, double *covar,
                                      double *stats, int *rank);

/* ---- packed batches: fits of any size in one call (extensions) --------------------------------------------- */
/* S fits laid back to back, CSR style, bucketed by size class (<= 16, 64, 256, 1024, 4096 samples, and above) inside the library:
 * what a caller of the ragged entries above had to do by hand when the counts of a batch span several classes.
 *   Layout      d_offsets[S + 1]: a DEVICE array of long long (HOST in the two host-pointer entries), non-decreasing; fit s has
 *               k_s = offsets[s + 1] - offsets[s] samples.  Its three planes are k_s doubles each, contiguous, at d_angles + 3 * offsets[s]
 *               -- the single-fit layout of brdf_hip_fit_dev -- and its measurements at d_x + offsets[s].  offsets[0] need not be 0;
 *               nothing outside [offsets[0], offsets[S]) is ever read.  The uniform batch angles[S][3][n] is offsets[s] = s * n.
 *               d_p[S][3], d_info[S][10] (or NULL), d_ret[S] (or NULL) are the uniform call's.
 *   Definition  for k_s >= 3, fit s returns the BYTES brdf_hip_fit_batch_dev returns for that fit alone with n = k_s (covar / stats /
 *               rank: those of brdf_hip_fit_stats_batch_dev), whatever else is in the batch and wherever the fit stands in it.
 *   Too few     0 <= k_s < 3 is levmar's n < m refusal, as in the ragged call: ret[s] = LM_ERROR, info[s] all zeros, p[s] as it came;
 *               the statistics are what the ragged pass writes for such a count (rank 0, zeros; sumsq and R2 over the samples there are).
 *   Decreasing  a negative difference of two offsets (and, in the device entries, one above INT_MAX) is treated as a count of 0.
 *   How         a plan on the device (count and class of every fit; a stable partition of the fit indices by class), then per class,
 *               in chunks of what the workspace holds: a gather of the chunk's segments into padded rows of the class's largest
 *               count, the ragged call of that class, a scatter of the results to the caller's rows.  Fits above 4096 samples are
 *               not copied: they run where they lie, one after the other, each spread over the chip, as in the uniform call.
 *   One wait    the call waits for `stream` ONCE, to read the plan (six fit counts, six largest counts) back.  With fits above 4096
 *               samples it waits again around them, as the uniform call does (their starting points travel to the host in one copy,
 *               their results back in one).  The rest is asynchronous on `stream`.
 *   Workspace   stream-ordered allocations (hipMallocAsync / hipFreeAsync) bounded by workspace_bytes; 0: 1 GiB.  A chunk holds
 *               max(1, workspace_bytes / bytes per padded fit) fits, bytes per padded fit = 8 * (4 * stride + 30) + 12, stride = the
 *               class's largest count (at least 3).  The size of a chunk never shows in a result.
 *   Checks      null pointers, S <= 0, workspace_bytes < 0, an unknown model / method, lb > ub -- and in the host-pointer entries
 *               offsets that decrease and a fit of more than INT_MAX samples -- are refused before any HIP call.
 *   Host entries  upload the offsets[S] - offsets[0] samples the batch covers; brdf_hip_fit_batch_packed returns the number of fits
 *               that ended in LM_ERROR (refused ones included), as brdf_hip_fit_batch does.
 * Not covered: per-sample weights (n <= 16 only: brdf_hip_fit_batch_weighted_dev), dscl, a packed brdf_hip_fit_batch_multi. */
int brdf_hip_fit_batch_packed_dev(int method, int model, const double *d_angles, const double *d_x, const long long *d_offsets, int S,
                                  double *d_p, const double *lb, const double *ub, int itmax, const double *opts, double *d_info, int *d_ret,
                                  long long workspace_bytes, void *stream);
int brdf_hip_fit_batch_packed(int method, int model, const double *angles, const double *x, const long long *offsets, int S, double *p,
                              const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret,
                              long long workspace_bytes);
int brdf_hip_fit_stats_batch_packed_dev(int method, int model, const double *d_angles, const double *d_x, const long long *d_offsets, int S,
                                        const double *d_p, const double *opts, double *d_covar, double *d_stats, int *d_rank,
                                        long long workspace_bytes, void *stream);
int brdf_hip_fit_stats_batch_packed(int method, int model, const double *angles, const double *x, const long long *offsets, int S,
                                    const double *p, const double *opts, double *covar, double *stats, int *rank, long long workspace_bytes);
/* ---- sigma-clipped packed batches (extensions) ------------------------------------------------------------------------------ */
/* Fit, drop the samples further than kappa sigma from the fit, fit the survivors again, until nothing more is dropped: the remedy for
 * samples a validity rule fixed before the fit cannot see (a highlight that does not clip, a cast shadow, an inter-reflection, a
 * pixel whose map entry names the wrong face).  The inputs are a packed batch, as for brdf_hip_fit_batch_packed_dev, plus kappa,
 * sigma_min and rounds.  No fit or statistics kernel of its own: the fits and the statistics are the packed entries'.
 *   Round 0      every fit runs from d_p on all of its samples: the bytes of brdf_hip_fit_batch_packed_dev.
 *   Settled      a fit that is refused (k < 3) or ends with ret < 0 is settled: it keeps those outputs and all of its samples.
 *   Clip rounds  r = 1 ... rounds, for every fit that is not settled, with its k current samples at its current p:
 *                  sumsq is stats[0] of brdf_hip_fit_stats_batch_packed_dev on the current sample set at p (the exact path, sums in
 *                  fixed-order trees).  A sumsq that is not finite settles the fit with nothing clipped.
 *                  sigma = fmax(sqrt(sumsq / (k - 3)), sigma_min) for k > 3; for k == 3, sigma = sigma_min.
 *                  Sample i survives iff fabs(x_i - f_i(p)) <= kappa * sigma, f on the exact path (the reference's own pow
 *                  expression, as the statistics pass evaluates it).  A NaN residual fails the comparison.
 *                  No sample dropped: the fit is settled.  Fewer than 3 survivors: the clip is NOT applied and the fit is settled.
 *                  Otherwise the survivors replace the fit's sample set, keeping their order -- clipping is monotone, a dropped
 *                  sample never returns -- and the fit runs again from its current p: its p, info and ret become the bytes of
 *                  brdf_hip_fit_batch_packed_dev on the survivors from that p, and rounds_used[s] = r.  A refit that ends with
 *                  ret < 0 settles the fit with those outputs.  The loop ends early when every fit is settled.
 *   Statistics   covar, stats and rank are the bytes of brdf_hip_fit_stats_batch_packed_dev at the returned p over the returned
 *                sample set.
 *   Invariant    every returned fit is a fit OF ITS RETURNED SAMPLE SET: p, info and ret are the packed call's bytes on that set
 *                from the previous round's p, the statistics the packed pass's bytes at its own p.  rounds = 0, or kappa = +inf,
 *                returns the bytes of the two packed entries, a mask of ones, kept = k and rounds_used = 0.
 *   Outputs      d_info[S][10], d_ret[S], d_covar[S][9], d_stats[S][BRDF_STATS_SZ], d_rank[S], d_kept[S] (the samples of the fit's
 *                returned set), d_rounds_used[S], d_mask[offsets[S] - offsets[0]] (1 = in the returned set, by the caller's
 *                sample position: sample i of fit s is d_mask[offsets[s] - offsets[0] + i]): DEVICE, each may be NULL.
 *   sigma_min    the floor of sigma: for 8-bit captures 1 / (255 sqrt(12)) = 0.0011320..., the quantisation's standard deviation,
 *                is recommended -- a fit that matches its samples to the last bit must not clip on rounding.  0 is allowed.
 *   Method       any BRDF_METHOD_*: the clip does not depend on it; the statistics use the method's Jacobian, as the packed pass does.
 *   Waits        the call waits for `stream` as the packed calls do, once per fit and per statistics call (round 0, and per clip
 *                round one statistics call and -- where a fit was clipped -- one refit; a last statistics call where the last
 *                round refitted), once to read offsets[0] and offsets[S] (with rounds > 0 or a mask), and once per clip round for
 *                one readback: is any fit still active?  With rounds > 0 or a mask it returns with the stream drained.
 *   Memory       per sample position 38 bytes with rounds > 0 (the working batch of survivors 32, the fit of the position 4, the
 *                round's decision 1, the mask 1 where d_mask is NULL), 32 bytes per surviving sample of the fits a round clips (its
 *                refit batch) and 24 bytes per 256 positions; per fit about 250 bytes; and the packed calls' own workspace_bytes
 *                (0: 1 GiB).  The caller's batch is never written.  rounds = 0 allocates nothing: it runs the packed calls' launches, one small
 *                kernel for d_kept and d_rounds_used and, with a mask, one wait for the extent and one more small kernel for the ones.
 *   Offsets      with rounds > 0 the device offsets must not descend (nor differ by more than INT_MAX): the clip rounds give every sample
 *                position ONE fit.  Checked on the device and read back with the extent; such a batch is refused before round 0 writes
 *                anything, where the packed entries -- and this one at rounds = 0 -- read the pair as a count of 0.
 *   Checks       refused before any HIP call, under the entry's name: everything the packed entries refuse; a kappa that is not > 0
 *                (a NaN included; +inf is allowed); a sigma_min that is negative or a NaN; rounds outside [0, 16].
 *   Host entry   uploads, runs, downloads, synchronises; returns the number of fits with ret < 0.
 * Not covered: clipping in the means capture by this entry (brdf_hip_fit_capture_means_dev: its fits see means, not samples --
 * brdf_hip_fit_capture_means_clipped_dev below clips it by grey-level intervals), in the masked
 * per-pixel capture (brdf_hip_fit_capture_masked_dev: 16-sample fits, too few to estimate sigma) and in the single-BRDF capture
 * (brdf_hip_fit_capture_single_faces_dev); a MAD or another robust scale; dscl; a multi-GPU variant. */
int brdf_hip_fit_batch_packed_clipped_dev(int method, int model, const double *d_angles, const double *d_x, const long long *d_offsets, int S,
                                          double *d_p, const double *lb, const double *ub, int itmax, const double *opts, double kappa,
                                          double sigma_min, int rounds, double *d_info, int *d_ret, double *d_covar, double *d_stats, int *d_rank,
                                          int *d_kept, int *d_rounds_used, unsigned char *d_mask, long long workspace_bytes, void *stream);
int brdf_hip_fit_batch_packed_clipped(int method, int model, const double *angles, const double *x, const long long *offsets, int S, double *p,
                                      const double *lb, const double *ub, int itmax, const double *opts, double kappa, double sigma_min, int rounds,
                                      double *info, int *ret, double *covar, double *stats, int *rank, int *kept, int *rounds_used,
                                      unsigned char *mask, long long workspace_bytes);
/* clip round `round` (1 ...) of the calling thread's last clipped call: the fits that were clipped and refitted in it, and the
 * samples it dropped.  LM_ERROR for a round the call did not run (it stops after the first round that clips nothing). */
int brdf_hip_last_clip_stats(int round, long long *active_fits, long long *clipped_samples);
/* class cls (0: <= 16 samples ... 4: <= 4096, 5: above) of the calling thread's last packed call: its fits, the row stride of its
 * launches (0 for an empty class; class 5: the largest count) and its chunks (class 5: one run per fit).  LM_ERROR for another cls. */
int brdf_hip_last_packed_stats(int cls, long long *fits, int *stride, int *chunks);
/* The kernel the calling thread's last batched launch chose (uniform, ragged, weighted, or one class of a packed call), so that a
 * caller who sets a tuning switch can see that it was obeyed.  *kernel: 0 one lane per fit, 1 four fits per wave, 2 one wave per fit,
 * 3 one workgroup per fit, 4 eight waves per fit, 5 the 512 x 8 geometry (BRDF_HIP_BATCH_BIG=0), 6 one lane per weighted fit;
 * *waves_per_simd: the chosen instance's launch bound (kernels 0 and 6: BRDF_HIP_LANE_WAVES; 0 where the kernel states none);
 * *grid: workgroups launched; *quorum, *maxwait: BRDF_HIP_LANE_QUORUM / _MAXWAIT as kernels 0 and 6 received them (0 elsewhere).
 * Any pointer may be NULL.  LM_ERROR while the thread has launched no batch. */
int brdf_hip_last_batch_launch(int *kernel, int *waves_per_simd, long long *grid, int *quorum, int *maxwait);

/* hx[i] = model(p; sample i) for device-resident planes; d_hx DEVICE pointer, p HOST pointer. */
int brdf_hip_model_eval_dev(int model, const double *d_angles, int n, const double *p, double *d_hx,
                            void *stream);

/* Synthetic sample generator on the device (bench support; bit-identical to brdf_amd/synth.py's
 * counter stream for the planes).  Fills d_angles[count][3][n], d_x[count][n] for surfels
 * [first, first+count) with per-surfel truth d_truth[count][3] (device) . */
int brdf_hip_synth_dev(int model, unsigned long long seed, long long first, int count, int n,
                       const double *d_truth, double *d_angles, double *d_x, void *stream);

/* ---- mesh + camera -> the capture entries' inputs: face normals and the pixel-to-face map ------------------ */
/* CBRDFdata::CalcFaceNormals (brdfdata.cpp:314-330) on the device, one lane per face:
 *   e1 = v2 - v1, e2 = v3 - v1, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), then Eigen's normalize():
 *   if ((n0^2 + n1^2) + n2^2 > 0) every component is divided by its square root, otherwise n stays as it is.
 * d_vertices[nv][3], d_faces[nf][3], d_normals[nf][3]: device.  A face with a vertex index outside [0, nv) gets a NaN normal.
 * Enqueues on `stream` and returns: 0, or LM_ERROR with a message in brdf_hip_last_error() (a null pointer; nv or nf outside
 * 1 ... INT_MAX: refused before any HIP call). */
int brdf_hip_face_normals_dev(const double *d_vertices, long long nv, const int *d_faces, long long nf, double *d_normals,
                              void *stream);

/* The pixel map every capture entry reads, from the mesh and the camera: replaces CBRDFdata::CalcPixel2SurfaceMapping
 * (brdfdata.cpp:629-681), which needs a live GL context.  model_view[16], projection[16] (column-major, as glGetDoublev returns
 * them) and viewport[4] are HOST arrays: the application's three glGet* results go in unchanged.
 *   Projection     gluProject's arithmetic: out_i = ((in0 m[i] + in1 m[4+i]) + in2 m[8+i]) + in3 m[12+i] with model_view (in3 = 1),
 *                  then with projection; w == 0 or anything not finite: the vertex is unprojectable; otherwise x, y, z are divided
 *                  by w, t = v 0.5 + 0.5, winX = t_x viewport[2] + viewport[0], winY likewise, winZ = t_z.
 *   mode 0         the reference's map: per face the centroid ((a + b) + c) / 3.0 per coordinate, projected;
 *                  if (winY >= 0 && winX >= 0) map[(int)winY][(int)winX] = face.  Of several faces in one pixel the HIGHEST index
 *                  wins (the reference's serial loop lets the last one win).  One deviation: the reference never checks the upper
 *                  bound and writes out of bounds; here (int)winX >= W or (int)winY >= H writes nothing and is counted.
 *   mode 1         rasterised and z-buffered.  A face is dropped when a vertex is unprojectable or has w <= 0 after the projection
 *                  matrix (there is no near-plane clipping), when its window-space area
 *                  A = (bx - ax)(cy - ay) - (by - ay)(cx - ax) is 0 or not finite, or when cull = 1 and A < 0.  Pixel (col, row) is
 *                  covered iff the three edge functions at its centre p = (col + 0.5, row + 0.5),
 *                    E0 = (bx - px)(cy - py) - (by - py)(cx - px), E1 = (cx - px)(ay - py) - (cy - py)(ax - px),
 *                    E2 = (ax - px)(by - py) - (ay - py)(bx - px),
 *                  each multiplied by the sign of A, are all >= 0 (inclusive: two faces sharing an edge both cover a centre on it)
 *                  and its depth z = ((E0 az + E1 bz) + E2 cz) / A lies in [0, 1].  The pixel's owner is the covering face of
 *                  least z, and among equal z the lowest face index.  Candidates are the pixels whose centres lie in the face's
 *                  bounding box, clamped to the viewport [0, W) x [0, H).
 *   d_pixel_map[H][W]  int32: face index or -1; row y is window row y, bottom-up -- the layout every capture entry reads.
 *   d_depth[H][W]      double, or NULL: the owner's z (mode 0: the centroid's winZ); 2.0 where no face owns the pixel.
 *   d_face_pixels[nf]  int32, or NULL: the number of pixels each face owns.
 *   stats[8]           HOST, or NULL: faces rasterised (mode 0: centroids written); faces dropped as unprojectable or w <= 0 (or
 *                      with a vertex index outside [0, nv)); dropped as degenerate; culled; wholly outside the viewport (mode 0:
 *                      winX < 0 or winY < 0); candidates visited; pixels owned; writes refused by mode 0's upper bound.
 * The result is exact and deterministic (integer atomics only): two calls give the same bytes.  Refused before any HIP call: H, W < 1,
 * H W, nv or nf beyond INT_MAX, nv or nf < 1, mode or cull outside 0 | 1, a null required pointer, a matrix or viewport entry that
 * is not finite, viewport[2] or viewport[3] <= 0.  Synchronises `stream` before returning.  Returns 0 or LM_ERROR. */
int brdf_hip_pixel_map_dev(const double *d_vertices, long long nv, const int *d_faces, long long nf, const double *model_view,
                           const double *projection, const double *viewport, int H, int W, int mode, int cull, int *d_pixel_map,
                           double *d_depth, int *d_face_pixels, long long *stats, void *stream);

/* ---- cast shadows: which lights a face can see, and that visibility painted into the captures ---------------- */
/* Per face one 64-bit word, bit l set iff light l is visible from the face's centre.  The reference has no counterpart (its
 * voxel-grid shadow code in brdfdata.cpp is commented out).  d_vertices[nv][3], d_faces[nf][3], d_normals[nf][3] (or NULL) and
 * d_face_lit[nf] are device arrays; leds[L][3], 1 <= L <= 64, and stats[5] (or NULL) are HOST arrays.
 *   dot3(x, y) = (x0 y0 + x1 y1) + x2 y2;   x cross y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0).
 *   Valid face     its three indices lie in [0, nv) and its nine coordinates are finite.  An invalid face has lit = 0 and
 *                  occludes nothing.
 *   Origin         o[k] = ((a[k] + b[k]) + c[k]) / 3.0 of the face's corners a, b, c: the centre the cosines use.
 *   Direction      d = P_l - o.
 *   Facing away    with normals: !(dot3(n_f, d) > 0).  The bit is clear; the pair counts in stats[2] and in neither stats[3] nor
 *                  stats[4].  Without normals no pair faces away.
 *   Shadowed       otherwise, iff some valid face g != f is hit; with v0, v1, v2 the corners of g:
 *                    e1 = v1 - v0, e2 = v2 - v0, h = d cross e2, a = dot3(e1, h), s = o - v0, q = s cross e1,
 *                    U = dot3(s, h), V = dot3(d, q), T = dot3(e2, q); if a < 0, U, V and T are negated; A = |a|;
 *                    hit iff A > 0 && U >= 0 && V >= 0 && U + V <= A && T > t_min A && T < (1.0 - t_min) A.
 *                  No division.  Edges are inclusive; a ray parallel to the occluder's plane misses; a NaN misses; an occluder
 *                  beyond the light or behind the origin casts nothing.  Coplanar neighbours do not shadow each other: the
 *                  origin is interior to f, and T is rounding noise below t_min A.
 *   Lit            a pair that neither faces away nor is shadowed.
 *   stats[5]       valid faces, invalid faces, pairs (valid face, light) facing away, pairs lit, pairs shadowed.
 * Brute force, nf^2 L tests and no acceleration structure: the result depends on mesh and rig alone, so it is computed once per
 * capture session.  Exact and deterministic (integer atomicAnd on the words only): two calls give the same bytes, those of the
 * NumPy twin brdf_amd.light_visibility_host.  Workspace O(nf).  Refused before any HIP call: a null required pointer, L outside
 * [1, 64], nv or nf < 1 or beyond INT_MAX, a light coordinate that is not finite, t_min outside [0, 0.5) or a NaN.  Synchronises
 * `stream` before returning.  Returns 0 or LM_ERROR. */
int brdf_hip_light_visibility_dev(const double *d_vertices, long long nv, const int *d_faces, long long nf, const double *d_normals,
                                  const double *leds, int L, double t_min, unsigned long long *d_face_lit, long long *stats,
                                  void *stream);

/* The visibility words into images: for light l and map pixel (y, x) whose entry f lies in [0, nf) and whose bit l of
 * d_face_lit[f] is clear, the three bytes at image row H - 1 - y, column x of image l become `level` (0 ... 255) -- the captures'
 * layout, as brdf_hip_capture_render_dev writes it.  Every other byte of d_out[L][H][W][3] is d_images'.  d_out may be d_images
 * itself (in place: only painted bytes are written); a buffer that overlaps it in part is refused.  d_shadowed[L] (device, or
 * NULL): the painted pixels per light.  Bit l means image l: for held-out lights compute a word for those lights.
 * This carries shadows into EVERY capture entry without a change to any of them: paint level = 0 and fit with v_min >= 1.  A mask
 * argument in the grouped validity rule itself, which would also serve v_min = 0 callers, would change every capture entry's ABI
 * and is left out on purpose.  One pass over the images.  Refused before any HIP call: a null required pointer, L outside
 * [1, 64], H, W or nf < 1, H W beyond INT_MAX, level outside 0 ... 255, a partial overlap.  Enqueues on `stream` and returns 0 or
 * LM_ERROR. */
int brdf_hip_capture_apply_visibility_dev(const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                          const unsigned long long *d_face_lit, int nf, int level, unsigned char *d_out,
                                          unsigned long long *d_shadowed, void *stream);

/* ---- the step before the fit: vectors -> cosines ---------------------------- */
/* Replaces CBRDFdata::GetCosLN / GetCosNH / GetCosRV (brdfdata.cpp:859-899, :902-943, :799-857), which the reference
 * evaluates per pixel / per face and per light on the host.  One launch fills, for S surfels, the three cosine planes
 * in the batched fitter's layout d_angles[S][3][L] (struct extraData's SoA planes, brdfdata.cpp:962-966, per surfel;
 * for L = 16 this is exactly what brdf_hip_fit_batch_dev reads with n = 16).
 *   d_vertices[nv][3], d_faces[nf][3] (vertex indices), d_face_normals[nf][3]: device, row-major (m_vertices, m_faces,
 *   face_normals); d_surfels[S]: face index of every surfel (the pixel map's entries, brdfdata.cpp:1197), or NULL for
 *   surfel s = face s; leds[L][3], view_origin[3]: HOST (m_led, m_p), L <= 64.
 *   rv_mode 0: GetCosRV's arithmetic exactly as written, including its slips (:835 builds the light vector from the
 *   centroid's x three times, :849 returns R.P); rv_mode 1: cos(R.V) of the geometry its comments describe.
 * Returns 0, or LM_ERROR with a message in brdf_hip_last_error(). */
int brdf_hip_cosines_dev(const double *d_vertices, const int *d_faces, const double *d_face_normals, const int *d_surfels,
                         long long S, const double *leds, int L, const double *view_origin, int rv_mode, double *d_angles,
                         void *stream);
/* CBRDFdata::InitLEDs (brdfdata.cpp:683-752): the capture rig's 16 LED positions, row-major [16][3] (host) */
void brdf_hip_led_table(double *leds16x3);

/* ---- the capture loop ---------------------------------------------------------- */
/* Replaces the pixel loop of CBRDFdata::CalcBRDFEquation (brdfdata.cpp:1188-1227) with its callees
 * GetIntensities_FromPixel (:945-960), GetCos* (:799-943), SolveEquation (:1077-1136: dlevmar_bc_dif, n = L) and
 * SaveValuesToSurface (:368-377).  For every pixel (x outer, y inner, as the reference walks) whose pixel-map entry is a
 * face index: the L intensities image_i(H-1-y, x)[channel] / 255.0 of each of the three channels (B, G, R) are fitted
 * from p0 and the result is stored in d_brdf_surfaces[face][channel] = {kd, ks, n}; when several pixels carry the same
 * face the LAST one in the reference's walk wins, as in the reference.  Faces no pixel carries are left untouched.
 *   d_images[L][H][W][3]: the L captures, 8-bit BGR, row-major (cv::Mat CV_8UC3); d_pixel_map[H][W]: face index or -1
 *   (pixelMap.at<int>(y, x)); mesh, leds, view_origin, rv_mode: as brdf_hip_cosines_dev; p0/lb/ub/opts: HOST.
 *   avg (host, or NULL): sum over all fits of kd, ks, n divided by (nf * 3), the statistics of brdfdata.cpp:1224-1226;
 *   n_pixels (host, or NULL): number of pixels that carried a face (3 fits each).
 * Synchronises `stream` before returning.  Returns 0, or LM_ERROR with a message in brdf_hip_last_error(). */
int brdf_hip_fit_capture_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                             const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                             const double *leds, const double *view_origin, int rv_mode, const double *p0, const double *lb,
                             const double *ub, int itmax, const double *opts, double *d_brdf_surfaces, double *avg,
                             long long *n_pixels, void *stream);

/* brdf_hip_fit_capture_dev followed by the statistics pass of brdf_hip_fit_stats_batch_dev (BRDF_METHOD_BC_DIF, the call's
 * opts) over the fits it stored: d_surface_covar[nf][3][9], d_surface_stats[nf][3][BRDF_STATS_SZ], d_surface_rank[nf][3]
 * (DEVICE, each may be NULL) receive, per face and channel, the statistics of the fit whose {kd, ks, n} went into
 * d_brdf_surfaces -- the face's LAST pixel.  Faces no pixel carries are left untouched in all maps.  d_brdf_surfaces, avg
 * and n_pixels are bit-identical to brdf_hip_fit_capture_dev's.  (The single-BRDF capture below already returns info[]; its
 * covariance is available through brdf_hip_fit_channels_dev.) */
int brdf_hip_fit_capture_stats_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                   const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                                   const double *leds, const double *view_origin, int rv_mode, const double *p0,
                                   const double *lb, const double *ub, int itmax, const double *opts, double *d_brdf_surfaces,
                                   double *avg, long long *n_pixels, void *stream, double *d_surface_covar,
                                   double *d_surface_stats, int *d_surface_rank);

/* brdf_hip_fit_capture_stats_dev with a validity rule: sample i (light i) of fit q = 3 pixel + channel takes part iff
 *   v_min <= value <= v_max, value being the 8-bit intensity image_i(H-1-y, x)[channel], AND
 *   every cosine plane the model reads is > cos_min: cos(L.N) always; cos(N.H) for Blinn-Phong and Ward; the third plane
 *   (cos(R.V) / cos(N.V)) for Phong and Ward.
 * v_min = 0, v_max = 255 switches the intensity test off, any cos_min < -1 the cosine test.  A fit's valid samples are moved to the
 * front of its rows, stably in light order (one more kernel behind the gather and the cosines), and the fits run as
 * brdf_hip_fit_batch_ragged_dev with these counts; the statistics tail is the ragged statistics pass.
 *   d_surface_count[nf][3] (DEVICE, may be NULL): the sample count of the fit whose result was stored for the face and channel;
 *   faces no pixel carries are left untouched.  A fit refused for count < 3 leaves p0 in d_brdf_surfaces, as any failed fit does:
 *   the count map is how the caller tells.
 * With both conditions off, d_brdf_surfaces, avg, n_pixels and the three statistics maps are bit-identical to
 * brdf_hip_fit_capture_stats_dev wherever the cosines are numbers.  A NaN cosine is never a sample, also with the rule switched off;
 * on such a face (a degenerate triangle with a NaN normal) the rule-off call refuses the fit -- count 0, p0 in d_brdf_surfaces,
 * sumsq = R2 = 0 -- where the unmasked capture stops it with reason 7: p0 as well, but a NaN sumsq and R2.  Returns LM_ERROR for v_min > v_max as for the other bad arguments, before any HIP call.
 * The same rule for the single-BRDF fit is brdf_hip_fit_capture_single_faces_dev below.  Not covered: the multi-GPU batch. */
int brdf_hip_fit_capture_masked_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                    const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                                    const double *leds, const double *view_origin, int rv_mode, const double *p0,
                                    const double *lb, const double *ub, int itmax, const double *opts, double *d_brdf_surfaces,
                                    double *avg, long long *n_pixels, void *stream, double *d_surface_covar,
                                    double *d_surface_stats, int *d_surface_rank, int v_min, int v_max, double cos_min,
                                    int *d_surface_count);

/* The capture with ONE fit per (face, channel) over the samples of ALL the face's pixels, where the three entries above fit every
 * pixel on its own (n = L) and keep the fit of the face's last pixel.  The capture becomes a packed batch on the device and the
 * packed entries above fit it (BRDF_METHOD_BC_DIF); no fit or statistics kernel of its own.  Capture, mesh, leds, view_origin,
 * rv_mode, p0 / lb / ub / itmax / opts as brdf_hip_fit_capture_dev.
 *   Which fits     one fit for every face f, 0 <= f < nf, that at least one pixel carries, and every channel c (B, G, R).  Pixel-map
 *                  entries outside [0, nf) are background, as in the entries above.
 *   Candidates     of fit (f, c): the face's pixels in the reference's walk (x outer, y inner), within a pixel the lights
 *                  i = 0 ... L-1.
 *   Validity rule  a candidate takes part iff v_min <= image_i(H-1-y, x)[c] <= v_max AND every cosine plane the model reads is
 *                  > cos_min -- the rule of brdf_hip_fit_capture_masked_dev, word for word; 0, 255, cos_min < -1 switches it off.
 *                  A NaN cosine is never a sample, also with the rule switched off; on such a face the rule-off call refuses the
 *                  fit (count 0) where the unmasked capture stops it with reason 7.
 *   Samples        the surviving candidates, in that order: the planes are the face's cosines (brdf_hip_cosines_dev, rv_mode as
 *                  given -- all pixels of a face share them), the measurement is value / 255.0.
 *   Result         fit (f, c) has the BYTES brdf_hip_fit_batch_packed_dev (BRDF_METHOD_BC_DIF) returns for that sample set -- by
 *                  that entry's contract the bytes of brdf_hip_fit_batch_dev on the fit alone at n = k, its number of samples --
 *                  from p0 with the call's box, itmax and opts.  The statistics maps hold the bytes of
 *                  brdf_hip_fit_stats_batch_packed_dev at the fitted point: k - 3 degrees of freedom.
 *   Too few        k < 3 is levmar's n < m refusal: ret = LM_ERROR, info all zeros, p0 in d_brdf_surfaces, the statistics the packed
 *                  pass writes for such a count (rank 0); d_surface_count tells.
 *   Maps           d_brdf_surfaces[nf][3][3] (required); d_surface_info[nf][3][10], d_surface_ret[nf][3], d_surface_covar[nf][3][9],
 *                  d_surface_stats[nf][3][BRDF_STATS_SZ], d_surface_rank[nf][3], d_surface_count[nf][3] (the fit's k): DEVICE, each may
 *                  be NULL.  Faces no pixel carries are left untouched in all of them.  d_face_pixels[nf] (DEVICE, may be NULL): the
 *                  pixels that carry the face, written for EVERY face (0 where none).
 *   Host scalars   avg[k] (or NULL): the sum over the (face, channel) rows this call wrote of d_brdf_surfaces[..][k], divided by
 *                  nf * 3 -- a reduction in a fixed order: two calls give the same bytes; n_pixels: the pixels that carry a face;
 *                  n_faces: the carried faces.
 *   Big faces      a fit above 4096 samples -- a face of more than 4096 / L pixels under the rule switched off -- runs through the
 *                  single-fit path, one after the other, as in the packed call.
 *   Memory         32 bytes per candidate sample at most (3 channels x pixels x L candidates; the packed planes and measurements
 *                  hold the valid ones), 24 bytes per carried pixel and the sort's scratch for the grouping, and the packed calls' own
 *                  workspace_bytes (0: 1 GiB).
 *   Refused before any HIP call: a NULL required pointer, L outside [1, 64], H, W or nf <= 0, 3 nf > INT_MAX, an unknown model,
 *                  v_min > v_max, a NaN cos_min, workspace_bytes < 0, lb > ub.  Refused once the counts are known: a face with
 *                  pixels x L > INT_MAX.  An allocation that fails returns LM_ERROR with the bytes asked for in the message.
 *   Empty capture  no carried face: returns 0 with n_pixels = n_faces = 0 and a zero avg; nothing is written but d_face_pixels.
 * Synchronises `stream` before returning.  Returns 0, or LM_ERROR with a message that names the entry in brdf_hip_last_error().
 * The count-weighted fit of per-light means -- the same minimiser from at most L samples per fit -- is brdf_hip_fit_capture_means_dev
 * below (L <= 16); the single-BRDF fit over the same grouped samples is brdf_hip_fit_capture_single_faces_dev. */
int brdf_hip_fit_capture_faces_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                   const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                   const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                   const double *opts, int v_min, int v_max, double cos_min, long long workspace_bytes,
                                   double *d_brdf_surfaces, double *d_surface_info, int *d_surface_ret, double *d_surface_covar,
                                   double *d_surface_stats, int *d_surface_rank, int *d_surface_count, int *d_face_pixels, double *avg,
                                   long long *n_pixels, long long *n_faces, void *stream);

/* brdf_hip_fit_capture_faces_dev with the sigma-clipped fit (brdf_hip_fit_batch_packed_clipped_dev: kappa, sigma_min, rounds as
 * there) in place of the packed fit and statistics.  Everything in front of the fit -- grouping, cosines, validity rule, packing --
 * and the scatter behind it are that entry's, and so are its arguments, maps, refusals (under this entry's name, plus the three new
 * arguments') and waits, plus the clipped call's.
 *   d_surface_count[nf][3]   keeps its meaning: the fit's candidate samples under the validity rule
 *   d_surface_kept[nf][3]    the returned sample set's size (DEVICE, may be NULL)
 *   d_surface_rounds[nf][3]  rounds_used (DEVICE, may be NULL)
 * Faces no pixel carries stay untouched in both new maps.  The statistics maps are taken over the returned sample sets.  With
 * rounds = 0 every map and scalar has the bytes of brdf_hip_fit_capture_faces_dev.  Memory: that entry's, plus the clipped call's
 * per valid sample and per fit. */
int brdf_hip_fit_capture_faces_clipped_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                           const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                           const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                           const double *opts, int v_min, int v_max, double cos_min, long long workspace_bytes,
                                           double *d_brdf_surfaces, double *d_surface_info, int *d_surface_ret, double *d_surface_covar,
                                           double *d_surface_stats, int *d_surface_rank, int *d_surface_count, int *d_face_pixels, double *avg,
                                           long long *n_pixels, long long *n_faces, void *stream, double kappa, double sigma_min, int rounds,
                                           int *d_surface_kept, int *d_surface_rounds);

/* brdf_hip_fit_capture_faces_dev as a WEIGHTED fit of per-light means.  All pixels of a face share the face's cosines, so the model
 * values f_l(p) are the same for every pixel of the face, and with c_l valid values v_pl under light l and their mean m_l
 *     sum_{p,l} (v_pl / 255 - f_l(p))^2  =  sum_l c_l (m_l - f_l(p))^2  +  within,   within = sum_{p,l} (v_pl / 255 - m_l)^2,
 * where `within` does not depend on p: the fit of the k = sum c_l samples and the fit of at most L means weighted by c_l have the same
 * minimiser and the same J^T J.  The weighted fit has n <= 16 whatever the face's pixel count (brdf_hip_fit_batch_weighted_dev).
 * Arguments and maps are brdf_hip_fit_capture_faces_dev's, without workspace_bytes, with one more optional map:
 *   Which fits, candidates, validity rule   those of brdf_hip_fit_capture_faces_dev, word for word (a NaN cosine is never a sample).
 *   Samples        of fit (f, c): the lights with at least one valid value, in ascending order: the face's cosines at that light,
 *                  x = S1 / (255 c), w = c, with c, S1 = sum v and S2 = sum v^2 accumulated as INTEGERS (their order cannot show: two
 *                  calls give the same bytes; no float atomics anywhere).  k = sum c;  within = sum_l (c S2 - S1^2) / (65025 c), the
 *                  numerator exactly in 64-bit integers, one division per light, added in ascending light order.
 *   Result         d_brdf_surfaces, d_surface_info, d_surface_ret: brdf_hip_fit_batch_weighted_dev (BRDF_METHOD_BC_DIF) on those rows
 *                  from p0.  info[1] is the WEIGHTED objective sum_l c_l (m_l - f_l(p))^2, without `within`.
 *   Statistics     brdf_hip_fit_stats_batch_weighted_dev with extra_ss = within and nobs = k: stats[0] = info[1] + within,
 *                  the covariance (k - 3 degrees of freedom), sigma, rho and R2 are the FULL-SAMPLE ones -- in exact
 *                  arithmetic brdf_hip_fit_capture_faces_dev's at the same p.
 *   Maps           d_surface_count[nf][3] = k, the fit's samples; d_surface_lights[nf][3] (DEVICE, may be NULL) = the lights with a
 *                  sample, the weighted fit's n; the rest as brdf_hip_fit_capture_faces_dev.  avg in a fixed order.
 *   Too few        fewer than 3 lights with a sample is levmar's n < m refusal: ret = LM_ERROR, info all zeros, p0 in d_brdf_surfaces,
 *                  rank 0 -- also where k >= 3: three samples under two lights do not determine three parameters here.  (L < 3: every
 *                  fit is refused and the statistics maps hold zeros.)
 *   One pixel      a face of one pixel under the rule switched off has weights 1, means v / 255, within = 0 and k = L: the bytes of
 *                  brdf_hip_fit_capture_faces_dev.
 *   Memory         per (carried face, channel, light) 20 bytes of integer sums and 40 bytes of the weighted rows, plus the grouping's
 *                  24 bytes per carried pixel and the sort's scratch.  No per-candidate array.
 *   Refused before any HIP call, under the entry's name: what brdf_hip_fit_capture_faces_dev refuses, and L outside [1, 16] (16 < L
 *                  <= 64 is brdf_hip_fit_capture_faces_dev's).  Refused once the counts are known: a face of more than 11 000 000
 *                  pixels (its sums of squares would leave 64-bit integers).
 * Synchronises `stream` before returning.  Returns 0, or LM_ERROR with a message that names the entry in brdf_hip_last_error(). */
int brdf_hip_fit_capture_means_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                   const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                   const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                   const double *opts, int v_min, int v_max, double cos_min, double *d_brdf_surfaces, double *d_surface_info,
                                   int *d_surface_ret, double *d_surface_covar, double *d_surface_stats, int *d_surface_rank, int *d_surface_count,
                                   int *d_surface_lights, int *d_face_pixels, double *avg, long long *n_pixels, long long *n_faces, void *stream);

/* brdf_hip_fit_capture_means_dev with sigma clipping: the fast capture and the robust one in one entry.  All pixels of a face share
 * the face's cosines, so whether a sample survives a clip round depends on (fit, light, grey level v) alone: a round's survivors
 * under one light are an interval of grey levels, "a dropped sample never returns" is an intersection of intervals, and the whole
 * clip state is two bytes per (fit, light).  A round accumulates the integer sums again under the intervals: no per-candidate array,
 * no float atomics.  This is the definition of brdf_hip_fit_batch_packed_clipped_dev, restated for means (kappa, sigma_min, rounds
 * as there; brdf_amd.clip_light_means is one round of it as NumPy code).  A fit is (carried face, channel); candidates and validity
 * rule are brdf_hip_fit_capture_means_dev's.
 *   Intervals    per (fit, light l) an interval [lo_l, hi_l] of grey levels: at the start [v_min, v_max] clamped to 0 ... 255 for a
 *                light whose cosines pass the rule, empty -- written lo = 1, hi = 0 -- for a light whose cosines fail.  The fit's
 *                current sample set: the valid candidates with lo_l <= v <= hi_l.
 *   Round 0      brdf_hip_fit_capture_means_dev's fit, with its bytes.
 *   Settled      a fit that is refused (fewer than 3 lights with a sample) or ends with ret < 0 is settled: it keeps its outputs and
 *                its samples.
 *   Clip rounds  r = 1 ... rounds, for every fit that is not settled, at its current p:
 *                  sumsq is stats[0] of brdf_hip_fit_stats_batch_weighted_dev on the current rows with extra_ss = within and
 *                  nobs = k: the full-sample sum of squares.  A sumsq that is not finite settles the fit with nothing clipped.
 *                  sigma = fmax(sqrt(sumsq / (k - 3)), sigma_min) for k > 3; for k == 3, sigma = sigma_min.
 *                  Grey level v under light l survives iff fabs(v / 255.0 - f_l(p)) <= kappa * sigma, f on the exact path (the
 *                  reference's own pow expression, as the statistics pass evaluates it).  A NaN residual fails the comparison.
 *                  The new interval of a light runs from the smallest to the largest surviving v inside the old one; it is empty
 *                  if none survives.
 *                  No sample dropped: the fit is settled.  Fewer than 3 lights keep a sample: the clip is NOT applied, the
 *                  intervals stay as they were, and the fit is settled.
 *                  Otherwise the intervals are adopted; count, sum v and sum v^2 per light, means, weights, within, k and the
 *                  lights are formed again from the survivors -- the integer arithmetic and the pack of round 0 --, the fit runs
 *                  again from its current p: its p, info and ret become the bytes of brdf_hip_fit_batch_weighted_dev on those rows
 *                  from that p, and rounds = r.  The loop ends early when every fit is settled.
 *   Statistics   the bytes of brdf_hip_fit_stats_batch_weighted_dev at the returned p over the returned rows, with their within and k.
 *   Maps         brdf_hip_fit_capture_means_dev's, and four more (DEVICE, each may be NULL):
 *                d_surface_kept[nf][3]      k of the returned set           d_surface_rounds[nf][3]   the last round that refitted
 *                d_surface_vlo[nf][3][L], d_surface_vhi[nf][3][L]  (unsigned char) the returned intervals, by the capture's own light
 *                index: with the images and the rule they rebuild the keep mask, as the packed entry's d_mask does.
 *                d_surface_count stays the UNCLIPPED sample count; d_surface_lights is the returned set's.  Faces no pixel carries
 *                are left untouched in every map.
 *   rounds = 0, or kappa = +inf: brdf_hip_fit_capture_means_dev's bytes in every map it has; kept = count, rounds 0, the initial
 *                intervals.
 *   Waits        that entry's, and one per clip round for one readback: is any fit still active?  Only the fits a round clipped
 *                are fitted again, as a dense batch.  brdf_hip_last_clip_stats reports the rounds.
 *   Memory       that entry's, plus per (carried face, channel, light) 4 bytes of intervals and, with rounds > 0, 40 bytes of the
 *                dense refit batch; per fit about 200 bytes.
 *   Refused      before any HIP call, under this entry's name: what brdf_hip_fit_capture_means_dev refuses (L outside [1, 16]
 *                included), a kappa that is not > 0 (+inf is allowed), a sigma_min that is negative or a NaN, rounds outside [0, 16].
 * Not covered: clipping in the masked per-pixel and the single-BRDF captures, L > 16, a MAD scale, dscl, a multi-GPU variant. */
int brdf_hip_fit_capture_means_clipped_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                           const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                           const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                           const double *opts, int v_min, int v_max, double cos_min, double *d_brdf_surfaces, double *d_surface_info,
                                           int *d_surface_ret, double *d_surface_covar, double *d_surface_stats, int *d_surface_rank, int *d_surface_count,
                                           int *d_surface_lights, int *d_face_pixels, double *avg, long long *n_pixels, long long *n_faces, void *stream,
                                           double kappa, double sigma_min, int rounds, int *d_surface_kept, int *d_surface_rounds,
                                           unsigned char *d_surface_vlo, unsigned char *d_surface_vhi);

/* Replaces CBRDFdata::CalcBRDFEquation_SingleBRDF (brdfdata.cpp:1138-1186) with SolveEquation_SingleBRDF (:992-1062): ONE
 * {kd, ks, n} per colour channel for the whole object, fitted with dlevmar_bc_dif to the L samples of every face the pixel
 * map shows (n = L x faces; the reference's call site passes p0 = {0,0,0}, itmax = 2000, opts = {1e-3,1e-15,1e-10,1e-50,1},
 * bounds [0,100]).  A face's measurements are those of its LAST pixel in the reference's walk (as its I.row(face) = ...
 * leaves them).  Arguments as brdf_hip_fit_capture_dev; single_brdf (HOST, [3 channels B,G,R][3]) receives the fits,
 * info (HOST [3][10], or NULL) levmar's info[] per channel, n_faces_used (HOST, or NULL) the faces that entered the fit.
 * Deviations: faces no pixel shows are left out (the reference feeds their uninitialised matrix rows to the solver) and
 * samples are paired with their own measurements (the reference's linear indexing at :1031 mis-pairs them).
 * Synchronises `stream`.  Returns 0, or LM_ERROR if any channel's fit failed / on bad arguments. */
int brdf_hip_fit_capture_single_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                    const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                                    const double *leds, const double *view_origin, int rv_mode, const double *p0,
                                    const double *lb, const double *ub, int itmax, const double *opts, double *single_brdf,
                                    double *info, long long *n_faces_used, void *stream);

/* The single-BRDF fit over EVERY valid sample: one {kd, ks, n} per colour channel for the whole object, fitted with dlevmar_bc_dif to
 * the samples of all pixels of all carried faces under the validity rule, where brdf_hip_fit_capture_single_dev takes each face's last
 * pixel and every light; with covariance and R2, and with the carried faces' residuals against the one fit: where on the object the
 * one-material assumption fails.  No fit or statistics kernel of its own.  Capture, mesh, leds, view_origin, rv_mode, p0 / lb / ub /
 * itmax / opts as brdf_hip_fit_capture_dev.
 *   Validity rule  that of brdf_hip_fit_capture_masked_dev / brdf_hip_fit_capture_faces_dev, word for word: 0, 255, cos_min < -1
 *                  switches it off; a NaN cosine is never a sample.
 *   Samples        of channel c (B, G, R): the carried faces in ascending order, within a face its pixels in the reference's walk (x
 *                  outer, y inner), within a pixel the lights 0 ... L-1, those the rule leaves -- the sample sets of
 *                  brdf_hip_fit_capture_faces_dev's fits (f, c), one behind the other.  The planes are the face's cosines, the
 *                  measurement is value / 255.0; K_c samples, laid out as a single fit reads them: planes [3][K_c], x [K_c].
 *   Fit            K_c >= 3: single_brdf[c], info[c], ret[c] are the BYTES brdf_hip_fit_dev(BRDF_METHOD_BC_DIF, model, ..., n = K_c,
 *                  p0, lb, ub, dscl = NULL, itmax, opts, ...) returns on that sample set (ret[c]: its return value), under the same
 *                  environment switches: every single-fit regime is the existing one, the resident launch and the launch chain.
 *   Statistics     covar[c], stats[c], rank[c]: the bytes of brdf_hip_fit_stats_batch_ragged_dev (BRDF_METHOD_BC_DIF) with S = 1,
 *                  stride max(K_c, 3) and counts = {K_c} at single_brdf[c]; for K_c >= 3 those of brdf_hip_fit_stats_batch_dev at
 *                  S = 1, n = K_c: K_c - 3 degrees of freedom.
 *   Too few        K_c < 3 is levmar's n < m refusal: ret[c] = LM_ERROR, info[c] all zeros, single_brdf[c] = p0, rank[c] = 0.  The
 *                  other channels are not affected.
 *   Face maps      d_face_count[nf][3] (DEVICE, may be NULL): the samples of (face f, channel c); d_face_sumsq[nf][3] (DEVICE, may be
 *                  NULL): the sum over them of (x_i - f(single_brdf[c]; sample i))^2, the model on the exact path (the reference's
 *                  own pow expression), as the statistics pass evaluates it.  A carried face whose samples the rule removed gets 0.0
 *                  and 0; faces no pixel carries are left untouched in both.  d_face_pixels[nf] (DEVICE, may be NULL) is written
 *                  for EVERY face.  A face's samples are cut into chunks of 1024 counted from its own first sample; a chunk is
 *                  summed by one fixed tree, the chunks' sums are added in ascending order: no float atomics, two calls give the same
 *                  bytes, and a face's value depends on its own samples, their order and single_brdf[c] only.  In exact arithmetic
 *                  the sum over f of d_face_sumsq[f][c] is stats[c][0] and info[c][1].
 *   Host outputs   single_brdf[3][3] (required); info[3][10], ret[3], covar[3][9], stats[3][BRDF_STATS_SZ], rank[3], count[3] (= K_c):
 *                  each may be NULL.  n_pixels: the pixels that carry a face; n_faces: the carried faces.
 *   Memory         32 bytes per valid sample (planes and measurement; no second copy of the planes), 24 bytes per carried pixel and
 *                  the sort's scratch for the grouping, 8 bytes per residual chunk.
 *   Refused before any HIP call, under the entry's name: a NULL required pointer (images, map, mesh, leds, view origin, p0,
 *                  single_brdf), L outside [1, 64], H, W or nf <= 0, 3 nf > INT_MAX, an unknown model, v_min > v_max, a NaN cos_min,
 *                  lb > ub.  Refused once the counts are known: K_c > INT_MAX.
 *   Empty capture  no carried face: every channel is refused, the call returns 3 with n_pixels = n_faces = 0, zero statistics, and
 *                  nothing is written on the device but d_face_pixels.
 * Synchronises `stream` before returning.  Returns the number of channels whose ret is LM_ERROR (0 ... 3), as brdf_hip_fit_batch
 * counts failed fits; LM_ERROR itself for bad arguments or a HIP failure, with a message that names the entry in
 * brdf_hip_last_error().  Not covered: the count-weighted fit of per-(face, light) means for the single BRDF (the single-fit regimes
 * take no weights), dscl, a multi-GPU variant. */
int brdf_hip_fit_capture_single_faces_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                          const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                          const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                          const double *opts, int v_min, int v_max, double cos_min, double *single_brdf, double *info, int *ret,
                                          double *covar, double *stats, int *rank, long long *count, double *d_face_sumsq, int *d_face_count,
                                          int *d_face_pixels, long long *n_pixels, long long *n_faces, void *stream);

/* ---- K materials per object ------------------------------------------------------------------------------------------------------
 * Between one fit per face (brdf_hip_fit_capture_faces_dev) and one per object (brdf_hip_fit_capture_single_faces_dev): a handful of
 * materials and a label per face, by Lloyd's iteration with levmar as the centroid step.  Three entries: the carried faces' residuals
 * against M candidate materials, one fit per (label, channel), and the loop around the two.  No fit or statistics kernel of their own:
 * the fits are ONE packed batch.  Capture, mesh, leds, view_origin, rv_mode and the validity rule as
 * brdf_hip_fit_capture_single_faces_dev; a material is [3][3]: channel (B, G, R), then {kd, ks, n}.
 *
 * brdf_hip_capture_face_residuals_dev: d_materials[M][3][3] (DEVICE) -> d_face_sumsq[nf][M][3], d_face_count[nf][3] (DEVICE, each may
 * be NULL).
 *   Value          for carried face f, material m, channel c: the sum over the face's valid samples of channel c of
 *                  (x_i - f(materials[m][c]; sample i))^2, the model on the exact path.  The summation is the one
 *                  brdf_hip_fit_capture_single_faces_dev uses for d_face_sumsq -- chunks of 1024 counted from the face's own first
 *                  sample, lane l of a wavefront adds samples l, l + 64, ... in that order, one fixed tree over the lanes, the chunks'
 *                  sums added in ascending order -- so column m has the BYTES that entry writes when its single_brdf equals
 *                  materials[m], whatever M is and wherever m stands.  A sum that is not finite is stored as it comes.  No float
 *                  atomics; two calls give the same bytes.  A carried face whose samples the rule removed gets 0.0 and 0; faces no
 *                  pixel carries are left untouched in both maps.  d_face_pixels[nf] (DEVICE, may be NULL) is written for EVERY face.
 *   Memory         32 bytes per valid sample, 24 bytes per carried pixel and the sort's scratch for the grouping, 8 M bytes per
 *                  residual chunk (at most K_c / 1024 + carried faces chunks per channel).
 *   Refused before any HIP call, under the entry's name: a NULL required pointer (images, map, mesh, leds, view origin, materials),
 *                  M < 1, 3 M > INT_MAX, L outside [1, 64], H, W or nf <= 0, 3 nf > INT_MAX, an unknown model, v_min > v_max, a NaN
 *                  cos_min.
 *
 * brdf_hip_fit_capture_labelled_dev: d_face_label[nf] (DEVICE int) and K; d_materials[K][3][3] (DEVICE) holds the starting points and
 * receives the results, as brdf_hip_fit_batch_packed_dev's p.  A face whose label is outside [0, K) takes part in nothing.
 *   Samples        of fit (k, c): the carried faces with label k in ascending face index, within a face its pixels in the reference's
 *                  walk, within a pixel the lights 0 ... L-1, those the rule leaves for channel c.
 *   Fit            the S = 3 K fits are rows c * K + k of one packed batch: materials[k][c], info[k][c], ret[k][c] have the BYTES
 *                  brdf_hip_fit_batch_packed_dev (BRDF_METHOD_BC_DIF, lb, ub, itmax, opts, workspace_bytes) returns for that batch from
 *                  the same starting points, covar / stats / rank those of brdf_hip_fit_stats_batch_packed_dev at the fitted points.
 *                  Fewer than 3 samples is the packed call's refusal: ret LM_ERROR, zero info, the material untouched, rank 0.
 *   Outputs        d_info[K][3][10], d_ret[K][3], d_covar[K][3][9], d_stats[K][3][BRDF_STATS_SZ], d_rank[K][3], d_count[K][3] (the
 *                  fit's samples), d_label_faces[K] (the carried faces of the label): DEVICE, each may be NULL.
 *   Memory         32 bytes per valid sample of a labelled face, 24 bytes per carried face and channel, 24 bytes per carried pixel and
 *                  the sorts' scratch, the packed calls' workspace_bytes (0: 1 GiB).  The samples are placed from the candidates: no
 *                  face-major copy of them is held.
 *   Refused before any HIP call, under the entry's name: a NULL required pointer (images, map, mesh, leds, view origin, face_label,
 *                  materials), K < 1, 3 K > INT_MAX, workspace_bytes < 0, L outside [1, 64], H, W or nf <= 0, 3 nf > INT_MAX, an
 *                  unknown model, v_min > v_max, a NaN cos_min, lb > ub.
 *   Empty capture  no carried face: every fit is refused (ret LM_ERROR, zeros in the other maps), the materials stay.
 *
 * brdf_hip_fit_capture_materials_dev: d_materials[K][3][3] holds the K seeds on entry; rounds in [0, 64].  All labels start at -1; then
 *   1 assign       the residuals of every carried face against the K current materials (the first entry's kernels);
 *                  cost[f][k] = (s[f][k][0] + s[f][k][1]) + s[f][k][2], a cost that is not finite is +inf; the new label is the least
 *                  cost, the lowest k on a tie; every cost +inf: the label stays.  The faces whose label changed are counted.
 *   2 settle/stop  nothing changed: settled.  `rounds` refits done: stop.
 *   3 refit        the second entry's fit on the new labels from the current materials (a refused fit keeps its material); when this
 *                  was refit number `rounds` the loop ends WITHOUT another assignment, otherwise go to 1.
 * So the returned materials are always the labelled fit's bytes on the returned labels from the materials of the round before;
 * rounds = 0 returns the seeds and one assignment.  One last residual pass against the returned materials fills the face maps.
 *   Outputs        d_face_label[nf] (DEVICE, required): the labels, -1 on faces no pixel carries or no material could take;
 *                  d_face_sumsq[nf][3] (may be NULL): the carried face's residual against its own material, +inf where its label is
 *                  -1; d_face_count[nf][3] (may be NULL); both untouched on faces no pixel carries.  The second entry's maps of the
 *                  last refit (ret LM_ERROR and zeros where none ran).  Host, each may be NULL: rounds_used (the refits), settled
 *                  (0 / 1), changed[rounds + 1] (the changed faces per assignment, -1 behind the last).
 *   Memory         that of the first entry with M = K plus that of the second: 64 bytes per valid sample -- one face-major copy for
 *                  the residuals, one label-major copy for the fits -- 24 bytes per carried pixel, 24 K bytes per carried face for
 *                  the cost table, 8 K bytes per residual chunk, the packed calls' workspace_bytes.
 *   Waits          per round one for the changed count and the packed call's own.
 *   Refused before any HIP call, under the entry's name: what the second entry refuses, and rounds outside [0, 64].
 * All three synchronise `stream` before returning and return 0, or LM_ERROR for bad arguments or a HIP failure with a message that
 * names the entry in brdf_hip_last_error().  Not covered: rounds over per-(face, light) means (they need weights above 16 samples),
 * clipping inside the loop, a multi-GPU variant, choosing K, seeds (the Python package has a seeding rule; C callers bring their own). */
int brdf_hip_capture_face_residuals_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                        const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                        const double *view_origin, int rv_mode, int v_min, int v_max, double cos_min, const double *d_materials, int M,
                                        double *d_face_sumsq, int *d_face_count, int *d_face_pixels, long long *n_pixels, long long *n_faces,
                                        void *stream);
int brdf_hip_fit_capture_labelled_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                      const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                      const double *view_origin, int rv_mode, const double *lb, const double *ub, int itmax, const double *opts, int v_min,
                                      int v_max, double cos_min, long long workspace_bytes, const int *d_face_label, int K, double *d_materials,
                                      double *d_info, int *d_ret, double *d_covar, double *d_stats, int *d_rank, int *d_count, int *d_label_faces,
                                      int *d_face_pixels, long long *n_pixels, long long *n_faces, void *stream);
int brdf_hip_fit_capture_materials_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                       const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                       const double *view_origin, int rv_mode, const double *lb, const double *ub, int itmax, const double *opts, int v_min,
                                       int v_max, double cos_min, long long workspace_bytes, int K, int rounds, double *d_materials, int *d_face_label,
                                       double *d_face_sumsq, int *d_face_count, double *d_info, int *d_ret, double *d_covar, double *d_stats, int *d_rank,
                                       int *d_count, int *d_label_faces, int *d_face_pixels, int *rounds_used, int *settled, long long *changed,
                                       long long *n_pixels, long long *n_faces, void *stream);

/* ---- rendering a fitted capture --------------------------------------------------------------------------------------------------
 * Parameters back into images: what the reference program shades the mesh with, as grey levels in the captures' own layout, the
 * differences to a set of captures, and the surfaces of a labelled result.  All pixels of a face share the face's cosines, so a
 * prediction depends on (face, channel, light) alone: a value table d_face_values[nf][3][Lr] and integer passes over the pixels.  No fit
 * or statistics kernel; no float atomics.  Mesh, view_origin, rv_mode, d_pixel_map as brdf_hip_fit_capture_faces_dev; leds[Lr][3] (HOST)
 * are ANY lights, 1 <= Lr <= 64: the fitted ones, some of them, or new positions; d_brdf_surfaces[nf][3][3] (DEVICE, read only).
 *
 * brdf_hip_capture_render_dev -> d_face_values[nf][3][Lr] (DEVICE double, may be NULL), d_rendered[Lr][H][W][3] (DEVICE 8-bit BGR, may
 * be NULL; not both).
 *   Value          (f, c, l): the model at d_brdf_surfaces[f][c] on face f's cosine triple under light l, on the exact path: the BYTES
 *                  of brdf_hip_model_eval_dev on brdf_hip_cosines_dev's planes for these lights.  Written for EVERY face.
 *   Grey level     t = 255.0 * v + 0.5;  q = !(t >= 0) ? 0 : (t >= 256.0 ? 255 : (int)t): a NaN value gives 0.
 *   Image          map pixel (y, x) with a face in [0, nf) writes q of (face, c, l) to d_rendered[l][H-1-y][x][c], the place the captures
 *                  read; any other pixel receives `background` (0 ... 255), or with background = -1 is left untouched.
 *   Cost           Lr H W 3 bytes written once, in 16-byte stores between the ends of each image; 8 + 1 bytes per (face, channel, light)
 *                  of tables.
 *   Refused before any HIP call, under the entry's name: a NULL required pointer (map, mesh, leds, view origin, brdf_surfaces), both
 *                  outputs NULL, Lr outside [1, 64], H, W or nf <= 0, 3 nf > INT_MAX, an unknown model, rv_mode not 0 or 1, background
 *                  outside [-1, 255].
 *
 * brdf_hip_capture_render_residuals_dev: the captures d_images[Lr][H][W][3] under these lights against the rendered grey levels, without
 * an image being rendered.  The validity rule v_min, v_max, cos_min as brdf_hip_fit_capture_masked_dev's (0, 255, cos_min < -1: off; a NaN
 * cosine is never a sample).
 *   Candidates     (carried pixel, light l, channel c); COMPARED iff it passes the rule.  d = measured - q, an integer in -255 ... 255.
 *   Outputs        DEVICE, each may be NULL.  d_light_count / _sum / _sumsq[Lr][3] (long long): the compared candidates, sum d, sum d^2;
 *                  d_face_light_count[nf][3][Lr] (int), d_face_light_sum / _sumsq[nf][3][Lr] (long long): the same per face, written
 *                  for EVERY face (zeros where no pixel carries it); d_abs_max[H][W][3], d_worst_light[H][W][3] (8-bit, at MAP
 *                  coordinates): max |d| over the pixel's compared lights and the light that attains it, the lowest on a tie -- 0 and
 *                  255 where nothing is compared and on background pixels; d_face_values as above; n_pixels (HOST): the carried pixels.
 *   Determinism    integer adds (LDS integer atomics, then one global integer atomic per touched word): their order cannot show, two
 *                  calls give the same bytes.
 *   Memory         24 bytes per carried pixel and the sort's scratch for the grouping, 9 bytes per (face, channel, light).
 *   Refused before any HIP call, under the entry's name: a NULL required pointer (images, map, mesh, leds, view origin, brdf_surfaces),
 *                  Lr outside [1, 64], H, W or nf <= 0, 3 nf > INT_MAX, an unknown model, rv_mode not 0 or 1, v_min > v_max, a NaN
 *                  cos_min.
 *
 * brdf_hip_surfaces_from_materials_dev: d_brdf_surfaces[f] = d_materials[d_face_label[f]] where the label is in [0, K), elsewhere
 * fill[3] (HOST: {kd, ks, n}) in each channel.  K = 1 with all labels 0 is the single-BRDF case: with it brdf_hip_fit_capture_labelled_dev,
 * _materials_dev and _single_faces_dev results render through the two entries above.  Refused before any HIP call: a NULL pointer,
 * nf <= 0, 3 nf > INT_MAX, K < 1.
 * All three synchronise `stream` before returning and return 0, or LM_ERROR for bad arguments or a HIP failure with a message that
 * names the entry in brdf_hip_last_error().  Not covered: float or HDR output, a tone curve, shadows or visibility, per-vertex shading. */
int brdf_hip_capture_render_dev(int model, int H, int W, const int *d_pixel_map, const double *d_vertices, const int *d_faces,
                                const double *d_face_normals, int nf, const double *leds, int Lr, const double *view_origin, int rv_mode,
                                const double *d_brdf_surfaces, int background, double *d_face_values, unsigned char *d_rendered, void *stream);
int brdf_hip_capture_render_residuals_dev(int model, const unsigned char *d_images, int Lr, int H, int W, const int *d_pixel_map,
                                          const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                          const double *view_origin, int rv_mode, const double *d_brdf_surfaces, int v_min, int v_max,
                                          double cos_min, long long *d_light_count, long long *d_light_sum, long long *d_light_sumsq,
                                          int *d_face_light_count, long long *d_face_light_sum, long long *d_face_light_sumsq,
                                          unsigned char *d_abs_max, unsigned char *d_worst_light, double *d_face_values, long long *n_pixels,
                                          void *stream);
int brdf_hip_surfaces_from_materials_dev(const int *d_face_label, int nf, const double *d_materials, int K, const double *fill,
                                         double *d_brdf_surfaces, void *stream);

/* ---- diagnostics ----------------------------------------------------------------------------------- */
int brdf_hip_device_count(void);
const char *brdf_hip_last_error(void);
/* counters of the most recent brdf_hip_fit_dev on this thread: passes launched, Jacobian passes,
 * evaluation passes, device time in microseconds between first and last pass (HIP events). */
int brdf_hip_last_fit_stats(long long *passes, long long *jac_passes, long long *eval_passes,
                            double *device_us);

/* kernel launches the most recent brdf_hip_fit_dev enqueued (its passes + the few run-ahead launches that found
 * the fit finished and returned at once): the population a profiler averages a kernel's duration over. */
long long brdf_hip_last_fit_launches(void);
/* Launch timing (off by default).  On: a resident fit (single or shared-channel launch) is bracketed by a HIP event pair recorded
 * on the fit's own stream right in front of and right behind the kernel launch; after the call, the kernel's duration in
 * microseconds as that stream saw it -- what rocprofv3 --kernel-trace reports for the same launch, plus the two event packets.
 * -1 when timing is off or the last fit ran as a chain of launches.  bench.py's roofline uses it. */
void brdf_hip_set_launch_timing(int on);
double brdf_hip_last_fit_kernel_us(void);
double brdf_hip_last_channels_kernel_us(void);

/* only meaningful in diagnostic builds (-DBRDF_STAMPS): shader cycles spent per section of the pass
 * kernel (launch chain: load state, fold, step, uniforms, persist, sweep, reduce; resident regime: -, sweep +
 * reduce, level-1 gather, level-2 gather + fold, step + uniforms), summed over the fit's passes. */
int brdf_hip_last_fit_stamps(long long *out8);
/* diagnostic builds only: [workgroup][8] s_memrealtime stamps / counters of one LM evaluation of the last resident fit; returns rows */
int brdf_hip_last_fit_trace(long long *out, int max_rows);

#ifdef __cplusplus
}
#endif
#endif /* BRDF_LEVMAR_H */
