// capi.hip -- the C ABI of libbrdf_hip.so (include/brdf_levmar.h).
//
// Host-side mirror of the reference's solver interface: dlevmar_dif / dlevmar_bc_dif keep the exact
// levmar.h:112-127 signatures and semantics (return value, info[], NULL-able opts/info/work/covar,
// stderr diagnostics, LM_ERROR instead of exit()).  Everything n-sized runs in the HIP kernels of
// stream_fit.hip / batch_fit.hip; there is no CPU evaluation path in this library.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include <cfloat>
#include <climits>
#include <vector>

#include "../../include/brdf_levmar.h"
#include "batch_fit.h"
#include "capture_fit.h"
#include "capture_materials.h"
#include "fit_host.h"
#include "fit_stats.h"
#include "clip_fit.h"
#include "light_visibility.h"
#include "packed_fit.h"
#include "pixel_map.h"
#include "weighted_fit.h"

using namespace brdf;

namespace {

// levmar documents a FOUR-element opts array for the analytic-Jacobian entry points (lm_core.c:70-75, lmbc_core.c:380):
// they are widened here so that nothing below ever reads a fifth element of the caller's array
struct Opts4 {
  double o[5];
  double *ptr;
  explicit Opts4(double *opts) : ptr(opts ? o : nullptr) {
    if (opts) {
      for (int i = 0; i < 4; ++i) o[i] = opts[i];
      o[4] = LM_DIFF_DELTA;
    }
  }
};

typedef void (*model_func_t)(double *, double *, int, int, void *);
constexpr int kMaxRegistered = 16;
model_func_t g_registered[kMaxRegistered] = {nullptr};
std::mutex g_reg_mutex;

bool is_registered(model_func_t f) {
  if (f == &BRDFFunc_hip) return true;
  std::lock_guard<std::mutex> lock(g_reg_mutex);
  for (int i = 0; i < kMaxRegistered; ++i)
    if (g_registered[i] == f) return true;
  return false;
}

// Grow-only device staging of the drop-in entry points (one per host thread, given back when the thread ends): a dlevmar_* call
// with host pointers uploads its planes and measurements here.  The first version hipMalloc'ed and hipFree'd two buffers per call --
// at the application's call site (brdfdata.cpp:1119: n = 16, once per pixel and colour channel) that pair cost more than the fit.
thread_local DeviceBlock<double> g_stage;
double *stage_get(size_t count) {
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return nullptr;
  if (g_stage.holds(count, cur)) return g_stage.ptr;
  const size_t want = count + count / 2 + 1024;
  if (g_stage.ensure(want, cur) != hipSuccess) {
    set_error("hipMalloc(%zu doubles) failed", want);
    return nullptr;
  }
  return g_stage.ptr;
}

// uploads the planes `modelInfo` reads (Blinn-Phong never reads plane 3, which the reference's per-surfel caller
// allocates and fills incorrectly, brdfdata.cpp:1095, :1102) into d[0, 3n): adjacent planes travel in one copy
hipError_t upload_planes(double *d, const double *angles, int n, int model) {
  if (model == MODEL_WARD) return hipMemcpy(d, angles, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice);
  if (model == MODEL_BLINN_PHONG) return hipMemcpy(d, angles, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice);
  hipError_t e = hipMemcpy(d, angles, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 2 * (size_t)n, angles + 2 * (size_t)n, sizeof(double) * n, hipMemcpyHostToDevice);
  return e;
}

int host_fit(MethodSpec ms, const char *who, model_func_t func, double *p, double *x, int m, int n, double *lb,
             double *ub, double *dscl, int itmax, double *opts, double *info, double *covar, void *adata) {
  if (!func) {
    set_error("%s(): func is NULL", who);
    return LM_ERROR;
  }
  if (!is_registered(func))  // arbitrary host callback: evaluated on the host, all n-sized algebra on the device
    return generic_fit_run(ms.machine, func, nullptr, p, x, m, n, lb, ub, dscl, itmax, opts, info, covar, adata);
  if (m != kM) {
    set_error("%s(): the BRDF models have exactly 3 parameters (got m=%d)", who, m);
    return LM_ERROR;
  }
  if (n < m) {  // lm_core.c:502-505, lmbc_core.c:440-443
    set_bad_input_error(who, 1, n, m);
    return LM_ERROR;
  }
  if (!adata || !p) {
    set_error("%s(): adata (struct extraData) and p must not be NULL", who);
    return LM_ERROR;
  }
  const brdf_extra_data *ed = static_cast<const brdf_extra_data *>(adata);
  if (!ed->angles) {
    set_error("%s(): extraData.angles is NULL", who);
    return LM_ERROR;
  }
  if (ed->modelInfo < 0 || ed->modelInfo >= MODEL_COUNT) {
    set_error("%s(): extraData.modelInfo=%d is not a known model (the reference would leave hx unwritten)", who,
              ed->modelInfo);
    return LM_ERROR;
  }
  double *stage = stage_get(4 * (size_t)n);
  if (!stage) return LM_ERROR;
  double *d_angles = stage, *d_x = stage + 3 * (size_t)n;
  hipError_t e = upload_planes(d_angles, ed->angles, n, ed->modelInfo);
  if (e == hipSuccess)  // "NULL implies a zero vector", lm_core.c:441 / misc_core.c:770
    e = x ? hipMemcpy(d_x, x, sizeof(double) * n, hipMemcpyHostToDevice) : hipMemset(d_x, 0, sizeof(double) * n);
  if (e != hipSuccess) {
    set_error("%s(): host->device copy failed: %s", who, hipGetErrorString(e));
    return LM_ERROR;
  }
  // (the fit has finished when this returns: launches of the chain still queued behind it only read its `done` word,
  // never the staging buffer, so the next call may overwrite the buffer at once)
  return stream_fit_run(stream_fit_args(ms, ed->modelInfo, d_angles, d_x, n, p, lb, ub, dscl, itmax, opts, info, covar, nullptr));
}

}  // namespace

namespace {
/* Axb_core.c:1197-1270 for a run-time m: Crout LU with implicit row scaling + partial pivoting, zero pivot -> LmLimits<Real>::eps(),
 * forward and back substitution.  Same operations in the same order as lm_machine.h: lu_solve<M> (which the fitter uses in
 * registers and which the reference's known answers pin bit for bit). */
template <class Real>
static int lu_noLapack(Real *A, Real *B, Real *x, int m, const char *who) {
  if (!A) return 1;  // Axb_core.c:1149-1157: "release the retained buffer" -- there is none here
  if (!B || !x || m <= 0) {
    set_error("%s(): bad arguments", who);
    return 0;
  }
  std::vector<Real> a(A, A + (size_t)m * m), scale(m);
  std::vector<int> perm(m);
  for (int i = 0; i < m; ++i) x[i] = B[i];
  for (int i = 0; i < m; ++i) {
    Real big = Real(0.0);
    for (int j = 0; j < m; ++j) {
      const Real t = std::fabs(a[(size_t)i * m + j]);
      if (t > big) big = t;
    }
    if (big == Real(0.0)) return 0;  // silently, as the reference does (its message is commented out, Axb_core.c:1202-1208)
    scale[i] = Real(1.0) / big;
  }
  for (int j = 0; j < m; ++j) {
    int pivot = j;
    Real big = Real(0.0);
    for (int i = 0; i < j; ++i) {
      Real s = a[(size_t)i * m + j];
      for (int k = 0; k < i; ++k) s -= a[(size_t)i * m + k] * a[(size_t)k * m + j];
      a[(size_t)i * m + j] = s;
    }
    for (int i = j; i < m; ++i) {
      Real s = a[(size_t)i * m + j];
      for (int k = 0; k < j; ++k) s -= a[(size_t)i * m + k] * a[(size_t)k * m + j];
      a[(size_t)i * m + j] = s;
      const Real t = scale[i] * std::fabs(s);
      if (t >= big) {
        big = t;
        pivot = i;
      }
    }
    if (j != pivot) {
      for (int k = 0; k < m; ++k) std::swap(a[(size_t)pivot * m + k], a[(size_t)j * m + k]);
      scale[pivot] = scale[j];
    }
    perm[j] = pivot;
    if (a[(size_t)j * m + j] == Real(0.0)) a[(size_t)j * m + j] = LmLimits<Real>::eps();
    if (j != m - 1) {
      const Real t = Real(1.0) / a[(size_t)j * m + j];
      for (int i = j + 1; i < m; ++i) a[(size_t)i * m + j] *= t;
    }
  }
  int first = 0;
  for (int i = 0; i < m; ++i) {
    const int ip = perm[i];
    Real s = x[ip];
    x[ip] = x[i];
    if (first != 0) {
      for (int jj = first - 1; jj < i; ++jj) s -= a[(size_t)i * m + jj] * x[jj];
    } else if (s != Real(0.0)) {
      first = i + 1;
    }
    x[i] = s;
  }
  for (int i = m - 1; i >= 0; --i) {
    Real s = x[i];
    for (int j = i + 1; j < m; ++j) s -= a[(size_t)i * m + j] * x[j];
    x[i] = s / a[(size_t)i * m + i];
  }
  return 1;
}

}  // namespace

extern "C" {

int dlevmar_dif(void (*func)(double *, double *, int, int, void *), double *p, double *x, int m, int n, int itmax,
                double *opts, double *info, double * /*work*/, double *covar, void *adata) {
  return host_fit({kDifMachine, false}, "dlevmar_dif", func, p, x, m, n, nullptr, nullptr, nullptr, itmax, opts, info,
                  covar, adata);
}

int dlevmar_bc_dif(void (*func)(double *, double *, int, int, void *), double *p, double *x, int m, int n,
                   double *lb, double *ub, double *dscl, int itmax, double *opts, double *info, double * /*work*/,
                   double *covar, void *adata) {
  return host_fit({kBcMachine, false}, "dlevmar_bc_dif", func, p, x, m, n, lb, ub, dscl, itmax, opts, info, covar,
                  adata);
}

int dlevmar_der(void (*func)(double *, double *, int, int, void *), void (*jacf)(double *, double *, int, int, void *),
                double *p, double *x, int m, int n, int itmax, double *opts, double *info, double * /*work*/, double *covar,
                void *adata) {
  if (!func) {
    set_error("dlevmar_der(): func is NULL");
    return LM_ERROR;
  }
  if (!jacf) {  // lm_core.c:126-130
    set_error("No function specified for computing the Jacobian in dlevmar_der(). If no such function is available, use "
              "dlevmar_dif() rather than dlevmar_der()");
    return LM_ERROR;
  }
  Opts4 o4(opts);
  opts = o4.ptr;
  if (is_registered(func) && jacf == &BRDFJac_hip)  // a built-in model with its own analytic Jacobian: all on the device
    return host_fit({kDerMachine, true}, "dlevmar_der", func, p, x, m, n, nullptr, nullptr, nullptr, itmax, opts, info, covar, adata);
  return generic_fit_run(kDerMachine, func, jacf, p, x, m, n, nullptr, nullptr, nullptr, itmax, opts, info, covar, adata);
}

int dlevmar_bc_der(void (*func)(double *, double *, int, int, void *), void (*jacf)(double *, double *, int, int, void *),
                   double *p, double *x, int m, int n, double *lb, double *ub, double *dscl, int itmax, double *opts,
                   double *info, double * /*work*/, double *covar, void *adata) {
  if (!func) {
    set_error("dlevmar_bc_der(): func is NULL");
    return LM_ERROR;
  }
  if (!jacf) {  // lmbc_core.c:445-449
    set_error("No function specified for computing the Jacobian in dlevmar_bc_der(). If no such function is available, "
              "use dlevmar_bc_dif() rather than dlevmar_bc_der()");
    return LM_ERROR;
  }
  Opts4 o4(opts);
  opts = o4.ptr;
  if (is_registered(func) && jacf == &BRDFJac_hip)  // a built-in model with its own analytic Jacobian: all on the device
    return host_fit({kBcMachine, true}, "dlevmar_bc_der", func, p, x, m, n, lb, ub, dscl, itmax, opts, info, covar, adata);
  return generic_fit_run(kBcMachine, func, jacf, p, x, m, n, lb, ub, dscl, itmax, opts, info, covar, adata);
}

/* scalar post-processing of the covariance the solvers return (misc_core.c:598-611); no n-sized work */
double dlevmar_stddev(double *covar, int m, int i) { return sqrt(covar[i * m + i]); }
double dlevmar_corcoef(double *covar, int m, int i, int j) { return covar[i * m + j] / sqrt(covar[i * m + i] * covar[j * m + j]); }

double dlevmar_R2(void (*func)(double *, double *, int, int, void *), double *p, double *x, int m, int n, void *adata) {
  if (!func || !p || m <= 0 || n <= 0) {
    set_error("dlevmar_R2(): bad arguments");
    return NAN;
  }
  std::vector<double> hx(n);
  (*func)(p, hx.data(), m, n, adata);  // misc_core.c:632
  double r2 = NAN;
  (void)r2_run(x, hx.data(), n, &r2);
  return r2;
}

int dAx_eq_b_LU_noLapack(double *A, double *B, double *x, int m) { return lu_noLapack<double>(A, B, x, m, "dAx_eq_b_LU_noLapack"); }
int sAx_eq_b_LU_noLapack(float *A, float *B, float *x, int m) { return lu_noLapack<float>(A, B, x, m, "sAx_eq_b_LU_noLapack"); }

/* ---- the single-precision twins, levmar/levmar.h:208-310 (instantiated in the reference from the same *_core.c files with
 * LM_REAL = float, lm.c:43-63; here: the same machines and kernels with Real = float).  The callbacks are the caller's host
 * code and run on the host; everything n-sized around them runs on the device, in float, in the reference's summation
 * order for n*m <= 65536.  (There is no registered-model shortcut: the BRDF application is double-only.) */
int slevmar_dif(void (*func)(float *, float *, int, int, void *), float *p, float *x, int m, int n, int itmax, float *opts,
                float *info, float * /*work*/, float *covar, void *adata) {
  return generic_fit_run_f(kDifMachine, func, nullptr, p, x, m, n, nullptr, nullptr, nullptr, itmax, opts, info, covar, adata);
}
int slevmar_bc_dif(void (*func)(float *, float *, int, int, void *), float *p, float *x, int m, int n, float *lb, float *ub,
                   float *dscl, int itmax, float *opts, float *info, float * /*work*/, float *covar, void *adata) {
  return generic_fit_run_f(kBcMachine, func, nullptr, p, x, m, n, lb, ub, dscl, itmax, opts, info, covar, adata);
}
int slevmar_der(void (*func)(float *, float *, int, int, void *), void (*jacf)(float *, float *, int, int, void *), float *p, float *x,
                int m, int n, int itmax, float *opts, float *info, float * /*work*/, float *covar, void *adata) {
  if (!jacf) {  // lm_core.c:126-130
    set_error("No function specified for computing the Jacobian in slevmar_der(). If no such function is available, use "
              "slevmar_dif() rather than slevmar_der()");
    return LM_ERROR;
  }
  float o5[5] = {0, 0, 0, 0, (float)LM_DIFF_DELTA};  // four documented elements (see Opts4)
  if (opts)
    for (int i = 0; i < 4; ++i) o5[i] = opts[i];
  return generic_fit_run_f(kDerMachine, func, jacf, p, x, m, n, nullptr, nullptr, nullptr, itmax, opts ? o5 : nullptr, info, covar, adata);
}
int slevmar_bc_der(void (*func)(float *, float *, int, int, void *), void (*jacf)(float *, float *, int, int, void *), float *p,
                   float *x, int m, int n, float *lb, float *ub, float *dscl, int itmax, float *opts, float *info, float * /*work*/,
                   float *covar, void *adata) {
  if (!jacf) {  // lmbc_core.c:445-449
    set_error("No function specified for computing the Jacobian in slevmar_bc_der(). If no such function is available, "
              "use slevmar_bc_dif() rather than slevmar_bc_der()");
    return LM_ERROR;
  }
  float o5[5] = {0, 0, 0, 0, (float)LM_DIFF_DELTA};
  if (opts)
    for (int i = 0; i < 4; ++i) o5[i] = opts[i];
  return generic_fit_run_f(kBcMachine, func, jacf, p, x, m, n, lb, ub, dscl, itmax, opts ? o5 : nullptr, info, covar, adata);
}
float slevmar_stddev(float *covar, int m, int i) { return (float)sqrt(covar[i * m + i]); }  /* misc_core.c:598-602 */
float slevmar_corcoef(float *covar, int m, int i, int j) { return (float)(covar[i * m + j] / sqrt(covar[i * m + i] * covar[j * m + j])); }
float slevmar_R2(void (*func)(float *, float *, int, int, void *), float *p, float *x, int m, int n, void *adata) {
  if (!func || !p || m <= 0 || n <= 0) {
    set_error("slevmar_R2(): bad arguments");
    return NAN;
  }
  std::vector<float> hx(n);
  (*func)(p, hx.data(), m, n, adata);
  float r2 = NAN;
  (void)r2_run_f(x, hx.data(), n, &r2);
  return r2;
}
void slevmar_chkjac(void (*func)(float *, float *, int, int, void *), void (*jacf)(float *, float *, int, int, void *), float *p, int m,
                    int n, void *adata, float *err) {
  if (!func || !jacf || !p || !err || m <= 0 || n <= 0) {
    set_error("slevmar_chkjac(): bad arguments");
    return;
  }
  std::vector<float> fvec(n), fjac((size_t)n * m), pp(m), fvecp(n);
  const float eps = sqrtf(FLT_EPSILON);
  (*func)(p, fvec.data(), m, n, adata);
  (*jacf)(p, fjac.data(), m, n, adata);
  for (int j = 0; j < m; ++j) {
    float temp = eps * fabsf(p[j]);
    if (temp == 0.0f) temp = eps;
    pp[j] = p[j] + temp;
  }
  (*func)(pp.data(), fvecp.data(), m, n, adata);
  (void)chkjac_err_run_f(fvec.data(), fjac.data(), fvecp.data(), p, m, n, err);
}

int brdf_hip_register_model(void (*func)(double *, double *, int, int, void *)) {
  if (!func) return -1;
  std::lock_guard<std::mutex> lock(g_reg_mutex);
  for (int i = 0; i < kMaxRegistered; ++i)
    if (g_registered[i] == func) return 0;
  for (int i = 0; i < kMaxRegistered; ++i)
    if (!g_registered[i]) {
      g_registered[i] = func;
      return 0;
    }
  set_error("brdf_hip_register_model(): table full (%d entries)", kMaxRegistered);
  return -1;
}

int brdf_hip_unregister_model(void (*func)(double *, double *, int, int, void *)) {
  std::lock_guard<std::mutex> lock(g_reg_mutex);
  for (int i = 0; i < kMaxRegistered; ++i)
    if (g_registered[i] == func) {
      g_registered[i] = nullptr;
      return 0;
    }
  return -1;
}

void BRDFFunc_hip(double *p, double *hx, int m, int n, void *adata) {
  const brdf_extra_data *ed = static_cast<const brdf_extra_data *>(adata);
  if (!p || !hx || !ed || !ed->angles || m != kM || n <= 0) {
    set_error("BRDFFunc_hip(): bad arguments");
    return;
  }
  if (ed->modelInfo < 0 || ed->modelInfo >= MODEL_COUNT) return;  // reference: hx left unwritten
  double *stage = stage_get(4 * (size_t)n);
  if (!stage) return;
  double *d_out = stage + 3 * (size_t)n;
  hipError_t e = upload_planes(stage, ed->angles, n, ed->modelInfo);
  if (e != hipSuccess) {
    set_error("BRDFFunc_hip(): host->device copy failed: %s", hipGetErrorString(e));
    return;
  }
  if (model_eval_run(ed->modelInfo, stage, n, p, d_out, nullptr) != 0) return;
  e = hipMemcpy(hx, d_out, sizeof(double) * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) set_error("BRDFFunc_hip(): device->host copy failed: %s", hipGetErrorString(e));
}

void BRDFJac_hip(double *p, double *jac, int m, int n, void *adata) {
  const brdf_extra_data *ed = static_cast<const brdf_extra_data *>(adata);
  if (!p || !jac || !ed || !ed->angles || m != kM || n <= 0) {
    set_error("BRDFJac_hip(): bad arguments");
    return;
  }
  if (ed->modelInfo < 0 || ed->modelInfo >= MODEL_COUNT) return;
  double *stage = stage_get(6 * (size_t)n);
  if (!stage) return;
  double *d_out = stage + 3 * (size_t)n;
  hipError_t e = upload_planes(stage, ed->angles, n, ed->modelInfo);
  if (e != hipSuccess) {
    set_error("BRDFJac_hip(): host->device copy failed: %s", hipGetErrorString(e));
    return;
  }
  if (model_jac_run(ed->modelInfo, stage, n, p, d_out, nullptr) != 0) return;
  e = hipMemcpy(jac, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) set_error("BRDFJac_hip(): device->host copy failed: %s", hipGetErrorString(e));
}

void dlevmar_chkjac(void (*func)(double *, double *, int, int, void *), void (*jacf)(double *, double *, int, int, void *),
                    double *p, int m, int n, void *adata, double *err) {
  if (!func || !jacf || !p || !err || m <= 0 || n <= 0) {
    set_error("dlevmar_chkjac(): bad arguments");
    return;
  }
  // misc_core.c:268-301: f(p), J(p), f(p + eps |p|) through the caller's callbacks; the n-sized comparison on the device
  std::vector<double> fvec(n), fjac((size_t)n * m), pp(m), fvecp(n);
  const double eps = sqrt(DBL_EPSILON);
  (*func)(p, fvec.data(), m, n, adata);
  (*jacf)(p, fjac.data(), m, n, adata);
  for (int j = 0; j < m; ++j) {
    double temp = eps * fabs(p[j]);
    if (temp == 0.0) temp = eps;
    pp[j] = p[j] + temp;
  }
  (*func)(pp.data(), fvecp.data(), m, n, adata);
  (void)chkjac_err_run(fvec.data(), fjac.data(), fvecp.data(), p, m, n, err);
}

int brdf_hip_fit_dev(int method, int model, const double *d_angles, const double *d_x, int n, double *p,
                     const double *lb, const double *ub, const double *dscl, int itmax, const double *opts,
                     double *info, double *covar, void *stream) {
  MethodSpec ms;
  (void)method_spec(method, &ms);  // (an unknown method: stream_fit_run's words)
  return stream_fit_run(stream_fit_args(ms, model, d_angles, d_x, n, p, lb, ub, dscl, itmax, opts, info, covar, static_cast<hipStream_t>(stream)));
}

int brdf_hip_fit_channels_dev(int method, int model, const double *d_angles, const double *d_x, long long x_stride, int n, int channels,
                              double *p, const double *lb, const double *ub, const double *dscl, int itmax, const double *opts,
                              double *info, double *covar, void *stream) {
  if (!d_angles || !d_x || !p || n <= 0 || channels < 1 || channels > 16 || (channels > 1 && x_stride < n)) {
    set_error("brdf_hip_fit_channels_dev(): bad arguments");
    return LM_ERROR;
  }
  MethodSpec ms;
  if (!method_spec(method, &ms) || model < 0 || model >= MODEL_COUNT) {
    set_error("brdf_hip_fit_channels_dev(): unknown method %d or model %d", method, model);
    return LM_ERROR;
  }
  return channels_fit_run(method, model, d_angles, d_x, x_stride, n, channels, p, lb, ub, dscl, itmax, opts, info, covar,
                          static_cast<hipStream_t>(stream));
}

/* diagnostic builds (-DBRDF_STAMPS) only: cycles per section of channel `channel`'s control wave, summed over its passes */
int brdf_hip_last_channels_stamps(int channel, long long *out8) {
  const FitStats st = channels_last_stats(channel);
  for (int i = 0; i < 8; ++i) out8[i] = st.stamps[i];
  return 0;
}

int brdf_hip_last_channels_stats(int channel, int *shared_launch, long long *passes, long long *jac_passes, double *device_us) {
  const FitStats st = channels_last_stats(channel);
  if (shared_launch) *shared_launch = channels_last_shared();
  if (passes) *passes = st.passes;
  if (jac_passes) *jac_passes = st.jac_passes;
  if (device_us) *device_us = st.device_us;
  return 0;
}

int brdf_hip_fit_batch_dev(int method, int model, const double *d_angles, const double *d_x, int S, int n,
                           double *d_p, const double *lb, const double *ub, int itmax, const double *opts,
                           double *d_info, int *d_ret, void *stream) {
  const BatchFitArgs a = {method, model, d_angles, d_x, S, n, d_p, lb, ub, itmax, opts, d_info, d_ret, static_cast<hipStream_t>(stream)};
  return batch_fit_enqueue(a, "brdf_hip_fit_batch_dev");
}

int brdf_hip_fit_batch_ragged_dev(int method, int model, const double *d_angles, const double *d_x, const int *d_counts, int S, int n,
                                  double *d_p, const double *lb, const double *ub, int itmax, const double *opts, double *d_info,
                                  int *d_ret, void *stream) {
  const BatchFitArgs a = {method, model, d_angles, d_x, S, n, d_p, lb, ub, itmax, opts, d_info, d_ret, static_cast<hipStream_t>(stream),
                          d_counts};  // (null: the uniform call)
  return batch_fit_enqueue(a, "brdf_hip_fit_batch_ragged_dev");
}

namespace {
// The host-pointer twins: the entry's own argument check on the host pointers (no HIP call before it), a HostCall (fit_host.h) for the
// device copies, the _dev twin's enqueue, one wait.  The fits return the number of fits with ret < 0.
int count_failed(const int *ret, int S) {
  int bad = 0;
  for (int s = 0; s < S; ++s) bad += ret[s] < 0;
  return bad;
}

// brdf_hip_fit_batch and its ragged twin (counts: host, or null)
int fit_batch_host(const char *who, int method, int model, const double *angles, const double *x, const int *counts, int S, int n, double *p,
                   const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret) {
  BatchFitArgs a = {method, model, angles, x, S, n, p, lb, ub, itmax, opts, info, ret, nullptr, counts};
  if (batch_fit_check(a, who) != 0) return LM_ERROR;
  std::vector<int> own_ret(ret ? 0 : S);
  if (!ret) ret = own_ret.data();
  const size_t sn = (size_t)S * n;
  HostCall h(who);
  a.d_angles = h.in(angles, 3 * sn);
  a.d_x = h.in(x, sn);
  a.d_counts = h.in(counts, S);
  a.d_p = h.inout(p, 3 * (size_t)S);
  a.d_info = h.out(info, 10 * (size_t)S);
  a.d_ret = h.out(ret, S);
  if (h.failed() || batch_fit_enqueue(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return count_failed(ret, S);
}

int fit_stats_host(const char *who, int method, int model, const double *angles, const double *x, const int *counts, int S, int n,
                   const double *p, const double *opts, double *covar, double *stats, int *rank) {
  FitStatsArgs a = {method, model, angles, x, S, n, p, opts, covar, stats, rank, nullptr, 0, nullptr, counts};
  if (fit_stats_check(a, who) != 0) return LM_ERROR;
  const size_t sn = (size_t)S * n;
  HostCall h(who);
  a.d_angles = h.in(angles, 3 * sn);
  a.d_x = h.in(x, sn);
  a.d_counts = h.in(counts, S);
  a.d_p = h.in(p, 3 * (size_t)S);
  a.d_covar = h.out(covar, 9 * (size_t)S);
  a.d_stats = h.out(stats, BRDF_STATS_SZ * (size_t)S);
  a.d_rank = h.out(rank, S);
  if (h.failed() || fit_stats_enqueue(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return 0;
}
}  // namespace

int brdf_hip_fit_batch(int method, int model, const double *angles, const double *x, int S, int n, double *p,
                       const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret) {
  return fit_batch_host("brdf_hip_fit_batch", method, model, angles, x, nullptr, S, n, p, lb, ub, itmax, opts, info, ret);
}

int brdf_hip_fit_batch_ragged(int method, int model, const double *angles, const double *x, const int *counts, int S, int n, double *p,
                              const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret) {
  return fit_batch_host("brdf_hip_fit_batch_ragged", method, model, angles, x, counts, S, n, p, lb, ub, itmax, opts, info, ret);
}

int brdf_hip_fit_stats_batch_dev(int method, int model, const double *d_angles, const double *d_x, int S, int n,
                                 const double *d_p, const double *opts, double *d_covar, double *d_stats, int *d_rank,
                                 void *stream) {
  const FitStatsArgs a = {method, model, d_angles, d_x, S, n, d_p, opts, d_covar, d_stats, d_rank, nullptr, 0, static_cast<hipStream_t>(stream)};
  return fit_stats_enqueue(a, "brdf_hip_fit_stats_batch_dev");
}

int brdf_hip_fit_stats_batch_ragged_dev(int method, int model, const double *d_angles, const double *d_x, const int *d_counts, int S,
                                        int n, const double *d_p, const double *opts, double *d_covar, double *d_stats, int *d_rank,
                                        void *stream) {
  const FitStatsArgs a = {method, model, d_angles, d_x, S, n, d_p, opts, d_covar, d_stats, d_rank, nullptr, 0, static_cast<hipStream_t>(stream),
                          d_counts};  // (null: the uniform call)
  return fit_stats_enqueue(a, "brdf_hip_fit_stats_batch_ragged_dev");
}

int brdf_hip_fit_stats_batch(int method, int model, const double *angles, const double *x, int S, int n, const double *p,
                             const double *opts, double *covar, double *stats, int *rank) {
  return fit_stats_host("brdf_hip_fit_stats_batch", method, model, angles, x, nullptr, S, n, p, opts, covar, stats, rank);
}

int brdf_hip_fit_stats_batch_ragged(int method, int model, const double *angles, const double *x, const int *counts, int S, int n,
                                    const double *p, const double *opts, double *covar, double *stats, int *rank) {
  return fit_stats_host("brdf_hip_fit_stats_batch_ragged", method, model, angles, x, counts, S, n, p, opts, covar, stats, rank);
}

/* ---- per-sample weights, n <= 16 (weighted_fit.hip; the statistics: fit_stats.hip) --------------------------------------------- */
int brdf_hip_fit_batch_weighted_dev(int method, int model, const double *d_angles, const double *d_x, const double *d_w, const int *d_counts,
                                    int S, int n, double *d_p, const double *lb, const double *ub, int itmax, const double *opts,
                                    double *d_info, int *d_ret, void *stream) {
  const WeightedFitArgs a = {{method, model, d_angles, d_x, S, n, d_p, lb, ub, itmax, opts, d_info, d_ret, static_cast<hipStream_t>(stream), d_counts},
                             d_w};
  return weighted_fit_enqueue(a, "brdf_hip_fit_batch_weighted_dev");
}

int brdf_hip_fit_batch_weighted(int method, int model, const double *angles, const double *x, const double *w, const int *counts, int S, int n,
                                double *p, const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret) {
  const char *who = "brdf_hip_fit_batch_weighted";
  WeightedFitArgs a = {{method, model, angles, x, S, n, p, lb, ub, itmax, opts, info, ret, nullptr, counts}, w};
  if (weighted_fit_check(a, who) != 0) return LM_ERROR;
  std::vector<int> own_ret(ret ? 0 : S);
  if (!ret) ret = own_ret.data();
  const size_t sn = (size_t)S * n;
  HostCall h(who);
  a.fit.d_angles = h.in(angles, 3 * sn);
  a.fit.d_x = h.in(x, sn);
  a.d_w = h.in(w, sn);
  a.fit.d_counts = h.in(counts, S);
  a.fit.d_p = h.inout(p, 3 * (size_t)S);
  a.fit.d_info = h.out(info, 10 * (size_t)S);
  a.fit.d_ret = h.out(ret, S);
  if (h.failed() || weighted_fit_enqueue(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return count_failed(ret, S);
}

int brdf_hip_fit_stats_batch_weighted_dev(int method, int model, const double *d_angles, const double *d_x, const double *d_w,
                                          const int *d_counts, int S, int n, const double *d_p, const double *opts, const double *d_extra_ss,
                                          const int *d_nobs, double *d_covar, double *d_stats, int *d_rank, void *stream) {
  const WeightedStatsArgs a = {{method, model, d_angles, d_x, S, n, d_p, opts, d_covar, d_stats, d_rank, nullptr, 0, static_cast<hipStream_t>(stream),
                                d_counts},
                               d_w, d_extra_ss, d_nobs};
  return weighted_stats_enqueue(a, "brdf_hip_fit_stats_batch_weighted_dev");
}

int brdf_hip_fit_stats_batch_weighted(int method, int model, const double *angles, const double *x, const double *w, const int *counts, int S,
                                      int n, const double *p, const double *opts, const double *extra_ss, const int *nobs, double *covar,
                                      double *stats, int *rank) {
  const char *who = "brdf_hip_fit_stats_batch_weighted";
  WeightedStatsArgs a = {{method, model, angles, x, S, n, p, opts, covar, stats, rank, nullptr, 0, nullptr, counts}, w, extra_ss, nobs};
  if (weighted_stats_check(a, who) != 0) return LM_ERROR;
  const size_t sn = (size_t)S * n;
  HostCall h(who);
  a.stats.d_angles = h.in(angles, 3 * sn);
  a.stats.d_x = h.in(x, sn);
  a.d_w = h.in(w, sn);
  a.stats.d_counts = h.in(counts, S);
  a.stats.d_p = h.in(p, 3 * (size_t)S);
  a.d_extra_ss = h.in(extra_ss, S);
  a.d_nobs = h.in(nobs, S);
  a.stats.d_covar = h.out(covar, 9 * (size_t)S);
  a.stats.d_stats = h.out(stats, BRDF_STATS_SZ * (size_t)S);
  a.stats.d_rank = h.out(rank, S);
  if (h.failed() || weighted_stats_enqueue(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return 0;
}

/* ---- packed batches (packed_fit.hip) ---------------------------------------------------------------------------------------- */
int brdf_hip_fit_batch_packed_dev(int method, int model, const double *d_angles, const double *d_x, const long long *d_offsets, int S,
                                  double *d_p, const double *lb, const double *ub, int itmax, const double *opts, double *d_info, int *d_ret,
                                  long long workspace_bytes, void *stream) {
  const PackedFitArgs a = {method, model, d_angles, d_x, d_offsets, S, d_p, lb, ub, itmax, opts, d_info, d_ret, workspace_bytes,
                           static_cast<hipStream_t>(stream)};
  return packed_fit_run(a, "brdf_hip_fit_batch_packed_dev");
}

int brdf_hip_fit_stats_batch_packed_dev(int method, int model, const double *d_angles, const double *d_x, const long long *d_offsets, int S,
                                        const double *d_p, const double *opts, double *d_covar, double *d_stats, int *d_rank,
                                        long long workspace_bytes, void *stream) {
  const PackedStatsArgs a = {method, model, d_angles, d_x, d_offsets, S, d_p, opts, d_covar, d_stats, d_rank, workspace_bytes,
                             static_cast<hipStream_t>(stream)};
  return packed_stats_run(a, "brdf_hip_fit_stats_batch_packed_dev");
}

namespace {
// what the host can see of host offsets (after the entry's own argument check): they must not decrease, and no fit has more than INT_MAX samples
int check_host_offsets(const char *who, const long long *offsets, int S) {
  for (int s = 0; s < S; ++s) {
    if (offsets[s + 1] < offsets[s]) {
      set_error("%s(): offsets decrease at fit %d (%lld after %lld)", who, s, offsets[s + 1], offsets[s]);
      return LM_ERROR;
    }
    if (offsets[s + 1] - offsets[s] > INT_MAX) {
      set_error("%s(): fit %d has %lld samples, more than INT_MAX", who, s, offsets[s + 1] - offsets[s]);
      return LM_ERROR;
    }
  }
  return 0;
}

// the samples [offsets[0], offsets[S]) and the offsets, rebased to 0, on the device
void upload_packed(HostCall &h, const double *angles, const double *x, const long long *offsets, int S, const double **d_angles, const double **d_x,
                   const long long **d_offsets) {
  const size_t total = (size_t)(offsets[S] - offsets[0]);
  std::vector<long long> rebased((size_t)S + 1);
  for (int s = 0; s <= S; ++s) rebased[s] = offsets[s] - offsets[0];
  *d_offsets = h.in(rebased.data(), rebased.size());
  *d_angles = h.in(angles + 3 * offsets[0], 3 * total);
  *d_x = h.in(x + offsets[0], total);
}
}  // namespace

int brdf_hip_fit_batch_packed(int method, int model, const double *angles, const double *x, const long long *offsets, int S, double *p,
                              const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret,
                              long long workspace_bytes) {
  const char *who = "brdf_hip_fit_batch_packed";
  PackedFitArgs a = {method, model, angles, x, offsets, S, p, lb, ub, itmax, opts, info, ret, workspace_bytes, nullptr};  // (host pointers: checked for null only)
  if (packed_fit_check(a, who) != 0 || check_host_offsets(who, offsets, S) != 0) return LM_ERROR;
  std::vector<int> own_ret(ret ? 0 : S);
  if (!ret) ret = own_ret.data();
  HostCall h(who);
  upload_packed(h, angles, x, offsets, S, &a.d_angles, &a.d_x, &a.d_offsets);
  a.d_p = h.inout(p, 3 * (size_t)S);
  a.d_info = h.out(info, 10 * (size_t)S);
  a.d_ret = h.out(ret, S);
  if (h.failed() || packed_fit_run(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return count_failed(ret, S);
}

int brdf_hip_fit_stats_batch_packed(int method, int model, const double *angles, const double *x, const long long *offsets, int S,
                                    const double *p, const double *opts, double *covar, double *stats, int *rank, long long workspace_bytes) {
  const char *who = "brdf_hip_fit_stats_batch_packed";
  PackedStatsArgs a = {method, model, angles, x, offsets, S, p, opts, covar, stats, rank, workspace_bytes, nullptr};  // (host pointers: checked for null only)
  if (packed_stats_check(a, who) != 0 || check_host_offsets(who, offsets, S) != 0) return LM_ERROR;
  HostCall h(who);
  upload_packed(h, angles, x, offsets, S, &a.d_angles, &a.d_x, &a.d_offsets);
  a.d_p = h.in(p, 3 * (size_t)S);
  a.d_covar = h.out(covar, 9 * (size_t)S);
  a.d_stats = h.out(stats, BRDF_STATS_SZ * (size_t)S);
  a.d_rank = h.out(rank, S);
  if (h.failed() || packed_stats_run(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return 0;
}

/* ---- sigma-clipped packed batches (clip_fit.hip) ------------------------------------------------------------------------------- */
int brdf_hip_fit_batch_packed_clipped_dev(int method, int model, const double *d_angles, const double *d_x, const long long *d_offsets, int S,
                                          double *d_p, const double *lb, const double *ub, int itmax, const double *opts, double kappa,
                                          double sigma_min, int rounds, double *d_info, int *d_ret, double *d_covar, double *d_stats, int *d_rank,
                                          int *d_kept, int *d_rounds_used, unsigned char *d_mask, long long workspace_bytes, void *stream) {
  const ClipFitArgs a = {{method, model, d_angles, d_x, d_offsets, S, d_p, lb, ub, itmax, opts, d_info, d_ret, workspace_bytes, static_cast<hipStream_t>(stream)},
                         {kappa, sigma_min, rounds}, d_covar, d_stats, d_rank, d_kept, d_rounds_used, d_mask};
  return clip_fit_run(a, "brdf_hip_fit_batch_packed_clipped_dev");
}

int brdf_hip_fit_batch_packed_clipped(int method, int model, const double *angles, const double *x, const long long *offsets, int S, double *p,
                                      const double *lb, const double *ub, int itmax, const double *opts, double kappa, double sigma_min, int rounds,
                                      double *info, int *ret, double *covar, double *stats, int *rank, int *kept, int *rounds_used,
                                      unsigned char *mask, long long workspace_bytes) {
  const char *who = "brdf_hip_fit_batch_packed_clipped";
  ClipFitArgs a = {{method, model, angles, x, offsets, S, p, lb, ub, itmax, opts, info, ret, workspace_bytes, nullptr},  // (host pointers: checked for null only)
                   {kappa, sigma_min, rounds}, covar, stats, rank, kept, rounds_used, mask};
  if (clip_fit_check(a, who) != 0 || check_host_offsets(who, offsets, S) != 0) return LM_ERROR;
  std::vector<int> own_ret(ret ? 0 : S);
  if (!ret) ret = own_ret.data();
  HostCall h(who);
  upload_packed(h, angles, x, offsets, S, &a.fit.d_angles, &a.fit.d_x, &a.fit.d_offsets);
  a.fit.d_p = h.inout(p, 3 * (size_t)S);
  a.fit.d_info = h.out(info, 10 * (size_t)S);
  a.fit.d_ret = h.out(ret, S);
  a.d_covar = h.out(covar, 9 * (size_t)S);
  a.d_stats = h.out(stats, BRDF_STATS_SZ * (size_t)S);
  a.d_rank = h.out(rank, S);
  a.d_kept = h.out(kept, S);
  a.d_rounds_used = h.out(rounds_used, S);
  a.d_mask = h.out(mask, (size_t)(offsets[S] - offsets[0]));
  if (h.failed() || clip_fit_run(a, who) != 0 || h.finish() != 0) return LM_ERROR;
  return count_failed(ret, S);
}

int brdf_hip_last_clip_stats(int round, long long *active_fits, long long *clipped_samples) {
  const ClipLastStats st = clip_last_stats();
  if (round < 1 || round > st.rounds) return LM_ERROR;
  if (active_fits) *active_fits = st.active[round - 1];
  if (clipped_samples) *clipped_samples = st.clipped[round - 1];
  return 0;
}

int brdf_hip_last_packed_stats(int cls, long long *fits, int *stride, int *chunks) {
  if (cls < 0 || cls >= kPackedClasses) return LM_ERROR;
  const PackedLastStats st = packed_last_stats();
  if (fits) *fits = st.fits[cls];
  if (stride) *stride = st.stride[cls];
  if (chunks) *chunks = st.chunks[cls];
  return 0;
}

int brdf_hip_last_batch_launch(int *kernel, int *waves_per_simd, long long *grid, int *quorum, int *maxwait) {
  const BatchLaunchRecord r = last_batch_launch();
  if (kernel) *kernel = r.kernel;
  if (waves_per_simd) *waves_per_simd = r.waves_per_simd;
  if (grid) *grid = r.grid;
  if (quorum) *quorum = r.quorum;
  if (maxwait) *maxwait = r.maxwait;
  return r.kernel < 0 ? LM_ERROR : 0;
}

int brdf_hip_model_eval_dev(int model, const double *d_angles, int n, const double *p, double *d_hx, void *stream) {
  return model_eval_run(model, d_angles, n, p, d_hx, static_cast<hipStream_t>(stream));
}

int brdf_hip_synth_dev(int model, unsigned long long seed, long long first, int count, int n,
                       const double *d_truth, double *d_angles, double *d_x, void *stream) {
  return synth_enqueue(model, seed, first, count, n, d_truth, d_angles, d_x, static_cast<hipStream_t>(stream));
}

int brdf_hip_cosines_dev(const double *d_vertices, const int *d_faces, const double *d_face_normals, const int *d_surfels,
                         long long S, const double *leds, int L, const double *view_origin, int rv_mode, double *d_angles,
                         void *stream) {
  return cosines_run(d_vertices, d_faces, d_face_normals, d_surfels, S, leds, L, view_origin, rv_mode, d_angles,
                     static_cast<hipStream_t>(stream));
}

void brdf_hip_led_table(double *leds16x3) { led_table(leds16x3); }

int brdf_hip_face_normals_dev(const double *d_vertices, long long nv, const int *d_faces, long long nf, double *d_normals, void *stream) {
  return face_normals_run(d_vertices, nv, d_faces, nf, d_normals, static_cast<hipStream_t>(stream));
}

int brdf_hip_pixel_map_dev(const double *d_vertices, long long nv, const int *d_faces, long long nf, const double *model_view,
                           const double *projection, const double *viewport, int H, int W, int mode, int cull, int *d_pixel_map,
                           double *d_depth, int *d_face_pixels, long long *stats, void *stream) {
  const PixelMapArgs a = {d_vertices, nv, d_faces, nf, model_view, projection, viewport, H, W, mode, cull, d_pixel_map, d_depth, d_face_pixels,
                          stats, static_cast<hipStream_t>(stream)};
  return pixel_map_run(a);
}

int brdf_hip_light_visibility_dev(const double *d_vertices, long long nv, const int *d_faces, long long nf, const double *d_normals,
                                  const double *leds, int L, double t_min, unsigned long long *d_face_lit, long long *stats, void *stream) {
  const LightVisibilityArgs a = {d_vertices, nv, d_faces, nf, d_normals, leds, L, t_min, d_face_lit, stats, static_cast<hipStream_t>(stream)};
  return light_visibility_run(a);
}

int brdf_hip_capture_apply_visibility_dev(const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                          const unsigned long long *d_face_lit, int nf, int level, unsigned char *d_out,
                                          unsigned long long *d_shadowed, void *stream) {
  const ApplyVisibilityArgs a = {d_images, L, H, W, d_pixel_map, d_face_lit, nf, level, d_out, d_shadowed, static_cast<hipStream_t>(stream)};
  return apply_visibility_run(a);
}

// the capture entries (capture_fit.h): what all seven take, in the order of CaptureArgs
#define CAPTURE_ARGS \
  {model, d_images, L, H, W, d_pixel_map, d_vertices, d_faces, d_face_normals, nf, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts, \
   static_cast<hipStream_t>(stream)}

int brdf_hip_fit_capture_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                             const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                             const double *leds, const double *view_origin, int rv_mode, const double *p0, const double *lb,
                             const double *ub, int itmax, const double *opts, double *d_brdf_surfaces, double *avg,
                             long long *n_pixels, void *stream) {
  const CaptureFitArgs a = {CAPTURE_ARGS, d_brdf_surfaces, avg, n_pixels, nullptr, nullptr, nullptr, nullptr};
  return capture_fit_run(a);
}

int brdf_hip_fit_capture_stats_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                   const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                                   const double *leds, const double *view_origin, int rv_mode, const double *p0,
                                   const double *lb, const double *ub, int itmax, const double *opts, double *d_brdf_surfaces,
                                   double *avg, long long *n_pixels, void *stream, double *d_surface_covar,
                                   double *d_surface_stats, int *d_surface_rank) {
  const CaptureFitArgs a = {CAPTURE_ARGS, d_brdf_surfaces, avg, n_pixels, d_surface_covar, d_surface_stats, d_surface_rank, nullptr};
  return capture_fit_run(a);
}

int brdf_hip_fit_capture_masked_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                    const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                                    const double *leds, const double *view_origin, int rv_mode, const double *p0,
                                    const double *lb, const double *ub, int itmax, const double *opts, double *d_brdf_surfaces,
                                    double *avg, long long *n_pixels, void *stream, double *d_surface_covar,
                                    double *d_surface_stats, int *d_surface_rank, int v_min, int v_max, double cos_min,
                                    int *d_surface_count) {
  const CaptureMask mask = {v_min, v_max, cos_min, d_surface_count};
  const CaptureFitArgs a = {CAPTURE_ARGS, d_brdf_surfaces, avg, n_pixels, d_surface_covar, d_surface_stats, d_surface_rank, &mask};
  return capture_fit_run(a);
}

int brdf_hip_fit_capture_faces_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                   const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                   const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                   const double *opts, int v_min, int v_max, double cos_min, long long workspace_bytes,
                                   double *d_brdf_surfaces, double *d_surface_info, int *d_surface_ret, double *d_surface_covar,
                                   double *d_surface_stats, int *d_surface_rank, int *d_surface_count, int *d_face_pixels, double *avg,
                                   long long *n_pixels, long long *n_faces, void *stream) {
  const CaptureFacesArgs a = {{CAPTURE_ARGS, v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, workspace_bytes, d_brdf_surfaces, d_surface_info,
                              d_surface_ret, d_surface_covar, d_surface_stats, d_surface_rank, d_surface_count, avg};
  return capture_faces_run(a);
}

int brdf_hip_fit_capture_faces_clipped_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                           const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                           const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                           const double *opts, int v_min, int v_max, double cos_min, long long workspace_bytes,
                                           double *d_brdf_surfaces, double *d_surface_info, int *d_surface_ret, double *d_surface_covar,
                                           double *d_surface_stats, int *d_surface_rank, int *d_surface_count, int *d_face_pixels, double *avg,
                                           long long *n_pixels, long long *n_faces, void *stream, double kappa, double sigma_min, int rounds,
                                           int *d_surface_kept, int *d_surface_rounds) {
  const CaptureClip clip = {kappa, sigma_min, rounds, d_surface_kept, d_surface_rounds};
  const CaptureFacesArgs a = {{CAPTURE_ARGS, v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, workspace_bytes, d_brdf_surfaces, d_surface_info,
                              d_surface_ret, d_surface_covar, d_surface_stats, d_surface_rank, d_surface_count, avg, &clip};
  return capture_faces_run(a);
}

int brdf_hip_fit_capture_means_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                   const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                   const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                   const double *opts, int v_min, int v_max, double cos_min, double *d_brdf_surfaces, double *d_surface_info,
                                   int *d_surface_ret, double *d_surface_covar, double *d_surface_stats, int *d_surface_rank, int *d_surface_count,
                                   int *d_surface_lights, int *d_face_pixels, double *avg, long long *n_pixels, long long *n_faces, void *stream) {
  const CaptureMeansArgs a = {{{CAPTURE_ARGS, v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, 0, d_brdf_surfaces, d_surface_info, d_surface_ret,
                               d_surface_covar, d_surface_stats, d_surface_rank, d_surface_count, avg},
                              d_surface_lights};
  return capture_means_run(a);
}

int brdf_hip_fit_capture_means_clipped_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                           const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                           const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                           const double *opts, int v_min, int v_max, double cos_min, double *d_brdf_surfaces, double *d_surface_info,
                                           int *d_surface_ret, double *d_surface_covar, double *d_surface_stats, int *d_surface_rank, int *d_surface_count,
                                           int *d_surface_lights, int *d_face_pixels, double *avg, long long *n_pixels, long long *n_faces, void *stream,
                                           double kappa, double sigma_min, int rounds, int *d_surface_kept, int *d_surface_rounds,
                                           unsigned char *d_surface_vlo, unsigned char *d_surface_vhi) {
  const CaptureMeansClip clip = {{kappa, sigma_min, rounds, d_surface_kept, d_surface_rounds}, d_surface_vlo, d_surface_vhi};
  const CaptureMeansArgs a = {{{CAPTURE_ARGS, v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, 0, d_brdf_surfaces, d_surface_info, d_surface_ret,
                               d_surface_covar, d_surface_stats, d_surface_rank, d_surface_count, avg},
                              d_surface_lights, &clip};
  return capture_means_run(a);
}

int brdf_hip_fit_capture_single_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                    const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf,
                                    const double *leds, const double *view_origin, int rv_mode, const double *p0,
                                    const double *lb, const double *ub, int itmax, const double *opts, double *single_brdf,
                                    double *info, long long *n_faces_used, void *stream) {
  const CaptureSingleArgs a = {CAPTURE_ARGS, single_brdf, info, n_faces_used};
  return capture_fit_single_run(a);
}

int brdf_hip_fit_capture_single_faces_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                          const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                          const double *view_origin, int rv_mode, const double *p0, const double *lb, const double *ub, int itmax,
                                          const double *opts, int v_min, int v_max, double cos_min, double *single_brdf, double *info, int *ret,
                                          double *covar, double *stats, int *rank, long long *count, double *d_face_sumsq, int *d_face_count,
                                          int *d_face_pixels, long long *n_pixels, long long *n_faces, void *stream) {
  const CaptureSingleFacesArgs a = {{CAPTURE_ARGS, v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, single_brdf, info, ret, covar, stats, rank,
                                    count, d_face_sumsq, d_face_count};
  return capture_single_faces_run(a);
}

// the materials entries (capture_materials.h) read no p0: their starting points are the materials
#define CAPTURE_ARGS_NO_START(lb_, ub_, itmax_, opts_) \
  {model, d_images, L, H, W, d_pixel_map, d_vertices, d_faces, d_face_normals, nf, leds, view_origin, rv_mode, nullptr, lb_, ub_, itmax_, opts_, \
   static_cast<hipStream_t>(stream)}

int brdf_hip_capture_face_residuals_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                        const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                        const double *view_origin, int rv_mode, int v_min, int v_max, double cos_min, const double *d_materials, int M,
                                        double *d_face_sumsq, int *d_face_count, int *d_face_pixels, long long *n_pixels, long long *n_faces,
                                        void *stream) {
  const CaptureResidualsArgs a = {{CAPTURE_ARGS_NO_START(nullptr, nullptr, 0, nullptr), v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, d_materials, M,
                                  d_face_sumsq, d_face_count};
  return capture_face_residuals_run(a);
}

int brdf_hip_fit_capture_labelled_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                      const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                      const double *view_origin, int rv_mode, const double *lb, const double *ub, int itmax, const double *opts, int v_min,
                                      int v_max, double cos_min, long long workspace_bytes, const int *d_face_label, int K, double *d_materials,
                                      double *d_info, int *d_ret, double *d_covar, double *d_stats, int *d_rank, int *d_count, int *d_label_faces,
                                      int *d_face_pixels, long long *n_pixels, long long *n_faces, void *stream) {
  const CaptureLabelledArgs a = {{CAPTURE_ARGS_NO_START(lb, ub, itmax, opts), v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, workspace_bytes,
                                 const_cast<int *>(d_face_label), K, d_materials, d_info, d_ret, d_covar, d_stats, d_rank, d_count, d_label_faces};
  return capture_labelled_run(a);
}

int brdf_hip_fit_capture_materials_dev(int model, const unsigned char *d_images, int L, int H, int W, const int *d_pixel_map,
                                       const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                       const double *view_origin, int rv_mode, const double *lb, const double *ub, int itmax, const double *opts, int v_min,
                                       int v_max, double cos_min, long long workspace_bytes, int K, int rounds, double *d_materials, int *d_face_label,
                                       double *d_face_sumsq, int *d_face_count, double *d_info, int *d_ret, double *d_covar, double *d_stats, int *d_rank,
                                       int *d_count, int *d_label_faces, int *d_face_pixels, int *rounds_used, int *settled, long long *changed,
                                       long long *n_pixels, long long *n_faces, void *stream) {
  const CaptureMaterialsArgs a = {{{CAPTURE_ARGS_NO_START(lb, ub, itmax, opts), v_min, v_max, cos_min, d_face_pixels, n_pixels, n_faces}, workspace_bytes,
                                   d_face_label, K, d_materials, d_info, d_ret, d_covar, d_stats, d_rank, d_count, d_label_faces},
                                  rounds, d_face_sumsq, d_face_count, rounds_used, settled, changed};
  return capture_materials_run(a);
}

// the rendering entries (capture_fit.h: capture_render.hip) fit nothing; their lights are the call's own
int brdf_hip_capture_render_dev(int model, int H, int W, const int *d_pixel_map, const double *d_vertices, const int *d_faces,
                                const double *d_face_normals, int nf, const double *leds, int Lr, const double *view_origin, int rv_mode,
                                const double *d_brdf_surfaces, int background, double *d_face_values, unsigned char *d_rendered, void *stream) {
  const unsigned char *d_images = nullptr;
  const int L = Lr;
  const CaptureRenderArgs a = {CAPTURE_ARGS_NO_START(nullptr, nullptr, 0, nullptr), d_brdf_surfaces, background, d_face_values, d_rendered};
  return capture_render_run(a);
}

int brdf_hip_capture_render_residuals_dev(int model, const unsigned char *d_images, int Lr, int H, int W, const int *d_pixel_map,
                                          const double *d_vertices, const int *d_faces, const double *d_face_normals, int nf, const double *leds,
                                          const double *view_origin, int rv_mode, const double *d_brdf_surfaces, int v_min, int v_max,
                                          double cos_min, long long *d_light_count, long long *d_light_sum, long long *d_light_sumsq,
                                          int *d_face_light_count, long long *d_face_light_sum, long long *d_face_light_sumsq,
                                          unsigned char *d_abs_max, unsigned char *d_worst_light, double *d_face_values, long long *n_pixels,
                                          void *stream) {
  const int L = Lr;
  const CaptureRenderResidualsArgs a = {{CAPTURE_ARGS_NO_START(nullptr, nullptr, 0, nullptr), v_min, v_max, cos_min, nullptr, n_pixels, nullptr},
                                        d_brdf_surfaces, d_light_count, d_light_sum, d_light_sumsq, d_face_light_count, d_face_light_sum,
                                        d_face_light_sumsq, d_abs_max, d_worst_light, d_face_values};
  return capture_render_residuals_run(a);
}

int brdf_hip_surfaces_from_materials_dev(const int *d_face_label, int nf, const double *d_materials, int K, const double *fill,
                                         double *d_brdf_surfaces, void *stream) {
  const SurfacesFromMaterialsArgs a = {d_face_label, nf, d_materials, K, fill, d_brdf_surfaces, static_cast<hipStream_t>(stream)};
  return surfaces_from_materials_run(a);
}

#undef CAPTURE_ARGS_NO_START
#undef CAPTURE_ARGS

int brdf_hip_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

const char *brdf_hip_last_error(void) { return get_error(); }

int brdf_hip_last_fit_stats(long long *passes, long long *jac_passes, long long *eval_passes, double *device_us) {
  const FitStats s = stream_fit_last_stats();
  if (passes) *passes = s.passes;
  if (jac_passes) *jac_passes = s.jac_passes;
  if (eval_passes) *eval_passes = s.eval_passes;
  if (device_us) *device_us = s.device_us;
  return 0;
}

long long brdf_hip_last_fit_launches(void) { return stream_fit_last_stats().launches; }

void brdf_hip_set_launch_timing(int on) { set_launch_timing(on != 0); }
double brdf_hip_last_fit_kernel_us(void) { return stream_fit_last_stats().kernel_us; }
double brdf_hip_last_channels_kernel_us(void) { return channels_last_shared() ? channels_last_stats(0).kernel_us : -1.0; }

/* diagnostic builds (-DBRDF_STAMPS) only: one epoch's timeline of every workgroup of the last resident fit */
int brdf_hip_last_fit_trace(long long *out, int max_rows) { return resident_fit_last_trace(out, max_rows); }

/* diagnostic builds (-DBRDF_STAMPS) only: cycles per section of the pass kernel, summed over passes */
int brdf_hip_last_fit_stamps(long long *out8) {
  const FitStats s = stream_fit_last_stats();
  for (int k = 0; k < 8; ++k) out8[k] = s.stamps[k];
  return 0;
}

}  // extern "C"
