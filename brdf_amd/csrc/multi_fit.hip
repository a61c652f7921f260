// multi_fit.hip -- brdf_hip_fit_batch_multi: brdf_hip_fit_batch over several GPUs of one process (include/brdf_levmar.h).
//
// Host code only: the device work is brdf_hip_fit_batch_dev's, unchanged.  The S fits are cut into contiguous shards by
// brdf_amd/dist.py's shard_range rule; one host thread per DISTINCT device of the list, started by the call and joined
// before it returns, sets its device, creates its own stream and runs that device's shards one after the other in list
// order (upload, brdf_hip_fit_batch_dev, download straight into the caller's slices of p / info / ret).  The library's
// workspaces are thread_local, so every worker brings its own and gives them back when it ends: nothing outlives the
// call.  A device listed twice never runs two shards of one call at the same time (a fit with n > 4096 takes the resident
// single-launch regime, which needs the whole chip).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/brdf_levmar.h"
#include "fit_host.h"

using namespace brdf;

namespace {

constexpr int kMaxDeviceList = 64;  // entries of a device list (and visible devices with devices == NULL)

struct ShardStats {
  int device;
  long long first, count;
  double ms[3];  // upload, fit, download as the device's stream saw them (HIP events); 0 if the phase did not run
};

// the calling thread's most recent brdf_hip_fit_batch_multi, for brdf_hip_last_multi_stats
thread_local std::vector<ShardStats> g_multi_stats;
// two host threads that call brdf_hip_fit_batch_multi at once run one after the other
std::mutex g_multi_mutex;

struct Call {
  int method, model;
  const double *angles, *x;
  int n;
  double *p;
  const double *lb, *ub;
  int itmax;
  const double *opts;
  double *info;
  int *ret;
};

// one device's part of a call: its shards (indices into the stats table), and what went wrong
struct Worker {
  int device;
  std::vector<int> shards;
  int bad = 0;          // fits that ended in LM_ERROR
  int failed_shard = -1;  // first shard that did not complete (the worker stops there)
  std::string err;
};

struct Events {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
};

void run_worker(const Call &c, Worker &w, std::vector<ShardStats> &stats) {
  auto fail = [&](int shard, const std::string &msg) {
    w.failed_shard = shard;
    w.err = msg;
  };
  const int first_shard = w.shards.front();
  hipError_t e = hipSetDevice(w.device);
  if (e != hipSuccess) return fail(first_shard, std::string("hipSetDevice failed: ") + hipGetErrorString(e));
  hipStream_t stream = nullptr;
  e = hipStreamCreate(&stream);
  if (e != hipSuccess) return fail(first_shard, std::string("hipStreamCreate failed: ") + hipGetErrorString(e));
  {
    // one set of buffers per device, sized for its largest shard
    long long most = 0;
    for (int k : w.shards) most = std::max(most, stats[k].count);
    const size_t sn = (size_t)most * c.n;
    DeviceBlock<double> d_angles, d_x, d_p, d_info;  // (on w.device, the worker's current device)
    DeviceBlock<int> d_ret;
    Events ev;
    std::vector<int> tmp_ret(c.ret ? 0 : (size_t)most);
    e = d_angles.ensure(3 * sn);
    if (e == hipSuccess) e = d_x.ensure(sn);
    if (e == hipSuccess) e = d_p.ensure(3 * (size_t)most);
    if (e == hipSuccess) e = d_info.ensure(10 * (size_t)most);
    if (e == hipSuccess) e = d_ret.ensure((size_t)most);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev.e[i]);
    if (e != hipSuccess) fail(first_shard, std::string("allocation failed: ") + hipGetErrorString(e));
    for (size_t i = 0; i < w.shards.size() && w.failed_shard < 0; ++i) {
      const int k = w.shards[i];
      ShardStats &st = stats[k];
      const size_t f = (size_t)st.first, cnt = (size_t)st.count, fn = f * c.n, cn = cnt * c.n;
      e = hipEventRecord(ev.e[0], stream);
      if (e == hipSuccess) e = hipMemcpyAsync(d_angles.ptr, c.angles + 3 * fn, sizeof(double) * 3 * cn, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess) e = hipMemcpyAsync(d_x.ptr, c.x + fn, sizeof(double) * cn, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess) e = hipMemcpyAsync(d_p.ptr, c.p + 3 * f, sizeof(double) * 3 * cnt, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess) e = hipEventRecord(ev.e[1], stream);
      if (e != hipSuccess) {
        fail(k, std::string("host->device copy failed: ") + hipGetErrorString(e));
        break;
      }
      if (brdf_hip_fit_batch_dev(c.method, c.model, d_angles.ptr, d_x.ptr, (int)cnt, c.n, d_p.ptr, c.lb, c.ub, c.itmax, c.opts,
                                 d_info.ptr, d_ret.ptr, stream) != 0) {
        fail(k, get_error());
        break;
      }
      e = hipEventRecord(ev.e[2], stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);  // the fit has to have succeeded before the caller's rows change
      if (e != hipSuccess) {
        fail(k, std::string("fit failed: ") + hipGetErrorString(e));
        break;
      }
      int *h_ret = c.ret ? c.ret + f : tmp_ret.data();
      e = hipMemcpyAsync(c.p + 3 * f, d_p.ptr, sizeof(double) * 3 * cnt, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess && c.info)
        e = hipMemcpyAsync(c.info + 10 * f, d_info.ptr, sizeof(double) * 10 * cnt, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipMemcpyAsync(h_ret, d_ret.ptr, sizeof(int) * cnt, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipEventRecord(ev.e[3], stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) {
        fail(k, std::string("device->host copy failed: ") + hipGetErrorString(e));
        break;
      }
      for (size_t s = 0; s < cnt; ++s) w.bad += h_ret[s] < 0;
      for (int ph = 0; ph < 3; ++ph) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.e[ph], ev.e[ph + 1]) == hipSuccess) st.ms[ph] = ms;
      }
    }
    (void)hipStreamSynchronize(stream);  // nothing of this call stays in flight (also after a failed enqueue)
  }
  (void)hipStreamDestroy(stream);
}

}  // namespace

extern "C" {

int brdf_hip_fit_batch_multi(int method, int model, const double *angles, const double *x, int S, int n, double *p,
                             const double *lb, const double *ub, int itmax, const double *opts, double *info, int *ret,
                             const int *devices, int ndev) {
  g_multi_stats.clear();
  // argument checks: no HIP call before these
  if (!angles || !x || !p || S <= 0 || n <= 0) {
    set_error("brdf_hip_fit_batch_multi(): bad arguments (need angles, x, p, S > 0, n > 0)");
    return LM_ERROR;
  }
  MethodSpec ms;
  if (!known_model_method(model, method, &ms, "brdf_hip_fit_batch_multi")) return LM_ERROR;
  if (devices && (ndev < 1 || ndev > kMaxDeviceList)) {
    set_error("brdf_hip_fit_batch_multi(): ndev = %d, the device list needs 1 to %d entries", ndev, kMaxDeviceList);
    return LM_ERROR;
  }
  int visible = 0;
  hipError_t e = hipGetDeviceCount(&visible);
  if (e != hipSuccess || visible < 1) {
    set_error("brdf_hip_fit_batch_multi(): no HIP device (%s)", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    return LM_ERROR;
  }
  std::vector<int> list;
  if (devices) {
    for (int k = 0; k < ndev; ++k) {
      if (devices[k] < 0 || devices[k] >= visible) {
        set_error("brdf_hip_fit_batch_multi(): devices[%d] = %d is not a device of this process (%d visible)", k, devices[k], visible);
        return LM_ERROR;
      }
      list.push_back(devices[k]);
    }
  } else {
    if (visible > kMaxDeviceList) {
      set_error("brdf_hip_fit_batch_multi(): %d visible devices, at most %d per call", visible, kMaxDeviceList);
      return LM_ERROR;
    }
    for (int d = 0; d < visible; ++d) list.push_back(d);
  }

  std::lock_guard<std::mutex> lock(g_multi_mutex);
  // shards: ceil(S / ndev) fits each, trailing shards short or empty (brdf_amd/dist.py shard_range)
  const int shards = (int)list.size();
  const long long per = ((long long)S + shards - 1) / shards;
  std::vector<ShardStats> stats(shards);
  std::vector<Worker> workers;
  for (int k = 0; k < shards; ++k) {
    ShardStats &st = stats[k];
    st.device = list[k];
    st.first = std::min((long long)S, k * per);
    st.count = std::min(per, (long long)S - st.first);
    st.ms[0] = st.ms[1] = st.ms[2] = 0.0;
    if (st.count == 0) continue;
    Worker *w = nullptr;
    for (Worker &o : workers)
      if (o.device == st.device) w = &o;
    if (!w) {
      workers.push_back(Worker{});
      w = &workers.back();
      w->device = st.device;
    }
    w->shards.push_back(k);
  }
  const Call c{method, model, angles, x, n, p, lb, ub, itmax, opts, info, ret};
  std::vector<std::thread> threads;
  threads.reserve(workers.size());
  for (Worker &w : workers) {
    try {
      threads.emplace_back(run_worker, std::cref(c), std::ref(w), std::ref(stats));
    } catch (const std::exception &ex) {
      w.failed_shard = w.shards.front();
      w.err = std::string("could not start a host thread: ") + ex.what();
    }
  }
  for (std::thread &t : threads) t.join();

  g_multi_stats = stats;
  int bad = 0, failed = -1;
  const Worker *culprit = nullptr;
  for (const Worker &w : workers) {
    bad += w.bad;
    if (w.failed_shard >= 0 && (failed < 0 || w.failed_shard < failed)) {
      failed = w.failed_shard;
      culprit = &w;
    }
  }
  if (culprit) {
    const ShardStats &st = stats[failed];
    set_error("brdf_hip_fit_batch_multi(): device %d, fits [%lld, %lld): %s", st.device, st.first, st.first + st.count,
              culprit->err.c_str());
    return LM_ERROR;
  }
  return bad;
}

int brdf_hip_last_multi_stats(int shard, int *device, long long *first, long long *count, double *ms3) {
  if (shard < 0 || shard >= (int)g_multi_stats.size()) return LM_ERROR;
  const ShardStats &st = g_multi_stats[shard];
  if (device) *device = st.device;
  if (first) *first = st.first;
  if (count) *count = st.count;
  if (ms3)
    for (int i = 0; i < 3; ++i) ms3[i] = st.ms[i];
  return 0;
}

}  // extern "C"
