// extern "C" entry points of include/soundml_amd.h.  Every function validates
// its arguments (raising the reference's Invalid_argument messages as
// SMX_INVALID_ARGUMENT) before any pointer is formed or device work enqueued,
// mirroring the discipline of the reference's stub layer
// (resample_stubs.c:228-276).  There is no CPU compute path here: the host
// entry points upload, launch the HIP kernels and download.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include <algorithm>

#include "smx_internal.hpp"

namespace smx {

static thread_local std::string g_last_error;
static std::atomic<int> g_interior{SMX_INTERIOR_F32};

void set_last_error(const std::string &message) { g_last_error = message; }

std::atomic<unsigned long long> g_kernel_launches{0};

int env_flag(const char *name) {
  const char *e = std::getenv(name);
  if (!e) return -1;
  if (e[0] == '\0' || !std::strcmp(e, "0") || !std::strcmp(e, "false") || !std::strcmp(e, "off")) return 0;
  return 1;
}
long env_int(const char *name, long fallback) {
  const char *e = std::getenv(name);
  return e && e[0] ? std::atol(e) : fallback;
}

bool fast_path_disabled() { return env_flag("SMX_DISABLE_FAST") == 1; }

void launch_stft(const StftJob &job) {
  if (job.count <= 0 || job.lead <= 0) return;
  if (launch_stft_fast(job)) return;
  launch_stft_generic(job);
}

namespace {

// ---- the device list of the host-pointer batch calls (smx_set_devices; round 6) ----------------------------------------------
// The reference's caller is ONE process handing over host tensors, "a batch of clips is one call" (stft.mli:211-250); its leading
// axes are independent by contract (stft.mli:214-218, tested per slice: stft_grid.ml:180-205).  With a device list set, a
// host-pointer batch call splits `lead` into contiguous clip ranges by the rule of soundml_amd/shard.py clip_range (the first
// lead % S shards own one clip more) and runs each range on its device from a host thread of its own: its own HIP streams, its own
// staging rings (transfer.cpp: per device), its own PCIe link; tables are built lazily per device as before.  No collective: every
// shard writes its slice of the caller's result.  A device may be listed more than once (virtual shards: two uploads of one device
// in flight at a time).
std::mutex g_devices_mutex;
std::vector<int> g_devices;   // empty: the calling thread's current device (smx_set_device), as rounds 1-5

std::vector<int> device_list() {
  std::lock_guard<std::mutex> g(g_devices_mutex);
  return g_devices;
}

// clips [lo, hi) of shard `rank` of `world` (soundml_amd/shard.py: clip_range)
void clip_range(int64_t total, int64_t world, int64_t rank, int64_t &lo, int64_t &hi) {
  const int64_t base = total / world, extra = total % world;
  lo = rank * base + std::min(rank, extra);
  hi = lo + base + (rank < extra ? 1 : 0);
}

// body(clip0, nclips) for every shard, on the shard's device; the first failure is rethrown as it was thrown (InvalidArgument
// stays InvalidArgument).  Without a device list: body(0, lead) on the caller's thread and device.
template <class F>
void for_each_shard(int64_t lead, F &&body) {
  const std::vector<int> devices = device_list();
  if (devices.empty() || lead <= 0) {
    body((int64_t)0, lead);
    return;
  }
  const int64_t shards = std::min<int64_t>((int64_t)devices.size(), lead);
  int caller_device = 0;
  SMX_HIP_CHECK(hipGetDevice(&caller_device));
  std::vector<std::exception_ptr> errors((size_t)shards);
  // the shards start their transfers together (a thread's first HIP call can take milliseconds: without the rendezvous the first
  // shard's upload was over before the last one's began, and the link sat idle in between)
  std::mutex gate_mutex;
  std::condition_variable gate_cv;
  int64_t arrived = 0;
  bool abandoned = false;   // a shard's thread could not start: nobody waits for it, and no shard runs
  auto rendezvous = [&] {
    std::unique_lock<std::mutex> g(gate_mutex);
    if (++arrived == shards) gate_cv.notify_all();
    else gate_cv.wait(g, [&] { return arrived == shards || abandoned; });
    return !abandoned;
  };
  auto run = [&](int64_t s) {
    bool met = false;
    try {
      const hipError_t set = hipSetDevice(devices[(size_t)s]);
      if (set == hipSuccess) (void)hipFree(nullptr);   // (the thread's HIP state for the device exists before the rendezvous)
      met = true;
      if (rendezvous()) {
        SMX_HIP_CHECK(set);
        set_transfer_share((int)shards);
        int64_t lo, hi;
        clip_range(lead, shards, s, lo, hi);
        if (hi > lo) body(lo, hi - lo);
      }
    } catch (...) {
      errors[(size_t)s] = std::current_exception();
      if (!met) rendezvous();   // (nobody waits for a shard that failed early)
    }
    set_transfer_share(1);
  };
  std::vector<std::thread> threads;
  int64_t s = 1;
  try {
    for (; s < shards; ++s) threads.emplace_back(run, s);
  } catch (const std::exception &e) {   // (a joinable std::thread destroyed unjoined would terminate the process)
    {
      std::lock_guard<std::mutex> g(gate_mutex);
      abandoned = true;
    }
    gate_cv.notify_all();
    for (auto &t : threads) t.join();
    (void)hipSetDevice(caller_device);
    throw Failure(format("soundml_amd: cannot start the host thread of shard %lld of %lld (%s)", (long long)s, (long long)shards,
                         e.what()));
  }
  run(0);   // the caller's thread takes the first shard
  for (auto &t : threads) t.join();
  (void)hipSetDevice(caller_device);
  for (auto &e : errors)
    if (e) std::rethrow_exception(e);
}

}  // namespace

// smx_internal.hpp states the contract; for_each_shard and the device list stay private to this file
void host_call(const char *name, const std::vector<HostIn> &in, const std::vector<HostOut> &out, int64_t lead, bool shard,
               const smx_stft_config *pipeline, const std::function<void(const void *const *, void *const *, int64_t, hipStream_t)> &dev) {
  require_device();
  auto one = [&](int64_t clip0, int64_t nc) {
    static const bool trace = env_flag("SMX_HOST_TRACE") == 1;   // diagnostic: where a host call's time goes
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    std::deque<DeviceScratch> scratch;
    std::vector<void *> d_in, d_out;
    for (const HostIn &i : in) d_in.push_back(i.host ? scratch.emplace_back((size_t)nc * i.clip_bytes).ptr : nullptr);
    for (const HostOut &o : out) d_out.push_back(o.host ? scratch.emplace_back((size_t)nc * o.clip_bytes).ptr : nullptr);
    const double t1 = now();
    const size_t in_clip = in[0].clip_bytes, out_clip = out[0].clip_bytes;
    // (without page-locked staging memory the pipelined form cannot run: the serial path's plain hipMemcpy still completes the call)
    if (pipeline && in.size() == 1 && out.size() == 1 && nc >= 8 && (size_t)nc * (in_clip + out_clip) >= ((size_t)128 << 20) &&
        in_clip > 0 && out_clip > 0 && env_flag("SMX_HOST_PIPELINE") != 0 && staging_available()) {
      int64_t unit = (int64_t)(((size_t)48 << 20) / std::max(in_clip, out_clip));   // ~48 MB of the larger side per unit
      unit = std::max<int64_t>(1, std::min<int64_t>(unit, (nc + 3) / 4));
      SMX_HIP_CHECK(hipStreamSynchronize(nullptr));   // the scratch arrays come from the null stream's pool
      (void)pipeline->tables();                      // (lazy tables are built before the threads start)
      pipelined_host_call(reinterpret_cast<const unsigned char *>(in[0].host) + (size_t)clip0 * in_clip, in_clip,
                          reinterpret_cast<unsigned char *>(out[0].host) + (size_t)clip0 * out_clip, out_clip, nc, unit, d_in[0], d_out[0],
                          [&](int64_t u0, int64_t un, hipStream_t stream) {
                            const void *d_unit = reinterpret_cast<const unsigned char *>(d_in[0]) + (size_t)u0 * in_clip;
                            void *d_result = reinterpret_cast<unsigned char *>(d_out[0]) + (size_t)u0 * out_clip;
                            dev(&d_unit, &d_result, un, stream);
                          });
      if (trace) fprintf(stderr, "[smx] host %s: allocate %.2f ms, pipelined upload / kernels / download %.2f (units of %lld clips)\n", name, t1 - t0, now() - t1, (long long)unit);
      return;
    }
    for (size_t i = 0; i < in.size(); ++i)
      if (in[i].host)
        copy_to_device(d_in[i], reinterpret_cast<const unsigned char *>(in[i].host) + (size_t)clip0 * in[i].clip_bytes, (size_t)nc * in[i].clip_bytes);
    const double t2 = now();
    dev(d_in.data(), d_out.data(), nc, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    const double t3 = now();
    for (size_t i = 0; i < out.size(); ++i)
      if (out[i].host)
        copy_to_host(reinterpret_cast<unsigned char *>(out[i].host) + (size_t)clip0 * out[i].clip_bytes, d_out[i], (size_t)nc * out[i].clip_bytes);
    if (trace)
      fprintf(stderr, "[smx] host %s: allocate %.2f ms, upload %.2f, kernels %.2f, download %.2f\n", name, t1 - t0, t2 - t1,
              t3 - t2, now() - t3);
  };
  if (shard) for_each_shard(lead, one);
  else one(0, lead);
}

// ---- shared with the modules' own files (smx_internal.hpp: "host glue shared between the modules") ----
int interior() { return g_interior.load(); }

void check_config(const void *c, const char *fn) {
  if (!c) throw Failure(format("%s: configuration handle is null", fn));
}

void check_rank_extents(const char *fn, int64_t lead, int64_t n) {
  if (lead < 0 || n < 0)
    throw Failure(format("%s: negative extent (lead %lld, n %lld)", fn, (long long)lead, (long long)n));
}

static void check_range(const smx_stft_config &c, int64_t n, int64_t p0, int64_t p1) {
  const int64_t total = c.frames(n);
  if (p0 < 0 || p0 > p1 || p1 > total)  // stft.ml:655-661
    throw InvalidArgument(format(
        "transform_range: cannot take frames [%lld, %lld) of a %lld-frame transform (the range must "
        "satisfy 0 <= p0 <= p1 <= frames)",
        (long long)p0, (long long)p1, (long long)total));
}

// the analysis of frames [p0, p0 + count) of x by c into out, dense ([lead; bins; count]); float64 audio has the float64 interior,
// float32 audio the library's (smx_set_interior)
StftJob stft_job(const smx_stft_config &c, const void *x, int in_bytes, int64_t lead, int64_t n, int64_t x_stride, int64_t p0,
                 int64_t count, OutMode mode, double power, void *out, hipStream_t stream) {
  StftJob job;
  job.cfg = &c;
  job.x = x;
  job.in_bytes = in_bytes;
  job.interior = in_bytes == 8 ? SMX_INTERIOR_F64 : g_interior.load();
  job.lead = lead;
  job.n = n;
  job.x_stride = x_stride;
  job.left = c.left_width();
  job.pad = c.pad;
  job.pad_value = c.pad_value;
  job.p0 = p0;
  job.count = count;
  job.mode = mode;
  job.power = power;
  job.out = out;
  job.out_stride = count;
  job.stream = stream;
  return job;
}

// device-resident analysis of frames [p0, p1)
void stft_range_dev(const smx_stft_config &c, const void *d_x, int in_bytes, int64_t lead, int64_t n,
                    int64_t x_stride, int64_t p0, int64_t p1, OutMode mode, double power, void *d_out,
                    hipStream_t stream) {
  check_rank_extents("transform_range", lead, n);
  if (x_stride < n) throw Failure("transform_range: x_stride is smaller than the signal length");
  check_range(c, n, p0, p1);
  if (p0 == p1 || lead == 0) return;  // frameless_spectrum: nothing to write (stft.ml:629-630)
  if (!d_x || !d_out) throw Failure("transform_range: null device pointer");
  launch_stft(stft_job(c, d_x, in_bytes, lead, n, x_stride, p0, p1 - p0, mode, power, d_out, stream));
}

// host-pointer analysis: the current device, or the device list's clip ranges side by side; a large batch pipelined
static void stft_range_host(const smx_stft_config &c, const void *x, int in_bytes, int64_t lead, int64_t n,
                            int64_t p0, int64_t p1, OutMode mode, double power, void *out) {
  check_rank_extents("transform", lead, n);
  check_range(c, n, p0, p1);
  if (p1 == p0 || lead == 0) return;
  if (!x || !out) throw Failure("transform: null pointer");
  const size_t out_clip = (size_t)c.bins() * (size_t)(p1 - p0) * (mode == OUT_COMPLEX ? 2 : 1) * (size_t)in_bytes;
  host_call("transform", {{x, (size_t)n * (size_t)in_bytes}}, out, out_clip, lead, true, &c,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              stft_range_dev(c, d_in[0], in_bytes, nc, n, n, p0, p1, mode, power, d_out, stream);
            });
}

// Stft.invert's checks (stft.ml:745-786), in the reference's order and wording, under the name of the operation that asks
void check_synthesis(const char *op, const smx_stft_config &c, int64_t bins, int64_t length, bool has_length) {
  if (bins != c.bins())
    throw InvalidArgument(format(
        "%s: cannot invert %lld frequency bins of a %lld-point transform (the bin axis must hold "
        "fft_size / 2 + 1 = %lld values)",
        op, (long long)bins, (long long)c.fft_size, (long long)c.bins()));
  if (has_length && length < 0)
    throw InvalidArgument(format("%s: cannot synthesise a signal of length %lld (length must be non-negative)", op,
                                 (long long)length));
  if (!stft_nola(c))
    throw InvalidArgument(format(
        "%s: cannot invert a %lld-point window advanced by %lld samples inside a %lld-point frame (the "
        "overlap-added squared window must stay above 1e-10 of its largest value at every position)",
        op, (long long)c.win_length, (long long)c.hop, (long long)c.fft_size));
}

// length < 0 means "not given" at the ABI only after the explicit has_length flag said so
void invert_dev(const smx_stft_config &c, const void *d_z, int z_bytes, int64_t lead, int64_t bins, int64_t frames,
                int has_length, int64_t length, void *d_out, hipStream_t stream) {
  if (lead < 0 || frames < 0) throw Failure("invert: negative extent");
  check_synthesis("invert", c, bins, length, has_length != 0);
  const int64_t out_len = has_length ? length : stft_output_length(c, frames);
  if (lead == 0 || out_len == 0) return;
  if (!d_out || (frames > 0 && !d_z)) throw Failure("invert: null device pointer");
  IstftJob job;
  job.cfg = &c;
  job.z = d_z;
  job.z_bytes = z_bytes;
  job.interior = z_bytes == 16 ? SMX_INTERIOR_F64 : g_interior.load();
  job.lead = lead;
  job.frames = frames;
  // only the frames the output can reach are inverted (stft.ml:915-921)
  const int64_t left = c.left_width();
  job.count = has_length ? std::min<int64_t>(frames, (length + left + c.hop - 1) / c.hop) : frames;
  job.out_len = out_len;
  job.out = d_out;
  job.stream = stream;
  launch_istft(job);
}

// host-pointer synthesis: the current device, or the device list's clip ranges side by side (every clip is synthesised on its
// own: stft.mli:214-218); a large batch pipelined
static void invert_host(const smx_stft_config &c, const void *z, int z_bytes, int64_t lead, int64_t bins, int64_t frames,
                        int has_length, int64_t length, void *out) {
  if (lead < 0 || frames < 0) throw Failure("invert: negative extent");
  check_synthesis("invert", c, bins, length, has_length != 0);
  const int64_t out_len = has_length ? length : stft_output_length(c, frames);
  if (lead == 0 || out_len == 0) return;
  if (!out || (frames > 0 && !z)) throw Failure("invert: null pointer");
  host_call("invert", {{z, (size_t)bins * (size_t)frames * (size_t)z_bytes}}, out, (size_t)out_len * (size_t)(z_bytes / 2), lead, true,
            &c, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              invert_dev(c, d_in[0], z_bytes, nc, bins, frames, has_length, length, d_out, stream);
            });
}

}  // namespace smx

using namespace smx;

// =============================== library =====================================
extern "C" {

const char *smx_last_error(void) { return g_last_error.c_str(); }
int smx_version(void) { return 100; }
unsigned long long smx_debug_kernel_launches(void) { return g_kernel_launches.load(); }

int smx_device_count(int *count) {
  return guarded([&] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    if (count) *count = n;
  });
}

int smx_set_device(int device) {
  return guarded([&] { SMX_HIP_CHECK(hipSetDevice(device)); });
}
int smx_set_devices(const int *devices, int n) {
  return guarded([&] {
    if (n < 0 || n > 1024) throw Failure(format("smx_set_devices: cannot list %d devices", n));
    if (n > 0 && !devices) throw Failure("smx_set_devices: null device list");
    int count = 0;
    if (n > 0 && (hipGetDeviceCount(&count) != hipSuccess || count < 1))
      throw Failure("soundml_amd: no HIP device is available (this library has no CPU fallback)");
    for (int i = 0; i < n; ++i)
      if (devices[i] < 0 || devices[i] >= count)
        throw Failure(format("smx_set_devices: device %d is not one of the %d visible devices", devices[i], count));
    std::lock_guard<std::mutex> g(g_devices_mutex);
    g_devices.assign(devices, devices + n);
  });
}
int smx_get_devices(int *devices, int capacity, int *n) {
  return guarded([&] {
    if (!n) throw Failure("smx_get_devices: null count pointer");
    const std::vector<int> d = device_list();
    *n = (int)d.size();
    if (devices)
      for (int i = 0; i < (int)d.size() && i < capacity; ++i) devices[i] = d[(size_t)i];
  });
}
int smx_shard_clip_range(int64_t total_clips, int64_t shards, int64_t shard, int64_t *lo, int64_t *hi) {
  return guarded([&] {
    if (!lo || !hi) throw Failure("smx_shard_clip_range: null result pointer");
    if (total_clips < 0) throw Failure("smx_shard_clip_range: negative clip count");
    if (shards < 1 || shard < 0 || shard >= shards)
      throw Failure(format("smx_shard_clip_range: shard %lld outside a list of %lld", (long long)shard, (long long)shards));
    clip_range(total_clips, shards, shard, *lo, *hi);
  });
}
int smx_debug_staging_peak(int *uploads, int *downloads, int reset) {
  return guarded([&] { staging_peak(uploads, downloads, reset != 0); });
}
int64_t smx_debug_clips_per_launch(int64_t tiles_per_clip, int threads) { return clips_per_launch(tiles_per_clip, threads); }

int smx_set_scratch_retention(int64_t bytes) {
  return guarded([&] {
    if (bytes < -1) throw Failure("set_scratch_retention: bytes must be >= 0, or -1 for the default");
    set_scratch_retention(bytes);
  });
}

int smx_set_interior(int interior) {
  return guarded([&] {
    if (interior != SMX_INTERIOR_F32 && interior != SMX_INTERIOR_F64)
      throw InvalidArgument(format("set_interior: unknown interior %d", interior));
    g_interior.store(interior);
  });
}
int smx_get_interior(void) { return g_interior.load(); }

int smx_synchronize(void *stream) {
  return guarded([&] { SMX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream)); });
}

// diagnostics (tests): Stft.transform of device-resident float32 audio into Griffin-Lim's internal frame-major layout
int smx_debug_stft_transform_frame_major_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, float *d_out,
                                                 int64_t pitch_floats, int64_t rows_per_clip, void *stream) {
  return guarded([&] {
    check_config(c, "transform");
    const StftJob job = stft_job(*c, d_x, 4, lead, n, n, 0, c->frames(n), OUT_COMPLEX, 0.0, d_out, (hipStream_t)stream);
    if (!launch_stft_complex_fm(job, d_out, pitch_floats, rows_per_clip)) throw Failure("transform (frame-major): not eligible");
  });
}

int smx_host_alloc(size_t bytes, void **ptr) {
  return guarded([&] {
    if (!ptr) throw Failure("smx_host_alloc: null result pointer");
    *ptr = nullptr;
    require_device();
    *ptr = host_alloc(bytes);
  });
}
int smx_host_free(void *ptr) {
  return guarded([&] { host_free(ptr); });
}

// =============================== Window ======================================
int smx_window_make(int kind, int periodic, int64_t n, double *out) {
  return guarded([&] {
    if (n >= 1 && !out) throw Failure("make: null output");
    window_make(kind, periodic != 0, n, out);
  });
}

int smx_window_make_param(int kind, double param, int periodic, int64_t n, double *out) {
  return guarded([&] {
    if (n >= 1 && !out) throw Failure("make: null output");
    window_make_param(kind, param, periodic != 0, n, out);
  });
}

int smx_window_cola(int kind, double param, int64_t length, int64_t hop, int *cola) {
  return guarded([&] {
    if (!cola) throw Failure("cola: null output");
    *cola = window_cola(kind, param, length, hop) ? 1 : 0;
  });
}

// Convert.hz_to_mel / mel_to_hz (convert.ml:70-102): the scalar maps the mel breakpoints are built from, on host values
int smx_hz_to_mel(int scale, const double *f, int64_t n, double *out) {
  return guarded([&] {
    if (scale != SMX_MEL_SLANEY && scale != SMX_MEL_HTK) throw InvalidArgument(format("hz_to_mel: unknown mel scale %d", scale));
    if (n > 0 && (!f || !out)) throw Failure("hz_to_mel: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = hz_to_mel(f[i], scale);
  });
}
int smx_mel_to_hz(int scale, const double *m, int64_t n, double *out) {
  return guarded([&] {
    if (scale != SMX_MEL_SLANEY && scale != SMX_MEL_HTK) throw InvalidArgument(format("mel_to_hz: unknown mel scale %d", scale));
    if (n > 0 && (!m || !out)) throw Failure("mel_to_hz: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = mel_to_hz(m[i], scale);
  });
}

// =============================== Stft.Config =================================
int smx_stft_config_create(int64_t fft_size, int64_t win_length, int64_t hop, int alignment, int pad,
                           double pad_value, int scale, int window_kind, const double *custom_window,
                           smx_stft_config **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null output handle");
    *out = stft_config_create(fft_size, win_length, hop, alignment, pad, pad_value, scale, window_kind,
                              custom_window);
  });
}
void smx_stft_config_destroy(smx_stft_config *c) { delete c; }
int64_t smx_stft_config_fft_size(const smx_stft_config *c) { return c ? c->fft_size : -1; }
int64_t smx_stft_config_hop(const smx_stft_config *c) { return c ? c->hop : -1; }
int64_t smx_stft_config_win_length(const smx_stft_config *c) { return c ? c->win_length : -1; }
int64_t smx_stft_config_bins(const smx_stft_config *c) { return c ? c->bins() : -1; }
int64_t smx_stft_config_left_width(const smx_stft_config *c) { return c ? c->left_width() : -1; }
int64_t smx_stft_config_right_width(const smx_stft_config *c) { return c ? c->right_width() : -1; }
int64_t smx_stft_config_latency(const smx_stft_config *c) {
  return c ? (c->alignment == SMX_ALIGN_CENTERED ? c->fft_size / 2 : 0) : -1;
}
int smx_stft_config_analysis_window(const smx_stft_config *c, double *out) {
  return guarded([&] {
    check_config(c, "analysis_window");
    std::memcpy(out, c->analysis_window.data(), c->analysis_window.size() * sizeof(double));
  });
}

// =============================== frame grid ==================================
int smx_stft_frames(const smx_stft_config *c, int64_t n, int64_t *out) {
  return guarded([&] {
    check_config(c, "frames");
    *out = c->frames(n);
  });
}
int smx_stft_first_complete(const smx_stft_config *c, int64_t *out) {
  return guarded([&] {
    check_config(c, "first_complete");
    *out = stft_first_complete(*c);
  });
}
int smx_stft_last_complete(const smx_stft_config *c, int64_t n, int64_t *out) {
  return guarded([&] {
    check_config(c, "last_complete");
    *out = stft_last_complete(*c, n);
  });
}
static void check_sample_rate(const char *op, int64_t sample_rate) {  // stft.ml:237-243
  if (sample_rate < 1)
    throw InvalidArgument(format(
        "%s: cannot use a sample rate of %lld Hz (sample_rate must be at least 1)", op,
        (long long)sample_rate));
}
int smx_stft_times(const smx_stft_config *c, int64_t sample_rate, int64_t n, double *out) {
  return guarded([&] {
    check_config(c, "times");
    check_sample_rate("times", sample_rate);
    if (n < 0)
      throw InvalidArgument(format(
          "times: cannot analyse a signal of length %lld (length must be non-negative)", (long long)n));
    const int64_t count = c->frames(n);
    for (int64_t p = 0; p < count; ++p)  // stft.ml:245-254: p*hop exact, one rounding
      out[p] = ((double)p * (double)c->hop) / (double)sample_rate;
  });
}
int smx_stft_frequencies(const smx_stft_config *c, int64_t sample_rate, double *out) {
  return guarded([&] {
    check_config(c, "frequencies");
    check_sample_rate("frequencies", sample_rate);
    const double step = (double)sample_rate / (double)c->fft_size;  // stft.ml:256-261
    for (int64_t k = 0; k < c->bins(); ++k) out[k] = (double)k * step;
  });
}

// =============================== transforms ==================================
int smx_stft_transform_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n,
                           float *out) {
  return guarded([&] {
    check_config(c, "transform");
    check_rank_extents("transform", lead, n);
    stft_range_host(*c, x, 4, lead, n, 0, c->frames(n), OUT_COMPLEX, 0.0, out);
  });
}
int smx_stft_transform_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n,
                           double *out) {
  return guarded([&] {
    check_config(c, "transform");
    check_rank_extents("transform", lead, n);
    stft_range_host(*c, x, 8, lead, n, 0, c->frames(n), OUT_COMPLEX, 0.0, out);
  });
}
int smx_stft_transform_range_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n,
                                 int64_t p0, int64_t p1, float *out) {
  return guarded([&] {
    check_config(c, "transform_range");
    stft_range_host(*c, x, 4, lead, n, p0, p1, OUT_COMPLEX, 0.0, out);
  });
}
int smx_stft_transform_range_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n,
                                 int64_t p0, int64_t p1, double *out) {
  return guarded([&] {
    check_config(c, "transform_range");
    stft_range_host(*c, x, 8, lead, n, p0, p1, OUT_COMPLEX, 0.0, out);
  });
}
int smx_stft_power_spectrum_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n,
                                double power, float *out) {
  return guarded([&] {
    check_config(c, "power_spectrum");
    check_rank_extents("power_spectrum", lead, n);
    stft_range_host(*c, x, 4, lead, n, 0, c->frames(n), OUT_POWER, power, out);
  });
}
int smx_stft_power_spectrum_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n,
                                double power, double *out) {
  return guarded([&] {
    check_config(c, "power_spectrum");
    check_rank_extents("power_spectrum", lead, n);
    stft_range_host(*c, x, 8, lead, n, 0, c->frames(n), OUT_POWER, power, out);
  });
}

// |frames [p0, p1)|^power from host memory: what an nx-tensor caller of a ranged power face gets (the OCaml stub's
// mode 1 honours its range through these instead of writing every frame)
int smx_stft_power_range_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, int64_t p0, int64_t p1,
                             double power, float *out) {
  return guarded([&] {
    check_config(c, "transform_range");
    stft_range_host(*c, x, 4, lead, n, p0, p1, OUT_POWER, power, out);
  });
}
int smx_stft_power_range_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, int64_t p0, int64_t p1,
                             double power, double *out) {
  return guarded([&] {
    check_config(c, "transform_range");
    stft_range_host(*c, x, 8, lead, n, p0, p1, OUT_POWER, power, out);
  });
}

int smx_stft_transform_range_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead,
                                     int64_t n, int64_t x_stride, int64_t p0, int64_t p1,
                                     float *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "transform_range");
    stft_range_dev(*c, d_x, 4, lead, n, x_stride, p0, p1, OUT_COMPLEX, 0.0, d_out, (hipStream_t)stream);
  });
}
int smx_stft_transform_range_f64_dev(const smx_stft_config *c, const double *d_x, int64_t lead,
                                     int64_t n, int64_t x_stride, int64_t p0, int64_t p1,
                                     double *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "transform_range");
    stft_range_dev(*c, d_x, 8, lead, n, x_stride, p0, p1, OUT_COMPLEX, 0.0, d_out, (hipStream_t)stream);
  });
}
int smx_stft_power_range_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n,
                                 int64_t x_stride, int64_t p0, int64_t p1, double power, float *d_out,
                                 void *stream) {
  return guarded([&] {
    check_config(c, "power_spectrum");
    stft_range_dev(*c, d_x, 4, lead, n, x_stride, p0, p1, OUT_POWER, power, d_out, (hipStream_t)stream);
  });
}
int smx_stft_power_range_f64_dev(const smx_stft_config *c, const double *d_x, int64_t lead, int64_t n,
                                 int64_t x_stride, int64_t p0, int64_t p1, double power,
                                 double *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "power_spectrum");
    stft_range_dev(*c, d_x, 8, lead, n, x_stride, p0, p1, OUT_POWER, power, d_out, (hipStream_t)stream);
  });
}

// ---- least-squares synthesis: Stft.invert (stft.ml:902-939) ----------------------------------------
int smx_stft_nola(const smx_stft_config *c, int *invertible) {
  return guarded([&] {
    check_config(c, "nola");
    if (invertible) *invertible = stft_nola(*c) ? 1 : 0;
  });
}
int smx_stft_output_length(const smx_stft_config *c, int64_t frames, int64_t *length) {
  return guarded([&] {
    check_config(c, "output_length");
    if (frames < 0) throw Failure("output_length: negative frame count");
    if (length) *length = stft_output_length(*c, frames);
  });
}
int smx_stft_invert_f32(const smx_stft_config *c, const float *z, int64_t lead, int64_t bins, int64_t frames,
                        int has_length, int64_t length, float *out) {
  return guarded([&] {
    check_config(c, "invert");
    invert_host(*c, z, 8, lead, bins, frames, has_length, length, out);
  });
}
int smx_stft_invert_f64(const smx_stft_config *c, const double *z, int64_t lead, int64_t bins, int64_t frames,
                        int has_length, int64_t length, double *out) {
  return guarded([&] {
    check_config(c, "invert");
    invert_host(*c, z, 16, lead, bins, frames, has_length, length, out);
  });
}
int smx_stft_invert_f32_dev(const smx_stft_config *c, const float *d_z, int64_t lead, int64_t bins, int64_t frames,
                            int has_length, int64_t length, float *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "invert");
    invert_dev(*c, d_z, 8, lead, bins, frames, has_length, length, d_out, (hipStream_t)stream);
  });
}
int smx_stft_invert_f64_dev(const smx_stft_config *c, const double *d_z, int64_t lead, int64_t bins, int64_t frames,
                            int has_length, int64_t length, double *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "invert");
    invert_dev(*c, d_z, 16, lead, bins, frames, has_length, length, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
