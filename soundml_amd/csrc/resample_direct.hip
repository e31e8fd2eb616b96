// Resample.Config / Resample.apply (resample.mli:91-197, resample.ml:872-1019): the plan of an arbitrary sample_rate -> target
// conversion, and the polyphase stage evaluated at its true cost of 2 K + 1 multiply-adds per output.
//
// The stage (resample.ml:1318-1326):   y[c][i] = sum_j bank[p_i][j] x[c][q_i - j],   j = 0 .. 2 K,
//   s_i = i M + K L,  p_i = s_i mod L,  q_i = s_i div L,  bank[p][j] = proto[p + j L],  x = 0 outside the stream.
// p_i depends on i mod L only ((i M) mod L), so the bank is stored in VISIT order and transposed: visit[j][r] =
// bank[(r M) mod L][j], r = i mod L.  Consecutive outputs (consecutive lanes) read consecutive addresses of one tap row.
//
// THE SUMMATION ORDER.  Every output is the same expression whatever computes it: four partial sums, tap j into partial
// sum j mod 4 by one fmaf each, in ascending j, over the bank padded with zero rows to a multiple of four taps; then
// (s0 + s1) + (s2 + s3).  A sample outside the stream enters as the value 0, never as a skipped tap.  Nothing in this
// depends on the tile, the tap chunk, the channel count, the staging mode or the position of the output in the call: the
// bit-for-bit contracts of apply (batch = rows, host = device, strided = contiguous) and the partition law of the
// streaming kernel rest on exactly that, and this file is built with -ffp-contract=off so that only the fmaf fuses.
#include "smx_internal.hpp"

using namespace smx;

namespace {

constexpr int64_t kBankBudgetBytes = 8 * 1024 * 1024;   // resample.ml:230
constexpr int kLdsFloats = 12288;                       // 48 KiB of samples per workgroup: three workgroups per CU
constexpr int kMaxFactor = 1 << 22;                     // tile offsets (p0 + t M, t < 256) stay inside 32 bits

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

double kaiser_numtaps(double att, double width) {   // resample.ml:113-116
  const double n = std::ceil((att - 7.95) / 2.285 / (M_PI * width) + 1.0);
  return std::fmod(n, 2.0) == 0.0 ? n + 1.0 : n;
}

std::string pp_bytes(double bytes) {   // resample.ml:530-538
  const char *unit = "KB";
  double v = bytes / 1024.0;
  if (bytes >= 1024.0 * 1024.0 * 1024.0) {
    v = bytes / (1024.0 * 1024.0 * 1024.0);
    unit = "GB";
  } else if (bytes >= 1024.0 * 1024.0) {
    v = bytes / (1024.0 * 1024.0);
    unit = "MB";
  }
  return v == std::floor(v) ? format("%.0f %s", v, unit) : format("%.1f %s", v, unit);
}

struct DirectArgs {
  const float *bank;                  // visit[j][r], taps4 rows of L
  const float *x;                     // x[c * x_stride + (a - x_base)] is sample a of channel c for x_lo <= a < x_hi; 0 elsewhere
  int64_t x_stride, x_base, x_lo, x_hi;
  float *y;                           // y[c * y_stride + (i - out_first)]
  int64_t y_stride, out_first, out_count, tiles;
  int l, m, k, taps4, span, chunk;    // span = ceil(T M / L) + 2;  chunk: taps staged at a time (a multiple of 4)
};

// One workgroup: T = blockDim.x consecutive outputs of one channel, one per thread.  STAGED: the samples the tile reads
// are staged in LDS, a chunk of taps at a time (window = the tile's input span + the chunk's taps), so K is unbounded;
// otherwise (an input span too long for LDS: very heavy decimation) each thread reads its samples from global memory.
template <bool STAGED>
__global__ __launch_bounds__(256) void resample_direct_kernel(DirectArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int t = (int)threadIdx.x, T = (int)blockDim.x;
  const int64_t c = (int64_t)blockIdx.x / a.tiles, tile = (int64_t)blockIdx.x - c * a.tiles;
  const int64_t i0 = a.out_first + tile * T;                 // 64-bit per workgroup: i M passes 2^32 in long clips
  const int64_t s0 = i0 * (int64_t)a.m + (int64_t)a.k * a.l;
  const int p0 = (int)(s0 % a.l), r0 = (int)(i0 % a.l);
  const int64_t q0 = s0 / a.l;
  const bool live = tile * T + t < a.out_count;
  const int tt = live ? t : 0;                               // idle lanes of the last tile shadow lane 0: every index stays in range
  const int dq = (p0 + tt * a.m) / a.l;                      // q_i - q0, in [0, span - 2]
  const int r = (r0 + tt) % a.l;
  const float *bank = a.bank + r;
  const float *xc = a.x + c * a.x_stride;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (STAGED) {
    const int len = a.span - 1 + a.chunk;
    for (int j0 = 0; j0 < a.taps4; j0 += a.chunk) {
      const int jn = min(a.chunk, a.taps4 - j0);             // a multiple of 4
      const int64_t w0 = q0 - j0 - (a.chunk - 1);            // xs[e] = sample w0 + e
      __syncthreads();
      for (int e = t; e < len; e += T) {
        const int64_t at = w0 + e;
        xs[e] = at >= a.x_lo && at < a.x_hi ? xc[at - a.x_base] : 0.0f;
      }
      __syncthreads();
      const float *b = bank + j0 * a.l;   // taps4 L stays far inside 32 bits (the 8 MiB bank budget)
      const float *xv = xs + dq + (a.chunk - 1);             // tap j0 + jj reads xv[-jj]: from dq + chunk - 1 down to dq >= 0
      for (int jj = 0; jj < jn; jj += 4) {
        s[0] = fmaf(b[(jj + 0) * a.l], xv[-(jj + 0)], s[0]);
        s[1] = fmaf(b[(jj + 1) * a.l], xv[-(jj + 1)], s[1]);
        s[2] = fmaf(b[(jj + 2) * a.l], xv[-(jj + 2)], s[2]);
        s[3] = fmaf(b[(jj + 3) * a.l], xv[-(jj + 3)], s[3]);
      }
    }
  } else {
    const int64_t q = q0 + dq;
    for (int j = 0; j < a.taps4; j += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t at = q - (j + u);
        const float v = at >= a.x_lo && at < a.x_hi ? xc[at - a.x_base] : 0.0f;
        s[u] = fmaf(bank[(j + u) * a.l], v, s[u]);
      }
    }
  }
  if (live) a.y[c * a.y_stride + tile * T + t] = (s[0] + s[1]) + (s[2] + s[3]);
}

}  // namespace

struct smx_resample_config {
  int64_t sample_rate = 0, target = 0;
  int quality = SMX_RESAMPLE_HIGH;
  double attenuation = 0.0, passband = 0.0;
  int64_t l = 1, m = 1, k = 0;
  double fc = 0.0, beta = 0.0;
  int executor = SMX_RESAMPLE_IDENTITY;
  std::vector<double> proto;                 // 2 K L + 1
  smx_resample_stage *stage = nullptr;       // the "ols" executor: the polyphase-block stage of fir.hip on this prototype
  // the "direct" executor's launch plan: a function of (L, M, K) alone
  int taps4 = 0, threads = 256, span = 0, chunk = 0;
  bool staged = true;

  const float *bank() const;                 // the visit-order bank in float32 on the current device, uploaded on first use
  ~smx_resample_config() {
    if (stage) smx_resample_stage_destroy(stage);
    for (auto &kv : banks_) (void)hipFree(kv.second);
  }

 private:
  mutable std::mutex mutex_;
  mutable std::map<int, float *> banks_;
};

const float *smx_resample_config::bank() const {
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(mutex_);
  auto it = banks_.find(device);
  if (it != banks_.end()) return it->second;
  std::vector<float> visit((size_t)taps4 * (size_t)l, 0.0f);
  const int64_t taps = (int64_t)proto.size();
  for (int64_t r = 0; r < l; ++r) {
    const int64_t p = (r * m) % l;
    for (int64_t j = 0; p + j * l < taps; ++j) visit[(size_t)(j * l + r)] = (float)proto[(size_t)(p + j * l)];
  }
  float *d = nullptr;
  SMX_HIP_CHECK(hipMalloc((void **)&d, visit.size() * sizeof(float)));
  hipError_t err = hipMemcpy(d, visit.data(), visit.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    (void)hipFree(d);
    SMX_HIP_CHECK(err);
  }
  banks_[device] = d;
  return d;
}

// Resample.Kernel of a "direct" config: the last 2 K samples of every channel on the device; a step runs the stage on
// [history ++ chunk] with ABSOLUTE output indices, so every partition of a signal totals apply bit for bit.
struct smx_resample_stream {
  const smx_resample_config *config = nullptr;   // borrowed: outlives the kernel
  int64_t channels = 0, max_block = 0, fed = 0, emitted = 0, hist = 0;
  float *history = nullptr;                      // [channels][hist]: samples fed - hist .. fed - 1 (zeros before the stream)
  bool drained = false;
  int device = 0;
  ~smx_resample_stream() {
    if (history) (void)hipFree(history);
  }
};

namespace {

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
int64_t out_frames(const smx_resample_config &c, int64_t n) { return ceil_div(n * c.l, c.m); }
// resample.ml:1298 `ready`: the outputs whose every input is among the first `fed` samples
int64_t stream_ready(const smx_resample_config &c, int64_t fed) { return fed > c.k ? ceil_div((fed - c.k) * c.l, c.m) : 0; }

void plan_direct(smx_resample_config &c) {
  c.taps4 = (int)((2 * c.k + 1 + 3) & ~int64_t(3));
  c.staged = false;
  c.threads = 256;
  for (int threads : {256, 64}) {
    const int64_t span = ceil_div((int64_t)threads * c.m, c.l) + 2;
    const int64_t want = std::min<int64_t>(c.taps4, 256);      // never stage fewer than 256 taps per barrier pair
    if (span + want > kLdsFloats) continue;
    c.staged = true;
    c.threads = threads;
    c.span = (int)span;
    c.chunk = (int)std::min<int64_t>(c.taps4, (kLdsFloats - span) & ~int64_t(3));
    return;
  }
}

// outputs out_first .. out_first + out_count - 1 of every channel from samples [x_lo, x_hi) held at d_x (sample x_base first)
void direct_run(const smx_resample_config &c, const float *d_x, int64_t x_stride, int64_t x_base, int64_t x_lo, int64_t x_hi,
                int64_t channels, float *d_y, int64_t y_stride, int64_t out_first, int64_t out_count, hipStream_t stream) {
  if (channels <= 0 || out_count <= 0) return;
  DirectArgs a;
  a.bank = c.bank();
  a.x = d_x; a.x_stride = x_stride; a.x_base = x_base; a.x_lo = x_lo; a.x_hi = x_hi;
  a.y = d_y; a.y_stride = y_stride; a.out_first = out_first; a.out_count = out_count;
  a.tiles = ceil_div(out_count, c.threads);
  a.l = (int)c.l; a.m = (int)c.m; a.k = (int)c.k; a.taps4 = c.taps4; a.span = c.span; a.chunk = c.chunk;
  const unsigned blocks = grid_x("resample", "output tiles", a.tiles * channels, (int)c.threads);   // channels fold into grid x
  if (c.staged) {
    const size_t lds = (size_t)(c.span - 1 + c.chunk) * sizeof(float);
    SMX_LAUNCH(resample_direct_kernel<true>, dim3(blocks), dim3(c.threads), lds, stream, a);
  } else {
    SMX_LAUNCH(resample_direct_kernel<false>, dim3(blocks), dim3(c.threads), 0, stream, a);
  }
  SMX_HIP_CHECK(hipGetLastError());
}

void apply_dev(const smx_resample_config &c, const float *d_x, int64_t channels, int64_t n, int64_t x_stride, float *d_y,
               int64_t y_stride, hipStream_t stream) {
  if (channels < 0 || n < 0) throw Failure("resample: negative extent");
  const int64_t n_out = out_frames(c, n);
  if (channels == 0 || n_out == 0) return;
  if (x_stride < n || y_stride < n_out) throw Failure("resample: stride smaller than the signal length");
  if (!d_x || !d_y) throw Failure("resample: null device pointer");
  switch (c.executor) {
    case SMX_RESAMPLE_IDENTITY:
      SMX_HIP_CHECK(hipMemcpy2DAsync(d_y, (size_t)y_stride * sizeof(float), d_x, (size_t)x_stride * sizeof(float),
                                     (size_t)n * sizeof(float), (size_t)channels, hipMemcpyDeviceToDevice, stream));
      return;
    case SMX_RESAMPLE_OLS:
      if (smx_resample_stage_apply_f32_dev(c.stage, d_x, channels, n, x_stride, d_y, y_stride, stream) != SMX_OK)
        throw Failure(smx_last_error());
      return;
    default:
      direct_run(c, d_x, x_stride, 0, 0, n, channels, d_y, y_stride, 0, n_out, stream);
  }
}

void copy_rows(float *dst, int64_t dst_stride, const float *src, int64_t src_stride, int64_t cols, int64_t rows, hipStream_t stream) {
  if (cols <= 0 || rows <= 0) return;
  SMX_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dst_stride * sizeof(float), src, (size_t)src_stride * sizeof(float),
                                 (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyDeviceToDevice, stream));
}

void stream_check(const smx_resample_stream *k) {
  if (!k || !k->config) throw Failure("resample_kernel: null kernel");
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  if (device != k->device) throw Failure("resample_kernel: the kernel was prepared on another device");
}

int64_t stream_step_dev(smx_resample_stream &k, const float *d_x, int64_t n, int64_t x_stride, float *d_y, int64_t y_stride,
                        hipStream_t stream) {
  const smx_resample_config &c = *k.config;
  if (k.drained)
    throw InvalidArgument("resample_kernel_step: cannot feed a kernel drained by flush (reset it before a new signal)");
  if (n < 0) throw Failure("resample_kernel_step: negative extent");
  if (n > k.max_block)
    throw InvalidArgument(format("resample_kernel_step: cannot feed a chunk of %lld samples to a kernel prepared for at most %lld",
                                 (long long)n, (long long)k.max_block));
  if (n == 0) return 0;
  if (!d_x || x_stride < n) throw Failure("resample_kernel_step: null chunk or stride smaller than the chunk");
  const int64_t n_out = stream_ready(c, k.fed + n) - k.emitted;
  if (n_out > 0 && (!d_y || y_stride < n_out)) throw Failure("resample_kernel_step: null output or stride smaller than the emitted run");
  smx::init_device_pool();
  const int64_t alen = k.hist + n, a_stride = (alen + 1) & ~int64_t(1);
  DeviceScratch av;   // [history ++ chunk]: samples fed - hist .. fed + n - 1
  av.pool((size_t)k.channels * (size_t)a_stride * sizeof(float), stream);
  copy_rows(av.as<float>(), a_stride, k.history, k.hist, k.hist, k.channels, stream);
  copy_rows(av.as<float>() + k.hist, a_stride, d_x, x_stride, n, k.channels, stream);
  const int64_t base = k.fed - k.hist;
  // the history starts as zeros, which is what the samples before the stream are: the window opens at `base` either way
  direct_run(c, av.as<float>(), a_stride, base, base, k.fed + n, k.channels, d_y, y_stride, k.emitted, n_out, stream);
  copy_rows(k.history, k.hist, av.as<float>() + n, a_stride, k.hist, k.channels, stream);
  k.fed += n;
  if (n_out > 0) k.emitted += n_out;
  return n_out > 0 ? n_out : 0;
}

int64_t stream_pending(const smx_resample_stream &k) { return k.drained ? 0 : out_frames(*k.config, k.fed) - k.emitted; }

int64_t stream_flush_dev(smx_resample_stream &k, float *d_y, int64_t y_stride, hipStream_t stream) {
  if (k.drained) return 0;   // a second flush has nothing (resample.mli:313-317)
  const int64_t n_out = stream_pending(k);
  k.drained = true;
  if (n_out <= 0) return 0;
  if (!d_y || y_stride < n_out) throw Failure("resample_kernel_flush: null output or stride smaller than the tail");
  const int64_t base = k.fed - k.hist;   // silence past the end of the stream: the window closes at `fed`
  direct_run(*k.config, k.history, k.hist, base, base, k.fed, k.channels, d_y, y_stride, k.emitted, n_out, stream);
  k.emitted += n_out;
  return n_out;
}

}  // namespace

extern "C" {

int smx_resample_config_create(int64_t sample_rate, int64_t target, int quality, double attenuation, double passband,
                               smx_resample_config **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null output handle");
    if (sample_rate < 1)
      throw InvalidArgument(format("create: cannot resample from %lld Hz (sample_rate must be at least 1)", (long long)sample_rate));
    if (target < 1)
      throw InvalidArgument(format("create: cannot resample to %lld Hz (target must be at least 1)", (long long)target));
    switch (quality) {   // resample.ml:519-526
      case SMX_RESAMPLE_FAST: attenuation = 100.0; passband = 0.913; break;
      case SMX_RESAMPLE_HIGH: attenuation = 126.0; passband = 0.913; break;
      case SMX_RESAMPLE_BEST: attenuation = 175.0; passband = 0.913; break;
      case SMX_RESAMPLE_CUSTOM: break;
      default: throw Failure("create: unknown quality");
    }
    if (!(std::isfinite(attenuation) && attenuation >= 40.0 && attenuation <= 200.0))
      throw InvalidArgument(format("create: cannot design a filter with %g dB of stop-band rejection (attenuation must be finite, "
                                   "in [40, 200])", attenuation));
    if (!(std::isfinite(passband) && passband >= 0.5 && passband <= 0.99))
      throw InvalidArgument(format("create: cannot preserve %g of the band (passband must be finite, in [0.5, 0.99])", passband));
    auto c = std::make_unique<smx_resample_config>();
    c->sample_rate = sample_rate; c->target = target;
    c->quality = quality; c->attenuation = attenuation; c->passband = passband;
    const int64_t g = gcd64(sample_rate, target);
    const int64_t l = target / g, m = sample_rate / g;
    c->l = l; c->m = m;
    if (l == 1 && m == 1) {
      c->proto.assign(1, 1.0);
      *out = c.release();
      return;
    }
    const double big = (double)std::max(l, m), small = (double)std::min(l, m);
    const double ntaps = kaiser_numtaps(attenuation, (1.0 - passband) / big);
    const double k_f = std::ceil((ntaps - 1.0) / (2.0 * (double)l));   // in float first: the budget check precedes any conversion
    const double bank_bytes = (double)l * (2.0 * k_f + 1.0) * 8.0;
    if (!(bank_bytes <= (double)kBankBudgetBytes))
      throw InvalidArgument(format("create: cannot resample %lld Hz to %lld Hz (%lld phases need a %s bank; the budget is %s, and no "
                                   "two-stage split brings it under)%s", (long long)sample_rate, (long long)target, (long long)l,
                                   pp_bytes(bank_bytes).c_str(), pp_bytes((double)kBankBudgetBytes).c_str(),
                                   big < 1.01 * small ? " hint: near-unity conversion is clock-drift correction, which the fixed-ratio "
                                                        "resampler does not do" : ""));
    if (l > kMaxFactor || m > kMaxFactor)
      throw Failure(format("create: this device path holds factors up to %d (L = %lld, M = %lld)", kMaxFactor, (long long)l, (long long)m));
    c->k = std::max<int64_t>(1, (int64_t)k_f);
    c->fc = (1.0 + passband) / (2.0 * big);
    c->beta = kaiser_beta(attenuation);
    c->proto.resize((size_t)(2 * c->k * l + 1));
    if (smx_resample_prototype(l, c->k, c->fc, c->beta, c->proto.data()) != SMX_OK) throw Failure(smx_last_error());
    c->executor = SMX_RESAMPLE_DIRECT;
    // resample.ml:951: a pure x2..4 or /2..4 stage runs by overlap-save where its geometry allows (and where the
    // polyphase-block stage of fir.hip takes the prototype)
    if ((m == 1 && l >= 2 && l <= 4) || (l == 1 && m >= 2 && m <= 4)) {
      int eligible = 0;
      if (smx_resample_ols_geom(sample_rate, l, m, c->k, nullptr, nullptr, nullptr, &eligible) != SMX_OK) throw Failure(smx_last_error());
      smx_resample_stage *st = nullptr;
      if (eligible && smx_resample_stage_create(c->proto.data(), l, m, c->k, &st) == SMX_OK) {
        if (smx_resample_stage_streams(st)) {
          c->stage = st;
          c->executor = SMX_RESAMPLE_OLS;
        } else {
          smx_resample_stage_destroy(st);
        }
      }
    }
    if (c->executor == SMX_RESAMPLE_DIRECT) plan_direct(*c);
    *out = c.release();
  });
}
void smx_resample_config_destroy(smx_resample_config *c) { delete c; }
int64_t smx_resample_config_sample_rate(const smx_resample_config *c) { return c ? c->sample_rate : -1; }
int64_t smx_resample_config_target(const smx_resample_config *c) { return c ? c->target : -1; }
int smx_resample_config_quality(const smx_resample_config *c, double *attenuation, double *passband) {
  if (!c) return -1;
  if (attenuation) *attenuation = c->attenuation;
  if (passband) *passband = c->passband;
  return c->quality;
}
int64_t smx_resample_config_l(const smx_resample_config *c) { return c ? c->l : -1; }
int64_t smx_resample_config_m(const smx_resample_config *c) { return c ? c->m : -1; }
int64_t smx_resample_config_latency(const smx_resample_config *c) { return c ? c->k : -1; }
int smx_resample_config_executor(const smx_resample_config *c) { return c ? c->executor : -1; }
const smx_resample_stage *smx_resample_config_stage(const smx_resample_config *c) { return c ? c->stage : nullptr; }
int smx_resample_config_design(const smx_resample_config *c, double *fc, double *beta) {
  return guarded([&] {
    if (!c) throw Failure("resample_config: null config");
    if (fc) *fc = c->fc;
    if (beta) *beta = c->beta;
  });
}
int smx_resample_config_output_latency(const smx_resample_config *c, int64_t *num, int64_t *den) {
  return guarded([&] {   // resample.ml:1031-1036
    if (!c || !num || !den) throw Failure("output_latency: null argument");
    const int64_t n = c->k * c->l;
    const int64_t g = n ? gcd64(n, c->m) : 1;
    *num = n ? n / g : 0;
    *den = n ? c->m / g : 1;
  });
}
int smx_resample_config_output_frames(const smx_resample_config *c, int64_t n, int64_t *out) {
  return guarded([&] {   // resample.ml:1038-1051
    if (!c || !out) throw Failure("output_frames: null argument");
    if (n < 0)
      throw InvalidArgument(format("output_frames: cannot resample a signal of length %lld (length must be non-negative)", (long long)n));
    if (n > 0 && n > INT64_MAX / c->l)
      throw InvalidArgument(format("output_frames: cannot resample a signal of length %lld (n * %lld overflows)", (long long)n,
                                   (long long)c->l));
    *out = out_frames(*c, n);
  });
}
int64_t smx_resample_config_prototype_length(const smx_resample_config *c) { return c ? (int64_t)c->proto.size() : -1; }
int smx_resample_config_prototype(const smx_resample_config *c, double *h) {
  return guarded([&] {
    if (!c || !h) throw Failure("prototype: null argument");
    std::copy(c->proto.begin(), c->proto.end(), h);
  });
}

int smx_resample_apply_f32_dev(const smx_resample_config *c, const float *d_x, int64_t channels, int64_t n, int64_t x_stride,
                               float *d_y, int64_t y_stride, void *stream) {
  return guarded([&] {
    if (!c) throw Failure("resample: null config");
    apply_dev(*c, d_x, channels, n, x_stride, d_y, y_stride, (hipStream_t)stream);
  });
}

// plain hipMalloc + hipMemcpy, not host_call: at these sizes its pooled scratch and staged copy measured slower (profiles/host_faces/NOTES.md)
int smx_resample_apply_f32(const smx_resample_config *c, const float *x, int64_t channels, int64_t n, float *y) {
  return guarded([&] {
    if (!c) throw Failure("resample: null config");
    if (channels < 0 || n < 0) throw Failure("resample: negative extent");
    const int64_t n_out = out_frames(*c, n);
    if (channels == 0 || n_out == 0) return;
    if (!x || !y) throw Failure("resample: null pointer");
    require_device();
    DeviceScratch dx, dy;
    dx.alloc((size_t)channels * (size_t)n * sizeof(float));
    dy.alloc((size_t)channels * (size_t)n_out * sizeof(float));
    SMX_HIP_CHECK(hipMemcpy(dx.ptr, x, (size_t)channels * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    apply_dev(*c, dx.as<float>(), channels, n, n, dy.as<float>(), n_out, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    SMX_HIP_CHECK(hipMemcpy(y, dy.ptr, (size_t)channels * (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost));
  });
}

/* ---- Resample.Kernel of a "direct" config (resample.mli:270-319) ---- */
int smx_resample_stream_prepare(const smx_resample_config *c, int64_t channels, int64_t max_block, smx_resample_stream **out) {
  return guarded([&] {
    if (!out) throw Failure("resample_kernel_prepare: null output handle");
    if (!c) throw Failure("resample_kernel_prepare: null config");
    if (channels < 1 || max_block < 1)
      throw InvalidArgument(format("resample_kernel_prepare: cannot prepare a kernel for %lld channels and chunks of %lld samples "
                                   "(both must be at least 1)", (long long)channels, (long long)max_block));
    if (c->executor != SMX_RESAMPLE_DIRECT)
      throw Failure("resample_kernel_prepare: only a config of the direct executor streams through this kernel");
    require_device();
    auto k = std::make_unique<smx_resample_stream>();
    k->config = c;
    k->channels = channels;
    k->max_block = max_block;
    k->hist = 2 * c->k;
    SMX_HIP_CHECK(hipGetDevice(&k->device));
    const size_t bytes = (size_t)channels * (size_t)k->hist * sizeof(float);
    SMX_HIP_CHECK(hipMalloc((void **)&k->history, bytes));
    SMX_HIP_CHECK(hipMemset(k->history, 0, bytes));
    *out = k.release();
  });
}
void smx_resample_stream_destroy(smx_resample_stream *k) { delete k; }
int smx_resample_stream_reset(smx_resample_stream *k) {
  return guarded([&] {
    stream_check(k);
    SMX_HIP_CHECK(hipDeviceSynchronize());   // steps on other streams may still read the history
    SMX_HIP_CHECK(hipMemset(k->history, 0, (size_t)k->channels * (size_t)k->hist * sizeof(float)));
    k->fed = k->emitted = 0;
    k->drained = false;
  });
}
int64_t smx_resample_stream_out_bound(const smx_resample_stream *k, int64_t n) {
  return k && k->config && n >= 0 ? ceil_div(n * k->config->l, k->config->m) + 1 : -1;
}
int64_t smx_resample_stream_pending(const smx_resample_stream *k) { return k && k->config ? stream_pending(*k) : -1; }

int smx_resample_stream_step_f32_dev(smx_resample_stream *k, const float *d_x, int64_t n, int64_t x_stride, float *d_y,
                                     int64_t y_stride, int64_t *n_out, void *stream) {
  return guarded([&] {
    stream_check(k);
    const int64_t got = stream_step_dev(*k, d_x, n, x_stride, d_y, y_stride, (hipStream_t)stream);
    if (n_out) *n_out = got;
  });
}
int smx_resample_stream_flush_f32_dev(smx_resample_stream *k, float *d_y, int64_t y_stride, int64_t *n_out, void *stream) {
  return guarded([&] {
    stream_check(k);
    const int64_t got = stream_flush_dev(*k, d_y, y_stride, (hipStream_t)stream);
    if (n_out) *n_out = got;
  });
}
// the host forms of step and flush are not batch calls (strided rows, a length known only after the run): no host_call
int smx_resample_stream_step_f32(smx_resample_stream *k, const float *x, int64_t n, int64_t x_stride, float *y, int64_t y_stride,
                                 int64_t *n_out) {
  return guarded([&] {
    stream_check(k);
    if (n_out) *n_out = 0;
    if (n > 0 && (!x || x_stride < n)) throw Failure("resample_kernel_step: null chunk or stride smaller than the chunk");
    if (n <= 0 || n > k->max_block || k->drained) {   // the checks and their messages live in one place
      (void)stream_step_dev(*k, nullptr, n, x_stride, nullptr, 0, nullptr);
      return;
    }
    const int64_t bound = smx_resample_stream_out_bound(k, n);
    DeviceScratch dx, dy;
    dx.alloc((size_t)k->channels * (size_t)n * sizeof(float));
    dy.alloc((size_t)k->channels * (size_t)bound * sizeof(float));
    SMX_HIP_CHECK(hipMemcpy2D(dx.ptr, (size_t)n * sizeof(float), x, (size_t)x_stride * sizeof(float), (size_t)n * sizeof(float),
                              (size_t)k->channels, hipMemcpyHostToDevice));
    const int64_t got = stream_step_dev(*k, dx.as<float>(), n, n, dy.as<float>(), bound, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (got > 0) {
      if (!y || y_stride < got) throw Failure("resample_kernel_step: null output or stride smaller than the emitted run");
      SMX_HIP_CHECK(hipMemcpy2D(y, (size_t)y_stride * sizeof(float), dy.ptr, (size_t)bound * sizeof(float), (size_t)got * sizeof(float),
                                (size_t)k->channels, hipMemcpyDeviceToHost));
    }
    if (n_out) *n_out = got;
  });
}
int smx_resample_stream_flush_f32(smx_resample_stream *k, float *y, int64_t y_stride, int64_t *n_out) {
  return guarded([&] {
    stream_check(k);
    if (n_out) *n_out = 0;
    const int64_t pending = stream_pending(*k);
    if (pending <= 0) {
      (void)stream_flush_dev(*k, nullptr, 0, nullptr);
      return;
    }
    if (!y || y_stride < pending) throw Failure("resample_kernel_flush: null output or stride smaller than the tail");
    DeviceScratch dy;
    dy.alloc((size_t)k->channels * (size_t)pending * sizeof(float));
    const int64_t got = stream_flush_dev(*k, dy.as<float>(), pending, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    SMX_HIP_CHECK(hipMemcpy2D(y, (size_t)y_stride * sizeof(float), dy.ptr, (size_t)pending * sizeof(float), (size_t)got * sizeof(float),
                              (size_t)k->channels, hipMemcpyDeviceToHost));
    if (n_out) *n_out = got;
  });
}

}  // extern "C"
