// Rhythm: the autocorrelation tempogram (Grosche, Mueller & Kurth 2010), the tempo under a log-normal prior and the
// dynamic-programming beat tracker (Ellis 2007) over device-resident onset envelopes env [lead; frames] (time fastest).
// include/soundml_amd.h words the definitions and DESIGN.md 4.8g the orders; everything is float64 inside.
//
// Tempogram, per frame t: y_j = w_j pad[t + j] (one rounding), a(tau) = sum_{j < W - tau} y_j y_{j + tau} as ONE ascending chain over j
// from 0.0, the product and the sum rounding one after the other (the file is built with -ffp-contract=off and no kernel here says
// fma: y is a rounded product, so its products are not exact and numpy could not restate a fused chain).
//
//   tempogram_tile_kernel     W <= 512: a workgroup takes 32 consecutive frames of a clip and builds their y as float64 in LDS; a
//                             lane owns one frame and a PAIR of blocks of 8 consecutive lags, block g with block G - 1 - g, so that
//                             every lane walks W + 8 steps of the triangle; the lags slide over y from registers (16 values of y per
//                             64 multiply-adds); the 32 lanes of a half-wave hold 32 consecutive frames of one lag: the store into
//                             [lag][frame] is a whole 128-byte line
//   tempogram_general_kernel  a workgroup per frame, a thread per lag, straight from memory, the same chains: every other W, and
//                             SMX_DISABLE_FAST=1 (tests: the same bits)
//   tempo_kernel              a workgroup per clip over the float64 normalised tempogram in scratch [clip][frame][lag]: a thread per
//                             lag adds the frames in ascending order, divides once, scores, and the workgroup picks the first argmax
//   beat_kernel               one wave per clip: the deviation (two ascending chains), the local score (a lane per frame), the
//                             recursion (the lanes hold the candidates, the argmax is a wave reduction that prefers the lowest
//                             index, cum lives in LDS), the median of the local maxima by counting, the walk back and the trimming
// The kernels of the beat tracker add, subtract, multiply, divide, compare and take two square roots (IEEE operations); exp and log
// live in the host tables below (libm, float64), log1p in tempo_kernel is the one device transcendental.
#include <cfloat>
#include <cstring>
#include <deque>

#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kLags = 8;                          // consecutive lags of a block
#ifndef SMX_RHYTHM_TILE_FRAMES
#define SMX_RHYTHM_TILE_FRAMES 32
#endif
constexpr int kTileFrames = SMX_RHYTHM_TILE_FRAMES;   // frames of a tile: the lanes of a half-wave
constexpr int kFastWin = 512;                     // the tile kernel's longest window: 32 pairs of blocks x 32 frames = 1024 lanes
constexpr int64_t kMaxWin = 16384;                // the longest window at all
constexpr int64_t kMaxPeriod = 4096;              // the longest beat period, in frames
constexpr int64_t kMaxBeatFrames = 8192;          // the longest clip the tracker takes: ls and cum of a clip live in LDS
constexpr int64_t kScratchBytes = 512ll << 20;    // the float64 tempogram of one launch of tempo; larger calls go clip range by clip range

struct TempogramArgs {
  const void *env;                // [lead; frames], rows stride apart
  const double *w;                // the window, W values
  void *out;                      // [lead; W; frames] in the dtype of env, or null
  double *wide;                   // [lead; frames; W] float64, normalised, before the rounding (tempo), or null
  int64_t lead, frames, stride, tiles;
  int W, b, norm, groups, pairs, ystride;
};

template <typename T>
__device__ __forceinline__ double padded(const T *row, int64_t s, int64_t n) { return (s >= 0 && s < n) ? (double)row[s] : 0.0; }

// 8 steps of the chains from step j on, every lag live: the window of 16 values of y is a ring of registers, its low half at B;
// the high half is fetched here, so that no value ever moves from one register to another
template <int B>
__device__ __forceinline__ void eight_steps(const double *y, int at, int j, double (&w)[2 * kLags], double (&acc)[kLags]) {
  double x[kLags];
#pragma unroll
  for (int i = 0; i < kLags; i += 2) {
    const double2 v = *reinterpret_cast<const double2 *>(y + at + kLags + i), u = *reinterpret_cast<const double2 *>(y + j + i);
    w[(B + kLags + i) % (2 * kLags)] = v.x, w[(B + kLags + i + 1) % (2 * kLags)] = v.y;
    x[i] = u.x, x[i + 1] = u.y;
  }
#pragma unroll
  for (int jj = 0; jj < kLags; ++jj)
#pragma unroll
    for (int k = 0; k < kLags; ++k) acc[k] = acc[k] + x[jj] * w[(B + jj + k) % (2 * kLags)];
}

// the chains of kLags consecutive lags from tau0 over y[0, W): lag tau0 + k takes the steps j < W - tau0 - k, in ascending order
__device__ __forceinline__ void slide(const double *y, int tau0, int W, double (&acc)[kLags]) {
  const int n = W - tau0;                         // steps of the block's first lag
#pragma unroll
  for (int k = 0; k < kLags; ++k) acc[k] = 0.0;
  int j = 0;
  if (n >= 2 * kLags - 1) {
    // y, tau0 and j are multiples of 8 doubles from a 16-byte aligned origin; steps j .. j + 7 have all 8 lags while j + 7 < n - 7
    double w[2 * kLags];
#pragma unroll
    for (int i = 0; i < kLags; i += 2) {
      const double2 v = *reinterpret_cast<const double2 *>(y + tau0 + i);
      w[i] = v.x, w[i + 1] = v.y;
    }
    while (j + 2 * kLags - 1 <= n) {
      eight_steps<0>(y, j + tau0, j, w, acc);
      j += kLags;
      if (j + 2 * kLags - 1 > n) break;
      eight_steps<kLags>(y, j + tau0, j, w, acc);
      j += kLags;
    }
  }
  for (; j < n; ++j) {
    const double xj = y[j];
#pragma unroll
    for (int k = 0; k < kLags; ++k)
      if (j + k < n) acc[k] = acc[k] + xj * y[j + tau0 + k];
  }
}

template <typename T>
__device__ __forceinline__ void put(const TempogramArgs &a, int64_t clip, int64_t t, int tau, double v, double a0) {
  if (a.norm && !(a0 < DBL_MIN)) v = v / a0;        // a NaN a(0) divides too: the whole frame is NaN then
  if (a.out) reinterpret_cast<T *>(a.out)[(clip * a.W + tau) * a.frames + t] = (T)v;
  if (a.wide) a.wide[(clip * a.frames + t) * a.W + tau] = v;
}

template <typename T>
__global__ void __launch_bounds__(1024) tempogram_tile_kernel(TempogramArgs a) {
  extern __shared__ __align__(16) unsigned char tile_lds[];
  double *y = reinterpret_cast<double *>(tile_lds);                        // [kTileFrames][ystride], rows 16-byte aligned
  double *a0 = y + (size_t)kTileFrames * a.ystride;                        // [kTileFrames]
  const int64_t clip = blockIdx.x / a.tiles, t0 = (blockIdx.x % a.tiles) * kTileFrames;
  const int nf = (int)(a.frames - t0 < kTileFrames ? a.frames - t0 : kTileFrames);
  const int W = a.W;
  const T *row = reinterpret_cast<const T *>(a.env) + clip * a.stride;
  for (int i = threadIdx.x; i < nf * a.ystride; i += blockDim.x) {
    const int f = i / a.ystride, j = i - f * a.ystride;
    y[i] = j < W ? a.w[j] * padded<T>(row, t0 + f + j - a.b, a.frames) : 0.0;   // the slack behind a row is read, never used
  }
  __syncthreads();

  const int f = threadIdx.x % kTileFrames, pair = threadIdx.x / kTileFrames;
  const bool live = f < nf && pair < a.pairs;
  const int g1 = pair, g2 = a.groups - 1 - pair;                          // g2 == g1: the middle block of an odd count, once
  const double *mine = y + (size_t)f * a.ystride;
  double first[kLags], second[kLags];
  if (live) {
    slide(mine, g1 * kLags, W, first);
    if (g2 > g1) slide(mine, g2 * kLags, W, second);
    if (g1 == 0) a0[f] = first[0];
  }
  __syncthreads();
  if (!live) return;
  const double d = a0[f];
#pragma unroll
  for (int k = 0; k < kLags; ++k)
    if (g1 * kLags + k < W) put<T>(a, clip, t0 + f, g1 * kLags + k, first[k], d);
  if (g2 > g1) {
#pragma unroll
    for (int k = 0; k < kLags; ++k)
      if (g2 * kLags + k < W) put<T>(a, clip, t0 + f, g2 * kLags + k, second[k], d);
  }
}

// a workgroup per frame, a thread per lag, any window
template <typename T>
__global__ void __launch_bounds__(256) tempogram_general_kernel(TempogramArgs a) {
  __shared__ double a0;
  const int64_t clip = blockIdx.x / a.frames, t = blockIdx.x % a.frames;
  const T *row = reinterpret_cast<const T *>(a.env) + clip * a.stride;
  const int64_t s0 = t - a.b;
  auto chain = [&](int tau) {
    double acc = 0.0;
    for (int j = 0; j < a.W - tau; ++j) {
      const double yj = a.w[j] * padded<T>(row, s0 + j, a.frames), yt = a.w[j + tau] * padded<T>(row, s0 + j + tau, a.frames);
      acc = acc + yj * yt;
    }
    return acc;
  };
  if (threadIdx.x == 0) a0 = chain(0);
  __syncthreads();
  const double d = a0;
  for (int tau = threadIdx.x; tau < a.W; tau += 256) put<T>(a, clip, t, tau, tau ? chain(tau) : d, d);
}

// ---- tempo -----------------------------------------------------------------------------------------------------------------------
struct TempoArgs {
  const double *wide;             // [lead; frames; W]
  const double *prior, *freq;     // [W] each
  int *lag;                       // [lead], or null
  void *out;                      // [lead] in the dtype of the call: bpm(lag), or the lag itself
  int64_t frames;
  int W, want_lag;
};

template <typename T>
__global__ void __launch_bounds__(256) tempo_kernel(TempoArgs a) {
  __shared__ double best_score[256];
  __shared__ int best_lag[256];
  __shared__ double m1;
  const int64_t clip = blockIdx.x;
  const double *base = a.wide + clip * a.frames * a.W;
  double score = 0.0;
  int lag = 0;                                    // 0: none yet
  for (int tau = threadIdx.x; tau < a.W; tau += 256) {
    double m = 0.0;
    for (int64_t t = 0; t < a.frames; ++t) m = m + base[t * a.W + tau];
    m = m / (double)a.frames;
    if (tau == 1) m1 = m;
    const double p = a.prior[tau];
    if (!(p > -HUGE_VAL)) continue;               // lag 0 and the tempi above max_tempo
    const double s = log1p(1e6 * m) + p;
    if (s == s && (lag == 0 || s > score)) score = s, lag = tau;   // a score that is NaN is never chosen
  }
  best_score[threadIdx.x] = score;
  best_lag[threadIdx.x] = lag;
  __syncthreads();
  if (threadIdx.x) return;
  for (int i = 1; i < 256; ++i) {
    const int l = best_lag[i];
    if (l && (lag == 0 || best_score[i] > score || (best_score[i] == score && l < lag))) score = best_score[i], lag = l;
  }
  if (a.W < 2 || m1 != m1) lag = 0;
  if (a.lag) a.lag[clip] = lag;
  const double v = lag == 0 ? __builtin_nan("") : a.want_lag ? (double)lag : a.freq[lag];
  reinterpret_cast<T *>(a.out)[clip] = (T)v;
}

// ---- the beat tracker ------------------------------------------------------------------------------------------------------------
struct BeatArgs {
  const void *env;                // [lead; frames], rows stride apart
  const int *lag;                 // [lead] the period of each clip, or null: `period` for all
  const double *freq;             // bpm of a lag (lag given)
  const int64_t *offsets;         // per period from pmin: where its g and its tx start in `tables`
  const double *tables;
  void *tempo, *beats;            // [lead], [lead; frames] in the dtype of env
  int *back, *list;               // scratch [lead; frames] each
  double *maxima;                 // scratch [lead; frames / 2 + 1]
  int64_t frames, stride;
  double bpm;
  int period, pmin, trim;
};

__device__ __forceinline__ int half_even(int p) {                 // round_half_even(p / 2)
  const int k = p >> 1;
  return (p & 1) ? k + (k & 1) : k;
}

template <typename T>
__global__ void __launch_bounds__(64) beat_kernel(BeatArgs a) {
  extern __shared__ __align__(16) unsigned char beat_lds[];
  __shared__ double s_value[2];
  __shared__ int s_count;
  const int lane = threadIdx.x, frames = (int)a.frames;
  const int64_t clip = blockIdx.x;
  double *ls = reinterpret_cast<double *>(beat_lds), *cum = ls + frames;   // cum holds env / sd until the recursion starts
  const T *row = reinterpret_cast<const T *>(a.env) + clip * a.stride;
  T *mask = reinterpret_cast<T *>(a.beats) + clip * a.frames;
  int *back = a.back + clip * a.frames, *list = a.list + clip * a.frames;
  double *maxima = a.maxima + clip * (a.frames / 2 + 1);
  const int p = a.lag ? a.lag[clip] : a.period;
  if (lane == 0) reinterpret_cast<T *>(a.tempo)[clip] = a.lag ? (T)(p ? a.freq[p] : __builtin_nan("")) : (T)a.bpm;
  for (int i = lane; i < frames; i += 64) mask[i] = (T)0;
  if (frames < 2 || p < 1) return;

  if (lane == 0) {
    double s = 0.0;
    for (int i = 0; i < frames; ++i) s = s + (double)row[i];
    const double mean = s / (double)frames;
    double q = 0.0;
    for (int i = 0; i < frames; ++i) {
      const double d = (double)row[i] - mean;
      q = q + d * d;
    }
    s_value[0] = sqrt(q / (double)(frames - 1));
  }
  __syncthreads();
  const double sd = s_value[0];
  if (!(sd > 0.0 && sd < HUGE_VAL)) return;       // zero, NaN or infinite: no beats
  for (int i = lane; i < frames; i += 64) cum[i] = (double)row[i] / sd;
  __syncthreads();

  const int64_t *off = a.offsets + 2 * (int64_t)(p - a.pmin);
  const double *g = a.tables + off[0], *tx = a.tables + off[1];
  bool finite = true;
  double top = -HUGE_VAL;
  for (int i = lane; i < frames; i += 64) {
    const int lo = i - p < 0 ? 0 : i - p, hi = i + p > frames - 1 ? frames - 1 : i + p;
    double acc = 0.0;
    for (int n = lo; n <= hi; ++n) acc = acc + cum[n] * g[i - n + p];
    ls[i] = acc;
    finite = finite && acc - acc == 0.0;
    top = acc > top ? acc : top;
  }
  for (int o = 32; o; o >>= 1) {
    const double other = __shfl_xor(top, o);
    top = other > top ? other : top;
    finite = __shfl_xor((int)finite, o) && finite;
  }
  __syncthreads();                                // every lane has read env / sd: cum is the recursion's from here
  if (!finite) return;

  const double enough = 0.01 * top;
  const int ncand = 2 * p - half_even(p) + 1;     // window_k = -2 p + k
  bool started = false;
  for (int i = 0; i < frames; ++i) {
    double bv = 0.0;
    int bk = -1;
    for (int k = lane; k < ncand; k += 64) {
      const int j = i - 2 * p + k;
      const double c = j >= 0 ? tx[k] + cum[j] : tx[k];
      if (bk < 0 || c > bv) bv = c, bk = k;
    }
    for (int o = 32; o; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int ok = __shfl_xor(bk, o);
      if (ok >= 0 && (bk < 0 || ov > bv || (ov == bv && ok < bk))) bv = ov, bk = ok;
    }
    const double here = ls[i];
    if (!started && here >= enough) started = true;
    if (lane == 0) {
      cum[i] = here + bv;
      back[i] = started ? i - 2 * p + bk : -1;
    }
    __syncthreads();
  }

  auto is_max = [&](int i) { return i >= 1 && cum[i] > cum[i - 1] && (i == frames - 1 || cum[i] >= cum[i + 1]); };
  if (lane == 0) {
    int n = 0;
    for (int i = 1; i < frames; ++i)
      if (is_max(i)) maxima[n++] = cum[i];
    s_count = n;
  }
  __syncthreads();
  const int n = s_count;
  if (n == 0) return;
  const int klo = (n - 1) / 2, khi = n / 2;
  for (int c = lane; c < n; c += 64) {
    const double v = maxima[c];
    int less = 0, equal = 0;
    for (int j = 0; j < n; ++j) {
      const double u = maxima[j];
      less += u < v;
      equal += u == v;
    }
    if (less <= klo && klo < less + equal) s_value[0] = v;
    if (less <= khi && khi < less + equal) s_value[1] = v;
  }
  __syncthreads();
  if (lane) return;
  const double med = klo == khi ? s_value[0] : (s_value[0] + s_value[1]) / 2.0;
  int last = -1;
  for (int i = frames - 1; i >= 1; --i)
    if (is_max(i) && 2.0 * cum[i] > med) {
      last = i;
      break;
    }
  if (last < 0) return;
  int nb = 0;
  for (int i = last; i >= 0; i = back[i]) list[nb++] = i;          // back[i] < i: the walk ends
  // beat q in ascending order is list[nb - 1 - q]
  auto smooth = [&](int q) {
    const double v = ls[list[nb - 1 - q]];
    double s = q > 0 ? 0.5 * ls[list[nb - q]] + v : v;
    if (q < nb - 1) s = s + 0.5 * ls[list[nb - 2 - q]];
    return s;
  };
  double th = 0.0;
  if (a.trim) {
    double ss = 0.0;
    for (int q = 0; q < nb; ++q) {
      const double s = smooth(q);
      ss = ss + s * s;
    }
    th = 0.5 * sqrt(ss / (double)nb);
  }
  int q0 = 0, q1 = nb - 1;
  while (q0 < nb && !(smooth(q0) > th)) ++q0;
  while (q1 >= q0 && !(smooth(q1) > th)) --q1;
  for (int q = q0; q <= q1; ++q) mask[list[nb - 1 - q]] = (T)1;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
// tables on the device, built once per key and device and kept: the holder keeps its table alive through the enqueue; the
// eviction's hipFree waits for the device, i.e. for every launch that reads it (declared in smx_internal.hpp: pitch.hip keeps
// pYIN's tables the same way)
}  // namespace

std::shared_ptr<void> cached_table(const std::string &key, const std::function<std::vector<unsigned char>()> &make) {
  static std::mutex mutex;
  static std::map<std::string, std::shared_ptr<void>> tables;
  static std::deque<std::string> order;
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  const std::string full = format("%d|", device) + key;
  std::lock_guard<std::mutex> lock(mutex);
  auto it = tables.find(full);
  if (it != tables.end()) return it->second;
  const std::vector<unsigned char> bytes = make();
  void *p = nullptr;
  SMX_HIP_CHECK(hipMalloc(&p, bytes.size() ? bytes.size() : 16));
  std::shared_ptr<void> owner(p, [](void *q) { (void)hipFree(q); });
  if (!bytes.empty()) SMX_HIP_CHECK(hipMemcpy(p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  if (order.size() >= 16) {
    tables.erase(order.front());
    order.pop_front();
  }
  order.push_back(full);
  tables[full] = owner;
  return owner;
}

namespace {

template <typename V>
std::vector<unsigned char> as_bytes(const std::vector<V> &v) {
  std::vector<unsigned char> out(v.size() * sizeof(V));
  if (!v.empty()) std::memcpy(out.data(), v.data(), out.size());
  return out;
}

int64_t half_even_host(int64_t p) {
  const int64_t k = p / 2;
  return (p & 1) ? k + (k & 1) : k;
}
int64_t candidates(int64_t p) { return 2 * p - half_even_host(p) + 1; }

void beat_tables(int64_t p, double tightness, double *g, double *tx) {
  for (int64_t k = -p; k <= p; ++k) {
    const double u = (double)k * 32.0 / (double)p;
    g[k + p] = std::exp(-0.5 * (u * u));
  }
  for (int64_t k = 0; k < candidates(p); ++k) {
    const double l = std::log(-(double)(-2 * p + k) / (double)p);
    tx[k] = -tightness * (l * l);
  }
}

double tempo_frequency(int64_t tau, int64_t sample_rate, int64_t hop) { return 60.0 * (double)sample_rate / ((double)hop * (double)tau); }

struct TempoPlan {
  int64_t sample_rate, hop, W;
  double start_bpm, std_bpm, max_tempo;
};

void tempo_prior(const TempoPlan &t, double *prior) {
  for (int64_t tau = 0; tau < t.W; ++tau) {
    const double bpm = tempo_frequency(tau, t.sample_rate, t.hop);
    const double z = (std::log2(bpm) - std::log2(t.start_bpm)) / t.std_bpm;
    prior[tau] = tau == 0 || bpm > t.max_tempo ? -HUGE_VAL : -0.5 * (z * z);
  }
}

void check_win(const char *fn, int64_t W) {
  if (W < 1 || W > kMaxWin)
    throw InvalidArgument(format("%s: cannot correlate windows of %lld frames (win_length must lie in [1, %lld])", fn, (long long)W, (long long)kMaxWin));
}

void check_grid(const char *fn, int64_t sample_rate, int64_t hop) {
  if (sample_rate < 1)
    throw InvalidArgument(format("%s: cannot analyse audio sampled at %lld Hz (sample_rate must be at least 1)", fn, (long long)sample_rate));
  if (hop < 1) throw InvalidArgument(format("%s: cannot advance frames by %lld samples (hop must be at least 1)", fn, (long long)hop));
}

void check_start(const char *fn, double start_bpm) {
  if (!(std::isfinite(start_bpm) && start_bpm > 0.0))
    throw InvalidArgument(format("%s: cannot centre the prior at %g beats per minute (start_bpm must be finite and positive)", fn, start_bpm));
}

// sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo, then whether any lag is left
void check_tempo(const char *fn, const TempoPlan &t) {
  check_grid(fn, t.sample_rate, t.hop);
  check_win(fn, t.W);
  check_start(fn, t.start_bpm);
  if (!(std::isfinite(t.std_bpm) && t.std_bpm > 0.0))
    throw InvalidArgument(format("%s: cannot use a prior %g octaves wide (std_bpm must be finite and positive)", fn, t.std_bpm));
  if (!(t.max_tempo > 0.0))
    throw InvalidArgument(format("%s: cannot cap the tempo at %g beats per minute (max_tempo must be positive)", fn, t.max_tempo));
  for (int64_t tau = 1; tau < t.W; ++tau)
    if (tempo_frequency(tau, t.sample_rate, t.hop) <= t.max_tempo) return;
  throw InvalidArgument(format("%s: no lag of a %lld-frame window is at or below %g beats per minute (win_length too short for max_tempo)", fn,
                               (long long)t.W, t.max_tempo));
}

struct BeatPlan {
  TempoPlan tempo;
  bool has_bpm;
  double bpm, tightness;
  int64_t period;                 // has_bpm
  bool trim;
};

int64_t beat_period(const char *fn, int64_t sample_rate, int64_t hop, double bpm) {
  if (!(std::isfinite(bpm) && bpm > 0.0))
    throw InvalidArgument(format("%s: cannot track beats at %g beats per minute (bpm must be finite and positive)", fn, bpm));
  const double frames = std::nearbyint(60.0 * (double)sample_rate / (double)hop / bpm);   // round half to even (the default mode)
  if (!(frames >= 1.0 && frames <= (double)kMaxPeriod))
    throw InvalidArgument(format("%s: a beat at %g beats per minute lasts %g frames (the period must lie in [1, %lld])", fn, bpm, frames,
                                 (long long)kMaxPeriod));
  return (int64_t)frames;
}

// sample_rate, hop, then bpm and its period, or win_length and start_bpm and the admissible lags; tightness last
void check_beat(const char *fn, BeatPlan &b) {
  check_grid(fn, b.tempo.sample_rate, b.tempo.hop);
  if (b.has_bpm) b.period = beat_period(fn, b.tempo.sample_rate, b.tempo.hop, b.bpm);
  else check_tempo(fn, b.tempo);
  if (!(std::isfinite(b.tightness) && b.tightness > 0.0))
    throw InvalidArgument(format("%s: cannot weigh the tempo by %g (tightness must be finite and positive)", fn, b.tightness));
}

void check_beat_frames(const char *fn, int64_t frames) {
  if (frames > kMaxBeatFrames)
    throw InvalidArgument(format("%s: cannot track a clip of %lld frames (at most %lld)", fn, (long long)frames, (long long)kMaxBeatFrames));
}

void fill(void *out, int elem_bytes, int64_t count, double v) {
  for (int64_t c = 0; c < count; ++c)
    if (elem_bytes == 8) reinterpret_cast<double *>(out)[c] = v;
    else reinterpret_cast<float *>(out)[c] = (float)v;
}

void check_extents(const char *fn, int64_t lead, int64_t frames, int64_t stride, bool device) {
  check_rank_extents(fn, lead, frames);
  if (device && stride < frames) throw Failure(format("%s: env_stride is smaller than the frame count", fn));
}

std::shared_ptr<void> window_table(int kind, double param, int64_t W) {
  return cached_table(format("window|%d|%a|%lld", kind, param, (long long)W), [&] {
    std::vector<double> w((size_t)W);
    window_make_param(kind, param, true, W, w.data());
    return as_bytes(w);
  });
}

// the window's values are the caller's to have checked (window_make_param words what is wrong with them)
template <typename T>
void tempogram_dev(const char *fn, const void *d_env, int64_t lead, int64_t frames, int64_t stride, int64_t W, const double *d_w, bool norm, void *d_out,
                   double *d_wide, hipStream_t stream) {
  if (lead == 0 || frames == 0) return;
  TempogramArgs a{};
  a.env = d_env, a.w = d_w, a.out = d_out, a.wide = d_wide;
  a.lead = lead, a.frames = frames, a.stride = stride;
  a.W = (int)W, a.b = (int)(W / 2), a.norm = norm ? 1 : 0;
  const bool tile = !fast_path_disabled() && W <= kFastWin;
  size_t lds = 0;
  int threads = 256;
  if (tile) {
    a.groups = (int)((W + kLags - 1) / kLags);
    a.pairs = (a.groups + 1) / 2;
    a.ystride = a.groups * kLags + kLags + 2;                              // rows 16-byte aligned, an odd number of 16-byte groups apart
    a.tiles = (frames + kTileFrames - 1) / kTileFrames;
    lds = ((size_t)kTileFrames * a.ystride + kTileFrames) * sizeof(double);
    threads = ((a.pairs * kTileFrames + 63) / 64) * 64;
  }
  // clip range by clip range (DESIGN.md "Launch extents"): a tile kernel's workgroup per tile, the general one's per frame
  const int64_t per_clip = tile ? a.tiles : frames, per_launch = std::max<int64_t>(1, clips_per_launch(per_clip, threads));
  for (int64_t c0 = 0; c0 < lead; c0 += per_launch) {
    a.lead = std::min(per_launch, lead - c0);
    a.env = reinterpret_cast<const T *>(d_env) + c0 * stride;
    a.out = d_out ? reinterpret_cast<T *>(d_out) + c0 * W * frames : nullptr;
    a.wide = d_wide ? d_wide + c0 * frames * W : nullptr;
    if (tile) {
      launch_tiles(fn, tempogram_tile_kernel<T>, a.lead * a.tiles, threads, lds, stream, a);
    } else {
      SMX_LAUNCH((tempogram_general_kernel<T>), dim3(grid_x(fn, "frames", a.lead * frames, 256)), dim3(256), 0, stream, a);
      SMX_HIP_CHECK(hipGetLastError());
    }
  }
}

void tempogram_any(const char *fn, int elem_bytes, const void *d_env, int64_t lead, int64_t frames, int64_t stride, int64_t W, const double *d_w, bool norm,
                   void *d_out, double *d_wide, hipStream_t stream) {
  if (elem_bytes == 8) tempogram_dev<double>(fn, d_env, lead, frames, stride, W, d_w, norm, d_out, d_wide, stream);
  else tempogram_dev<float>(fn, d_env, lead, frames, stride, W, d_w, norm, d_out, d_wide, stream);
}

std::shared_ptr<void> prior_table(const TempoPlan &t) {
  return cached_table(format("prior|%lld|%lld|%lld|%a|%a|%a", (long long)t.sample_rate, (long long)t.hop, (long long)t.W, t.start_bpm, t.std_bpm, t.max_tempo),
                      [&] {
                        std::vector<double> v((size_t)(2 * t.W));   // the prior, then the lags' tempi
                        tempo_prior(t, v.data());
                        for (int64_t tau = 0; tau < t.W; ++tau) v[(size_t)(t.W + tau)] = tempo_frequency(tau, t.sample_rate, t.hop);
                        return as_bytes(v);
                      });
}

// the lag of every clip into d_lag (or null) and bpm(lag) or the lag itself into d_out [lead]; the float64 tempogram passes
// through stream-ordered scratch, the float32 one is never written
void tempo_dev(const char *fn, const TempoPlan &t, int elem_bytes, const void *d_env, int64_t lead, int64_t frames, int64_t stride, bool want_lag,
               int *d_lag, void *d_out, hipStream_t stream) {
  if (lead == 0) return;
  if (!d_out || (!d_env && frames)) throw Failure(format("%s: null device pointer", fn));
  const auto window = window_table(SMX_WINDOW_HANN, 0.0, t.W), prior = prior_table(t);
  const int64_t per_clip = std::max<int64_t>(1, frames * t.W * 8);
  const int64_t step = std::max<int64_t>(1, std::min({lead, kScratchBytes / per_clip, clips_per_launch(1, 256)}));   // tempo_kernel: a workgroup per clip
  init_device_pool();
  DeviceScratch scratch;
  scratch.pool((size_t)(step * per_clip), stream);
  for (int64_t c0 = 0; c0 < lead; c0 += step) {
    const int64_t nc = std::min(step, lead - c0);
    tempogram_any(fn, elem_bytes, (const char *)d_env + c0 * stride * elem_bytes, nc, frames, stride, t.W, (const double *)window.get(), true, nullptr,
                  scratch.as<double>(), stream);
    TempoArgs a{};
    a.wide = scratch.as<double>();
    a.prior = (const double *)prior.get();
    a.freq = a.prior + t.W;
    a.lag = d_lag ? d_lag + c0 : nullptr;
    a.out = (char *)d_out + c0 * elem_bytes;
    a.frames = frames;
    a.W = (int)t.W;
    a.want_lag = want_lag ? 1 : 0;
    if (elem_bytes == 8) SMX_LAUNCH((tempo_kernel<double>), dim3(grid_x(fn, "clips", nc, 256)), dim3(256), 0, stream, a);
    else SMX_LAUNCH((tempo_kernel<float>), dim3(grid_x(fn, "clips", nc, 256)), dim3(256), 0, stream, a);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

// g and tx of the periods pmin .. pmax in one allocation: 2 offsets (in doubles) per period, then the values
std::shared_ptr<void> beat_table(int64_t pmin, int64_t pmax, double tightness) {
  return cached_table(format("beat|%lld|%lld|%a", (long long)pmin, (long long)pmax, tightness), [&] {
    const int64_t np = pmax - pmin + 1;
    std::vector<int64_t> off((size_t)(2 * np));
    int64_t at = 2 * np;                            // an int64 is as wide as a double
    for (int64_t p = pmin; p <= pmax; ++p) {
      off[(size_t)(2 * (p - pmin))] = at;
      at += 2 * p + 1;
      off[(size_t)(2 * (p - pmin) + 1)] = at;
      at += candidates(p);
    }
    std::vector<double> all((size_t)at);
    std::memcpy(all.data(), off.data(), off.size() * sizeof(int64_t));
    for (int64_t p = pmin; p <= pmax; ++p)
      beat_tables(p, tightness, all.data() + off[(size_t)(2 * (p - pmin))], all.data() + off[(size_t)(2 * (p - pmin) + 1)]);
    return as_bytes(all);
  });
}

void beat_dev(const char *fn, const BeatPlan &b, int elem_bytes, const void *d_env, int64_t lead, int64_t frames, int64_t stride, void *d_tempo,
              void *d_beats, hipStream_t stream) {
  check_beat_frames(fn, frames);
  if (lead == 0) return;
  if (!d_tempo || (frames && (!d_env || !d_beats))) throw Failure(format("%s: null device pointer", fn));
  grid_x(fn, "clips", lead, 64);                   // beat_kernel: a wave per clip; refused before any scratch is taken
  const int64_t pmin = b.has_bpm ? b.period : 1, pmax = b.has_bpm ? b.period : std::max<int64_t>(1, b.tempo.W - 1);
  const auto tables = beat_table(pmin, pmax, b.tightness);
  std::shared_ptr<void> prior;
  init_device_pool();
  DeviceScratch scratch;
  const size_t ints = (size_t)lead * (size_t)frames, maxima = (size_t)lead * (size_t)(frames / 2 + 1);
  scratch.pool(maxima * 8 + (2 * ints + (size_t)lead) * 4 + 16, stream);
  BeatArgs a{};
  a.maxima = scratch.as<double>();
  a.back = reinterpret_cast<int *>(a.maxima + maxima);
  a.list = a.back + ints;
  int *d_lag = a.list + ints;
  if (!b.has_bpm) {
    prior = prior_table(b.tempo);
    tempo_dev(fn, b.tempo, elem_bytes, d_env, lead, frames, stride, false, d_lag, d_tempo, stream);
    a.lag = d_lag;
    a.freq = (const double *)prior.get() + b.tempo.W;
  }
  a.env = d_env, a.tempo = d_tempo, a.beats = d_beats;
  a.offsets = (const int64_t *)tables.get();
  a.tables = (const double *)tables.get();
  a.frames = frames, a.stride = stride;
  a.bpm = b.bpm;
  a.period = (int)b.period, a.pmin = (int)pmin, a.trim = b.trim ? 1 : 0;
  const size_t lds = (size_t)std::max<int64_t>(1, frames) * 16;
  if (elem_bytes == 8) launch_tiles(fn, beat_kernel<double>, lead, 64, lds, stream, a);
  else launch_tiles(fn, beat_kernel<float>, lead, 64, lds, stream, a);
}

// ---- the three faces ---------------------------------------------------------------------------------------------------------------
void tempogram_call(bool device, const void *env, int elem_bytes, int64_t lead, int64_t frames, int64_t stride, int64_t W, int kind, double param, int norm,
                    void *out, hipStream_t stream) {
  const char *fn = "tempogram";
  check_win(fn, W);
  std::vector<double> probe((size_t)W);
  window_make_param(kind, param, true, W, probe.data());       // words what is wrong with the window
  check_extents(fn, lead, frames, stride, device);
  if (lead == 0 || frames == 0) return;
  if (!env || !out) throw Failure(format("%s: null pointer", fn));
  if (device) {
    const auto w = window_table(kind, param, W);
    tempogram_any(fn, elem_bytes, env, lead, frames, stride, W, (const double *)w.get(), norm != 0, out, nullptr, stream);
    return;
  }
  host_call(fn, {{env, (size_t)frames * (size_t)elem_bytes}}, out, (size_t)W * (size_t)frames * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t st) {
              const auto w = window_table(kind, param, W);
              tempogram_any(fn, elem_bytes, d_in[0], nc, frames, frames, W, (const double *)w.get(), norm != 0, d_out, nullptr, st);
            });
}

void tempo_call(bool device, const void *env, int elem_bytes, int64_t lead, int64_t frames, int64_t stride, const TempoPlan &t, int want_lag, void *out,
                hipStream_t stream) {
  const char *fn = "tempo";
  check_tempo(fn, t);
  check_extents(fn, lead, frames, stride, device);
  if (lead == 0) return;
  if (!out || (!env && frames)) throw Failure(format("%s: null pointer", fn));
  if (device) {
    tempo_dev(fn, t, elem_bytes, env, lead, frames, stride, want_lag != 0, nullptr, out, stream);
    return;
  }
  if (frames == 0) {                              // the mean over no frames
    fill(out, elem_bytes, lead, std::nan(""));
    return;
  }
  host_call(fn, {{env, (size_t)frames * (size_t)elem_bytes}}, out, (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t st) {
              tempo_dev(fn, t, elem_bytes, d_in[0], nc, frames, frames, want_lag != 0, nullptr, d_out, st);
            });
}

void beat_call(bool device, const void *env, int elem_bytes, int64_t lead, int64_t frames, int64_t stride, BeatPlan b, void *tempo, void *beats,
               hipStream_t stream) {
  const char *fn = "beat_track";
  check_beat(fn, b);
  check_extents(fn, lead, frames, stride, device);
  if (device) {
    beat_dev(fn, b, elem_bytes, env, lead, frames, stride, tempo, beats, stream);
    return;
  }
  check_beat_frames(fn, frames);
  if (lead == 0) return;
  if (!tempo || (frames && (!env || !beats))) throw Failure(format("%s: null pointer", fn));
  if (frames == 0) {
    fill(tempo, elem_bytes, lead, b.has_bpm ? b.bpm : std::nan(""));   // no frames: no mask, and the mean over no frames
    return;
  }
  host_call(fn, {{env, (size_t)frames * (size_t)elem_bytes}}, {HostOut{tempo, (size_t)elem_bytes}, HostOut{beats, (size_t)frames * (size_t)elem_bytes}}, lead,
            false, nullptr, [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t st) {
              beat_dev(fn, b, elem_bytes, d_in[0], nc, frames, frames, d_out[0], d_out[1], st);
            });
}

BeatPlan beat_plan(int64_t sample_rate, int64_t hop, int has_bpm, double bpm, int64_t W, double start_bpm, double tightness, int trim) {
  return BeatPlan{TempoPlan{sample_rate, hop, W, start_bpm, 1.0, 320.0}, has_bpm != 0, bpm, tightness, 0, trim != 0};
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Rhythm ----------------------------------------------------------------------------------------------------------------------
int smx_rhythm_tempogram_f32(const float *env, int64_t lead, int64_t frames, int64_t win_length, int window, double window_param, int norm, float *out) {
  return guarded([&] { tempogram_call(false, env, 4, lead, frames, frames, win_length, window, window_param, norm, out, nullptr); });
}
int smx_rhythm_tempogram_f64(const double *env, int64_t lead, int64_t frames, int64_t win_length, int window, double window_param, int norm, double *out) {
  return guarded([&] { tempogram_call(false, env, 8, lead, frames, frames, win_length, window, window_param, norm, out, nullptr); });
}
int smx_rhythm_tempogram_gpu_f32(const float *d_env, int64_t lead, int64_t frames, int64_t env_stride, int64_t win_length, int window, double window_param,
                                 int norm, float *d_out, void *stream) {
  return guarded([&] { tempogram_call(true, d_env, 4, lead, frames, env_stride, win_length, window, window_param, norm, d_out, (hipStream_t)stream); });
}
int smx_rhythm_tempo_f32(const float *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int64_t win_length, double start_bpm, double std_bpm,
                         double max_tempo, int want_lag, float *out) {
  return guarded([&] { tempo_call(false, env, 4, lead, frames, frames, {sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo}, want_lag, out, nullptr); });
}
int smx_rhythm_tempo_f64(const double *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int64_t win_length, double start_bpm,
                         double std_bpm, double max_tempo, int want_lag, double *out) {
  return guarded([&] { tempo_call(false, env, 8, lead, frames, frames, {sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo}, want_lag, out, nullptr); });
}
int smx_rhythm_tempo_gpu_f32(const float *d_env, int64_t lead, int64_t frames, int64_t env_stride, int64_t sample_rate, int64_t hop, int64_t win_length,
                             double start_bpm, double std_bpm, double max_tempo, int want_lag, float *d_out, void *stream) {
  return guarded([&] {
    tempo_call(true, d_env, 4, lead, frames, env_stride, {sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo}, want_lag, d_out, (hipStream_t)stream);
  });
}
int smx_rhythm_beat_track_f32(const float *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int has_bpm, double bpm, int64_t win_length,
                              double start_bpm, double tightness, int trim, float *tempo, float *beats) {
  return guarded([&] {
    beat_call(false, env, 4, lead, frames, frames, beat_plan(sample_rate, hop, has_bpm, bpm, win_length, start_bpm, tightness, trim), tempo, beats, nullptr);
  });
}
int smx_rhythm_beat_track_f64(const double *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int has_bpm, double bpm, int64_t win_length,
                              double start_bpm, double tightness, int trim, double *tempo, double *beats) {
  return guarded([&] {
    beat_call(false, env, 8, lead, frames, frames, beat_plan(sample_rate, hop, has_bpm, bpm, win_length, start_bpm, tightness, trim), tempo, beats, nullptr);
  });
}
int smx_rhythm_beat_track_gpu_f32(const float *d_env, int64_t lead, int64_t frames, int64_t env_stride, int64_t sample_rate, int64_t hop, int has_bpm,
                                  double bpm, int64_t win_length, double start_bpm, double tightness, int trim, float *d_tempo, float *d_beats, void *stream) {
  return guarded([&] {
    beat_call(true, d_env, 4, lead, frames, env_stride, beat_plan(sample_rate, hop, has_bpm, bpm, win_length, start_bpm, tightness, trim), d_tempo, d_beats,
              (hipStream_t)stream);
  });
}
int smx_rhythm_tempo_frequencies(int64_t win_length, int64_t sample_rate, int64_t hop, double *out) {
  return guarded([&] {
    check_grid("tempo_frequencies", sample_rate, hop);
    check_win("tempo_frequencies", win_length);
    if (!out) return;
    for (int64_t tau = 0; tau < win_length; ++tau) out[tau] = tempo_frequency(tau, sample_rate, hop);
  });
}
int smx_rhythm_tempo_prior(int64_t win_length, int64_t sample_rate, int64_t hop, double start_bpm, double std_bpm, double max_tempo, double *out) {
  return guarded([&] {
    const TempoPlan t{sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo};
    check_tempo("tempo_prior", t);
    if (out) tempo_prior(t, out);
  });
}
int smx_rhythm_beat_period(int64_t sample_rate, int64_t hop, double bpm, int64_t *period) {
  return guarded([&] {
    check_grid("beat_track", sample_rate, hop);
    const int64_t p = beat_period("beat_track", sample_rate, hop, bpm);
    if (period) *period = p;
  });
}
int smx_rhythm_beat_tables(int64_t period, double tightness, double *g, double *tx) {
  return guarded([&] {
    if (period < 1 || period > kMaxPeriod)
      throw InvalidArgument(format("beat_tables: cannot tabulate a period of %lld frames (the period must lie in [1, %lld])", (long long)period,
                                   (long long)kMaxPeriod));
    if (!(std::isfinite(tightness) && tightness > 0.0))
      throw InvalidArgument(format("beat_tables: cannot weigh the tempo by %g (tightness must be finite and positive)", tightness));
    if (g && tx) beat_tables(period, tightness, g, tx);
  });
}

}  // extern "C"
