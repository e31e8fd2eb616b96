// Octave-band spectral contrast (contrast.ml:60-206) and spectral-flux onset strength (onset.ml:73-199) over device-resident
// data [lead; bins; frames] (frames fastest).
//
// Both have a float64 interior and round once to the data's dtype; frames sit across lanes, so every load of a bin row is one
// coalesced run of 64 frames, and every frame's value is computed by one thread in a fixed order: a leading slice of a call
// that involves no whole-tensor maximum equals the batched call bit for bit.
//
//   contrast:  a wave owns 64 frames of one band.  The mean of the `take` smallest and of the `take` largest magnitudes of
//              the band is an EXACT selection, ties included, made on the values in their own dtype (the cast to float64 is
//              monotonic).  take <= 16: two sorted register lists of `take` entries, a row enters both as one median of three
//              per entry.  Larger takes (and SMX_DISABLE_FAST): the take-th value is found by bisection on the bits of an
//              order-preserving integer key, one counting walk of the band per bit; the mean is then the values beyond it
//              plus as many copies of it as are missing.  On the clamped logarithmic path the
//              means go to float64 scratch, a small launch finds their two whole-tensor maxima (ordered integer keys, one
//              ordinary vector atomic per workgroup) and another forms the decibel difference.
//   flux:      one thread per output frame walks the rows in order: max(0, s[m, u] - s[m, u - lag]) summed in float64.
//              From audio the rows are the mel spectrogram's, turned into decibels under the whole tensor's 80 dB clamp as
//              they are read (the maximum is a launch of its own: the logarithm is monotonic).
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kMaxBands = 64;     // every band holds a bin of its own: n_bands + 1 <= log2(fft_size) + 2
constexpr int kListCap = 16;      // the longest register list; a larger take goes the general way
constexpr int kDepth = 8;         // loads in flight per thread
constexpr double kAmin = 1e-10;   // Convert.power_to_db's floor (convert.ml:46); reference 1: the offset is zero
constexpr double kTopDb = 80.0;

struct Band {
  int lo, sub_len, take;          // contrast.ml:33-36
};

enum ContrastMode { CONTRAST_LINEAR = 0, CONTRAST_LOG = 1, CONTRAST_LOG_CLAMPED = 2 };

// an order-preserving integer key of a value's bits (mfcc.hip keeps its decibel maxima the same way)
template <typename T> struct OrderedKey;
template <> struct OrderedKey<float> {
  using U = unsigned;
  static __device__ __forceinline__ U of(float v) { const U b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
  static __device__ __forceinline__ float back(U k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct OrderedKey<double> {
  using U = unsigned long long;
  static __device__ __forceinline__ U of(double v) {
    const U b = (U)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double back(U k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
  }
};

__device__ __forceinline__ double decibels(double v) {     // convert.ml:30-50 at gain 10, reference 1
  const double decade = 10.0 / log(10.0);
  return log(v > kAmin ? v : kAmin) * decade;
}

// the largest key of a workgroup of 256 threads to one address: one atomic per workgroup (thousands of atomics on one address cost
// more than the pass over the data: the contrast kernel with one per wave took 0.39 ms where it takes 0.15 without)
__device__ __forceinline__ void block_max_key(unsigned long long key, unsigned long long *to) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(key, off);
    key = o > key ? o : key;
  }
  __shared__ unsigned long long part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) key = part[w] > key ? part[w] : key;
    atomicMax(to, key);
  }
}

// walks rows [0, len) of one frame column in order, kDepth loads in flight at a time
template <typename T, typename F>
__device__ __forceinline__ void for_rows(const T *col, int64_t frames, int len, F &&f) {
  int j = 0;
  for (; j + kDepth <= len; j += kDepth) {
    T v[kDepth];
#pragma unroll
    for (int i = 0; i < kDepth; ++i) v[i] = col[(int64_t)(j + i) * frames];
#pragma unroll
    for (int i = 0; i < kDepth; ++i) f(v[i]);
  }
  for (; j < len; ++j) f(col[(int64_t)j * frames]);
}

struct Means {
  double valley, peak;
  bool bad;                       // a negative or NaN magnitude was seen
};

// the middle one of three values of which lo <= hi is known: where a new value lands between two neighbours of a sorted list
__device__ __forceinline__ float between(float lo, float v, float hi) { return __builtin_amdgcn_fmed3f(lo, v, hi); }
__device__ __forceinline__ double between(double lo, double v, double hi) { return fmax(fmin(v, hi), lo); }

// take = TAKE <= kListCap: the TAKE smallest values ascending and the TAKE largest descending, kept sorted in registers.  A new
// value enters a list as one median of three per entry (entry i becomes the middle of its lower neighbour, the value and itself),
// so a row costs 2 TAKE instructions whether or not it changes anything.  (A wave-uniform test that skips a row no lane has to
// insert would skip next to nothing: lane by lane the chance is take / row, and a wave holds 64 frames.)
template <typename T, int TAKE>
__device__ __forceinline__ Means select_lists(const T *col, int64_t frames, int len) {
  T lo[TAKE], hi[TAKE];
#pragma unroll
  for (int i = 0; i < TAKE; ++i) lo[i] = (T)INFINITY, hi[i] = (T)-INFINITY;
  bool bad = false;
  for_rows(col, frames, len, [&](T v) {
    bad |= !(v >= (T)0);
#pragma unroll
    for (int i = TAKE - 1; i > 0; --i) lo[i] = between(lo[i - 1], v, lo[i]), hi[i] = between(hi[i], v, hi[i - 1]);
    lo[0] = v < lo[0] ? v : lo[0];
    hi[0] = v > hi[0] ? v : hi[0];
  });
  double valley = 0.0, peak = 0.0;
#pragma unroll
  for (int i = 0; i < TAKE; ++i) valley += (double)lo[i], peak += (double)hi[i];
  return {valley / (double)TAKE, peak / (double)TAKE, bad};
}

template <typename T, int TAKE = kListCap>
__device__ __forceinline__ Means select_by_take(const T *col, int64_t frames, int len, int take) {
  if constexpr (TAKE > 1) {
    if (take < TAKE) return select_by_take<T, TAKE - 1>(col, frames, len, take);
  }
  return select_lists<T, TAKE>(col, frames, len);
}

// any take <= len: the take-th smallest and the take-th largest key by bisection on the key's bits, both in one counting walk
// of the band per bit
template <typename T>
__device__ __noinline__ Means select_general(const T *col, int64_t frames, int len, int take) {
  using K = OrderedKey<T>;
  using U = typename K::U;
  // the k-th smallest key is the largest value with fewer than k keys under it: its bits are settled from the top
  const int k_low = take, k_high = len - take + 1;
  U low = 0, high = 0;
  for (int bit = 8 * (int)sizeof(U) - 1; bit >= 0; --bit) {
    const U try_low = low | ((U)1 << bit), try_high = high | ((U)1 << bit);
    int under_low = 0, under_high = 0;
    for_rows(col, frames, len, [&](T v) {
      const U key = K::of(v);
      under_low += key < try_low ? 1 : 0;
      under_high += key < try_high ? 1 : 0;
    });
    if (under_low < k_low) low = try_low;
    if (under_high < k_high) high = try_high;
  }
  double valley = 0.0, peak = 0.0;
  int under = 0, over = 0;
  bool bad = false;
  for_rows(col, frames, len, [&](T v) {
    bad |= !(v >= (T)0);
    const U key = K::of(v);
    if (key < low) valley += (double)v, ++under;
    if (key > high) peak += (double)v, ++over;
  });
  valley += (double)(take - under) * (double)K::back(low);
  peak += (double)(take - over) * (double)K::back(high);
  return {valley / (double)take, peak / (double)take, bad};
}

struct ContrastArgs {
  const void *s;                  // [lead; bins; frames]
  void *out;                      // [lead; rows; frames]
  double *valley, *peak;          // [lead; rows; frames] float64 scratch (CONTRAST_LOG_CLAMPED)
  unsigned long long *keys;       // the largest valley, the largest peak (ordered keys; a launch of their own finds them)
  int *invalid;                   // or null: magnitudes are not checked
  int64_t lead, bins, frames, ftiles;
  int rows, mode, general;
  Band band[kMaxBands];
};

template <typename T>
__global__ void __launch_bounds__(64) contrast_kernel(ContrastArgs a) {
  const int64_t clip = blockIdx.x / a.ftiles, tile = blockIdx.x % a.ftiles;
  const int k = a.rows - 1 - (int)blockIdx.y;               // the top band first: it is the longest walk
  const Band b = a.band[k];
  const int64_t t = tile * 64 + threadIdx.x;
  const bool live = t < a.frames;
  const int64_t tc = live ? t : a.frames - 1;               // idle lanes shadow the last frame (no stores)
  const T *col = reinterpret_cast<const T *>(a.s) + (clip * a.bins + b.lo) * a.frames + tc;
  Means m;
  if (a.general || b.take > kListCap) m = select_general<T>(col, a.frames, b.sub_len, b.take);
  else m = select_by_take<T>(col, a.frames, b.sub_len, b.take);
  if (a.invalid && m.bad && live) atomicOr(a.invalid, 1);
  const int64_t at = (clip * a.rows + k) * a.frames + t;
  if (a.mode == CONTRAST_LOG_CLAMPED) {
    if (live) a.valley[at] = m.valley, a.peak[at] = m.peak;
    return;
  }
  if (!live) return;
  const double r = a.mode == CONTRAST_LINEAR ? m.peak - m.valley : decibels(m.peak) - decibels(m.valley);
  reinterpret_cast<T *>(a.out)[at] = (T)r;
}

// contrast.ml:200-203: each side's decibels clamped under the maximum of its own whole tensor
template <typename T>
__global__ void __launch_bounds__(256) contrast_db_kernel(const double *valley, const double *peak, const unsigned long long *keys,
                                                          T *out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double valley_floor = decibels(OrderedKey<double>::back(keys[0])) - kTopDb;
  const double peak_floor = decibels(OrderedKey<double>::back(keys[1])) - kTopDb;
  double v = decibels(valley[i]), p = decibels(peak[i]);
  v = v > valley_floor ? v : valley_floor;
  p = p > peak_floor ? p : peak_floor;
  out[i] = (T)(p - v);
}

// the largest value of tensor blockIdx.y of `total` elements each, as an ordered key of its float64 form, to key[blockIdx.y]
template <typename T>
__global__ void __launch_bounds__(256) max_key_kernel(const T *s, int64_t total, unsigned long long *key) {
  s += (int64_t)blockIdx.y * total;
  unsigned long long best = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const unsigned long long k = OrderedKey<double>::of((double)s[i]);
    best = k > best ? k : best;
  }
  block_max_key(best, key + blockIdx.y);
}

template <typename T>
void launch_max_key(const T *s, int64_t total, int tensors, unsigned long long *key, hipStream_t stream) {
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 2047) / 2048, 1024);
  SMX_LAUNCH(max_key_kernel<T>, dim3(blocks, (unsigned)tensors), dim3(256), 0, stream, s, total, key);
  SMX_HIP_CHECK(hipGetLastError());
}

struct FluxArgs {
  const void *s;                  // [lead; bins; frames]: decibels, or (LOG) powers
  void *out;                      // [lead; frames]
  const unsigned long long *max_key;   // LOG: the largest power of the whole tensor
  int64_t lead, bins, frames, ftiles, lag, shift;
};

// onset.ml:73-122 on one chunk: out[t] = z[t - shift], z[u] = mean over rows of max(0, s[., u] - s[., u - lag]), 0 for u < lag
template <typename T, bool LOG>
__global__ void __launch_bounds__(256) flux_kernel(FluxArgs a) {
  const int64_t clip = blockIdx.x / a.ftiles, t = (blockIdx.x % a.ftiles) * 256 + threadIdx.x;
  if (t >= a.frames) return;
  const int64_t u = t - a.shift;
  double z = 0.0;
  if (u >= a.lag) {
    const T *cur = reinterpret_cast<const T *>(a.s) + clip * a.bins * a.frames + u;
    const T *old = cur - a.lag;
    double floor_db = 0.0;
    if constexpr (LOG) floor_db = decibels(OrderedKey<double>::back(*a.max_key)) - kTopDb;
    auto level = [&](T x) {
      if constexpr (!LOG) return (double)x;
      const double db = decibels((double)x);
      return db > floor_db ? db : floor_db;
    };
    double sum = 0.0;
    int64_t m = 0;
    for (; m + 4 <= a.bins; m += 4) {
      T c[4], o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = cur[(m + i) * a.frames], o[i] = old[(m + i) * a.frames];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double d = level(c[i]) - level(o[i]);
        sum += d > 0.0 ? d : 0.0;
      }
    }
    for (; m < a.bins; ++m) {
      const double d = level(cur[m * a.frames]) - level(old[m * a.frames]);
      sum += d > 0.0 ? d : 0.0;
    }
    z = sum / (double)a.bins;
  }
  reinterpret_cast<T *>(a.out)[clip * a.frames + t] = (T)z;
}

// ---- the band plan (contrast.ml:50-142), host integers and float64 as the reference writes them -----------------------------
double rint_even(double x) {      // contrast.ml:52-58
  const double fl = std::floor(x), d = x - fl;
  if (d > 0.5) return fl + 1.0;
  if (d < 0.5) return fl;
  return std::fmod(fl, 2.0) == 0.0 ? fl : fl + 1.0;
}

struct ContrastParams {
  int64_t n_bands = 6;
  double f_min = 200.0, quantile = 0.02;
  bool linear = false, clamped = true;
  int64_t sample_rate = 0;
};

std::vector<Band> contrast_plan(const char *fn, const ContrastParams &q, int64_t fft_size) {
  if (q.n_bands < 1)
    throw InvalidArgument(format("%s: cannot divide the spectrum into %lld octave bands (n_bands must be at least 1)", fn,
                                 (long long)q.n_bands));
  if (!(std::isfinite(q.f_min) && q.f_min > 0.0))
    throw InvalidArgument(format("%s: cannot start the first octave band at %g Hz (f_min must be finite and positive)", fn, q.f_min));
  if (!(q.quantile > 0.0 && q.quantile < 1.0))
    throw InvalidArgument(format("%s: cannot average the %g quantile of each band (quantile must lie strictly between 0 and 1)", fn,
                                 q.quantile));
  if (q.sample_rate < 1)
    throw InvalidArgument(format("%s: cannot use a sample rate of %lld Hz (sample_rate must be at least 1)", fn, (long long)q.sample_rate));
  auto edge = [&](int64_t j) { return j == 0 ? 0.0 : q.f_min * std::pow(2.0, (double)(j - 1)); };
  const double nyquist = 0.5 * (double)q.sample_rate;
  if (edge(q.n_bands) >= nyquist)
    throw InvalidArgument(format(
        "%s: cannot start the top octave band at %g Hz at a sample rate of %lld Hz (every band must start below the Nyquist "
        "frequency %g; lower f_min or n_bands)", fn, edge(q.n_bands), (long long)q.sample_rate, nyquist));
  const int64_t bins = fft_size / 2 + 1;
  const double step = 1.0 / ((double)fft_size * (1.0 / (double)q.sample_rate));
  std::vector<Band> plan;
  for (int64_t k = 0; k <= q.n_bands; ++k) {
    const double f_low = edge(k), f_high = edge(k + 1);
    int64_t lo0 = -1, hi0 = -1;
    for (int64_t i = 0; i < bins; ++i) {
      const double f = (double)i * step;
      if (f >= f_low && f <= f_high) {
        if (lo0 < 0) lo0 = i;
        hi0 = i;
      }
    }
    if (lo0 < 0)
      throw InvalidArgument(format(
          "%s: cannot resolve the octave band [%g, %g] Hz with an FFT of size %lld at a sample rate of %lld Hz (the band spans no "
          "FFT bin; raise fft_size or lower n_bands)", fn, f_low, f_high, (long long)fft_size, (long long)q.sample_rate));
    const int64_t lo = k > 0 ? lo0 - 1 : lo0, hi = k == q.n_bands ? bins - 1 : hi0;
    const int64_t count = hi - lo + 1;
    const int64_t take = std::max<int64_t>(1, (int64_t)rint_even(q.quantile * (double)count));
    const int64_t sub_len = (k == q.n_bands ? hi : hi - 1) - lo + 1;
    if (sub_len < 1)
      throw InvalidArgument(format(
          "%s: cannot resolve the octave band [%g, %g] Hz with an FFT of size %lld at a sample rate of %lld Hz (the band spans no "
          "FFT bin below its top edge; raise fft_size or lower n_bands)", fn, f_low, f_high, (long long)fft_size,
          (long long)q.sample_rate));
    if (lo + sub_len > 2147483647LL) throw Failure(format("%s: too many bins", fn));
    plan.push_back(Band{(int)lo, (int)sub_len, (int)std::min(take, sub_len)});
  }
  return plan;
}

// ---- contrast.ml:155-206 `apply` on device-resident magnitudes ---------------------------------------------------------------
void contrast_apply_dev(const char *fn, const std::vector<Band> &plan, const ContrastParams &q, bool check_magnitudes, const void *d_s,
                        int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *d_out, hipStream_t stream) {
  if (lead == 0 || bins == 0 || frames == 0) return;       // the broadcast-consistent empty result
  if (!d_s || !d_out) throw Failure(format("%s: null device pointer", fn));
  if (plan.size() > (size_t)kMaxBands) throw Failure(format("%s: more than %d bands", fn, kMaxBands));
  ContrastArgs a{};
  a.s = d_s;
  a.out = d_out;
  a.lead = lead;
  a.bins = bins;
  a.frames = frames;
  a.ftiles = (frames + 63) / 64;
  a.rows = (int)plan.size();
  a.mode = q.linear ? CONTRAST_LINEAR : (q.clamped ? CONTRAST_LOG_CLAMPED : CONTRAST_LOG);
  a.general = fast_path_disabled() ? 1 : 0;
  for (size_t k = 0; k < plan.size(); ++k) a.band[k] = plan[k];
  const int64_t total = lead * (int64_t)a.rows * frames;
  // scratch: the two maxima, the verdict on the magnitudes, then the float64 means of the clamped path
  const size_t means = a.mode == CONTRAST_LOG_CLAMPED ? (size_t)total * sizeof(double) : 0;
  DeviceScratch scratch;
  scratch.pool(32 + 2 * means, stream);
  SMX_HIP_CHECK(hipMemsetAsync(scratch.ptr, 0, 32, stream));
  a.keys = scratch.as<unsigned long long>();
  if (check_magnitudes) a.invalid = reinterpret_cast<int *>(scratch.as<unsigned char>() + 16);
  if (means) {
    a.valley = reinterpret_cast<double *>(scratch.as<unsigned char>() + 32);
    a.peak = a.valley + total;
  }
  const dim3 grid(grid_x(fn, "frame tiles", lead * a.ftiles, 64), (unsigned)a.rows);
  if (elem_bytes == 8) SMX_LAUNCH(contrast_kernel<double>, grid, dim3(64), 0, stream, a);
  else SMX_LAUNCH(contrast_kernel<float>, grid, dim3(64), 0, stream, a);
  SMX_HIP_CHECK(hipGetLastError());
  if (means) {
    launch_max_key<double>(a.valley, total, 2, a.keys, stream);          // valley and peak lie one behind the other
    const unsigned blocks = grid_x(fn, "frame tiles", (total + 255) / 256, 256);
    if (elem_bytes == 8)
      SMX_LAUNCH(contrast_db_kernel<double>, dim3(blocks), dim3(256), 0, stream, a.valley, a.peak, a.keys, (double *)d_out, total);
    else
      SMX_LAUNCH(contrast_db_kernel<float>, dim3(blocks), dim3(256), 0, stream, a.valley, a.peak, a.keys, (float *)d_out, total);
    SMX_HIP_CHECK(hipGetLastError());
  }
  if (check_magnitudes) {         // the reference refuses such a spectrogram: the verdict has to reach the host
    int invalid = 0;
    SMX_HIP_CHECK(hipMemcpyAsync(&invalid, a.invalid, sizeof(int), hipMemcpyDeviceToHost, stream));
    void *used = scratch.ptr;     // released behind the copy and before the wait: the stream is idle when the verdict is in
    scratch.ptr = nullptr;
    SMX_HIP_CHECK(smx::pool_free_async(used, stream));
    SMX_HIP_CHECK(hipStreamSynchronize(stream));
    if (invalid)
      throw InvalidArgument(format(
          "%s: cannot analyse a spectrogram with negative or NaN values (a magnitude spectrogram is non-negative)", fn));
  }
}

void check_extents(const char *fn, int64_t lead, int64_t bins, int64_t frames) {
  if (lead < 0 || bins < 0 || frames < 0)
    throw Failure(format("%s: negative extent (lead %lld, bins %lld, frames %lld)", fn, (long long)lead, (long long)bins,
                         (long long)frames));
}

// fft_size 0: spectral_contrast_of_spectrogram (contrast.ml:223-252), the FFT size implied by the bin count, the magnitudes
// checked.  Otherwise the body of spectral_contrast_stage (contrast.ml:254-261): a plan built for fft_size meets a chunk.
std::vector<Band> check_of_spectrogram(const ContrastParams &q, int64_t fft_size, int64_t lead, int64_t bins, int64_t frames) {
  const char *fn = fft_size ? "spectral_contrast_stage" : "spectral_contrast_of_spectrogram";
  check_extents(fn, lead, bins, frames);
  if (fft_size) {
    if (fft_size < 0) throw Failure(format("%s: negative fft_size", fn));
    std::vector<Band> plan = contrast_plan(fn, q, fft_size);
    if (bins != fft_size / 2 + 1)
      throw InvalidArgument(format("%s: cannot band %lld frequency bins with a plan built for an FFT of size %lld (%lld bins)", fn,
                                   (long long)bins, (long long)fft_size, (long long)(fft_size / 2 + 1)));
    return plan;
  }
  if (bins < 2)
    throw InvalidArgument(format(
        "%s: cannot derive bin frequencies for a %lld-bin spectrogram (the implied FFT size is %lld; a magnitude spectrogram holds "
        "fft_size / 2 + 1 bins)", fn, (long long)bins, (long long)(2 * (bins - 1))));
  return contrast_plan(fn, q, 2 * (bins - 1));
}

void contrast_of_spectrogram_dev(const ContrastParams &q, int64_t fft_size, const void *d_s, int elem_bytes, int64_t lead, int64_t bins,
                                 int64_t frames, void *d_out, hipStream_t stream) {
  const std::vector<Band> plan = check_of_spectrogram(q, fft_size, lead, bins, frames);
  contrast_apply_dev(fft_size ? "spectral_contrast_stage" : "spectral_contrast_of_spectrogram", plan, q, fft_size == 0, d_s, elem_bytes,
                     lead, bins, frames, d_out, stream);
}

void contrast_of_spectrogram_host(const ContrastParams &q, int64_t fft_size, const void *s, int elem_bytes, int64_t lead, int64_t bins,
                                  int64_t frames, void *out) {
  const std::vector<Band> plan = check_of_spectrogram(q, fft_size, lead, bins, frames);
  if (lead == 0 || bins == 0 || frames == 0) return;
  if (!s || !out) throw Failure("spectral_contrast_of_spectrogram: null pointer");
  const size_t row = (size_t)frames * (size_t)elem_bytes;
  host_call("spectral_contrast_of_spectrogram", {{s, (size_t)bins * row}}, out, plan.size() * row, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              contrast_of_spectrogram_dev(q, fft_size, d_in[0], elem_bytes, nc, bins, frames, d_out, stream);
            });
}

// spectral_contrast (contrast.ml:208-218): the magnitude spectrogram into scratch, then apply under the clamp
void spectral_contrast_dev(const smx_stft_config &sc, const ContrastParams &q, const void *d_x, int in_bytes, int64_t lead, int64_t n,
                           int64_t x_stride, void *d_out, hipStream_t stream) {
  const char *fn = "spectral_contrast";
  const std::vector<Band> plan = contrast_plan(fn, q, sc.fft_size);
  check_rank_extents(fn, lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!d_x || !d_out) throw Failure("spectral_contrast: null device pointer");
  DeviceScratch spec;
  spec.pool((size_t)lead * (size_t)sc.bins() * (size_t)count * (size_t)in_bytes, stream);
  stft_range_dev(sc, d_x, in_bytes, lead, n, x_stride, 0, count, OUT_POWER, 1.0, spec.ptr, stream);
  contrast_apply_dev(fn, plan, q, false, spec.ptr, in_bytes, lead, sc.bins(), count, d_out, stream);
}

void spectral_contrast_host(const smx_stft_config &sc, const ContrastParams &q, const void *x, int in_bytes, int64_t lead, int64_t n,
                            void *out) {
  const std::vector<Band> plan = contrast_plan("spectral_contrast", q, sc.fft_size);
  check_rank_extents("spectral_contrast", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure("spectral_contrast: null pointer");
  host_call("spectral_contrast", {{x, (size_t)n * (size_t)in_bytes}}, out, plan.size() * (size_t)count * (size_t)in_bytes, lead, false,
            nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              spectral_contrast_dev(sc, q, d_in[0], in_bytes, nc, n, n, d_out, stream);
            });
}

// ---- onset.ml ----------------------------------------------------------------------------------------------------------------
void check_lag(const char *fn, int64_t lag) {               // onset.ml:29-34
  if (lag < 1)
    throw InvalidArgument(format("%s: cannot difference frames at a lag of %lld (lag must be at least 1)", fn, (long long)lag));
}

template <bool LOG>
void launch_flux(const char *fn, FluxArgs a, int elem_bytes, hipStream_t stream) {
  a.ftiles = (a.frames + 255) / 256;
  // clip range by clip range (DESIGN.md "Launch extents"); the LOG clamp's maximum is the whole tensor's and stays the caller's
  const int64_t lead = a.lead, per_launch = std::max<int64_t>(1, clips_per_launch(a.ftiles, 256));
  const char *s = reinterpret_cast<const char *>(a.s);
  char *out = reinterpret_cast<char *>(a.out);
  for (int64_t c0 = 0; c0 < lead; c0 += per_launch) {
    a.lead = std::min(per_launch, lead - c0);
    a.s = s + c0 * a.bins * a.frames * elem_bytes;
    a.out = out + c0 * a.frames * elem_bytes;
    const dim3 grid(grid_x(fn, "frame tiles", a.lead * a.ftiles, 256));
    if (elem_bytes == 8) SMX_LAUNCH((flux_kernel<double, LOG>), grid, dim3(256), 0, stream, a);
    else SMX_LAUNCH((flux_kernel<float, LOG>), grid, dim3(256), 0, stream, a);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

// the one-chunk state_step (onset.ml:82-122) with an empty carry: decibels in, no clamp, no shift
void check_onset_flux(int64_t lag, int64_t lead, int64_t bins, int64_t frames) {
  const char *fn = "onset_strength_stage";
  check_lag(fn, lag);
  check_extents(fn, lead, bins, frames);
  if (lead == 0 || bins == 0)
    throw InvalidArgument(format("%s: cannot aggregate a chunk with a zero-size axis (bins and channels must be at least 1)", fn));
}

void onset_flux_dev(int64_t lag, const void *d_s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *d_out,
                    hipStream_t stream) {
  check_onset_flux(lag, lead, bins, frames);
  if (frames == 0) return;
  if (!d_s || !d_out) throw Failure("onset_strength_stage: null device pointer");
  FluxArgs a{};
  a.s = d_s;
  a.out = d_out;
  a.lead = lead;
  a.bins = bins;
  a.frames = frames;
  a.lag = lag;
  launch_flux<false>("onset_strength_stage", a, elem_bytes, stream);
}

void onset_flux_host(int64_t lag, const void *s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *out) {
  check_onset_flux(lag, lead, bins, frames);
  if (frames == 0) return;
  if (!s || !out) throw Failure("onset_strength_stage: null pointer");
  const size_t row = (size_t)frames * (size_t)elem_bytes;
  host_call("onset_flux", {{s, (size_t)bins * row}}, out, row, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              onset_flux_dev(lag, d_in[0], elem_bytes, nc, bins, frames, d_out, stream);
            });
}

void check_onset(const smx_stft_config &sc, const smx_mel_config &mc, int64_t lag) {      // onset.ml:153-163
  check_lag("onset_strength", lag);
  if (sc.fft_size != mc.fft_size)
    throw InvalidArgument(format(
        "onset_strength: cannot project a %lld-point STFT through a filterbank built for an FFT of size %lld (the two "
        "configurations must agree on fft_size)", (long long)sc.fft_size, (long long)mc.fft_size));
}

// onset_strength (onset.ml:153-199): mel_spectrogram, decibels under the whole tensor's clamp, flux, the centred shift
void onset_strength_dev(const smx_stft_config &sc, const smx_mel_config &mc, int64_t lag, const void *d_x, int in_bytes, int64_t lead,
                        int64_t n, int64_t x_stride, void *d_out, hipStream_t stream) {
  check_onset(sc, mc, lag);
  check_rank_extents("onset_strength", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!d_x || !d_out) throw Failure("onset_strength: null device pointer");
  const int64_t total = lead * mc.n_mels * count;
  DeviceScratch mel;
  mel.pool(256 + (size_t)total * (size_t)in_bytes, stream);           // the maximum's key, then the mel spectrogram
  void *d_mel = mel.as<unsigned char>() + 256;
  SMX_HIP_CHECK(hipMemsetAsync(mel.ptr, 0, 256, stream));
  mel_spectrogram_dev(sc, mc, d_x, in_bytes, lead, n, x_stride, 2.0, d_mel, stream);
  if (in_bytes == 8) launch_max_key<double>((const double *)d_mel, total, 1, mel.as<unsigned long long>(), stream);
  else launch_max_key<float>((const float *)d_mel, total, 1, mel.as<unsigned long long>(), stream);
  FluxArgs a{};
  a.s = d_mel;
  a.out = d_out;
  a.max_key = mel.as<unsigned long long>();
  a.lead = lead;
  a.bins = mc.n_mels;
  a.frames = count;
  a.lag = lag;
  a.shift = sc.alignment == SMX_ALIGN_CENTERED ? sc.fft_size / (2 * sc.hop) : 0;
  launch_flux<true>("onset_strength", a, in_bytes, stream);
}

void onset_strength_host(const smx_stft_config &sc, const smx_mel_config &mc, int64_t lag, const void *x, int in_bytes, int64_t lead,
                         int64_t n, void *out) {
  check_onset(sc, mc, lag);
  check_rank_extents("onset_strength", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure("onset_strength: null pointer");
  host_call("onset_strength", {{x, (size_t)n * (size_t)in_bytes}}, out, (size_t)count * (size_t)in_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              onset_strength_dev(sc, mc, lag, d_in[0], in_bytes, nc, n, n, d_out, stream);
            });
}

ContrastParams contrast_params(int64_t n_bands, double f_min, double quantile, int linear, int64_t sample_rate, int clamped) {
  ContrastParams q;
  q.n_bands = n_bands;
  q.f_min = f_min;
  q.quantile = quantile;
  q.linear = linear != 0;
  q.sample_rate = sample_rate;
  q.clamped = clamped != 0;
  return q;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Spectral contrast (contrast.ml) ---------------------------------------------------------------------------------------
int smx_spectral_contrast_plan(int64_t n_bands, double f_min, double quantile, int64_t sample_rate, int64_t fft_size, int64_t *lo,
                               int64_t *sub_len, int64_t *take) {
  return guarded([&] {
    if (fft_size < 0) throw Failure("spectral_contrast: negative fft_size");
    const std::vector<Band> plan = contrast_plan("spectral_contrast", contrast_params(n_bands, f_min, quantile, 0, sample_rate, 1), fft_size);
    for (size_t k = 0; k < plan.size(); ++k) {
      if (lo) lo[k] = plan[k].lo;
      if (sub_len) sub_len[k] = plan[k].sub_len;
      if (take) take[k] = plan[k].take;
    }
  });
}
int smx_spectral_contrast_f32(const smx_stft_config *sc, const float *x, int64_t lead, int64_t n, int64_t n_bands, double f_min,
                              double quantile, int linear, int64_t sample_rate, float *out) {
  return guarded([&] {
    check_config(sc, "spectral_contrast");
    spectral_contrast_host(*sc, contrast_params(n_bands, f_min, quantile, linear, sample_rate, 1), x, 4, lead, n, out);
  });
}
int smx_spectral_contrast_f64(const smx_stft_config *sc, const double *x, int64_t lead, int64_t n, int64_t n_bands, double f_min,
                              double quantile, int linear, int64_t sample_rate, double *out) {
  return guarded([&] {
    check_config(sc, "spectral_contrast");
    spectral_contrast_host(*sc, contrast_params(n_bands, f_min, quantile, linear, sample_rate, 1), x, 8, lead, n, out);
  });
}
int smx_spectral_contrast_dev_f32(const smx_stft_config *sc, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t n_bands,
                                  double f_min, double quantile, int linear, int64_t sample_rate, float *d_out, void *stream) {
  return guarded([&] {
    check_config(sc, "spectral_contrast");
    spectral_contrast_dev(*sc, contrast_params(n_bands, f_min, quantile, linear, sample_rate, 1), d_x, 4, lead, n, x_stride, d_out,
                          (hipStream_t)stream);
  });
}
int smx_spectral_contrast_of_spectrogram_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t fft_size, int64_t n_bands,
                                             double f_min, double quantile, int linear, int64_t sample_rate, int clamped, float *out) {
  return guarded([&] {
    contrast_of_spectrogram_host(contrast_params(n_bands, f_min, quantile, linear, sample_rate, clamped), fft_size, s, 4, lead, bins, frames, out);
  });
}
int smx_spectral_contrast_of_spectrogram_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t fft_size, int64_t n_bands,
                                             double f_min, double quantile, int linear, int64_t sample_rate, int clamped, double *out) {
  return guarded([&] {
    contrast_of_spectrogram_host(contrast_params(n_bands, f_min, quantile, linear, sample_rate, clamped), fft_size, s, 8, lead, bins, frames, out);
  });
}
int smx_spectral_contrast_of_spectrogram_dev_f32(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t fft_size,
                                                 int64_t n_bands, double f_min, double quantile, int linear, int64_t sample_rate,
                                                 int clamped, float *d_out, void *stream) {
  return guarded([&] {
    contrast_of_spectrogram_dev(contrast_params(n_bands, f_min, quantile, linear, sample_rate, clamped), fft_size, d_s, 4, lead, bins, frames,
                                d_out, (hipStream_t)stream);
  });
}

// ---- Onset strength (onset.ml) ---------------------------------------------------------------------------------------------
int smx_onset_strength_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *x, int64_t lead, int64_t n, int64_t lag,
                           float *out) {
  return guarded([&] {
    check_config(sc, "onset_strength");
    check_config(mc, "onset_strength");
    onset_strength_host(*sc, *mc, lag, x, 4, lead, n, out);
  });
}
int smx_onset_strength_f64(const smx_stft_config *sc, const smx_mel_config *mc, const double *x, int64_t lead, int64_t n, int64_t lag,
                           double *out) {
  return guarded([&] {
    check_config(sc, "onset_strength");
    check_config(mc, "onset_strength");
    onset_strength_host(*sc, *mc, lag, x, 8, lead, n, out);
  });
}
int smx_onset_strength_dev_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *d_x, int64_t lead, int64_t n,
                               int64_t x_stride, int64_t lag, float *d_out, void *stream) {
  return guarded([&] {
    check_config(sc, "onset_strength");
    check_config(mc, "onset_strength");
    onset_strength_dev(*sc, *mc, lag, d_x, 4, lead, n, x_stride, d_out, (hipStream_t)stream);
  });
}
int smx_onset_flux_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t lag, float *out) {
  return guarded([&] { onset_flux_host(lag, s, 4, lead, bins, frames, out); });
}
int smx_onset_flux_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t lag, double *out) {
  return guarded([&] { onset_flux_host(lag, s, 8, lead, bins, frames, out); });
}
int smx_onset_flux_dev_f32(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t lag, float *d_out, void *stream) {
  return guarded([&] { onset_flux_dev(lag, d_s, 4, lead, bins, frames, d_out, (hipStream_t)stream); });
}

}  // extern "C"
