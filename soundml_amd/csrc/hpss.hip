// Harmonic/percussive separation by median filtering (hpss.ml:22-61, 294-347, 436-459) on a device-resident plane stack
// [lead; bins; frames], frames fastest.
//
//   harm[b, t] = rank k_h / 2 of the ascending window of k_h frames [t - k_h / 2, t + k_h - 1 - k_h / 2] of row b
//   perc[b, t] = rank k_p / 2 of the ascending window of k_p bins of column t            (hpss.ml:43-50)
//   indices outside the axis reflect half-sample-symmetrically with period 2 n, any overhang (hpss.ml:69-75)
//   mask_h = softmask(harm, perc * m_h), mask_p = softmask(perc, harm * m_p)               (hpss.ml:325-347)
//
// Both filters SELECT: every value is mapped to an unsigned key whose integer order is the floating-point order, the
// rank-k/2 key is found exactly, and mapped back -- the output is one of the inputs bit for bit, and the two filters draw from
// the same values, so harm == perc holds exactly where both picked one cell (a hard mask is 0 on both sides there).
// NaN inputs: unspecified, as in the reference.  -0.0 sorts below +0.0.
//
// Two kernels behind one epilogue (the masks and products are the same device function, so they agree bit for bit):
//   hpss_general_kernel   any k_h, k_p >= 1, float32 / float64: one thread per cell, the rank found by bisection on the key's
//                         bits (count the window's keys below a candidate, one bit per pass): O(bits * k) reads per cell
//                         through the cache, the reflected index walked instead of recomputed.  Slow; the yardstick.
//   hpss_fast31_kernel    k_h = k_p = 31, float32, planes of at least 128 x 128: a workgroup owns 32 bins x 64 frames, stages the
//                         62 x 94 halo tile once in LDS as keys (reflection folded into the load index; the complex face takes
//                         |z| here), and every thread sorts its two 31-value windows in registers with Batcher's odd-even
//                         merge network on v_min_u32 / v_max_u32 (the comparators that cannot reach rank 15 are dead code).
// harm and perc never go to memory: the kernel reads the plane once and writes the two results.
// Built with -ffp-contract=off (csrc/Makefile): x / z, m / (m + r) and (mag * mask) * phase round as written.
#include <utility>

#include "smx_internal.hpp"

namespace smx {
namespace {

enum { P_ONE = 0, P_TWO = 1, P_ANY = 2, P_INF = 3 };

template <typename T> struct Key;
template <> struct Key<float> {
  typedef uint32_t U;
  static constexpr int bits = 32;
  static __device__ __forceinline__ U of(float v) {
    const U u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  }
  static __device__ __forceinline__ float back(U k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
  static __device__ __forceinline__ float tiny() { return 1.1754943508222875e-38f; }
};
template <> struct Key<double> {
  typedef uint64_t U;
  static constexpr int bits = 64;
  static __device__ __forceinline__ U of(double v) {
    const U u = (U)__double_as_longlong(v);
    return u ^ ((u >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double back(U k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull)));
  }
  static __device__ __forceinline__ double tiny() { return 2.2250738585072014e-308; }
};

__device__ __forceinline__ float magnitude(float re, float im) { return hypotf(re, im); }
__device__ __forceinline__ double magnitude(double re, double im) { return hypot(re, im); }
__device__ __forceinline__ float power_of(float x, float p) { return powf(x, p); }
__device__ __forceinline__ double power_of(double x, double p) { return pow(x, p); }

// hpss.ml:309-310: unit and square exponents are the identity and one multiply
template <int PC, typename T>
__device__ __forceinline__ T powered(T x, T p) {
  if (PC == P_ONE) return x;
  if (PC == P_TWO) return x * x;
  return power_of(x, p);
}

// hpss.ml:325-338
template <int PC, typename T>
__device__ __forceinline__ T softmask(T x, T r, T p, bool split_zeros) {
  if (PC == P_INF) return x > r ? (T)1 : (T)0;
  T z = x > r ? x : r;
  const bool bad = z < Key<T>::tiny();
  z = bad ? (T)1 : z;
  const T m = powered<PC>(x / z, p);
  const T q = powered<PC>(r / z, p);
  const T share = m / (m + q);
  return bad ? (split_zeros ? (T)0.5 : (T)0) : share;
}

struct HpssArgs {
  const void *src;     // the plane: real, or interleaved complex (mode HPSS_STFT)
  const void *mag;     // general kernel, HPSS_STFT: |z| as a real plane
  void *out_h, *out_p; // either may be null
  int64_t lead, bins, frames, kernel_h, kernel_p;
  double power, margin_h, margin_p;
};

// masks / products / complex components of one cell from its two medians (hpss.ml:342-347, 416-420, 446-459)
template <int MODE, int PC, typename T>
__device__ __forceinline__ void finish_cell(const HpssArgs &a, int64_t cell, T s, T harm, T perc) {
  const T m_h = (T)a.margin_h, m_p = (T)a.margin_p, p = (T)a.power;
  const bool split_zeros = a.margin_h == 1.0 && a.margin_p == 1.0;
  const T mask_h = softmask<PC>(harm, perc * m_h, p, split_zeros);
  const T mask_p = softmask<PC>(perc, harm * m_p, p, split_zeros);
  T *out_h = reinterpret_cast<T *>(a.out_h), *out_p = reinterpret_cast<T *>(a.out_p);
  if (MODE == HPSS_MASKS) {
    if (out_h) out_h[cell] = mask_h;
    if (out_p) out_p[cell] = mask_p;
  } else if (MODE == HPSS_SPECTROGRAM) {
    if (out_h) out_h[cell] = s * mask_h;
    if (out_p) out_p[cell] = s * mask_p;
  } else {
    const T *z = reinterpret_cast<const T *>(a.src);
    const T re = z[2 * cell], im = z[2 * cell + 1];
    const T one_at_zero = s == (T)0 ? (T)1 : (T)0;
    const T denominator = s + one_at_zero;
    const T phase_re = re / denominator + one_at_zero;
    const T phase_im = im / denominator;
    if (out_h) {
      const T t = s * mask_h;
      out_h[2 * cell] = t * phase_re;
      out_h[2 * cell + 1] = t * phase_im;
    }
    if (out_p) {
      const T t = s * mask_p;
      out_p[2 * cell] = t * phase_re;
      out_p[2 * cell + 1] = t * phase_im;
    }
  }
}

// ---- the general path ---------------------------------------------------------------------------------------------------------
// rank k / 2 of the k values line[refl(i - k / 2 + j, n) * stride], j < k
template <typename T>
__device__ T select_rank(const T *line, int64_t stride, int64_t n, int64_t i, int64_t k) {
  typedef typename Key<T>::U U;
  const int64_t period = 2 * n;
  int64_t q = (i - k / 2) % period;
  if (q < 0) q += period;
  const int64_t first = q < n ? q : period - 1 - q;
  const int64_t first_dir = q < n ? 1 : -1;
  const int64_t rank = k / 2;
  U found = 0;   // the largest key v with |{keys < v}| <= rank: the key at that rank
  for (int bit = Key<T>::bits - 1; bit >= 0; --bit) {
    const U candidate = found | ((U)1 << bit);
    int64_t below = 0, idx = first, dir = first_dir;
    for (int64_t j = 0; j < k; ++j) {
      below += Key<T>::of(line[idx * stride]) < candidate ? 1 : 0;
      idx += dir;
      if (idx == n) {
        idx = n - 1;
        dir = -1;
      } else if (idx < 0) {
        idx = 0;
        dir = 1;
      }
    }
    if (below <= rank) found = candidate;
  }
  return Key<T>::back(found);
}

template <int MODE, int PC, typename T>
__global__ void __launch_bounds__(256) hpss_general_kernel(HpssArgs a) {
  const int64_t plane = a.bins * a.frames;
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.lead * plane) return;
  const int64_t within = cell % plane;
  const int64_t b = within / a.frames, t = within - b * a.frames;
  const T *s = reinterpret_cast<const T *>(MODE == HPSS_STFT ? a.mag : a.src) + (cell - within);
  const T harm = select_rank(s + b * a.frames, (int64_t)1, a.frames, t, a.kernel_h);
  const T perc = select_rank(s + t, a.frames, a.bins, b, a.kernel_p);
  finish_cell<MODE, PC, T>(a, cell, s[within], harm, perc);
}

template <typename T>
__global__ void __launch_bounds__(256) hpss_magnitude_kernel(const T *z, T *mag, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) mag[i] = magnitude(z[2 * i], z[2 * i + 1]);
}

// ---- the 31 x 31 float32 path -----------------------------------------------------------------------------------------------
constexpr int K31 = 31, HALO = K31 / 2;
constexpr int TILE_B = 32, TILE_F = 64;
constexpr int TILE_ROWS = TILE_B + K31 - 1, TILE_COLS = TILE_F + K31 - 1;   // 62 x 94 keys = 23 312 bytes of LDS

// Batcher's odd-even merge sort of 32 keys as a comparator list, built at compile time (191 comparators)
struct Network {
  int count;
  unsigned char lo[192], hi[192];
};
constexpr Network make_network() {
  Network t{};
  const int n = 32;
  for (int p = 1; p < n; p <<= 1)
    for (int k = p; k >= 1; k >>= 1)
      for (int j = k % p; j + k < n; j += 2 * k)
        for (int i = 0; i < k && i + j + k < n; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            t.lo[t.count] = (unsigned char)(i + j);
            t.hi[t.count] = (unsigned char)(i + j + k);
            ++t.count;
          }
  return t;
}
constexpr int NETWORK_COMPARATORS = make_network().count;

template <int C>
__device__ __forceinline__ void compare_exchange(uint32_t (&v)[32]) {
  constexpr Network net = make_network();
  const uint32_t x = v[net.lo[C]], y = v[net.hi[C]];
  v[net.lo[C]] = x < y ? x : y;
  v[net.hi[C]] = x < y ? y : x;
}
template <int... C>
__device__ __forceinline__ void sort32(uint32_t (&v)[32], std::integer_sequence<int, C...>) {
  (compare_exchange<C>(v), ...);
}
// rank 15 of 31 keys: the 32nd is the largest key there is, so it stays last and rank 15 of 32 is rank 15 of 31
__device__ __forceinline__ uint32_t median31(uint32_t (&v)[32]) {
  v[31] = 0xFFFFFFFFu;
  sort32(v, std::make_integer_sequence<int, NETWORK_COMPARATORS>());
  return v[15];
}

// one fold of the half-sample-symmetric reflection: exact for -n <= i < 2 n (the launcher admits planes of >= 128 x 128 only)
__device__ __forceinline__ int reflect_once(int i, int n) {
  i = i < 0 ? -1 - i : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);
}

template <int MODE, int PC>
__global__ void __launch_bounds__(256) hpss_fast31_kernel(HpssArgs a, int tiles_f, int tiles_b) {
  __shared__ uint32_t tile[TILE_ROWS * TILE_COLS];
  const int bins = (int)a.bins, frames = (int)a.frames;
  const int tile_f = blockIdx.x % tiles_f;
  const int tile_b = (blockIdx.x / tiles_f) % tiles_b;
  const int64_t clip = blockIdx.x / (tiles_f * tiles_b);
  const int b0 = tile_b * TILE_B, t0 = tile_f * TILE_F;
  const int64_t origin = clip * a.bins * a.frames;
  const float *src = reinterpret_cast<const float *>(a.src);

  for (int idx = threadIdx.x; idx < TILE_ROWS * TILE_COLS; idx += 256) {
    const int r = idx / TILE_COLS, c = idx - r * TILE_COLS;
    const int64_t at = origin + (int64_t)reflect_once(b0 - HALO + r, bins) * frames + reflect_once(t0 - HALO + c, frames);
    float v;
    if (MODE == HPSS_STFT) {
      const float2 z = reinterpret_cast<const float2 *>(src)[at];
      v = magnitude(z.x, z.y);
    } else {
      v = src[at];
    }
    tile[idx] = Key<float>::of(v);
  }
  __syncthreads();

  const int lt = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int lb = wave; lb < TILE_B; lb += 4) {
    const int b = b0 + lb, t = t0 + lt;
    if (b >= bins) break;   // (the same for the whole wave)
    uint32_t v[32];
#pragma unroll
    for (int j = 0; j < K31; ++j) v[j] = tile[(lb + HALO) * TILE_COLS + lt + j];
    const float harm = Key<float>::back(median31(v));
#pragma unroll
    for (int j = 0; j < K31; ++j) v[j] = tile[(lb + j) * TILE_COLS + lt + HALO];
    const float perc = Key<float>::back(median31(v));
    const float s = Key<float>::back(tile[(lb + HALO) * TILE_COLS + lt + HALO]);
    if (t < frames) finish_cell<MODE, PC, float>(a, origin + (int64_t)b * frames + t, s, harm, perc);
  }
}

int power_class(double power) {
  if (!std::isfinite(power)) return P_INF;
  if (power == 1.0) return P_ONE;
  if (power == 2.0) return P_TWO;
  return P_ANY;
}

template <int MODE, int PC>
void launch_fast31(const HpssArgs &a, hipStream_t stream) {
  const int tiles_f = (int)((a.frames + TILE_F - 1) / TILE_F), tiles_b = (int)((a.bins + TILE_B - 1) / TILE_B);
  SMX_LAUNCH((hpss_fast31_kernel<MODE, PC>), dim3((unsigned)(a.lead * tiles_f * tiles_b)), dim3(256), 0, stream, a, tiles_f, tiles_b);
}

template <int MODE, int PC, typename T>
void launch_general(const HpssArgs &a, hipStream_t stream) {
  const int64_t cells = a.lead * a.bins * a.frames;
  SMX_LAUNCH((hpss_general_kernel<MODE, PC, T>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, a);
}

template <int MODE, int PC>
void launch_mode_power(const HpssArgs &a, int elem_bytes, bool fast, hipStream_t stream) {
  if (fast) launch_fast31<MODE, PC>(a, stream);
  else if (elem_bytes == 4) launch_general<MODE, PC, float>(a, stream);
  else launch_general<MODE, PC, double>(a, stream);
}

template <int MODE>
void launch_mode(const HpssArgs &a, int elem_bytes, bool fast, hipStream_t stream) {
  switch (power_class(a.power)) {
    case P_ONE: return launch_mode_power<MODE, P_ONE>(a, elem_bytes, fast, stream);
    case P_TWO: return launch_mode_power<MODE, P_TWO>(a, elem_bytes, fast, stream);
    case P_ANY: return launch_mode_power<MODE, P_ANY>(a, elem_bytes, fast, stream);
    default: return launch_mode_power<MODE, P_INF>(a, elem_bytes, fast, stream);
  }
}

}  // namespace

bool hpss_takes_fast_path(const HpssJob &job) {
  return job.elem_bytes == 4 && job.kernel_h == K31 && job.kernel_p == K31 && job.bins >= 128 && job.frames >= 128 &&
         job.bins < (1 << 24) && job.frames < (1 << 24) && !fast_path_disabled();
}

void launch_hpss(const HpssJob &job) {
  if (job.lead <= 0 || job.bins <= 0 || job.frames <= 0) return;
  const int64_t cells = job.lead * job.bins * job.frames;
  const bool fast = hpss_takes_fast_path(job);
  const int64_t blocks = fast ? job.lead * ((job.frames + TILE_F - 1) / TILE_F) * ((job.bins + TILE_B - 1) / TILE_B) : (cells + 255) / 256;
  if (blocks > clips_per_launch(1, 256)) throw Failure("hpss: the spectrogram has too many cells for one launch (pass it in slices of its leading axes)");
  HpssArgs a;
  a.src = job.s;
  a.mag = nullptr;
  a.out_h = job.out_h;
  a.out_p = job.out_p;
  a.lead = job.lead;
  a.bins = job.bins;
  a.frames = job.frames;
  a.kernel_h = job.kernel_h;
  a.kernel_p = job.kernel_p;
  a.power = job.power;
  a.margin_h = job.margin_h;
  a.margin_p = job.margin_p;
  DeviceScratch mag;
  if (job.mode == HPSS_STFT && !fast) {   // the general kernel reads each window value bits * k times: |z| once, as a plane
    init_device_pool();
    mag.pool((size_t)cells * (size_t)job.elem_bytes, job.stream);
    if (job.elem_bytes == 4)
      SMX_LAUNCH((hpss_magnitude_kernel<float>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, job.stream,
                 reinterpret_cast<const float *>(job.s), mag.as<float>(), cells);
    else
      SMX_LAUNCH((hpss_magnitude_kernel<double>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, job.stream,
                 reinterpret_cast<const double *>(job.s), mag.as<double>(), cells);
    a.mag = mag.ptr;
  }
  switch (job.mode) {
    case HPSS_MASKS: launch_mode<HPSS_MASKS>(a, job.elem_bytes, fast, job.stream); break;
    case HPSS_SPECTROGRAM: launch_mode<HPSS_SPECTROGRAM>(a, job.elem_bytes, fast, job.stream); break;
    default: launch_mode<HPSS_STFT>(a, job.elem_bytes, fast, job.stream); break;
  }
  SMX_HIP_CHECK(hipGetLastError());
}

}  // namespace smx

// ---- the C ABI's side: Hpss ------------------------------------------------------------------------------------------------
namespace smx {
namespace {

// ---- Hpss (hpss.ml:351-504): checks in the reference's order and words, then one launch ---------------------------------
struct HpssParams {
  const char *fn = "hpss";
  int64_t kernel_h = 31, kernel_p = 31;
  double power = 2.0, margin_h = 1.0, margin_p = 1.0;
};

// check_kernel, check_power, check_margin (hpss.ml:373-396); rank and dtype are what the entry point's signature states
void check_hpss(const HpssParams &q) {
  if (q.kernel_h < 1 || q.kernel_p < 1)
    throw InvalidArgument(format("%s: cannot median-filter with a kernel of (%lld, %lld) (both kernel sizes must be at least 1)", q.fn,
                                 (long long)q.kernel_h, (long long)q.kernel_p));
  if (std::isnan(q.power) || q.power <= 0.0)
    throw InvalidArgument(format("%s: cannot raise the mask to the power %g (power must be strictly positive, or infinite for a hard mask)",
                                 q.fn, std::isnan(q.power) ? std::fabs(q.power) : q.power));
  if (!(std::isfinite(q.margin_h) && std::isfinite(q.margin_p) && q.margin_h >= 1.0 && q.margin_p >= 1.0))
    throw InvalidArgument(format("%s: cannot bias the decision by a margin of (%g, %g) (both margins must be finite and at least 1)", q.fn,
                                 std::isnan(q.margin_h) ? std::fabs(q.margin_h) : q.margin_h,
                                 std::isnan(q.margin_p) ? std::fabs(q.margin_p) : q.margin_p));
}

void check_hpss_plane(const HpssParams &q, int64_t lead, int64_t bins, int64_t frames) {
  if (lead < 0 || bins < 0 || frames < 0)
    throw Failure(format("%s: negative extent (lead %lld, bins %lld, frames %lld)", q.fn, (long long)lead, (long long)bins,
                         (long long)frames));
  check_hpss(q);
}

// hpss_masks / hpss_of_spectrogram / hpss_of_stft on device-resident planes; either result pointer may be null
void hpss_dev(int mode, const HpssParams &q, const void *d_s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *d_h,
              void *d_p, hipStream_t stream) {
  check_hpss_plane(q, lead, bins, frames);
  if (lead == 0 || bins == 0 || frames == 0) return;   // nothing to separate
  if (!d_s || (!d_h && !d_p)) throw Failure(format("%s: null device pointer", q.fn));
  HpssJob job;
  job.mode = mode;
  job.s = d_s;
  job.elem_bytes = elem_bytes;
  job.lead = lead;
  job.bins = bins;
  job.frames = frames;
  job.kernel_h = q.kernel_h;
  job.kernel_p = q.kernel_p;
  job.power = q.power;
  job.margin_h = q.margin_h;
  job.margin_p = q.margin_p;
  job.out_h = d_h;
  job.out_p = d_p;
  job.stream = stream;
  launch_hpss(job);
}

void hpss_host(int mode, const HpssParams &q, const void *s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *h, void *p) {
  check_hpss_plane(q, lead, bins, frames);
  if (lead == 0 || bins == 0 || frames == 0) return;
  if (!s || (!h && !p)) throw Failure(format("%s: null pointer", q.fn));
  const size_t plane = (size_t)bins * (size_t)frames * (size_t)elem_bytes * (mode == HPSS_STFT ? 2 : 1);
  host_call(q.fn, {{s, plane}}, {{h, plane}, {p, plane}}, lead, true, nullptr,
            [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t stream) {
              hpss_dev(mode, q, d_in[0], elem_bytes, nc, bins, frames, d_out[0], d_out[1], stream);
            });
}

// `separate` (hpss.ml:477-492): Stft.transform -> hpss_of_stft -> Stft.invert ~length:n of the components that are wanted.  The
// checks of all three run before any device work
void check_separate(const HpssParams &q, const smx_stft_config *c, int64_t lead, int64_t n) {
  check_hpss(q);
  check_config(c, q.fn);
  check_rank_extents(q.fn, lead, n);
  check_synthesis("invert", *c, c->bins(), n, true);
}

// The three complex planes live in scratch and the batch goes through in clip chunks that keep them bounded: every clip is
// analysed, separated and synthesised on its own (stft.mli:214-218), so a chunk's result is the slice of the whole batch's.
void separate_dev(const HpssParams &q, const smx_stft_config &c, const void *d_x, int in_bytes, int64_t lead, int64_t n, void *d_h,
                  void *d_p, hipStream_t stream) {
  check_separate(q, &c, lead, n);
  if (lead == 0 || n == 0) return;
  if (!d_x || (!d_h && !d_p)) throw Failure(format("%s: null device pointer", q.fn));
  const int64_t bins = c.bins(), frames = c.frames(n);
  const size_t plane = (size_t)bins * (size_t)frames * 2 * (size_t)in_bytes;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(lead, (int64_t)(((size_t)256 << 20) / std::max<size_t>(plane, 1))));
  init_device_pool();
  DeviceScratch z, z_h, z_p;
  z.pool(std::max<size_t>(16, (size_t)chunk * plane), stream);
  if (d_h) z_h.pool(std::max<size_t>(16, (size_t)chunk * plane), stream);
  if (d_p) z_p.pool(std::max<size_t>(16, (size_t)chunk * plane), stream);
  const size_t row = (size_t)n * (size_t)in_bytes;
  for (int64_t c0 = 0; c0 < lead; c0 += chunk) {
    const int64_t nc = std::min(chunk, lead - c0);
    stft_range_dev(c, reinterpret_cast<const unsigned char *>(d_x) + (size_t)c0 * row, in_bytes, nc, n, n, 0, frames, OUT_COMPLEX, 2.0,
                   z.ptr, stream);
    hpss_dev(HPSS_STFT, q, z.ptr, in_bytes, nc, bins, frames, z_h.ptr, z_p.ptr, stream);
    if (d_h) invert_dev(c, z_h.ptr, 2 * in_bytes, nc, bins, frames, 1, n, reinterpret_cast<unsigned char *>(d_h) + (size_t)c0 * row, stream);
    if (d_p) invert_dev(c, z_p.ptr, 2 * in_bytes, nc, bins, frames, 1, n, reinterpret_cast<unsigned char *>(d_p) + (size_t)c0 * row, stream);
  }
}

void separate_host(const HpssParams &q, const smx_stft_config *c, const void *x, int in_bytes, int64_t lead, int64_t n, void *h, void *p) {
  check_separate(q, c, lead, n);
  if (lead == 0 || n == 0) return;
  if (!x || (!h && !p)) throw Failure(format("%s: null pointer", q.fn));
  const size_t row = (size_t)n * (size_t)in_bytes;
  host_call(q.fn, {{x, row}}, {{h, row}, {p, row}}, lead, true, nullptr,
            [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t stream) {
              separate_dev(q, *c, d_in[0], in_bytes, nc, n, d_out[0], d_out[1], stream);
            });
}

HpssParams hpss_params(const char *fn, int64_t kernel_h, int64_t kernel_p, double power, double margin_h, double margin_p) {
  HpssParams q;
  q.fn = fn;
  q.kernel_h = kernel_h;
  q.kernel_p = kernel_p;
  q.power = power;
  q.margin_h = margin_h;
  q.margin_p = margin_p;
  return q;
}

// the signal face's name: `hpss` returns the pair, `harmonic` / `percussive` one of them (hpss.ml:494-504)
const char *separate_name(const void *h, const void *p) { return h && p ? "hpss" : (h ? "harmonic" : (p ? "percussive" : "hpss")); }

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Harmonic/percussive separation (hpss.ml) ------------------------------------------------------
#define SMX_HPSS_ARGS int64_t kernel_h, int64_t kernel_p, double power, double margin_h, double margin_p
#define SMX_HPSS_Q(fn) hpss_params(fn, kernel_h, kernel_p, power, margin_h, margin_p)
int smx_hpss_masks_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, float *mask_h, float *mask_p) {
  return guarded([&] { hpss_host(HPSS_MASKS, SMX_HPSS_Q("hpss_masks"), s, 4, lead, bins, frames, mask_h, mask_p); });
}
int smx_hpss_masks_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, double *mask_h, double *mask_p) {
  return guarded([&] { hpss_host(HPSS_MASKS, SMX_HPSS_Q("hpss_masks"), s, 8, lead, bins, frames, mask_h, mask_p); });
}
int smx_hpss_masks_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, float *d_mask_h, float *d_mask_p,
                           void *stream) {
  return guarded([&] {
    hpss_dev(HPSS_MASKS, SMX_HPSS_Q("hpss_masks"), d_s, 4, lead, bins, frames, d_mask_h, d_mask_p, (hipStream_t)stream);
  });
}
int smx_hpss_of_spectrogram_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, float *h, float *p) {
  return guarded([&] { hpss_host(HPSS_SPECTROGRAM, SMX_HPSS_Q("hpss_of_spectrogram"), s, 4, lead, bins, frames, h, p); });
}
int smx_hpss_of_spectrogram_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, double *h, double *p) {
  return guarded([&] { hpss_host(HPSS_SPECTROGRAM, SMX_HPSS_Q("hpss_of_spectrogram"), s, 8, lead, bins, frames, h, p); });
}
int smx_hpss_of_spectrogram_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, float *d_h, float *d_p,
                                    void *stream) {
  return guarded([&] {
    hpss_dev(HPSS_SPECTROGRAM, SMX_HPSS_Q("hpss_of_spectrogram"), d_s, 4, lead, bins, frames, d_h, d_p, (hipStream_t)stream);
  });
}
int smx_hpss_of_stft_c64(const float *z, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, float *z_h, float *z_p) {
  return guarded([&] { hpss_host(HPSS_STFT, SMX_HPSS_Q("hpss_of_stft"), z, 4, lead, bins, frames, z_h, z_p); });
}
int smx_hpss_of_stft_c128(const double *z, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, double *z_h, double *z_p) {
  return guarded([&] { hpss_host(HPSS_STFT, SMX_HPSS_Q("hpss_of_stft"), z, 8, lead, bins, frames, z_h, z_p); });
}
int smx_hpss_of_stft_c64_dev(const float *d_z, int64_t lead, int64_t bins, int64_t frames, SMX_HPSS_ARGS, float *d_z_h, float *d_z_p,
                             void *stream) {
  return guarded([&] { hpss_dev(HPSS_STFT, SMX_HPSS_Q("hpss_of_stft"), d_z, 4, lead, bins, frames, d_z_h, d_z_p, (hipStream_t)stream); });
}
int smx_hpss_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, SMX_HPSS_ARGS, float *y_h, float *y_p) {
  return guarded([&] { separate_host(SMX_HPSS_Q(separate_name(y_h, y_p)), c, x, 4, lead, n, y_h, y_p); });
}
int smx_hpss_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, SMX_HPSS_ARGS, double *y_h, double *y_p) {
  return guarded([&] { separate_host(SMX_HPSS_Q(separate_name(y_h, y_p)), c, x, 8, lead, n, y_h, y_p); });
}
int smx_hpss_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, SMX_HPSS_ARGS, float *d_y_h, float *d_y_p,
                     void *stream) {
  return guarded([&] {
    const HpssParams q = SMX_HPSS_Q(separate_name(d_y_h, d_y_p));
    check_hpss(q);
    check_config(c, q.fn);
    separate_dev(q, *c, d_x, 4, lead, n, d_y_h, d_y_p, (hipStream_t)stream);
  });
}
#undef SMX_HPSS_ARGS
#undef SMX_HPSS_Q

}  // extern "C"
