// Spectral-shape features (spectral.ml:171-255) and the linear-frequency chroma projection (chroma.ml:285-317)
// over a device-resident spectrogram [lead; bins; frames] (frames fastest).
//
// Both are reductions along the bin axis with a float64 interior and one rounding to the spectrogram's dtype,
// in the reference's operation order for float64 input (normalise the frame, then weight, then reduce; s^power floored,
// then the two means); float32 input divides by the frame's sum after the weighted reduction instead of before it (one
// walk over the spectrogram less; the same value to a rounding of the float64 interior).  Frames sit across lanes, so every load of a bin row is one coalesced run of 64 frames; the
// features are HBM-bound (one to three passes over the spectrogram, the later ones mostly from L2 / MALL).
//
//   features:  a workgroup owns 64 frames; its Q = 4 waves each walk a quarter of the bins and the partial
//              sums meet in LDS in a fixed order ((q0 + q1) + (q2 + q3): deterministic).  The roll-off is a
//              running sum compared against a threshold, so it keeps the sequential order: Q = 1.
//   chroma:    one thread per frame accumulates a chunk of 12 chroma rows in float64 registers, the weights of a
//              bin (transposed table, uniform address) come through scalar loads; raw projections go to a
//              float64 scratch, the per-frame normalisation is a second small launch.
#include <cfloat>
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

struct SpectralArgs {
  const void *s;
  void *out;
  const double *freqs;      // device [bins] or null
  const void *centroid;     // device [lead; frames] or null
  double step, p, inv_p, power;
  int64_t lead, bins, frames, ftiles;
  int *invalid;
};

__device__ __forceinline__ double pow_fixed(double v, double p) {   // Nx.pow_s with the common exponents exact
  if (p == 2.0) return v * v;
  if (p == 1.0) return v;
  return pow(v, p);
}

// walks bins [k0, k1) of one frame column in order, kDepth loads in flight at a time
constexpr int kDepth = 8;
template <typename T, typename F>
__device__ __forceinline__ void for_bins(const T *col, int64_t frames, int64_t k0, int64_t k1, F &&f) {
  int64_t k = k0;
  for (; k + kDepth <= k1; k += kDepth) {
    T v[kDepth];
#pragma unroll
    for (int j = 0; j < kDepth; ++j) v[j] = col[(k + j) * frames];
#pragma unroll
    for (int j = 0; j < kDepth; ++j) f(k + j, (double)v[j]);
  }
  for (; k < k1; ++k) f(k, (double)col[k * frames]);
}

// A workgroup = four waves: the Q bin ranges of one 64-frame tile, or (Q = 1, the sequential roll-off walk) four
// neighbouring tiles, whose 256-byte row pieces are then one contiguous run per row and workgroup (0.46 -> 0.38 ms at
// C2; sixteen-wave workgroups of 4 tiles x 4 ranges measured slower for the other three features).
template <int Q> constexpr int tiles_of = Q == 1 ? 4 : 1;
template <typename T, int FEATURE, int Q>
__global__ void __launch_bounds__(64 * Q * tiles_of<Q>) spectral_kernel(SpectralArgs a) {
  constexpr int kTiles = tiles_of<Q>;
  __shared__ double red_all[kTiles][2][Q][64];
  const int fx = threadIdx.x & 63, q = (threadIdx.x >> 6) % Q, sub = threadIdx.x / (64 * Q);
  double (*red)[Q][64] = red_all[sub];
  const int64_t groups = (a.ftiles + kTiles - 1) / kTiles;
  const int64_t clip = blockIdx.x / groups, tile = (blockIdx.x % groups) * kTiles + sub;
  const int64_t t = tile * 64 + fx;                    // a tile past the last one shadows the last frame too
  const bool live = t < a.frames;
  const int64_t tc = live ? t : a.frames - 1;          // idle lanes shadow the last frame (no stores)
  const T *col = reinterpret_cast<const T *>(a.s) + clip * a.bins * a.frames + tc;
  const int64_t bq = (a.bins + Q - 1) / Q;
  const int64_t k0 = q * bq, k1 = (k0 + bq < a.bins) ? k0 + bq : a.bins;
  auto fq = [&](int64_t k) { return a.freqs ? a.freqs[k] : (double)k * a.step; };
  // partial sums of the Q waves meet in a fixed order
  auto combine = [&](double v, int slot) {
    if constexpr (Q == 1) return v;
    red[slot][q][fx] = v;
    __syncthreads();
    const double r = (red[slot][0][fx] + red[slot][1][fx]) + (red[slot][2][fx] + red[slot][3][fx]);
    __syncthreads();
    return r;
  };
  bool bad = false;
  double result = 0.0;

  if constexpr (FEATURE == SPECTRAL_FLATNESS) {
    // sum of logs as the log of a product: mantissas multiply (renormalised every 8 factors, so the product stays
    // above 2^-9), exponents add as integers; one log per wave instead of one per bin (the float64 log was what this
    // feature spent its time on: 246 M of them at C2).  Same value to a few ulp of the float64 sum.
    double prod = 1.0, sa = 0.0;
    int64_t esum = 0;
    for_bins(col, a.frames, k0, k1, [&](int64_t k, double v) {
      bad |= !(v >= 0.0);
      const double pw = pow_fixed(v, a.power);
      const double f = pw > a.p ? pw : a.p;            // a.p = amin > 0
      sa += f;
      if (f < INFINITY) {
        prod *= __builtin_amdgcn_frexp_mant(f);
        esum += __builtin_amdgcn_frexp_exp(f);
      } else {
        prod = f;                                       // an infinite (or NaN) bin: the sum of logs is that too
      }
      if (((k - k0) & 7) == 7) {                        // wave-uniform
        if (prod < INFINITY) {
          esum += __builtin_amdgcn_frexp_exp(prod);
          prod = __builtin_amdgcn_frexp_mant(prod);
        }
      }
    });
    double sl = log(prod) + (double)esum * 0.693147180559945309417232121458;
    sl = combine(sl, 0);
    sa = combine(sa, 1);
    result = exp(sl / (double)a.bins) / (sa / (double)a.bins);
  } else if constexpr (FEATURE == SPECTRAL_ROLLOFF) {
    double cum = 0.0;
    for_bins(col, a.frames, 0, a.bins, [&](int64_t, double v) {
      bad |= !(v >= 0.0);
      cum += v;
    });
    const double threshold = cum * a.p;                // a.p = roll_percent; the total is the last cumulative value
    cum = 0.0;
    double best = INFINITY;
    for_bins(col, a.frames, 0, a.bins, [&](int64_t k, double v) {
      cum += v;
      const double f = fq(k);
      best = (cum >= threshold && f < best) ? f : best;
    });
    result = best;
  } else {
    // one walk gives the frame's sum and its first moment: sum(f_k (v_k / len)) is evaluated as sum(f_k v_k) / len, the
    // same value to a rounding of the float64 interior (the reference normalises first: spectral.ml:155-163, 171-196)
    // float32 spectrograms only: with float64 input f_k v_k can overflow where f_k (v_k / len) does not, so that dtype
    // keeps the reference's order and its extra walk
    constexpr bool kFused = sizeof(T) == 4;
    double len = 0.0, m1 = 0.0;
    const bool need_c = !(FEATURE == SPECTRAL_BANDWIDTH && a.centroid);
    for_bins(col, a.frames, k0, k1, [&](int64_t k, double v) {
      bad |= !(v >= 0.0);
      len += v;
      if (kFused && need_c) m1 += fq(k) * v;
    });
    len = combine(len, 0);
    const double safe = len < DBL_MIN ? 1.0 : len;     // spectral.ml:155-163
    double c64;
    if (!need_c) {
      c64 = (double)reinterpret_cast<const T *>(a.centroid)[clip * a.frames + tc];
    } else if constexpr (kFused) {
      c64 = combine(m1, 1) / safe;
    } else {
      for_bins(col, a.frames, k0, k1, [&](int64_t k, double v) { m1 += fq(k) * (v / safe); });
      c64 = combine(m1, 1);
    }
    if constexpr (FEATURE == SPECTRAL_CENTROID) {
      result = c64;
    } else {
      double w = 0.0;
      for_bins(col, a.frames, k0, k1, [&](int64_t k, double v) {
        const double deviation = fabs(c64 - fq(k));
        w += (kFused ? v : v / safe) * pow_fixed(deviation, a.p);
      });
      w = combine(w, 0);
      if (kFused) w /= safe;
      result = a.p == 2.0 ? sqrt(w) : (a.p == 1.0 ? w : pow(w, a.inv_p));
    }
  }
  if (bad && live) atomicOr(a.invalid, 1);
  if (live && q == 0) reinterpret_cast<T *>(a.out)[clip * a.frames + t] = (T)result;
}

template <typename T, int FEATURE, int Q>
void launch_feature(const SpectralArgs &whole, hipStream_t stream) {
  constexpr int kTiles = tiles_of<Q>, kThreads = 64 * Q * kTiles;
  const int64_t groups = (whole.ftiles + kTiles - 1) / kTiles;
  const int64_t per_launch = std::max<int64_t>(1, clips_per_launch(groups, kThreads));   // clip range by clip range (DESIGN.md "Launch extents")
  for (int64_t c0 = 0; c0 < whole.lead; c0 += per_launch) {
    SpectralArgs a = whole;
    a.lead = std::min(per_launch, whole.lead - c0);
    a.s = reinterpret_cast<const T *>(whole.s) + c0 * whole.bins * whole.frames;
    a.out = reinterpret_cast<T *>(whole.out) + c0 * whole.frames;
    if (whole.centroid) a.centroid = reinterpret_cast<const T *>(whole.centroid) + c0 * whole.frames;
    SMX_LAUNCH((spectral_kernel<T, FEATURE, Q>), dim3(grid_x("spectral", "frame tiles", a.lead * groups, kThreads)), dim3(kThreads), 0, stream, a);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

template <typename T>
void dispatch_feature(int feature, const SpectralArgs &a, hipStream_t stream) {
  switch (feature) {
    case SPECTRAL_CENTROID: launch_feature<T, SPECTRAL_CENTROID, 4>(a, stream); break;
    case SPECTRAL_BANDWIDTH: launch_feature<T, SPECTRAL_BANDWIDTH, 4>(a, stream); break;
    case SPECTRAL_ROLLOFF: launch_feature<T, SPECTRAL_ROLLOFF, 1>(a, stream); break;
    case SPECTRAL_FLATNESS: launch_feature<T, SPECTRAL_FLATNESS, 4>(a, stream); break;
    default: throw Failure("spectral: unknown feature");
  }
}

// ---- chroma ------------------------------------------------------------------------------------------------
constexpr int kChromaChunk = 12;   // chroma rows accumulated per pass over the bins

struct ChromaArgs {
  const void *s;            // [lead; bins; frames]
  double *raw;              // [lead; n_chroma; frames] float64 scratch
  const double *wt;         // [bins; rows_pad], rows_pad = n_chroma rounded up to a multiple of kChromaChunk
  int64_t rows_pad;
  void *out;                // [lead; n_chroma; frames]
  int64_t lead, bins, frames, ftiles;
  int n_chroma, norm;
  double norm_p, inv_p, tiny;
};

template <typename T>
__global__ void __launch_bounds__(256) chroma_project_kernel(ChromaArgs a) {
  const int64_t clip = blockIdx.x / a.ftiles, tile = blockIdx.x % a.ftiles;
  const int64_t t = tile * 256 + threadIdx.x;
  if (t >= a.frames) return;
  const int c0 = blockIdx.y * kChromaChunk;
  const T *col = reinterpret_cast<const T *>(a.s) + clip * a.bins * a.frames + t;
  const double *wt = a.wt + c0;                        // rows padded with zeros to a whole chunk: no guards below
  double acc[kChromaChunk];
#pragma unroll
  for (int i = 0; i < kChromaChunk; ++i) acc[i] = 0.0;
  int64_t k = 0;
  for (; k + kDepth <= a.bins; k += kDepth) {
    T v[kDepth];
#pragma unroll
    for (int j = 0; j < kDepth; ++j) v[j] = col[(k + j) * a.frames];
#pragma unroll
    for (int j = 0; j < kDepth; ++j) {
      const double *w = wt + (k + j) * a.rows_pad;     // uniform: scalar loads
      const double d = (double)v[j];
#pragma unroll
      for (int i = 0; i < kChromaChunk; ++i) acc[i] += w[i] * d;
    }
  }
  for (; k < a.bins; ++k) {
    const double *w = wt + k * a.rows_pad;
    const double d = (double)col[k * a.frames];
#pragma unroll
    for (int i = 0; i < kChromaChunk; ++i) acc[i] += w[i] * d;
  }
  double *raw = a.raw + (clip * a.n_chroma + c0) * a.frames + t;
#pragma unroll
  for (int i = 0; i < kChromaChunk; ++i)
    if (c0 + i < a.n_chroma) raw[(int64_t)i * a.frames] = acc[i];
}

// chroma.ml:58-88: each frame divided by its own length in the norm; lengths below `tiny` divide by one
template <typename T>
__global__ void __launch_bounds__(256) chroma_normalise_kernel(ChromaArgs a) {
  const int64_t clip = blockIdx.x / a.ftiles, tile = blockIdx.x % a.ftiles;
  const int64_t t = tile * 256 + threadIdx.x;
  if (t >= a.frames) return;
  const double *raw = a.raw + clip * a.n_chroma * a.frames + t;
  T *out = reinterpret_cast<T *>(a.out) + clip * a.n_chroma * a.frames + t;
  double length = 1.0;
  if (a.norm != SMX_CHROMA_NORM_NONE) {
    double acc = 0.0;
    for (int c = 0; c < a.n_chroma; ++c) {
      const double m = fabs(raw[(int64_t)c * a.frames]);
      if (a.norm == SMX_CHROMA_NORM_INF) acc = m > acc ? m : acc;
      else acc += pow_fixed(m, a.norm_p);
    }
    if (a.norm == SMX_CHROMA_NORM_P && a.norm_p != 1.0) acc = a.norm_p == 2.0 ? sqrt(acc) : pow(acc, a.inv_p);
    length = acc < a.tiny ? 1.0 : acc;
  }
  for (int c = 0; c < a.n_chroma; ++c) {
    const double v = raw[(int64_t)c * a.frames];
    out[(int64_t)c * a.frames] = (T)(a.norm == SMX_CHROMA_NORM_NONE ? v : v / length);
  }
}

}  // namespace

bool launch_spectral(const SpectralJob &job) {
  if (job.lead <= 0 || job.bins <= 0 || job.frames <= 0) return true;
  SpectralArgs a{};
  a.s = job.s;
  a.out = job.out;
  a.centroid = job.centroid;
  a.step = job.step;
  a.p = job.p;
  a.inv_p = 1.0 / job.p;
  a.power = job.power;
  a.lead = job.lead;
  a.bins = job.bins;
  a.frames = job.frames;
  a.ftiles = (job.frames + 63) / 64;
  // scratch: the invalid-entry flag, then the caller's frequency grid
  const size_t grid_bytes = job.freqs ? (size_t)job.bins * sizeof(double) : 0;
  unsigned char *scratch = nullptr;
  SMX_HIP_CHECK(smx::pool_malloc_async((void **)&scratch, 16 + grid_bytes, job.stream));
  a.invalid = reinterpret_cast<int *>(scratch);
  SMX_HIP_CHECK(hipMemsetAsync(scratch, 0, 16, job.stream));
  if (job.freqs) {
    a.freqs = reinterpret_cast<const double *>(scratch + 16);
    SMX_HIP_CHECK(hipMemcpyAsync(scratch + 16, job.freqs, grid_bytes, hipMemcpyHostToDevice, job.stream));
    SMX_HIP_CHECK(hipStreamSynchronize(job.stream));   // the grid is the caller's pageable memory
  }
  if (job.elem_bytes == 8) dispatch_feature<double>(job.feature, a, job.stream);
  else dispatch_feature<float>(job.feature, a, job.stream);
  int invalid = 0;
  SMX_HIP_CHECK(hipMemcpyAsync(&invalid, a.invalid, sizeof(int), hipMemcpyDeviceToHost, job.stream));
  SMX_HIP_CHECK(smx::pool_free_async(scratch, job.stream));   // behind the copy and before the wait: the stream is idle when the verdict is in
  SMX_HIP_CHECK(hipStreamSynchronize(job.stream));
  return invalid == 0;
}

void launch_chroma(const ChromaJob &job) {
  if (job.lead <= 0 || job.frames <= 0) return;
  const int64_t n_chroma = job.config ? job.config->n_chroma : job.n_chroma;
  ChromaArgs a{};
  a.s = job.s;
  a.out = job.out;
  a.wt = job.config ? job.config->device_weights() : job.weights_t;
  a.lead = job.lead;
  a.bins = job.config ? job.config->bins() : job.bins;
  a.frames = job.frames;
  a.ftiles = (job.frames + 255) / 256;
  a.n_chroma = (int)n_chroma;
  a.rows_pad = (n_chroma + kChromaChunk - 1) / kChromaChunk * kChromaChunk;
  a.norm = job.norm;
  a.norm_p = job.norm_p;
  a.inv_p = job.norm == SMX_CHROMA_NORM_P ? 1.0 / job.norm_p : 1.0;
  a.tiny = job.elem_bytes == 8 ? DBL_MIN : (double)FLT_MIN;   // chroma.ml:42-55 smallest_normal
  const int64_t chunks = (n_chroma + kChromaChunk - 1) / kChromaChunk;
  if (chunks > kMaxGridYZ) throw Failure("chroma: too many tiles for one launch");
  const unsigned blocks = grid_x("chroma", "tiles", a.lead * a.ftiles, 256);
  SMX_HIP_CHECK(smx::pool_malloc_async((void **)&a.raw, (size_t)job.lead * (size_t)n_chroma * (size_t)job.frames * sizeof(double),
                               job.stream));
  if (job.elem_bytes == 8) {
    SMX_LAUNCH(chroma_project_kernel<double>, dim3(blocks, (unsigned)chunks), dim3(256), 0, job.stream, a);
    SMX_LAUNCH(chroma_normalise_kernel<double>, dim3(blocks), dim3(256), 0, job.stream, a);
  } else {
    SMX_LAUNCH(chroma_project_kernel<float>, dim3(blocks, (unsigned)chunks), dim3(256), 0, job.stream, a);
    SMX_LAUNCH(chroma_normalise_kernel<float>, dim3(blocks), dim3(256), 0, job.stream, a);
  }
  SMX_HIP_CHECK(hipGetLastError());
  SMX_HIP_CHECK(smx::pool_free_async(a.raw, job.stream));
}

}  // namespace smx

// ---- the C ABI's side: Spectral.*, Chroma.apply, Soundml.chroma_stft -------------------------------------------------------
namespace smx {
namespace {

// ---- Spectral.* (spectral.ml:27-255): checks in the reference's order and words, then one launch -------------
const char *spectral_op(int feature) {
  switch (feature) {
    case SPECTRAL_CENTROID: return "spectral_centroid";
    case SPECTRAL_BANDWIDTH: return "spectral_bandwidth";
    case SPECTRAL_ROLLOFF: return "spectral_rolloff";
    default: return "spectral_flatness";
  }
}

struct SpectralParams {
  int feature = SPECTRAL_CENTROID;
  double p = 2.0, power = 2.0;          // p: bandwidth exponent | roll_percent | amin
  const double *freqs = nullptr;        // host
  int64_t n_freqs = 0, sample_rate = 0;
  bool has_centroid = false;
  int64_t c_rows = 0, c_frames = 0;
};

// everything that does not read the data; returns the FFT-grid step (0 with a custom grid)
double check_spectral(const SpectralParams &q, int64_t lead, int64_t bins, int64_t frames) {
  const char *op = spectral_op(q.feature);
  if (lead < 0 || bins < 0 || frames < 0)
    throw Failure(format("%s: negative extent (lead %lld, bins %lld, frames %lld)", op, (long long)lead,
                         (long long)bins, (long long)frames));
  if (q.feature == SPECTRAL_BANDWIDTH && !(std::isfinite(q.p) && q.p > 0.0))
    throw InvalidArgument(format("%s: cannot raise deviations to the power %g (p must be finite and positive)", op, q.p));
  if (q.feature == SPECTRAL_ROLLOFF && !(q.p > 0.0 && q.p < 1.0))
    throw InvalidArgument(format(
        "%s: cannot keep %g of the spectral energy (roll_percent must lie strictly between 0 and 1)", op, q.p));
  double step = 0.0;
  if (q.feature == SPECTRAL_FLATNESS) {
    if (!(std::isfinite(q.p) && q.p > 0.0))
      throw InvalidArgument(format("%s: cannot floor the spectrum at %g (amin must be finite and positive)", op, q.p));
    if (!(std::isfinite(q.power) && q.power > 0.0))
      throw InvalidArgument(format(
          "%s: cannot raise magnitudes to the power %g (power must be finite and positive)", op, q.power));
    return step;
  }
  // grid (spectral.ml:105-136)
  if (q.sample_rate < 1)
    throw InvalidArgument(format("%s: cannot use a sample rate of %lld Hz (sample_rate must be at least 1)", op,
                                 (long long)q.sample_rate));
  if (q.freqs) {
    if (q.n_freqs != bins)
      throw InvalidArgument(format(
          "%s: cannot pair %lld bin frequencies with %lld bins (freqs holds one frequency per bin)", op,
          (long long)q.n_freqs, (long long)bins));
  } else {
    if (bins < 2)
      throw InvalidArgument(format(
          "%s: cannot derive bin frequencies for a %lld-bin spectrogram (the implied FFT size is %lld; pass "
          "freqs explicitly)", op, (long long)bins, (long long)(2 * (bins - 1))));
    const int64_t fft_size = 2 * (bins - 1);
    step = 1.0 / ((double)fft_size * (1.0 / (double)q.sample_rate));
  }
  if (q.feature == SPECTRAL_BANDWIDTH && q.has_centroid && (q.c_rows != 1 || q.c_frames != frames))
    throw InvalidArgument(format(
        "%s: cannot reuse a centroid with %lld rows over %lld frames for a %lld-frame spectrogram (centroid must "
        "be [...; 1; frames], one frequency per frame)", op, (long long)q.c_rows, (long long)q.c_frames,
        (long long)frames));
  return step;
}

SpectralParams spectral_params(int feature, double p, double power, const double *freqs, int64_t n_freqs, int64_t sample_rate,
                               const void *centroid, int64_t c_rows, int64_t c_frames) {
  SpectralParams q;
  q.feature = feature;
  q.p = p;
  q.power = power;
  q.freqs = freqs;
  q.n_freqs = n_freqs;
  q.sample_rate = sample_rate;
  q.has_centroid = centroid != nullptr;
  q.c_rows = c_rows;
  q.c_frames = c_frames;
  return q;
}

void spectral_dev(const SpectralParams &q, const void *d_s, int elem_bytes, int64_t lead, int64_t bins,
                  int64_t frames, const void *d_centroid, void *d_out, hipStream_t stream) {
  const double step = check_spectral(q, lead, bins, frames);
  if (lead == 0 || bins == 0 || frames == 0) return;   // empty_feature: all zero by contract, nothing to reduce
  if (!d_s || !d_out) throw Failure(format("%s: null device pointer", spectral_op(q.feature)));
  SpectralJob job;
  job.feature = q.feature;
  job.s = d_s;
  job.elem_bytes = elem_bytes;
  job.lead = lead;
  job.bins = bins;
  job.frames = frames;
  job.freqs = q.freqs;
  job.step = step;
  job.p = q.p;
  job.power = q.power;
  job.centroid = q.has_centroid ? d_centroid : nullptr;
  job.out = d_out;
  job.stream = stream;
  if (!launch_spectral(job))
    throw InvalidArgument(format(
        "%s: cannot analyse a spectrogram with negative or NaN values (a magnitude spectrogram is non-negative)",
        spectral_op(q.feature)));
}

void spectral_host(const SpectralParams &q, const void *s, int elem_bytes, int64_t lead, int64_t bins,
                   int64_t frames, const void *centroid, void *out) {
  check_spectral(q, lead, bins, frames);
  if (lead == 0 || bins == 0 || frames == 0) return;
  if (!s || !out) throw Failure(format("%s: null pointer", spectral_op(q.feature)));
  const size_t row = (size_t)frames * (size_t)elem_bytes;
  host_call(spectral_op(q.feature), {{s, (size_t)bins * row}, {centroid, row}}, out, row, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              spectral_dev(q, d_in[0], elem_bytes, nc, bins, frames, d_in[1], d_out, stream);
            });
}

}  // namespace

// ---- Chroma.apply / Soundml.chroma_stft (chroma.ml:285-317, soundml.ml:97-107) ------------------------------
void check_chroma_norm(const char *op, int norm, double norm_p) {   // chroma.ml:30-40
  if (norm == SMX_CHROMA_NORM_NONE || norm == SMX_CHROMA_NORM_INF) return;
  if (norm != SMX_CHROMA_NORM_P) throw Failure(format("%s: unknown norm %d", op, norm));
  if (!(std::isfinite(norm_p) && norm_p > 0.0))
    throw InvalidArgument(format(
        "%s: cannot normalise in the %g-norm (the exponent must be finite and positive)", op, norm_p));
}

void chroma_apply_dev(const smx_chroma_config &c, const void *d_s, int elem_bytes, int64_t lead, int64_t bins,
                      int64_t frames, int norm, double norm_p, void *d_out, hipStream_t stream) {
  check_chroma_norm("apply", norm, norm_p);
  if (lead < 0 || bins < 0 || frames < 0)
    throw Failure(format("apply: negative extent (lead %lld, bins %lld, frames %lld)", (long long)lead,
                         (long long)bins, (long long)frames));
  if (bins != c.bins())
    throw InvalidArgument(format(
        "apply: cannot project %lld frequency bins through a matrix built for an FFT of size %lld (%lld bins)",
        (long long)bins, (long long)c.fft_size, (long long)c.bins()));
  if (lead == 0 || frames == 0) return;
  if (!d_s || !d_out) throw Failure("apply: null device pointer");
  ChromaJob job;
  job.config = &c;
  job.s = d_s;
  job.elem_bytes = elem_bytes;
  job.lead = lead;
  job.frames = frames;
  job.norm = norm;
  job.norm_p = norm_p;
  job.out = d_out;
  job.stream = stream;
  launch_chroma(job);
}

namespace {

void chroma_apply_host(const smx_chroma_config &c, const void *s, int elem_bytes, int64_t lead, int64_t bins,
                       int64_t frames, int norm, double norm_p, void *out) {
  check_chroma_norm("apply", norm, norm_p);
  if (bins != c.bins() || lead <= 0 || frames <= 0) {   // the checks and the empty case, nothing to upload
    chroma_apply_dev(c, nullptr, elem_bytes, lead, bins, frames, norm, norm_p, nullptr, nullptr);
    return;
  }
  if (!s || !out) throw Failure("apply: null pointer");
  host_call("chroma_apply", {{s, (size_t)bins * (size_t)frames * (size_t)elem_bytes}}, out,
            (size_t)c.n_chroma * (size_t)frames * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              chroma_apply_dev(c, d_in[0], elem_bytes, nc, bins, frames, norm, norm_p, d_out, stream);
            });
}

void check_chroma_stft(const smx_stft_config &sc, const smx_chroma_config &cc) {   // soundml.ml:98-106
  if (sc.fft_size != cc.fft_size)
    throw InvalidArgument(format(
        "chroma_stft: cannot project a %lld-point STFT through a filterbank built for an FFT of size %lld (the two "
        "configurations must agree on fft_size)", (long long)sc.fft_size, (long long)cc.fft_size));
}

void chroma_stft_dev(const smx_stft_config &sc, const smx_chroma_config &cc, const void *d_x, int in_bytes,
                     int64_t lead, int64_t n, int64_t x_stride, double power, int norm, double norm_p, void *d_out,
                     hipStream_t stream) {
  check_chroma_stft(sc, cc);
  check_chroma_norm("apply", norm, norm_p);
  check_rank_extents("chroma_stft", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!d_x || !d_out) throw Failure("chroma_stft: null device pointer");
  void *spec = nullptr;
  SMX_HIP_CHECK(smx::pool_malloc_async(&spec, (size_t)lead * (size_t)sc.bins() * (size_t)count * (size_t)in_bytes, stream));
  stft_range_dev(sc, d_x, in_bytes, lead, n, x_stride, 0, count, OUT_POWER, power, spec, stream);
  chroma_apply_dev(cc, spec, in_bytes, lead, sc.bins(), count, norm, norm_p, d_out, stream);
  SMX_HIP_CHECK(smx::pool_free_async(spec, stream));
}

void chroma_stft_host(const smx_stft_config &sc, const smx_chroma_config &cc, const void *x, int in_bytes,
                      int64_t lead, int64_t n, double power, int norm, double norm_p, void *out) {
  check_chroma_stft(sc, cc);
  check_chroma_norm("apply", norm, norm_p);
  check_rank_extents("chroma_stft", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure("chroma_stft: null pointer");
  host_call("chroma_stft", {{x, (size_t)n * (size_t)in_bytes}}, out, (size_t)cc.n_chroma * (size_t)count * (size_t)in_bytes, lead, false,
            nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              chroma_stft_dev(sc, cc, d_in[0], in_bytes, nc, n, n, power, norm, norm_p, d_out, stream);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Spectral.* (spectral.ml:171-255) ---------------------------------------------------------------
int smx_spectral_centroid_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, const double *freqs, int64_t n_freqs, int64_t sample_rate, float *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_CENTROID, 2.0, 2.0, freqs, n_freqs, sample_rate, nullptr, 0, 0), s, 4, lead, bins, frames, nullptr, out); });
}
int smx_spectral_centroid_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, const double *freqs, int64_t n_freqs, int64_t sample_rate, double *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_CENTROID, 2.0, 2.0, freqs, n_freqs, sample_rate, nullptr, 0, 0), s, 8, lead, bins, frames, nullptr, out); });
}
int smx_spectral_centroid_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, const double *freqs, int64_t n_freqs, int64_t sample_rate, float *d_out, void *stream) {
  return guarded([&] { spectral_dev(spectral_params(SPECTRAL_CENTROID, 2.0, 2.0, freqs, n_freqs, sample_rate, nullptr, 0, 0), d_s, 4, lead, bins, frames, nullptr, d_out, (hipStream_t)stream); });
}
int smx_spectral_bandwidth_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, double p, const double *freqs, int64_t n_freqs, const float *centroid, int64_t c_rows, int64_t c_frames, int64_t sample_rate, float *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_BANDWIDTH, p, 2.0, freqs, n_freqs, sample_rate, centroid, c_rows, c_frames), s, 4, lead, bins, frames, centroid, out); });
}
int smx_spectral_bandwidth_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, double p, const double *freqs, int64_t n_freqs, const double *centroid, int64_t c_rows, int64_t c_frames, int64_t sample_rate, double *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_BANDWIDTH, p, 2.0, freqs, n_freqs, sample_rate, centroid, c_rows, c_frames), s, 8, lead, bins, frames, centroid, out); });
}
int smx_spectral_bandwidth_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, double p, const double *freqs, int64_t n_freqs, const float *d_centroid, int64_t c_rows, int64_t c_frames, int64_t sample_rate, float *d_out, void *stream) {
  return guarded([&] { spectral_dev(spectral_params(SPECTRAL_BANDWIDTH, p, 2.0, freqs, n_freqs, sample_rate, d_centroid, c_rows, c_frames), d_s, 4, lead, bins, frames, d_centroid, d_out, (hipStream_t)stream); });
}
int smx_spectral_rolloff_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, double roll_percent, const double *freqs, int64_t n_freqs, int64_t sample_rate, float *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_ROLLOFF, roll_percent, 2.0, freqs, n_freqs, sample_rate, nullptr, 0, 0), s, 4, lead, bins, frames, nullptr, out); });
}
int smx_spectral_rolloff_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, double roll_percent, const double *freqs, int64_t n_freqs, int64_t sample_rate, double *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_ROLLOFF, roll_percent, 2.0, freqs, n_freqs, sample_rate, nullptr, 0, 0), s, 8, lead, bins, frames, nullptr, out); });
}
int smx_spectral_rolloff_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, double roll_percent, const double *freqs, int64_t n_freqs, int64_t sample_rate, float *d_out, void *stream) {
  return guarded([&] { spectral_dev(spectral_params(SPECTRAL_ROLLOFF, roll_percent, 2.0, freqs, n_freqs, sample_rate, nullptr, 0, 0), d_s, 4, lead, bins, frames, nullptr, d_out, (hipStream_t)stream); });
}
int smx_spectral_flatness_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, double amin, double power, float *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_FLATNESS, amin, power, nullptr, 0, 0, nullptr, 0, 0), s, 4, lead, bins, frames, nullptr, out); });
}
int smx_spectral_flatness_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, double amin, double power, double *out) {
  return guarded([&] { spectral_host(spectral_params(SPECTRAL_FLATNESS, amin, power, nullptr, 0, 0, nullptr, 0, 0), s, 8, lead, bins, frames, nullptr, out); });
}
int smx_spectral_flatness_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, double amin, double power, float *d_out, void *stream) {
  return guarded([&] { spectral_dev(spectral_params(SPECTRAL_FLATNESS, amin, power, nullptr, 0, 0, nullptr, 0, 0), d_s, 4, lead, bins, frames, nullptr, d_out, (hipStream_t)stream); });
}

// ---- Chroma (chroma.ml:95-317, soundml.ml:97-107) ---------------------------------------------------
int smx_chroma_config_create(int64_t n_chroma, double tuning, double ctroct, int has_octwidth, double octwidth,
                             int base_c, int64_t sample_rate, int64_t fft_size, smx_chroma_config **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null output handle");
    *out = chroma_config_create(n_chroma, tuning, ctroct, has_octwidth != 0, octwidth, base_c != 0, sample_rate, fft_size);
  });
}
void smx_chroma_config_destroy(smx_chroma_config *c) { delete c; }
int64_t smx_chroma_config_n_chroma(const smx_chroma_config *c) { return c ? c->n_chroma : -1; }
int64_t smx_chroma_config_bins(const smx_chroma_config *c) { return c ? c->bins() : -1; }
int64_t smx_chroma_config_fft_size(const smx_chroma_config *c) { return c ? c->fft_size : -1; }
int smx_chroma_filterbank(const smx_chroma_config *c, double *out) {
  return guarded([&] {
    check_config(c, "filterbank");
    if (!out) throw Failure("filterbank: null pointer");
    std::memcpy(out, c->weights.data(), c->weights.size() * sizeof(double));
  });
}
int smx_chroma_apply_f32(const smx_chroma_config *c, const float *s, int64_t lead, int64_t bins, int64_t frames,
                         int norm, double norm_p, float *out) {
  return guarded([&] {
    check_config(c, "apply");
    chroma_apply_host(*c, s, 4, lead, bins, frames, norm, norm_p, out);
  });
}
int smx_chroma_apply_f64(const smx_chroma_config *c, const double *s, int64_t lead, int64_t bins, int64_t frames,
                         int norm, double norm_p, double *out) {
  return guarded([&] {
    check_config(c, "apply");
    chroma_apply_host(*c, s, 8, lead, bins, frames, norm, norm_p, out);
  });
}
int smx_chroma_apply_f32_dev(const smx_chroma_config *c, const float *d_s, int64_t lead, int64_t bins,
                             int64_t frames, int norm, double norm_p, float *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "apply");
    chroma_apply_dev(*c, d_s, 4, lead, bins, frames, norm, norm_p, d_out, (hipStream_t)stream);
  });
}
int smx_chroma_stft_f32(const smx_stft_config *sc, const smx_chroma_config *cc, const float *x, int64_t lead,
                        int64_t n, double power, int norm, double norm_p, float *out) {
  return guarded([&] {
    check_config(sc, "chroma_stft");
    check_config(cc, "chroma_stft");
    chroma_stft_host(*sc, *cc, x, 4, lead, n, power, norm, norm_p, out);
  });
}
int smx_chroma_stft_f64(const smx_stft_config *sc, const smx_chroma_config *cc, const double *x, int64_t lead,
                        int64_t n, double power, int norm, double norm_p, double *out) {
  return guarded([&] {
    check_config(sc, "chroma_stft");
    check_config(cc, "chroma_stft");
    chroma_stft_host(*sc, *cc, x, 8, lead, n, power, norm, norm_p, out);
  });
}
int smx_chroma_stft_f32_dev(const smx_stft_config *sc, const smx_chroma_config *cc, const float *d_x,
                            int64_t lead, int64_t n, int64_t x_stride, double power, int norm, double norm_p,
                            float *d_out, void *stream) {
  return guarded([&] {
    check_config(sc, "chroma_stft");
    check_config(cc, "chroma_stft");
    chroma_stft_dev(*sc, *cc, d_x, 4, lead, n, x_stride, power, norm, norm_p, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
