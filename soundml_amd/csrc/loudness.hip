// Programme loudness and true peak (ITU-R BS.1770-4, EBU Tech 3341; not in the reference) over device-resident audio
// [clips; channels; n], time fastest.  DESIGN.md 4.8l states every order once; this file is built with -ffp-contract=off, so every
// product and every sum below rounds on its own.
//
// K-weighting is the two-section cascade of BS.1770 run by Iir's stated order (4.8k): blocks of B = 256 samples counted from the
// first sample of the call (of the stream since reset), the state entering a block from the chain s_{b+1} = M s_b + w_b, the
// weighted samples y of block b the serial cascade from s_b, float64, never rounded and never stored.  The gating grid is counted
// from the same sample: steps of `step` = (rate + 5) / 10 samples, blocks of four steps.  A PIECE is the intersection of an Iir
// block with a step (step >= 800 > B: a block holds one or two); its sum is acc = acc + y y over its samples ascending from 0.
// A step's energy is the sum of its pieces ascending from 0, kept per channel in a buffer of step energies; whichever kernel
// closes a piece adds it there, and the launches follow one another on the stream, so the order is the same on every route.
//
//   the block route        Iir's zero-state pass and chain (iir_block_states) leave s_b in scratch; then
//     loud_block_e_kernel  a wave owns kSpanBlocks blocks of one channel staged through LDS as Iir's y pass stages them; lane l
//                          reruns block l from s_b and, instead of storing y, sums y y into the block's one or two pieces
//     loud_step_add_kernel a lane per (channel, step): the pieces of the step among the blocks just run, ascending, onto the buffer
//   loud_general_kernel    a lane per channel walks samples serially from the records (Iir's 6 S doubles and the open piece's
//                          partial sum): heads up to a block edge, tails, streams, SMX_DISABLE_FAST=1
//   loud_combine_kernel    window sums of step energies (4: a gating block, 30: short-term) ascending, times 1 / samples, then the
//                          channel sum e = (G_0 z_0 + G_1 z_1) + ... ascending; -0.691 + 10 log10 e where asked
//   loud_gate_kernel       a wave per clip, two ascending passes over e: the absolute gate, then the relative one
//   loud_peak_kernel       4x oversampling by the 49-tap Kaiser sinc, a span and 12 samples of history in LDS, max |y| per channel
//                          by an integer atomic max on the bits of the non-negative result (order-independent)
//   loud_gain_kernel / loud_scale_kernel   normalize: one float64 gain per clip, applied with one rounding
#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kBlock = kIirBlock, kSpanBlocks = kIirSpanBlocks;
constexpr int kS = 2, kN = 2 * kS;           // the shelf and the high-pass
constexpr int kPhase = 32, kLogPhase = 5;    // samples of every block of the span that lie in LDS at a time
constexpr int kPitch = kPhase + 1;           // LDS row pitch in elements: odd, the lanes' walks hit distinct banks
constexpr int kAhead = 8;
constexpr int kMaxChannels = 32;
constexpr int64_t kMinRate = 8000;
constexpr int kTaps = 49, kHist = 12;        // y[4 i + p] reads x[i - 12 .. i]
constexpr int kPeakThreads = 256, kPeakSpan = 4 * kPeakThreads;   // a lane owns four consecutive samples

struct Weights {
  double g[kMaxChannels];
};
struct Taps {
  double h[kTaps];
};

// ---- the weighted energy ------------------------------------------------------------------------------------------------------
// a lane per row: samples [i0, i1) of the call, the first of them `gpos` samples into the stream
template <typename X>
__global__ void __launch_bounds__(64) loud_general_kernel(IirCoef k, const X *x, int64_t x_stride, const double *M, double *iir, double *part,
                                                          double *steps, int64_t cap, int64_t rows, int64_t i0, int64_t i1, int64_t gpos, int64_t step) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= rows) return;
  double s[kN], w[kN], r[kN];
  double *rec = iir + c * 3 * kN;
#pragma unroll
  for (int i = 0; i < kN; ++i) s[i] = rec[i], w[i] = rec[kN + i], r[i] = rec[2 * kN + i];
  double acc = part[c];
  int pos = (int)(gpos % kBlock);
  int64_t sp = gpos % step, at = gpos / step;
  const X *row = x + c * x_stride;
  double *mine = steps + c * cap;
  for (int64_t t = i0; t < i1; ++t) {
    const double u = (double)row[t];
    const double y = iir_cascade<kS>(k, u, r);
    (void)iir_cascade<kS>(k, u, w);
    acc = acc + y * y;
    const bool block_edge = ++pos == kBlock, step_edge = ++sp == step;
    if (block_edge) {
      double next[kN];
#pragma unroll
      for (int i = 0; i < kN; ++i) {
        double a = M[i * kN] * s[0];
#pragma unroll
        for (int j = 1; j < kN; ++j) a = a + M[i * kN + j] * s[j];
        next[i] = a + w[i];
      }
#pragma unroll
      for (int i = 0; i < kN; ++i) s[i] = next[i], r[i] = next[i], w[i] = 0.0;
      pos = 0;
    }
    if (block_edge || step_edge) {   // the piece closes
      mine[at] = mine[at] + acc;
      acc = 0.0;
    }
    if (step_edge) sp = 0, ++at;
  }
#pragma unroll
  for (int i = 0; i < kN; ++i) rec[i] = s[i], rec[kN + i] = w[i], rec[2 * kN + i] = r[i];
  part[c] = acc;
}

// positions [ph kPhase, (ph + 1) kPhase) of the nblk blocks that start at sample i0 of the row into the wave's LDS rows
template <typename X>
__device__ __forceinline__ void stage_phase(const X *row, int64_t i0, int nblk, int ph, X *rows) {
  const int lane = threadIdx.x, count = nblk * kPhase;
  X v[kPhase];
#pragma unroll
  for (int u = 0; u < kPhase; ++u) {   // every lane loads, past the end the last valid sample again: the loads stay in flight together
    const int e = u * 64 + lane < count ? u * 64 + lane : count - 1;
    v[u] = row[i0 + (int64_t)(e >> kLogPhase) * kBlock + ph * kPhase + (e & (kPhase - 1))];
  }
#pragma unroll
  for (int u = 0; u < kPhase; ++u) {
    const int e = u * 64 + lane;
    if (e < count) rows[(e >> kLogPhase) * kPitch + (e & (kPhase - 1))] = v[u];
  }
}

// pieces [rows; nb; 2]: the sum of y y over the samples of block b before its step edge (all of them where it has none), and behind it
template <typename X>
__global__ void __launch_bounds__(64) loud_block_e_kernel(IirCoef k, const X *x, int64_t x_stride, int64_t first, int64_t nb, int64_t spans,
                                                          const double *ws, int64_t g0, int64_t step, double *pieces) {
  extern __shared__ __align__(16) unsigned char loud_lds[];
  X *rows = reinterpret_cast<X *>(loud_lds);
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x / spans, b0 = (blockIdx.x % spans) * kSpanBlocks;
  const int nblk = (int)(nb - b0 < kSpanBlocks ? nb - b0 : kSpanBlocks);
  const X *mine = rows + lane * kPitch;
  const double *s = ws + (c * nb + b0 + (lane < nblk ? lane : 0)) * kN;
  double z[kN];
#pragma unroll
  for (int i = 0; i < kN; ++i) z[i] = s[i];
  // the block's first `cut` samples belong to the step its first sample lies in
  const int64_t gs = g0 + (b0 + lane) * kBlock, to_edge = (gs / step + 1) * step - gs;
  const int cut = to_edge < kBlock ? (int)to_edge : kBlock;
  double before = 0.0, behind = 0.0;
  for (int ph = 0; ph < kBlock / kPhase; ++ph) {
    if (ph) __syncthreads();
    stage_phase<X>(x + c * x_stride, first + b0 * kBlock, nblk, ph, rows);
    __syncthreads();
    if (lane < nblk) {
      for (int t = 0; t < kPhase; t += kAhead) {
        X v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = mine[t + u];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const double y = iir_cascade<kS>(k, (double)v[u], z);
          const double yy = y * y;
          const bool head = ph * kPhase + t + u < cut;   // a sum that gets +0.0 keeps its bits: squares are not negative
          before = before + (head ? yy : 0.0);
          behind = behind + (head ? 0.0 : yy);
        }
      }
    }
  }
  if (lane >= nblk) return;
  double *p = pieces + (c * nb + b0 + lane) * 2;
  p[0] = before, p[1] = behind;
}

// a lane per (row, step at0 + i): the pieces that the nb blocks from stream position g0 on hold of that step, ascending, onto steps
__global__ void __launch_bounds__(256) loud_step_add_kernel(const double *pieces, int64_t nb, int64_t g0, int64_t step, int64_t at0, int64_t count,
                                                            double *steps, int64_t cap, int64_t rows) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, c = idx / count;
  if (c >= rows) return;
  const int64_t at = at0 + idx % count, g1 = g0 + nb * kBlock;
  const int64_t lo = at * step > g0 ? at * step : g0, hi = (at + 1) * step < g1 ? (at + 1) * step : g1;
  if (lo >= hi) return;
  double acc = steps[c * cap + at];
  for (int64_t b = (lo - g0) / kBlock; b <= (hi - 1 - g0) / kBlock; ++b) {
    const int64_t gs = g0 + b * kBlock;
    acc = acc + pieces[(c * nb + b) * 2 + (gs / step == at ? 0 : 1)];
  }
  steps[c * cap + at] = acc;
}

// blocks [j0, j0 + count) of `window` steps each: z[c, j] = (((E[j] + E[j+1]) + ...) inv, e[j] = (G_0 z[0, j] + G_1 z[1, j]) + ...
template <typename O>
__global__ void __launch_bounds__(256) loud_combine_kernel(const double *steps, int64_t cap, int64_t clips, int channels, int64_t j0, int64_t count,
                                                           int window, double inv, Weights g, double *z_out, double *e_out, O *lufs_out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, clip = idx / count;
  if (clip >= clips) return;
  const int64_t j = idx % count;
  double e = 0.0;
  for (int c = 0; c < channels; ++c) {
    const double *s = steps + (clip * channels + c) * cap + j0 + j;
    double acc = s[0];
    for (int i = 1; i < window; ++i) acc = acc + s[i];
    const double z = acc * inv;
    if (z_out) z_out[(clip * channels + c) * count + j] = z;
    const double t = g.g[c] * z;
    e = c ? e + t : t;
  }
  if (e_out) e_out[clip * count + j] = e;
  if (lufs_out) lufs_out[clip * count + j] = (O)(-0.691 + 10.0 * log10(e));
}

// a wave per clip: every lane carries the same ascending sums; mask bit 0: through the absolute gate, bit 1: through both
template <typename O>
__global__ void __launch_bounds__(64) loud_gate_kernel(const double *e, int64_t nb, double e_abs, O *out, unsigned char *mask) {
  const int lane = threadIdx.x;
  const int64_t clip = blockIdx.x;
  const double *mine = e + clip * nb;
  double sum = 0.0;
  int64_t passed = 0;
  for (int64_t base = 0; base < nb; base += 64) {
    const double v = base + lane < nb ? mine[base + lane] : 0.0;
    const int live = (int)(nb - base < 64 ? nb - base : 64);
    for (int i = 0; i < live; ++i) {
      const double t = __shfl(v, i);
      if (t > e_abs) sum = sum + t, ++passed;
    }
  }
  const double relative = passed ? 0.1 * (sum / (double)passed) : 0.0;
  sum = 0.0, passed = 0;
  for (int64_t base = 0; base < nb; base += 64) {
    const double v = base + lane < nb ? mine[base + lane] : 0.0;
    const int live = (int)(nb - base < 64 ? nb - base : 64);
    if (mask && lane < live) mask[clip * nb + base + lane] = (unsigned char)((v > e_abs ? 1 : 0) | (v > e_abs && v > relative ? 2 : 0));
    for (int i = 0; i < live; ++i) {
      const double t = __shfl(v, i);
      if (t > e_abs && t > relative) sum = sum + t, ++passed;
    }
  }
  if (lane == 0) out[clip] = passed ? (O)(-0.691 + 10.0 * log10(sum / (double)passed)) : (O)(-INFINITY);
}

// ---- true peak ----------------------------------------------------------------------------------------------------------------
// out must enter as zeros; O is the result's type, its non-negative values ordered as their bits are
template <typename X, typename O>
__global__ void __launch_bounds__(kPeakThreads) loud_peak_kernel(Taps h, const X *x, int64_t x_stride, int64_t n, int64_t spans, O *out) {
  __shared__ __align__(16) X lds[kPeakSpan + kHist + 8];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / spans, s0 = (blockIdx.x % spans) * kPeakSpan;
  const X *p = x + row * x_stride;
  int a = 0;   // float32: the span's first sample lies `a` elements behind a 16-byte boundary, and the staged range begins at one
  if constexpr (sizeof(X) == 4) {
    a = (int)((reinterpret_cast<uintptr_t>(p + s0) & 15) >> 2);
    const int64_t from = s0 - kHist - a;
    const int vectors = (kPeakSpan + kHist + a + 3) / 4;
    for (int v = tid; v < vectors; v += kPeakThreads) {
      const int64_t i = from + 4 * v;
      float4 f;
      if (i >= 0 && i + 3 < n) {
        f = *reinterpret_cast<const float4 *>(p + i);
      } else {   // zeros outside the signal
        f.x = i >= 0 && i < n ? p[i] : 0.0f;
        f.y = i + 1 >= 0 && i + 1 < n ? p[i + 1] : 0.0f;
        f.z = i + 2 >= 0 && i + 2 < n ? p[i + 2] : 0.0f;
        f.w = i + 3 >= 0 && i + 3 < n ? p[i + 3] : 0.0f;
      }
      *reinterpret_cast<float4 *>(lds + 4 * v) = f;
    }
  } else {
    for (int e = tid; e < kPeakSpan + kHist; e += kPeakThreads) {
      const int64_t i = s0 - kHist + e;
      lds[e] = i >= 0 && i < n ? p[i] : (X)0;
    }
  }
  __syncthreads();
  // the lane's samples s0 + 4 tid + q, q < 4: w[12 + q - j] is x[i - j]
  double w[kHist + 4];
#pragma unroll
  for (int e = 0; e < kHist + 4; ++e) w[e] = (double)lds[a + 4 * tid + e];
  double m = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (s0 + 4 * tid + q >= n) continue;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
      double acc = h.h[ph] * w[kHist + q];
#pragma unroll
      for (int j = 1; ph + 4 * j < kTaps; ++j) acc = acc + h.h[ph + 4 * j] * w[kHist + q - j];
      m = fmax(m, fabs(acc));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
  if ((tid & 63) != 0) return;
  if constexpr (sizeof(O) == 4) atomicMax(reinterpret_cast<unsigned int *>(out) + row, __float_as_uint((float)m));
  else atomicMax(reinterpret_cast<unsigned long long *>(out) + row, (unsigned long long)__double_as_longlong(m));
}

// ---- normalize ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) loud_gain_kernel(const double *integrated, const double *peaks, int64_t clips, int channels, double target,
                                                        int has_ceiling, double ceiling, double *gain) {
  const int64_t clip = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (clip >= clips) return;
  const double i = integrated[clip];
  double g = i == -INFINITY ? 1.0 : pow(10.0, (target - i) / 20.0);
  if (has_ceiling) {
    double peak = 0.0;
    for (int c = 0; c < channels; ++c) peak = fmax(peak, peaks[clip * channels + c]);
    if (g * peak > ceiling) g = ceiling / peak;
  }
  gain[clip] = g;
}

template <typename X>
__global__ void __launch_bounds__(256) loud_scale_kernel(const X *x, int64_t x_stride, int64_t n, int64_t rows, int channels, const double *gain, X *out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, row = idx / n;
  if (row >= rows) return;
  const int64_t i = idx % n;
  out[row * n + i] = (X)(gain[row / channels] * (double)x[row * x_stride + i]);
}

__global__ void __launch_bounds__(256) loud_grow_kernel(const double *from, int64_t from_cap, double *to, int64_t to_cap, int64_t rows) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, row = idx / to_cap;
  if (row >= rows) return;
  const int64_t i = idx % to_cap;
  to[idx] = i < from_cap ? from[row * from_cap + i] : 0.0;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------
// BS.1770-4's two sections from their analogue prototypes by the bilinear transform (the constants reproduce the printed 48 kHz
// table), rows b0 b1 b2 1 a1 a2
void k_weighting(int64_t rate, double *sos) {
  if (rate < kMinRate)
    throw InvalidArgument(format("k_weighting: cannot weight audio at %lld Hz (rate must be at least %lld)", (long long)rate, (long long)kMinRate));
  const double pi = 3.14159265358979323846, fs = (double)rate;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    sos[0] = (Vh + Vb * K / Q + K * K) / a0, sos[1] = 2.0 * (K * K - Vh) / a0, sos[2] = (Vh - Vb * K / Q + K * K) / a0;
    sos[3] = 1.0, sos[4] = 2.0 * (K * K - 1.0) / a0, sos[5] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
    sos[6] = 1.0, sos[7] = -2.0, sos[8] = 1.0;
    sos[9] = 1.0, sos[10] = 2.0 * (K * K - 1.0) / a0, sos[11] = (1.0 - K / Q + K * K) / a0;
  }
}

// h[k] = sinc((k - 24) / 4) kaiser(49, 8.0)[k], scaled so that the taps sum to 4 (each phase then has unit gain at DC to rounding)
void true_peak_taps(double *h) {
  const double pi = 3.14159265358979323846, beta = 8.0;
  double sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double t = (double)(k - 24) / 4.0, r = (double)(k - 24) / 24.0;
    const double sinc = k == 24 ? 1.0 : std::sin(pi * t) / (pi * t);
    h[k] = sinc * (bessel_i0(beta * std::sqrt(1.0 - r * r)) / bessel_i0(beta));
    sum = sum + h[k];
  }
  for (int k = 0; k < kTaps; ++k) h[k] = h[k] * (4.0 / sum);
}

struct Grid {
  int64_t rate = 0, step = 0, block = 0;
  std::shared_ptr<IirCore> core;
  int64_t blocks(int64_t n) const { return n < block ? 0 : (n - block) / step + 1; }
};

// the grid and the cascade of a rate, the latter built once per rate and kept (its block matrix lies on each device once)
Grid grid_of(const char *fn, int64_t rate) {
  if (rate < kMinRate)
    throw InvalidArgument(format("%s: cannot meter audio at %lld Hz (rate must be at least %lld)", fn, (long long)rate, (long long)kMinRate));
  static std::mutex mutex;
  static std::map<int64_t, std::shared_ptr<IirCore>> cores;
  Grid g;
  g.rate = rate, g.step = (rate + 5) / 10, g.block = 4 * g.step;
  std::lock_guard<std::mutex> lock(mutex);
  auto it = cores.find(rate);
  if (it == cores.end()) {
    double sos[12];
    k_weighting(rate, sos);
    it = cores.emplace(rate, iir_make_core(sos, kS)).first;
  }
  g.core = it->second;
  return g;
}

Weights weights_of(const char *fn, const double *weights, int64_t channels) {
  if (channels < 1 || channels > kMaxChannels)
    throw InvalidArgument(format("%s: cannot meter %lld channels (channels must lie in [1, %d])", fn, (long long)channels, kMaxChannels));
  Weights w{};
  for (int64_t c = 0; c < channels; ++c) {
    w.g[c] = weights ? weights[c] : 1.0;
    if (!(w.g[c] >= 0.0) || !std::isfinite(w.g[c]))
      throw InvalidArgument(format("%s: cannot weight channel %lld by %g (weights must be finite and not negative)", fn, (long long)c, w.g[c]));
  }
  return w;
}

void check_audio(const char *fn, int64_t clips, int64_t channels, int64_t n, int64_t x_stride) {
  if (clips < 0 || channels < 0 || n < 0) throw Failure(format("%s: negative extent (clips %lld, channels %lld, n %lld)", fn, (long long)clips, (long long)channels, (long long)n));
  if (x_stride < n) throw Failure(format("%s: x_stride is smaller than the signal length", fn));
}

int64_t blocks_for(int64_t count, int threads) { return (count + threads - 1) / threads; }

// the per-channel state of an energy run: Iir's records, the open piece's partial sum, the step energies [rows; cap]
struct EnergyState {
  double *iir = nullptr, *part = nullptr, *steps = nullptr;
  int64_t cap = 0;
};

void zero_state(const EnergyState &st, int64_t rows, hipStream_t stream) {
  SMX_HIP_CHECK(hipMemsetAsync(st.iir, 0, (size_t)rows * 3 * kN * sizeof(double), stream));
  SMX_HIP_CHECK(hipMemsetAsync(st.part, 0, (size_t)rows * sizeof(double), stream));
  SMX_HIP_CHECK(hipMemsetAsync(st.steps, 0, (size_t)rows * (size_t)st.cap * sizeof(double), stream));
}

template <typename X>
void launch_general(const char *fn, const Grid &g, const X *d_x, int64_t x_stride, const EnergyState &st, int64_t rows, int64_t i0, int64_t i1, int64_t pos0,
                    hipStream_t stream) {
  SMX_LAUNCH((loud_general_kernel<X>), dim3(grid_x(fn, "workgroups", blocks_for(rows, 64), 64)), dim3(64), 0, stream, iir_coef(*g.core), d_x, x_stride,
             iir_device_matrix(*g.core), st.iir, st.part, st.steps, st.cap, rows, i0, i1, pos0 + i0, g.step);
  SMX_HIP_CHECK(hipGetLastError());
}

// samples [0, m) of `rows` rows, the first of them pos0 samples into the stream, onto the state: every step that ends inside
// (and the open one's closed pieces) is in st.steps afterwards.  st.cap > (pos0 + m - 1) / step.
template <typename X>
void energy_pass(const char *fn, const Grid &g, const X *d_x, int64_t x_stride, const EnergyState &st, int64_t rows, int64_t m, int64_t pos0,
                 hipStream_t stream) {
  if (rows == 0 || m == 0) return;
  const int at = (int)(pos0 % kBlock);
  const int64_t head = at ? std::min<int64_t>(m, kBlock - at) : 0;
  const int64_t nb = fast_path_disabled() ? 0 : (m - head) / kBlock;
  if (nb == 0) return launch_general<X>(fn, g, d_x, x_stride, st, rows, 0, m, pos0, stream);
  if (head) launch_general<X>(fn, g, d_x, x_stride, st, rows, 0, head, pos0, stream);
  const int64_t spans = (nb + kSpanBlocks - 1) / kSpanBlocks, g0 = pos0 + head;
  grid_x(fn, "block spans", rows * spans, 64);   // refused before the scratch is taken
  DeviceScratch ws, pieces;
  ws.pool((size_t)rows * (size_t)nb * kN * sizeof(double), stream);
  pieces.pool((size_t)rows * (size_t)nb * 2 * sizeof(double), stream);
  iir_block_states(fn, *g.core, d_x, (int)sizeof(X), x_stride, st.iir, rows, head, nb, ws.as<double>(), stream);
  launch_tiles(fn, loud_block_e_kernel<X>, rows * spans, 64, (size_t)kSpanBlocks * kPitch * sizeof(X), stream, iir_coef(*g.core), d_x, x_stride, head, nb, spans,
               (const double *)ws.as<double>(), g0, g.step, pieces.as<double>());
  const int64_t at0 = g0 / g.step, count = (g0 + nb * kBlock - 1) / g.step - at0 + 1;
  SMX_LAUNCH(loud_step_add_kernel, dim3(grid_x(fn, "workgroups", blocks_for(rows * count, 256), 256)), dim3(256), 0, stream, (const double *)pieces.as<double>(), nb,
             g0, g.step, at0, count, st.steps, st.cap, rows);
  SMX_HIP_CHECK(hipGetLastError());
  if (head + nb * kBlock < m) launch_general<X>(fn, g, d_x, x_stride, st, rows, head + nb * kBlock, m, pos0, stream);
}

// the state of an offline call, in scratch of the stream
struct Energies {
  DeviceScratch iir, part, steps;
  EnergyState st;
  template <typename X>
  void run(const char *fn, const Grid &g, const X *d_x, int64_t x_stride, int64_t rows, int64_t n, hipStream_t stream) {
    st.cap = n / g.step + 1;
    iir.pool((size_t)rows * 3 * kN * sizeof(double), stream);
    part.pool((size_t)rows * sizeof(double), stream);
    steps.pool((size_t)rows * (size_t)st.cap * sizeof(double), stream);
    st.iir = iir.as<double>(), st.part = part.as<double>(), st.steps = steps.as<double>();
    zero_state(st, rows, stream);
    energy_pass<X>(fn, g, d_x, x_stride, st, rows, n, 0, stream);
  }
};

template <typename O>
void launch_combine(const char *fn, const EnergyState &st, int64_t clips, int64_t channels, int64_t j0, int64_t count, int window, double inv,
                    const Weights &w, double *z_out, double *e_out, O *lufs_out, hipStream_t stream) {
  if (clips == 0 || count == 0) return;
  SMX_LAUNCH((loud_combine_kernel<O>), dim3(grid_x(fn, "workgroups", blocks_for(clips * count, 256), 256)), dim3(256), 0, stream, (const double *)st.steps, st.cap,
             clips, (int)channels, j0, count, window, inv, w, z_out, e_out, lufs_out);
  SMX_HIP_CHECK(hipGetLastError());
}

// E_abs = 10^((-70 + 0.691) / 10): a block passes the absolute gate when its energy exceeds it
double absolute_gate() { return std::pow(10.0, (-70.0 + 0.691) / 10.0); }

// the first `nb` gating blocks of the state through both gates: d_out [clips], d_mask [clips; nb] or null
template <typename O>
void gate_state(const char *fn, const Grid &g, const EnergyState &st, int64_t clips, int64_t channels, int64_t nb, const Weights &w, O *d_out,
                unsigned char *d_mask, hipStream_t stream) {
  if (clips == 0) return;
  DeviceScratch e;
  e.pool(std::max<size_t>(16, (size_t)clips * (size_t)nb * sizeof(double)), stream);
  launch_combine<O>(fn, st, clips, channels, 0, nb, 4, 1.0 / (double)g.block, w, nullptr, e.as<double>(), nullptr, stream);
  SMX_LAUNCH((loud_gate_kernel<O>), dim3(grid_x(fn, "clips", clips, 64)), dim3(64), 0, stream, (const double *)e.as<double>(), nb, absolute_gate(), d_out, d_mask);
  SMX_HIP_CHECK(hipGetLastError());
}

// ---- the faces on device-resident audio ---------------------------------------------------------------------------------------
template <typename X>
void block_energy_dev(int64_t rate, const X *d_x, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, double *d_z, hipStream_t stream) {
  const char *fn = "block_energy";
  const Grid g = grid_of(fn, rate);
  const Weights w = weights_of(fn, nullptr, channels);
  check_audio(fn, clips, channels, n, x_stride);
  const int64_t nb = g.blocks(n);
  if (clips == 0 || nb == 0) return;
  if (!d_x || !d_z) throw Failure("block_energy: null device pointer");
  Energies en;
  en.run<X>(fn, g, d_x, x_stride, clips * channels, n, stream);
  launch_combine<double>(fn, en.st, clips, channels, 0, nb, 4, 1.0 / (double)g.block, w, d_z, nullptr, nullptr, stream);
}

template <typename X>
void momentary_dev(int64_t rate, const X *d_x, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, const double *weights, int short_term,
                   X *d_out, hipStream_t stream) {
  const char *fn = short_term ? "short_term" : "momentary";
  const Grid g = grid_of(fn, rate);
  const Weights w = weights_of(fn, weights, channels);
  check_audio(fn, clips, channels, n, x_stride);
  const int window = short_term ? 30 : 4;
  const int64_t count = std::max<int64_t>(0, g.blocks(n) - (window - 4));
  if (clips == 0 || count == 0) return;
  if (!d_x || !d_out) throw Failure(format("%s: null device pointer", fn));
  Energies en;
  en.run<X>(fn, g, d_x, x_stride, clips * channels, n, stream);
  launch_combine<X>(fn, en.st, clips, channels, 0, count, window, 1.0 / (double)(window * g.step), w, nullptr, nullptr, d_out, stream);
}

template <typename X, typename O>
void integrated_dev(const char *fn, int64_t rate, const X *d_x, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, const double *weights, O *d_out,
                    unsigned char *d_mask, hipStream_t stream) {
  const Grid g = grid_of(fn, rate);
  const Weights w = weights_of(fn, weights, channels);
  check_audio(fn, clips, channels, n, x_stride);
  if (clips == 0) return;
  if ((n && !d_x) || !d_out) throw Failure(format("%s: null device pointer", fn));
  Energies en;
  en.run<X>(fn, g, d_x, x_stride, clips * channels, n, stream);
  gate_state<O>(fn, g, en.st, clips, channels, g.blocks(n), w, d_out, d_mask, stream);
}

template <typename X, typename O>
void true_peak_dev(const char *fn, const X *d_x, int64_t rows, int64_t n, int64_t x_stride, O *d_out, hipStream_t stream) {
  check_audio(fn, rows, 1, n, x_stride);
  if (rows == 0) return;
  if ((n && !d_x) || !d_out) throw Failure(format("%s: null device pointer", fn));
  SMX_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)rows * sizeof(O), stream));
  if (n == 0) return;
  Taps h;
  true_peak_taps(h.h);
  const int64_t spans = (n + kPeakSpan - 1) / kPeakSpan;
  SMX_LAUNCH((loud_peak_kernel<X, O>), dim3(grid_x(fn, "spans", rows * spans, kPeakThreads)), dim3(kPeakThreads), 0, stream, h, d_x, x_stride, n, spans, d_out);
  SMX_HIP_CHECK(hipGetLastError());
}

template <typename X>
void normalize_dev(int64_t rate, const X *d_x, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, double target, int has_ceiling, double ceiling,
                   const double *weights, X *d_out, hipStream_t stream) {
  const char *fn = "normalize";
  (void)grid_of(fn, rate);
  (void)weights_of(fn, weights, channels);
  check_audio(fn, clips, channels, n, x_stride);
  if (!std::isfinite(target)) throw InvalidArgument(format("normalize: cannot aim at %g LUFS (target must be finite)", target));
  if (has_ceiling && !(ceiling > 0.0 && std::isfinite(ceiling)))
    throw InvalidArgument(format("normalize: cannot hold peaks under %g (peak_ceiling is a linear amplitude: positive and finite)", ceiling));
  if (clips == 0 || n == 0) return;
  if (!d_x || !d_out) throw Failure("normalize: null device pointer");
  const int64_t rows = clips * channels;
  DeviceScratch loud, peaks, gain;
  loud.pool((size_t)clips * sizeof(double), stream);
  gain.pool((size_t)clips * sizeof(double), stream);
  integrated_dev<X, double>(fn, rate, d_x, clips, channels, n, x_stride, weights, loud.as<double>(), nullptr, stream);
  if (has_ceiling) {
    peaks.pool((size_t)rows * sizeof(double), stream);
    true_peak_dev<X, double>(fn, d_x, rows, n, x_stride, peaks.as<double>(), stream);
  }
  SMX_LAUNCH(loud_gain_kernel, dim3(grid_x(fn, "workgroups", blocks_for(clips, 256), 256)), dim3(256), 0, stream, (const double *)loud.as<double>(),
             (const double *)peaks.as<double>(), clips, (int)channels, target, has_ceiling, ceiling, gain.as<double>());
  SMX_HIP_CHECK(hipGetLastError());
  SMX_LAUNCH((loud_scale_kernel<X>), dim3(grid_x(fn, "workgroups", blocks_for(rows * n, 256), 256)), dim3(256), 0, stream, d_x, x_stride, n, rows, (int)channels,
             (const double *)gain.as<double>(), d_out);
  SMX_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace smx

// Loudness.Meter: the state of clips x channels channels on the device, the position since reset on the host
struct smx_loudness_meter {
  smx::Grid grid;
  smx::Weights weights{};
  int64_t clips = 0, channels = 0, position = 0;
  int device = 0;
  smx::EnergyState st;
  std::vector<double *> retired;   // outgrown step buffers: launches already enqueued may still read them
  bool fresh = true, drained = false;
  int64_t rows() const { return clips * channels; }
  int64_t blocks(int64_t position_) const { return std::max<int64_t>(0, position_ / grid.step - 3); }
  ~smx_loudness_meter() {
    for (double *p : {st.iir, st.part, st.steps})
      if (p) (void)hipFree(p);
    for (double *p : retired) (void)hipFree(p);
  }
};

namespace smx {
namespace {

constexpr int64_t kMeterSteps = 64;   // the step buffer's first capacity

// room for the steps that [0, end) touches; the host doubles the capacity by the position alone
void meter_reserve(smx_loudness_meter &m, int64_t end, hipStream_t stream) {
  const int64_t rows = m.rows(), need = end / m.grid.step + 1;
  if (!m.st.iir) {
    SMX_HIP_CHECK(hipGetDevice(&m.device));
    m.st.cap = std::max(kMeterSteps, need);
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&m.st.iir), (size_t)rows * 3 * kN * sizeof(double)));
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&m.st.part), (size_t)rows * sizeof(double)));
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&m.st.steps), (size_t)rows * (size_t)m.st.cap * sizeof(double)));
    m.fresh = true;
  }
  if (need > m.st.cap) {
    const int64_t cap = std::max(2 * m.st.cap, need);
    double *wider = nullptr;
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&wider), (size_t)rows * (size_t)cap * sizeof(double)));
    m.retired.push_back(m.st.steps);
    if (!m.fresh) {
      SMX_LAUNCH(loud_grow_kernel, dim3(grid_x("step", "workgroups", blocks_for(rows * cap, 256), 256)), dim3(256), 0, stream, (const double *)m.st.steps, m.st.cap,
                 wider, cap, rows);
      SMX_HIP_CHECK(hipGetLastError());
    }
    m.st.steps = wider, m.st.cap = cap;
  }
  if (m.fresh) zero_state(m.st, rows, stream);
  m.fresh = false;
}

// -> the momentary loudness of the blocks that completed, [clips; k] with k = blocks(position + len) - blocks(position)
template <typename X>
void meter_step_dev(smx_loudness_meter &m, const X *d_x, int64_t len, int64_t x_stride, X *d_out, hipStream_t stream) {
  const char *fn = "step";
  if (m.drained) throw InvalidArgument("step: cannot feed a drained meter (flush closed the stream; reset before reusing)");
  if (len < 0) throw Failure("step: negative chunk length");
  if (x_stride < len) throw Failure("step: x_stride is smaller than the chunk length");
  if (len == 0) return;
  const int64_t j0 = m.blocks(m.position), k = m.blocks(m.position + len) - j0;
  if (!d_x || (k && !d_out)) throw Failure("step: null device pointer");
  meter_reserve(m, m.position + len, stream);
  energy_pass<X>(fn, m.grid, d_x, x_stride, m.st, m.rows(), len, m.position, stream);
  launch_combine<X>(fn, m.st, m.clips, m.channels, j0, k, 4, 1.0 / (double)m.grid.block, m.weights, nullptr, nullptr, d_out, stream);
  m.position += len;
}

enum { READ_INTEGRATED = 0, READ_SHORT_TERM = 1 };

int64_t meter_read_count(const smx_loudness_meter &m, int what) {
  if (what == READ_INTEGRATED) return 1;
  if (what == READ_SHORT_TERM) return std::max<int64_t>(0, m.blocks(m.position) - 26);
  throw Failure(format("read: unknown quantity %d", what));
}

template <typename O>
void meter_read_dev(smx_loudness_meter &m, int what, O *d_out, hipStream_t stream) {
  const char *fn = "read";
  const int64_t count = meter_read_count(m, what);
  if (count == 0) return;
  if (!d_out) throw Failure("read: null device pointer");
  meter_reserve(m, m.position, stream);
  if (what == READ_INTEGRATED) gate_state<O>(fn, m.grid, m.st, m.clips, m.channels, m.blocks(m.position), m.weights, d_out, nullptr, stream);
  else launch_combine<O>(fn, m.st, m.clips, m.channels, 0, count, 30, 1.0 / (double)(30 * m.grid.step), m.weights, nullptr, nullptr, d_out, stream);
}

// ---- the faces on host arrays -------------------------------------------------------------------------------------------------
// one upload / run / download (host_call) of `clips` clips of in_clip bytes each into results of out_clip bytes each
template <typename F>
void on_host(const char *fn, const void *x, size_t in_clip, void *out, size_t out_clip, int64_t clips, F &&dev) {
  if (clips == 0 || out_clip == 0) return;
  if (!x || !out) throw Failure(format("%s: null pointer", fn));
  host_call(fn, {{x, std::max<size_t>(in_clip, 1)}}, out, out_clip, clips, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) { dev(d_in[0], d_out, nc, stream); });
}

template <typename X>
void block_energy_host(int64_t rate, const X *x, int64_t clips, int64_t channels, int64_t n, double *z) {
  block_energy_dev<X>(rate, nullptr, 0, channels, n, n, nullptr, nullptr);   // the checks, before a device is asked for
  check_audio("block_energy", clips, channels, n, n);
  const int64_t nb = grid_of("block_energy", rate).blocks(n);
  on_host("block_energy", x, (size_t)channels * n * sizeof(X), z, (size_t)channels * nb * sizeof(double), clips,
          [&](const void *d_x, void *d_z, int64_t nc, hipStream_t stream) {
            block_energy_dev<X>(rate, reinterpret_cast<const X *>(d_x), nc, channels, n, n, reinterpret_cast<double *>(d_z), stream);
          });
}

template <typename X>
void momentary_host(int64_t rate, const X *x, int64_t clips, int64_t channels, int64_t n, const double *weights, int short_term, X *out) {
  const char *fn = short_term ? "short_term" : "momentary";
  momentary_dev<X>(rate, nullptr, 0, channels, n, n, weights, short_term, nullptr, nullptr);
  check_audio(fn, clips, channels, n, n);
  const int64_t count = std::max<int64_t>(0, grid_of(fn, rate).blocks(n) - (short_term ? 26 : 0));
  on_host(fn, x, (size_t)channels * n * sizeof(X), out, (size_t)count * sizeof(X), clips, [&](const void *d_x, void *d_out, int64_t nc, hipStream_t stream) {
    momentary_dev<X>(rate, reinterpret_cast<const X *>(d_x), nc, channels, n, n, weights, short_term, reinterpret_cast<X *>(d_out), stream);
  });
}

template <typename X>
void integrated_host(int64_t rate, const X *x, int64_t clips, int64_t channels, int64_t n, const double *weights, X *out, unsigned char *mask) {
  const char *fn = "integrated";
  integrated_dev<X, X>(fn, rate, nullptr, 0, channels, n, n, weights, nullptr, nullptr, nullptr);
  check_audio(fn, clips, channels, n, n);
  if (clips == 0) return;
  if ((n && !x) || !out) throw Failure("integrated: null pointer");
  const int64_t nb = grid_of(fn, rate).blocks(n);
  if (nb == 0) {   // nothing to gate: no launch
    for (int64_t c = 0; c < clips; ++c) out[c] = (X)(-INFINITY);
    return;
  }
  host_call(fn, {{x, (size_t)channels * n * sizeof(X)}}, {HostOut{out, sizeof(X)}, HostOut{mask, (size_t)nb}}, clips, false, nullptr,
            [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t stream) {
              integrated_dev<X, X>(fn, rate, reinterpret_cast<const X *>(d_in[0]), nc, channels, n, n, weights, reinterpret_cast<X *>(d_out[0]),
                                   reinterpret_cast<unsigned char *>(d_out[1]), stream);
            });
}

template <typename X>
void true_peak_host(const X *x, int64_t rows, int64_t n, X *out) {
  const char *fn = "true_peak";
  check_audio(fn, rows, 1, n, n);
  if (rows == 0) return;
  if ((n && !x) || !out) throw Failure("true_peak: null pointer");
  if (n == 0) {
    for (int64_t r = 0; r < rows; ++r) out[r] = (X)0;
    return;
  }
  on_host(fn, x, (size_t)n * sizeof(X), out, sizeof(X), rows, [&](const void *d_x, void *d_out, int64_t nc, hipStream_t stream) {
    true_peak_dev<X, X>(fn, reinterpret_cast<const X *>(d_x), nc, n, n, reinterpret_cast<X *>(d_out), stream);
  });
}

template <typename X>
void normalize_host(int64_t rate, const X *x, int64_t clips, int64_t channels, int64_t n, double target, int has_ceiling, double ceiling, const double *weights,
                    X *out) {
  normalize_dev<X>(rate, nullptr, 0, channels, n, n, target, has_ceiling, ceiling, weights, nullptr, nullptr);
  check_audio("normalize", clips, channels, n, n);
  on_host("normalize", x, (size_t)channels * n * sizeof(X), out, (size_t)channels * n * sizeof(X), clips,
          [&](const void *d_x, void *d_out, int64_t nc, hipStream_t stream) {
            normalize_dev<X>(rate, reinterpret_cast<const X *>(d_x), nc, channels, n, n, target, has_ceiling, ceiling, weights, reinterpret_cast<X *>(d_out), stream);
          });
}

template <typename X>
void meter_step_host(smx_loudness_meter &m, const X *x, int64_t len, X *out) {
  if (m.drained || len <= 0) return meter_step_dev<X>(m, nullptr, len, len, nullptr, nullptr);
  if (!x) throw Failure("step: null pointer");
  const int64_t k = m.blocks(m.position + len) - m.blocks(m.position);
  if (k && !out) throw Failure("step: null pointer");
  host_call("step", {{x, (size_t)m.channels * len * sizeof(X)}}, {HostOut{k ? out : nullptr, (size_t)k * sizeof(X)}}, m.clips, false, nullptr,
            [&](const void *const *d_in, void *const *d_out, int64_t, hipStream_t stream) {
              meter_step_dev<X>(m, reinterpret_cast<const X *>(d_in[0]), len, len, reinterpret_cast<X *>(d_out[0]), stream);
            });
}

template <typename X>
void meter_read_host(smx_loudness_meter &m, int what, X *out) {
  const int64_t count = meter_read_count(m, what);
  if (count == 0) return;
  if (!out) throw Failure("read: null pointer");
  if (what == READ_INTEGRATED && m.blocks(m.position) == 0) {   // nothing to gate: no launch
    for (int64_t c = 0; c < m.clips; ++c) out[c] = (X)(-INFINITY);
    return;
  }
  require_device();
  const size_t bytes = (size_t)m.clips * (size_t)count * sizeof(X);
  DeviceScratch d_out(bytes);
  meter_read_dev<X>(m, what, d_out.as<X>(), nullptr);
  SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
  copy_to_host(out, d_out.ptr, bytes);
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Loudness ----------------------------------------------------------------------------------------------------------------
int64_t smx_loudness_min_rate(void) { return kMinRate; }
int64_t smx_loudness_max_channels(void) { return kMaxChannels; }
int64_t smx_loudness_step(int64_t rate) { return (rate + 5) / 10; }
int64_t smx_loudness_blocks(int64_t rate, int64_t n) {
  const int64_t step = (rate + 5) / 10;
  return step < 1 || n < 4 * step ? 0 : (n - 4 * step) / step + 1;
}
double smx_loudness_absolute_gate(void) { return absolute_gate(); }
int smx_loudness_k_weighting(int64_t rate, double *sos) {
  return guarded([&] {
    if (!sos) throw Failure("k_weighting: null pointer");
    double rows[12];
    k_weighting(rate, rows);
    std::copy(rows, rows + 12, sos);
  });
}
int smx_loudness_true_peak_taps(double *h) {
  return guarded([&] {
    if (!h) throw Failure("true_peak_taps: null pointer");
    true_peak_taps(h);
  });
}
int smx_loudness_block_energy_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double *z) {
  return guarded([&] { block_energy_host<float>(rate, x, clips, channels, n, z); });
}
int smx_loudness_block_energy_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double *z) {
  return guarded([&] { block_energy_host<double>(rate, x, clips, channels, n, z); });
}
int smx_loudness_block_energy_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, int64_t rate,
                                       double *d_z) {
  return guarded([&] { block_energy_dev<float>(rate, d_x, clips, channels, n, x_stride, d_z, (hipStream_t)stream); });
}
int smx_loudness_momentary_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights, int short_term, float *out) {
  return guarded([&] { momentary_host<float>(rate, x, clips, channels, n, weights, short_term, out); });
}
int smx_loudness_momentary_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights, int short_term,
                               double *out) {
  return guarded([&] { momentary_host<double>(rate, x, clips, channels, n, weights, short_term, out); });
}
int smx_loudness_momentary_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, int64_t rate,
                                    const double *weights, int short_term, float *d_out) {
  return guarded([&] { momentary_dev<float>(rate, d_x, clips, channels, n, x_stride, weights, short_term, d_out, (hipStream_t)stream); });
}
int smx_loudness_integrated_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights, float *out,
                                unsigned char *mask) {
  return guarded([&] { integrated_host<float>(rate, x, clips, channels, n, weights, out, mask); });
}
int smx_loudness_integrated_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights, double *out,
                                unsigned char *mask) {
  return guarded([&] { integrated_host<double>(rate, x, clips, channels, n, weights, out, mask); });
}
int smx_loudness_integrated_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, int64_t rate,
                                     const double *weights, float *d_out, unsigned char *d_mask) {
  return guarded([&] { integrated_dev<float, float>("integrated", rate, d_x, clips, channels, n, x_stride, weights, d_out, d_mask, (hipStream_t)stream); });
}
int smx_loudness_true_peak_f32(const float *x, int64_t rows, int64_t n, float *out) {
  return guarded([&] { true_peak_host<float>(x, rows, n, out); });
}
int smx_loudness_true_peak_f64(const double *x, int64_t rows, int64_t n, double *out) {
  return guarded([&] { true_peak_host<double>(x, rows, n, out); });
}
int smx_loudness_true_peak_card_f32(const float *d_x, void *stream, int64_t rows, int64_t n, int64_t x_stride, float *d_out) {
  return guarded([&] { true_peak_dev<float, float>("true_peak", d_x, rows, n, x_stride, d_out, (hipStream_t)stream); });
}
int smx_loudness_normalize_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double target, int has_ceiling, double ceiling,
                               const double *weights, float *out) {
  return guarded([&] { normalize_host<float>(rate, x, clips, channels, n, target, has_ceiling, ceiling, weights, out); });
}
int smx_loudness_normalize_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double target, int has_ceiling, double ceiling,
                               const double *weights, double *out) {
  return guarded([&] { normalize_host<double>(rate, x, clips, channels, n, target, has_ceiling, ceiling, weights, out); });
}
int smx_loudness_normalize_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride, int64_t rate, double target,
                                    int has_ceiling, double ceiling, const double *weights, float *d_out) {
  return guarded([&] { normalize_dev<float>(rate, d_x, clips, channels, n, x_stride, target, has_ceiling, ceiling, weights, d_out, (hipStream_t)stream); });
}
int smx_loudness_meter_prepare(int64_t rate, int64_t clips, int64_t channels, const double *weights, smx_loudness_meter **out) {
  return guarded([&] {
    if (!out) throw Failure("prepare: null result pointer");
    const Grid g = grid_of("prepare", rate);
    const Weights w = weights_of("prepare", weights, channels);
    if (clips < 1) throw InvalidArgument(format("prepare: cannot keep the state of %lld clips (the leading axes must not be empty)", (long long)clips));
    auto *m = new smx_loudness_meter;
    m->grid = g, m->weights = w, m->clips = clips, m->channels = channels;
    *out = m;
  });
}
void smx_loudness_meter_destroy(smx_loudness_meter *m) { delete m; }
int smx_loudness_meter_reset(smx_loudness_meter *m) {
  return guarded([&] {
    check_config(m, "reset");
    m->position = 0, m->fresh = true, m->drained = false;
  });
}
int smx_loudness_meter_flush(smx_loudness_meter *m) {
  return guarded([&] {
    check_config(m, "flush");
    m->drained = true;
  });
}
int64_t smx_loudness_meter_position(const smx_loudness_meter *m) { return m ? m->position : 0; }
int smx_loudness_meter_step_f32(smx_loudness_meter *m, const float *x, int64_t len, float *out) {
  return guarded([&] {
    check_config(m, "step");
    meter_step_host<float>(*m, x, len, out);
  });
}
int smx_loudness_meter_step_f64(smx_loudness_meter *m, const double *x, int64_t len, double *out) {
  return guarded([&] {
    check_config(m, "step");
    meter_step_host<double>(*m, x, len, out);
  });
}
int smx_loudness_meter_step_card_f32(smx_loudness_meter *m, void *stream, const float *d_x, int64_t len, int64_t x_stride, float *d_out) {
  return guarded([&] {
    check_config(m, "step");
    meter_step_dev<float>(*m, d_x, len, x_stride, d_out, (hipStream_t)stream);
  });
}
int smx_loudness_meter_read_f32(smx_loudness_meter *m, int what, float *out) {
  return guarded([&] {
    check_config(m, "read");
    meter_read_host<float>(*m, what, out);
  });
}
int smx_loudness_meter_read_f64(smx_loudness_meter *m, int what, double *out) {
  return guarded([&] {
    check_config(m, "read");
    meter_read_host<double>(*m, what, out);
  });
}
int smx_loudness_meter_read_card_f32(smx_loudness_meter *m, void *stream, int what, float *d_out) {
  return guarded([&] {
    check_config(m, "read");
    meter_read_dev<float>(*m, what, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
