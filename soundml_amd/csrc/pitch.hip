// Pitch: YIN fundamental-frequency tracking (de Cheveigne & Kawahara 2002) over device-resident audio [lead; n] (time fastest).
//
// The grid is that of rms (energy.hip): border = frame_length / 2 virtual zeros on each side, frame p covers padded positions
// [p hop, p hop + frame_length); border 0 is the uncentred "frames of a segment" call of the stage.
//
// Per frame, samples x_0 .. x_{frame_length - 1}, W = frame_length / 2, everything in float64:
//   r(tau) = sum_{j < W} x_j x_{j + tau}       j < W is cut into consecutive blocks of blk = min(hop, W) from the frame's start, the
//                                              last may be short; a block's partial is ONE ascending chain over j starting from 0.0;
//                                              the frame's r is the first block's partial, the others added in ascending order
//   P(i)   = sum_{j < i} x_j^2                 one ascending chain from the frame's first sample, P(0) = 0
//   e(tau) = P(tau + W) - P(tau)
//   d(tau) = max(0, (e(0) + e(tau)) - 2 r(tau)),  c(tau) = c(tau - 1) + d(tau),  d'(tau) = (d(tau) tau) / c(tau), 1 where c = 0
// Float32 samples: every product is exact in float64, so fma is meant and named; float64 samples: the product and the sum round one
// after the other (the file is built with -ffp-contract=off).  The order is a function of the frame's own samples, so a full block k
// of frame p is block 0 of frame p + k and the short last block's chain is a prefix of a full block's: the tile kernel computes
// every hop block of its span once and the frames pick theirs.
//
//   yin_tile_kernel      float32, hop a multiple of 8 with 64 <= hop <= W: a workgroup stages the span of its frames in LDS once
//                        (aligned 16-byte loads, borders as zeros at the fetch); a lane owns kLags consecutive lags of one hop block
//                        and slides them over the block from registers (one new sample and one broadcast x_j per kLags multiply-adds);
//                        then a lane per (frame, lag) adds the frame's partials in order
//   yin_general_kernel   a workgroup per frame straight from memory, a thread per lag, the same order: every other geometry and
//                        float64; SMX_DISABLE_FAST=1 forces it (tests: the same bits)
//   yin_finish_kernel    both routes leave r in scratch [lag][frame]; a lane per frame walks the lags once (P, e, d, c, d') and picks
//                        the lag as they go by, then the parabolic shift, f0 and the aperiodicity; the samples reach the lanes
//                        through an LDS tile, a contiguous row per frame
#include <type_traits>

#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kLags = 8;                         // consecutive lags of a lane
constexpr int kTileBytes = 64 * 1024;            // samples and partials of one tile in LDS
constexpr int kTileFrames = 16;                  // most frames of a tile
constexpr int kInFlight = 8;                     // 16-byte loads in flight per thread while a tile is staged
constexpr int kSlack = 2 * kLags;                // zeros behind a tile's samples: the lags past pmax of the last lane read them
constexpr int64_t kScratchBytes = 512ll << 20;   // r of one launch; larger calls go clip range by clip range

struct PitchArgs {
  const void *x;                  // [lead; n], rows x_stride apart
  double *r;                      // scratch [lags; lead * frames]
  void *f0, *ap, *diff;           // [lead; frames] twice, [lead; lags; frames]; each may be null
  int64_t lead, n, x_stride, frames, border, fl, hop, tiles, total;   // tiles: workgroups per clip; total = lead * frames
  double sample_rate, threshold;
  int W, pmin, pmax, lags;        // lags = pmax + 1
  int tile_frames, nfull, rest, groups;   // the tile kernel: frames per tile, full blocks per frame, the short block's length, lanes per block
};

template <typename T>
__device__ __forceinline__ T sample_at(const T *row, int64_t s, int64_t n) { return (s >= 0 && s < n) ? row[s] : (T)0; }

// acc + a b: float32 samples' products are exact in float64, fma is meant; float64 samples round twice
template <typename T>
__device__ __forceinline__ double mul_add(double a, double b, double acc) {
  if constexpr (sizeof(T) == 4) return fma(a, b, acc);
  return acc + a * b;
}

// the chain of one block for kLags consecutive lags from tau0: s[j] is x_j, steps j0 <= j < j1 in ascending order
__device__ __forceinline__ void slide(const float *s, int tau0, int j0, int j1, double (&acc)[kLags]) {
  int j = j0;
  auto step = [&]() {
    const double xj = (double)s[j];
#pragma unroll
    for (int k = 0; k < kLags; ++k) acc[k] = fma(xj, (double)s[j + tau0 + k], acc[k]);
    ++j;
  };
  while ((j & (kLags - 1)) && j < j1) step();
  if (j + kLags <= j1) {
    // s, tau0 and j are multiples of 8 elements from a 16-byte aligned origin: whole float4 reads
    double w[2 * kLags];
    {
      const float4 a = *reinterpret_cast<const float4 *>(s + j + tau0), b = *reinterpret_cast<const float4 *>(s + j + tau0 + 4);
      w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    }
    for (; j + kLags <= j1; j += kLags) {
      const float4 a = *reinterpret_cast<const float4 *>(s + j + tau0 + 8), b = *reinterpret_cast<const float4 *>(s + j + tau0 + 12);
      w[8] = a.x, w[9] = a.y, w[10] = a.z, w[11] = a.w, w[12] = b.x, w[13] = b.y, w[14] = b.z, w[15] = b.w;
      const float4 xa = *reinterpret_cast<const float4 *>(s + j), xb = *reinterpret_cast<const float4 *>(s + j + 4);
      const double x[kLags] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
      for (int jj = 0; jj < kLags; ++jj)
#pragma unroll
        for (int k = 0; k < kLags; ++k) acc[k] = fma(x[jj], w[jj + k], acc[k]);
#pragma unroll
      for (int i = 0; i < kLags; ++i) w[i] = w[i + kLags];
    }
  }
  while (j < j1) step();
}

__global__ void __launch_bounds__(256) yin_tile_kernel(PitchArgs a) {
  extern __shared__ __align__(16) unsigned char tile_lds[];
  const int64_t clip = blockIdx.x / a.tiles, p0 = (blockIdx.x % a.tiles) * a.tile_frames;
  const int nf = (int)(a.frames - p0 < a.tile_frames ? a.frames - p0 : a.tile_frames);
  const int hop = (int)a.hop, fl = (int)a.fl;
  const float *row = reinterpret_cast<const float *>(a.x) + clip * a.x_stride;
  const int64_t s0 = p0 * a.hop - a.border;                 // the tile's first padded position as a signal index: LDS element 0
  const int span = (nf - 1) * hop + fl;
  // 16-byte groups by address: group g holds signal indices s0 - shift + 4 g ..; element e of the tile is signal index s0 + e
  const int shift = (int)(((int64_t)(reinterpret_cast<uintptr_t>(row) / sizeof(float)) + s0) & 3);
  const int groups = (shift + span + 3) / 4;
  float *smp = reinterpret_cast<float *>(tile_lds);
  const int cap = (a.tile_frames - 1) * hop + fl + kSlack;  // floats of a full tile, a multiple of 8
  const int lpad = a.groups * kLags;
  const int slots = a.tile_frames + a.nfull;                // hop blocks of a full tile
  double *full = reinterpret_cast<double *>(tile_lds + (size_t)cap * 4);   // [slots][lpad] chains over a whole block
  double *head = full + (size_t)slots * lpad;                              // [slots][lpad] over its first `rest` steps (rest > 0)

  for (int g0 = threadIdx.x; g0 < groups; g0 += 256 * kInFlight) {
    float4 q[kInFlight];
    bool whole[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int g = g0 + u * 256;
      const int64_t s = s0 - shift + (int64_t)g * 4;
      whole[u] = g < groups && s >= 0 && s + 4 <= a.n;
      if (whole[u]) q[u] = *reinterpret_cast<const float4 *>(row + s);
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int g = g0 + u * 256;
      if (g >= groups) continue;
      const int64_t s = s0 - shift + (int64_t)g * 4;
      float *e = reinterpret_cast<float *>(&q[u]);
      if (!whole[u]) {                                      // a group that meets a border: element by element
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = sample_at<float>(row, s + i, a.n);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int at = g * 4 - shift + i;
        if (at >= 0 && at < span) smp[at] = e[i];
      }
    }
  }
  if (threadIdx.x < kSlack) smp[span + threadIdx.x] = 0.0f;
  __syncthreads();

  // hop block u of the tile starts at element u hop; the blocks behind the last frame's full ones are walked for their first
  // `rest` steps only
  const int units = nf + a.nfull - 1 + (a.rest ? 1 : 0);
  for (int item = threadIdx.x; item < units * a.groups; item += 256) {
    const int u = item / a.groups, tau0 = (item % a.groups) * kLags;
    const float *s = smp + u * hop;
    const bool whole = u < nf + a.nfull - 1;
    double acc[kLags];
#pragma unroll
    for (int k = 0; k < kLags; ++k) acc[k] = 0.0;
    if (a.rest) {
      slide(s, tau0, 0, a.rest, acc);
#pragma unroll
      for (int k = 0; k < kLags; ++k) head[(size_t)u * lpad + tau0 + k] = acc[k];
      if (whole) slide(s, tau0, a.rest, hop, acc);
    } else {
      slide(s, tau0, 0, hop, acc);
    }
    if (whole) {
#pragma unroll
      for (int k = 0; k < kLags; ++k) full[(size_t)u * lpad + tau0 + k] = acc[k];
    }
  }
  __syncthreads();

  const int64_t first = clip * a.frames + p0;
  for (int i = threadIdx.x; i < nf * a.lags; i += 256) {
    const int f = i % nf, tau = i / nf;
    double r = full[(size_t)f * lpad + tau];                 // hop <= W: a frame has at least one full block
    for (int k = 1; k < a.nfull; ++k) r += full[(size_t)(f + k) * lpad + tau];
    if (a.rest) r += head[(size_t)(f + a.nfull) * lpad + tau];
    a.r[(int64_t)tau * a.total + first + f] = r;
  }
}

// a workgroup per frame, a thread per lag, any geometry and either sample width
template <typename T>
__global__ void __launch_bounds__(256) yin_general_kernel(PitchArgs a) {
  const int64_t g = blockIdx.x, clip = g / a.frames, p = g % a.frames;
  const T *row = reinterpret_cast<const T *>(a.x) + clip * a.x_stride;
  const int64_t s0 = p * a.hop - a.border;
  const int blk = a.hop < a.W ? (int)a.hop : a.W;
  for (int tau = threadIdx.x; tau < a.lags; tau += 256) {
    double r = 0.0;
    for (int b0 = 0; b0 < a.W; b0 += blk) {
      const int b1 = b0 + blk < a.W ? b0 + blk : a.W;
      double acc = 0.0;
      for (int j = b0; j < b1; ++j)
        acc = mul_add<T>((double)sample_at<T>(row, s0 + j, a.n), (double)sample_at<T>(row, s0 + j + tau, a.n), acc);
      r = b0 == 0 ? acc : r + acc;
    }
    a.r[(int64_t)tau * a.total + g] = r;
  }
}

// a lane per frame, a wave per 64 consecutive frames: the lags in ascending order, everything of a frame in its lane's registers.
// The chains of the 64 frames advance in step, kSteps samples at a time: the wave fetches each frame's next kSteps samples as one
// contiguous row (half a wave per row, borders as zeros) into an LDS tile, and lane f then walks row f.  r comes from the scratch
// (consecutive frames: one contiguous read per lag), eight lags ahead of their use.
constexpr int kSteps = 32;

template <typename T>
__global__ void __launch_bounds__(64) yin_finish_kernel(PitchArgs a) {
  __shared__ T tile[2][64][kSteps + 1];                     // rows 33 apart: lane f on row f meets no other lane's bank
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * 64 + lane;
  const bool live = g < a.total;
  const int64_t clip = live ? g / a.frames : 0, p = live ? g % a.frames : 0;
  const long long row_at = clip * a.x_stride, s0 = p * a.hop - a.border;   // the frame's first padded position as a signal index
  const T *x = reinterpret_cast<const T *>(a.x);
  const double *col = a.r + (live ? g : 0);                 // lag tau at col[tau total]
  T *diff = a.diff && live ? reinterpret_cast<T *>(a.diff) + clip * a.lags * a.frames + p : nullptr;
  const bool choose = a.f0 != nullptr;

  // samples [i0, i0 + kSteps) of every frame of the wave into tile[which]
  auto stage = [&](int which, int i0) {
    const int k = lane & (kSteps - 1);
    T v[32];                                                // all 32 rows' loads are in flight before the first is parked
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const int f = 2 * i + (lane >> 5);
      const long long s = __shfl(s0, f) + i0 + k, at = __shfl(row_at, f);
      const bool there = __shfl((int)live, f) && s >= 0 && s < a.n;
      v[i] = there ? x[at + s] : (T)0;
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) tile[which][2 * i + (lane >> 5)][k] = v[i];
  };

  double upper = 0.0, lower = 0.0, c = 0.0;                 // P(tau + W), P(tau), c(tau)
  for (int i0 = 0; i0 < a.W; i0 += kSteps) {
    stage(0, i0);
    __syncthreads();
    const int steps = a.W - i0 < kSteps ? a.W - i0 : kSteps;
    for (int k = 0; k < steps; ++k) {
      const double v = (double)tile[0][lane][k];
      upper = mul_add<T>(v, v, upper);
    }
    __syncthreads();
  }
  const double e0 = upper;
  if (diff) diff[0] = (T)1.0;

  // the choice, as the lags go by: the first trough below the threshold, and the least d' with the smallest lag
  bool found = false;
  int trough = 0, lowest = 0;
  double before = 1.0, here = 1.0;                          // d'(tau - 2), d'(tau - 1)
  double ta = 0.0, tb = 0.0, tc = 0.0, la = 0.0, lb = 0.0, lc = 0.0;   // d' around the trough and around the least

  for (int t0 = 1; t0 <= a.pmax; t0 += kSteps) {
    stage(0, t0 - 1);
    stage(1, t0 + a.W - 1);
    __syncthreads();
    const int steps = a.pmax - t0 + 1 < kSteps ? a.pmax - t0 + 1 : kSteps;
    for (int k0 = 0; k0 < steps; k0 += 8) {
      double r[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = k0 + u < steps ? col[(int64_t)(t0 + k0 + u) * a.total] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u, tau = t0 + k;
        if (k >= steps) break;
        const double lo = (double)tile[0][lane][k], hi = (double)tile[1][lane][k];
        lower = mul_add<T>(lo, lo, lower);
        upper = mul_add<T>(hi, hi, upper);
        const double e = upper - lower;
        const double t = (e0 + e) - 2.0 * r[u];
        const double d = t < 0.0 ? 0.0 : t;                 // a NaN stays one
        c = c + d;
        const double dn = c == 0.0 ? 1.0 : (d * (double)tau) / c;
        if (diff) diff[(int64_t)tau * a.frames] = (T)dn;
        if (choose && tau - 1 >= a.pmin) {                  // lag tau - 1 has both neighbours now
          if (!found && here < a.threshold && here <= before && here < dn) found = true, trough = tau - 1, ta = before, tb = here, tc = dn;
          if (tau - 1 == a.pmin || here < lb) lowest = tau - 1, la = before, lb = here, lc = dn;
        }
        before = here;
        here = dn;
      }
    }
    __syncthreads();
  }
  if (!choose || !live) return;
  // lag pmax has no neighbour behind it
  if (!found && here < a.threshold && here <= before) found = true, trough = a.pmax, ta = before, tb = here;
  if (here < lb) lowest = a.pmax, la = before, lb = here;
  const int chosen = found ? trough : lowest;
  const double u = found ? ta : la, v = found ? tb : lb, w = found ? tc : lc;
  double shift = 0.0;
  if (chosen - 1 >= 1 && chosen + 1 <= a.pmax) {
    const double den = (u - 2.0 * v) + w;
    if (den > 0.0) {
      const double s = (0.5 * (u - w)) / den;
      if (fabs(s) <= 1.0) shift = s;
    }
  }
  double f0 = a.sample_rate / ((double)chosen + shift), ap = v;
  // a non-finite sample: the frame has no pitch and no voicing measure
  if (!isfinite(e0) || !isfinite(c)) f0 = ap = __builtin_nan("");
  reinterpret_cast<T *>(a.f0)[g] = (T)f0;
  if (a.ap) reinterpret_cast<T *>(a.ap)[g] = (T)ap;
}

// ---- the host side -------------------------------------------------------------------------------------------------------------
struct PitchPlan {
  int64_t sample_rate, fl, hop;
  double fmin, fmax, threshold;
  int64_t pmin, pmax;
};

// the parameters, in the order of the header; `threshold` is checked where a lag is chosen
PitchPlan check_pitch(const char *fn, int64_t sample_rate, double fmin, double fmax, int64_t fl, int64_t hop, bool choose, double threshold) {
  if (sample_rate < 1)
    throw InvalidArgument(format("%s: cannot analyse audio sampled at %lld Hz (sample_rate must be at least 1)", fn, (long long)sample_rate));
  if (fl < 4) throw InvalidArgument(format("%s: cannot analyse frames of %lld samples (frame_length must be at least 4)", fn, (long long)fl));
  if (hop < 1) throw InvalidArgument(format("%s: cannot advance frames by %lld samples (hop must be at least 1)", fn, (long long)hop));
  const double sr = (double)sample_rate;
  if (!(std::isfinite(fmin) && std::isfinite(fmax) && 0.0 < fmin && fmin < fmax && fmax <= sr / 2.0))
    throw InvalidArgument(format("%s: cannot search between %g and %g Hz at %lld Hz (fmin and fmax must be finite with 0 < fmin < fmax <= sample_rate / 2)",
                                 fn, fmin, fmax, (long long)sample_rate));
  if (choose && !(std::isfinite(threshold) && threshold > 0.0))
    throw InvalidArgument(format("%s: cannot accept troughs below %g (trough_threshold must be finite and positive)", fn, threshold));
  PitchPlan plan{sample_rate, fl, hop, fmin, fmax, threshold, 0, 0};
  const int64_t cap = fl - fl / 2 - 1;
  const double longest = std::ceil(sr / fmin);
  plan.pmin = (int64_t)std::floor(sr / fmax);
  plan.pmax = longest < (double)cap ? (int64_t)longest : cap;
  if (plan.pmax <= plan.pmin)
    throw InvalidArgument(format("%s: cannot search lags %lld to %lld in frames of %lld samples (frame_length too short for fmin)", fn,
                                 (long long)plan.pmin, (long long)plan.pmax, (long long)fl));
  return plan;
}

int64_t count_frames(int64_t fl, int64_t hop, int64_t n) {
  if (n == 0) return 0;
  const int64_t padded = n + 2 * (fl / 2);
  return padded < fl ? 0 : 1 + (padded - fl) / hop;
}

// workgroups of 256 lanes a tile of nf frames keeps busy, in rounds
int64_t tile_rounds(int64_t nf, int64_t nfull, int64_t rest, int64_t groups) { return ((nf + nfull - 1 + (rest ? 1 : 0)) * groups + 255) / 256; }

// frames per tile of the tile kernel, or 0: the general kernel.  A function of the geometry, the lag range and the sample width.
int tile_frames(const PitchPlan &plan, int elem_bytes) {
  const int64_t W = plan.fl / 2, hop = plan.hop;
  if (fast_path_disabled() || elem_bytes != 4 || plan.fl % 2 || hop % 8 || hop < 64 || hop > W) return 0;
  const int64_t nfull = W / hop, rest = W - nfull * hop, groups = (plan.pmax + kLags) / kLags;
  int best = 0;
  for (int64_t nf = 1; nf <= kTileFrames; ++nf) {
    const int64_t bytes = ((nf - 1) * hop + plan.fl + kSlack) * 4 + (nf + nfull) * groups * kLags * 8 * (rest ? 2 : 1);
    if (bytes > kTileBytes) break;
    // the most frames per round of lanes; of equals the larger tile (fewer blocks computed twice)
    if (!best || nf * tile_rounds(best, nfull, rest, groups) >= best * tile_rounds(nf, nfull, rest, groups)) best = (int)nf;
  }
  return best;
}

template <typename T>
void launch_pitch(const char *fn, PitchArgs a, const PitchPlan &plan, hipStream_t stream) {
  a.tile_frames = tile_frames(plan, (int)sizeof(T));
  if (a.tile_frames) {
    if constexpr (sizeof(T) == 4) {
      a.tiles = (a.frames + a.tile_frames - 1) / a.tile_frames;
      if (a.lead * a.tiles > 2147483647LL) throw Failure(format("%s: too many frame tiles for one launch", fn));
      a.nfull = (int)(a.W / a.hop);
      a.rest = (int)(a.W - a.nfull * a.hop);
      a.groups = (a.pmax + kLags) / kLags;
      const size_t lds = (size_t)((a.tile_frames - 1) * a.hop + a.fl + kSlack) * 4 +
                         (size_t)(a.tile_frames + a.nfull) * a.groups * kLags * 8 * (a.rest ? 2 : 1);
      SMX_LAUNCH(yin_tile_kernel, dim3((unsigned)(a.lead * a.tiles)), dim3(256), lds, stream, a);
    }
  } else {
    if (a.total > 2147483647LL) throw Failure(format("%s: too many frames for one launch", fn));
    SMX_LAUNCH((yin_general_kernel<T>), dim3((unsigned)a.total), dim3(256), 0, stream, a);
  }
  SMX_HIP_CHECK(hipGetLastError());
  SMX_LAUNCH((yin_finish_kernel<T>), dim3((unsigned)((a.total + 63) / 64)), dim3(64), 0, stream, a);
  SMX_HIP_CHECK(hipGetLastError());
}

// frames [0, count) of rows extended by `border` virtual zeros on each side; the parameters are the caller's to check.
// d_f0 / d_ap [lead; count] or d_diff [lead; pmax + 1; count]
void pitch_dev(const char *fn, const PitchPlan &plan, int64_t border, const void *d_x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride,
               int64_t count, void *d_f0, void *d_ap, void *d_diff, hipStream_t stream) {
  if (lead == 0 || count == 0) return;
  if (x_stride < n) throw Failure(format("%s: x_stride is smaller than the signal length", fn));
  if (!d_x || !(d_f0 || d_diff)) throw Failure(format("%s: null device pointer", fn));
  PitchArgs a{};
  a.n = n;
  a.x_stride = x_stride;
  a.frames = count;
  a.border = border;
  a.fl = plan.fl;
  a.hop = plan.hop;
  a.sample_rate = (double)plan.sample_rate;
  a.threshold = plan.threshold;
  a.W = (int)(plan.fl / 2);
  a.pmin = (int)plan.pmin;
  a.pmax = (int)plan.pmax;
  a.lags = a.pmax + 1;
  if (plan.fl > 2147483647LL / 2 || count > (int64_t)1 << 40) throw Failure(format("%s: frames too long or too many", fn));
  const int64_t per_clip = count * a.lags * 8;
  const int64_t step = std::max<int64_t>(1, std::min<int64_t>(lead, kScratchBytes / per_clip));
  init_device_pool();
  DeviceScratch scratch;
  scratch.pool((size_t)(step * per_clip), stream);
  a.r = scratch.as<double>();
  for (int64_t c0 = 0; c0 < lead; c0 += step) {
    a.lead = std::min(step, lead - c0);
    a.total = a.lead * count;
    a.x = (const char *)d_x + c0 * x_stride * elem_bytes;
    a.f0 = d_f0 ? (char *)d_f0 + c0 * count * elem_bytes : nullptr;
    a.ap = d_ap ? (char *)d_ap + c0 * count * elem_bytes : nullptr;
    a.diff = d_diff ? (char *)d_diff + c0 * a.lags * count * elem_bytes : nullptr;
    if (elem_bytes == 8) launch_pitch<double>(fn, a, plan, stream);
    else launch_pitch<float>(fn, a, plan, stream);
  }
}

// the segment call's bookkeeping, as energy_frames'
void check_segment(const char *fn, int64_t fl, int64_t hop, int64_t n, int64_t count) {
  if (count < 0) throw Failure(format("%s: negative frame count", fn));
  if (count > 0 && (n < fl || (n - fl) / hop < count - 1))
    throw Failure(format("%s: %lld frames of %lld samples at hop %lld do not fit a segment of %lld samples", fn, (long long)count, (long long)fl,
                         (long long)hop, (long long)n));
}

enum PitchFace { FACE_YIN = 0, FACE_DIFFERENCE = 1, FACE_FRAMES = 2 };
const char *face_name(int face) { return face == FACE_YIN ? "yin" : face == FACE_DIFFERENCE ? "yin_difference" : "yin_stage"; }

struct PitchCall {
  int face;
  int64_t sample_rate;
  double fmin, fmax;
  int64_t fl, hop;
  double threshold;
  int64_t count;                  // FACE_FRAMES
};

// the parameters, then the extents; the frame count and the plan of the call
PitchPlan check_call(const PitchCall &q, int64_t lead, int64_t n, int64_t &count) {
  const char *fn = face_name(q.face);
  const PitchPlan plan = check_pitch(fn, q.sample_rate, q.fmin, q.fmax, q.fl, q.hop, q.face != FACE_DIFFERENCE, q.threshold);
  check_rank_extents(fn, lead, n);
  if (q.face == FACE_FRAMES) check_segment(fn, q.fl, q.hop, n, q.count);
  count = q.face == FACE_FRAMES ? q.count : count_frames(q.fl, q.hop, n);
  return plan;
}

void pitch_resident(const PitchCall &q, const void *d_x, int64_t lead, int64_t n, int64_t x_stride, void *d_first, void *d_ap, hipStream_t stream) {
  int64_t count = 0;
  const PitchPlan plan = check_call(q, lead, n, count);
  const bool diff = q.face == FACE_DIFFERENCE;
  pitch_dev(face_name(q.face), plan, q.face == FACE_FRAMES ? 0 : q.fl / 2, d_x, 4, lead, n, x_stride, count, diff ? nullptr : d_first,
            diff ? nullptr : d_ap, diff ? d_first : nullptr, stream);
}

void pitch_host(const PitchCall &q, const void *x, int elem_bytes, int64_t lead, int64_t n, void *first, void *ap) {
  const char *fn = face_name(q.face);
  int64_t count = 0;
  const PitchPlan plan = check_call(q, lead, n, count);
  if (lead == 0 || count == 0) return;
  if (!x || !first) throw Failure(format("%s: null pointer", fn));
  const bool diff = q.face == FACE_DIFFERENCE;
  const size_t row = (size_t)count * (size_t)elem_bytes;
  const int64_t border = q.face == FACE_FRAMES ? 0 : q.fl / 2;
  host_call(fn, {{x, (size_t)n * (size_t)elem_bytes}}, {HostOut{first, diff ? row * (size_t)(plan.pmax + 1) : row}, HostOut{diff ? nullptr : ap, row}},
            lead, false, nullptr, [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t stream) {
              pitch_dev(fn, plan, border, d_in[0], elem_bytes, nc, n, n, count, diff ? nullptr : d_out[0], diff ? nullptr : d_out[1],
                        diff ? d_out[0] : nullptr, stream);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Pitch ---------------------------------------------------------------------------------------------------------------------
int smx_yin_f32(const float *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop,
                double trough_threshold, float *f0, float *aperiodicity) {
  return guarded([&] { pitch_host({FACE_YIN, sample_rate, fmin, fmax, frame_length, hop, trough_threshold, 0}, x, 4, lead, n, f0, aperiodicity); });
}
int smx_yin_f64(const double *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop,
                double trough_threshold, double *f0, double *aperiodicity) {
  return guarded([&] { pitch_host({FACE_YIN, sample_rate, fmin, fmax, frame_length, hop, trough_threshold, 0}, x, 8, lead, n, f0, aperiodicity); });
}
int smx_yin_resident_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t sample_rate, double fmin, double fmax,
                         int64_t frame_length, int64_t hop, double trough_threshold, float *d_f0, float *d_aperiodicity, void *stream) {
  return guarded([&] {
    pitch_resident({FACE_YIN, sample_rate, fmin, fmax, frame_length, hop, trough_threshold, 0}, d_x, lead, n, x_stride, d_f0, d_aperiodicity,
                   (hipStream_t)stream);
  });
}
int smx_yin_difference_f32(const float *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                           int64_t hop, float *out) {
  return guarded([&] { pitch_host({FACE_DIFFERENCE, sample_rate, fmin, fmax, frame_length, hop, 0.0, 0}, x, 4, lead, n, out, nullptr); });
}
int smx_yin_difference_f64(const double *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                           int64_t hop, double *out) {
  return guarded([&] { pitch_host({FACE_DIFFERENCE, sample_rate, fmin, fmax, frame_length, hop, 0.0, 0}, x, 8, lead, n, out, nullptr); });
}
int smx_yin_difference_resident_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t sample_rate, double fmin, double fmax,
                                    int64_t frame_length, int64_t hop, float *d_out, void *stream) {
  return guarded([&] {
    pitch_resident({FACE_DIFFERENCE, sample_rate, fmin, fmax, frame_length, hop, 0.0, 0}, d_x, lead, n, x_stride, d_out, nullptr, (hipStream_t)stream);
  });
}
int smx_yin_frames_f32(const float *x, int64_t lead, int64_t n, int64_t count, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                       int64_t hop, double trough_threshold, float *f0, float *aperiodicity) {
  return guarded([&] { pitch_host({FACE_FRAMES, sample_rate, fmin, fmax, frame_length, hop, trough_threshold, count}, x, 4, lead, n, f0, aperiodicity); });
}
int smx_yin_frames_f64(const double *x, int64_t lead, int64_t n, int64_t count, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                       int64_t hop, double trough_threshold, double *f0, double *aperiodicity) {
  return guarded([&] { pitch_host({FACE_FRAMES, sample_rate, fmin, fmax, frame_length, hop, trough_threshold, count}, x, 8, lead, n, f0, aperiodicity); });
}
int smx_yin_frames_resident_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t count, int64_t sample_rate, double fmin,
                                double fmax, int64_t frame_length, int64_t hop, double trough_threshold, float *d_f0, float *d_aperiodicity,
                                void *stream) {
  return guarded([&] {
    pitch_resident({FACE_FRAMES, sample_rate, fmin, fmax, frame_length, hop, trough_threshold, count}, d_x, lead, n, x_stride, d_f0, d_aperiodicity,
                   (hipStream_t)stream);
  });
}

}  // extern "C"
