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
// pYIN's observation (pyin_trough_kernel, pyin_observe_kernel) follows yin's kernels below and shares the walk of d' with the finish
// kernel (walk_lags); its decoder is pyin.hip.
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
using WalkTile = T[2][64][kSteps + 1];                      // rows 33 apart: lane f on row f meets no other lane's bank

// the frame of a lane of the walk
struct WalkLane {
  int lane;
  int64_t g, clip, p;                                       // the frame among the launch's, its clip and its index there
  bool live;
};

__device__ __forceinline__ WalkLane walk_lane(const PitchArgs &a) {
  WalkLane w;
  w.lane = threadIdx.x;
  w.g = (int64_t)blockIdx.x * 64 + w.lane;
  w.live = w.g < a.total;
  w.clip = w.live ? w.g / a.frames : 0;
  w.p = w.live ? w.g % a.frames : 0;
  return w;
}

// THE walk of d': P, e, d, c and d'(tau) for tau = 1 .. pmax in ascending order, on_lag(tau, d'(tau)) as each goes by; e(0) and
// c(pmax) are left in e0 and c.  yin's choice and pYIN's troughs are both made from this one statement.
template <typename T, typename F>
__device__ __forceinline__ void walk_lags(const PitchArgs &a, const WalkLane &w, WalkTile<T> &tile, double &e0, double &c, F &&on_lag) {
  const int lane = w.lane;
  const bool live = w.live;
  const long long row_at = w.clip * a.x_stride, s0 = w.p * a.hop - a.border;   // the frame's first padded position as a signal index
  const T *x = reinterpret_cast<const T *>(a.x);
  const double *col = a.r + (live ? w.g : 0);               // lag tau at col[tau total]

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

  double upper = 0.0, lower = 0.0;                          // P(tau + W), P(tau)
  c = 0.0;
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
  e0 = upper;

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
        on_lag(tau, c == 0.0 ? 1.0 : (d * (double)tau) / c);
      }
    }
    __syncthreads();
  }
}

// the parabola through d' around a lag with both neighbours in [1, pmax]: the shift of its vertex, 0 where it has none
__device__ __forceinline__ double parabolic_shift(double u, double v, double w) {
  const double den = (u - 2.0 * v) + w;
  if (den > 0.0) {
    const double s = (0.5 * (u - w)) / den;
    if (fabs(s) <= 1.0) return s;
  }
  return 0.0;
}

template <typename T>
__global__ void __launch_bounds__(64) yin_finish_kernel(PitchArgs a) {
  __shared__ WalkTile<T> tile;
  const WalkLane w = walk_lane(a);
  const int64_t g = w.g;
  T *diff = a.diff && w.live ? reinterpret_cast<T *>(a.diff) + w.clip * a.lags * a.frames + w.p : nullptr;
  const bool choose = a.f0 != nullptr;
  if (diff) diff[0] = (T)1.0;

  // the choice, as the lags go by: the first trough below the threshold, and the least d' with the smallest lag
  bool found = false;
  int trough = 0, lowest = 0;
  double before = 1.0, here = 1.0;                          // d'(tau - 2), d'(tau - 1)
  double ta = 0.0, tb = 0.0, tc = 0.0, la = 0.0, lb = 0.0, lc = 0.0;   // d' around the trough and around the least
  double e0, c;
  walk_lags<T>(a, w, tile, e0, c, [&](int tau, double dn) {
    if (diff) diff[(int64_t)tau * a.frames] = (T)dn;
    if (choose && tau - 1 >= a.pmin) {                      // lag tau - 1 has both neighbours now
      if (!found && here < a.threshold && here <= before && here < dn) found = true, trough = tau - 1, ta = before, tb = here, tc = dn;
      if (tau - 1 == a.pmin || here < lb) lowest = tau - 1, la = before, lb = here, lc = dn;
    }
    before = here;
    here = dn;
  });
  if (!choose || !w.live) return;
  // lag pmax has no neighbour behind it
  if (!found && here < a.threshold && here <= before) found = true, trough = a.pmax, ta = before, tb = here;
  if (here < lb) lowest = a.pmax, la = before, lb = here;
  const int chosen = found ? trough : lowest;
  const double u = found ? ta : la, v = found ? tb : lb, wn = found ? tc : lc;
  const double shift = chosen - 1 >= 1 && chosen + 1 <= a.pmax ? parabolic_shift(u, v, wn) : 0.0;
  double f0 = a.sample_rate / ((double)chosen + shift), ap = v;
  // a non-finite sample: the frame has no pitch and no voicing measure
  if (!isfinite(e0) || !isfinite(c)) f0 = ap = __builtin_nan("");
  reinterpret_cast<T *>(a.f0)[g] = (T)f0;
  if (a.ap) reinterpret_cast<T *>(a.ap)[g] = (T)ap;
}

// ---- pYIN's observation -----------------------------------------------------------------------------------------
//   pyin_trough_kernel    the walk above, a lane per frame: every trough of d' in [pmin, pmax] as the lags go by, its height and the
//                         pitch bin of its refined period (a binary search of the host-built edges: comparisons only), into scratch
//                         [trough][frame]; the count per frame, -1 for a frame yin would give NaN
//   pyin_observe_kernel   a wave per frame, a lane per trough: the thresholds in ascending order, N_k and q(r, k) from one ballot each;
//                         then a lane per pitch bin adds the troughs that land in it in ascending order, and the wave adds the bins
struct PyinArgs {
  const double *thr, *beta, *cb, *E, *Z, *edge;   // the host tables; cb[K] = beta[0] + .. + beta[K - 1], ascending
  double *tg;                     // scratch: heights [maxr][total]
  int *tbin, *tcnt;               // bins [maxr][total], troughs per frame [total]
  unsigned char *work;            // kTroughBytes per trough and frame where a frame's troughs do not fit LDS, else null
  double *s_rest, *s_value;       // the sparse float64 observation for the decoder, or null: per frame the unvoiced states' value,
  int *s_count, *s_bin;           // the number of occupied voiced bins, their bins (ascending) and values [frame][maxr]
  void *out, *prob;               // [lead; 2 n_bins; frames] and [lead; frames] in the dtype of the input, each may be null
  int64_t frames, total;
  double no_trough;
  int nthr, n_bins, maxr;
};
constexpr int kTroughBytes = 24;  // height, probability, bin (padded)

template <typename T>
__global__ void __launch_bounds__(64) pyin_trough_kernel(PitchArgs a, PyinArgs q) {
  __shared__ WalkTile<T> tile;
  const WalkLane w = walk_lane(a);
  int count = 0;
  // a trough at tau with d' u, v, wn around it (inner: both neighbours exist)
  auto emit = [&](int tau, double u, double v, double wn, bool inner) {
    const double shift = inner ? parabolic_shift(u, v, wn) : 0.0;
    const double f = a.sample_rate / ((double)tau + shift);
    int lo = 0, hi = q.n_bins - 1;                          // the number of edges <= f: edge[1 .. n_bins - 1] ascend
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (q.edge[mid] <= f) lo = mid;
      else hi = mid - 1;
    }
    if (w.live && count < q.maxr) {
      q.tg[(int64_t)count * a.total + w.g] = v;
      q.tbin[(int64_t)count * a.total + w.g] = lo;
    }
    ++count;
  };
  double before = 1.0, here = 1.0, e0, c;                   // d'(tau - 2), d'(tau - 1)
  walk_lags<T>(a, w, tile, e0, c, [&](int tau, double dn) {
    if (tau - 1 >= a.pmin && here <= before && here < dn) emit(tau - 1, before, here, dn, true);   // pmin >= 2: tau - 2 >= 1
    before = here;
    here = dn;
  });
  if (!w.live) return;
  if (here <= before) emit(a.pmax, before, here, 0.0, false);
  if (count > q.maxr) count = q.maxr;                       // (non-adjacent lags: it cannot be)
  q.tcnt[w.g] = isfinite(e0) && isfinite(c) ? count : -1;
}

template <typename T>
__global__ void __launch_bounds__(64) pyin_observe_kernel(PyinArgs q) {
  extern __shared__ __align__(16) unsigned char trough_lds[];
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x, clip = g / q.frames, p = g % q.frames;
  unsigned char *base = q.work ? q.work + (size_t)g * (size_t)q.maxr * kTroughBytes : trough_lds;
  double *height = reinterpret_cast<double *>(base), *prob = height + q.maxr;
  int *bin = reinterpret_cast<int *>(prob + q.maxr);
  int R = q.tcnt[g];
  const bool sound = R >= 0;
  R = R < 0 ? 0 : R > q.maxr ? q.maxr : R;
  for (int r = lane; r < R; r += 64) {
    height[r] = q.tg[(int64_t)r * q.total + g];
    bin[r] = q.tbin[(int64_t)r * q.total + g];
    prob[r] = 0.0;
  }
  __syncthreads();
  const unsigned long long behind = (1ull << lane) - 1ull;
  for (int k = 1; k <= q.nthr; ++k) {
    const double thr = q.thr[k], bk = q.beta[k - 1];
    int N = 0;
    for (int r0 = 0; r0 < R; r0 += 64) N += __popcll(__ballot(r0 + lane < R && height[r0 + lane] < thr));
    if (N == 0) continue;
    const double z = q.Z[N];
    int seen = 0;
    for (int r0 = 0; r0 < R; r0 += 64) {
      const int r = r0 + lane;
      const bool below = r < R && height[r] < thr;
      const unsigned long long mask = __ballot(below);
      if (below) prob[r] = prob[r] + (z * q.E[seen + __popcll(mask & behind)]) * bk;
      seen += __popcll(mask);
    }
  }
  __syncthreads();
  if (R > 0) {
    int least = 0;                                          // the first trough of least height (every lane walks them all)
    double low = height[0];
    for (int r = 1; r < R; ++r)
      if (height[r] < low) low = height[r], least = r;
    int K0 = 0;
    for (int k0 = 1; k0 <= q.nthr; k0 += 64) K0 += __popcll(__ballot(k0 + lane <= q.nthr && q.thr[k0 + lane <= q.nthr ? k0 + lane : 0] <= low));
    if (lane == 0 && K0 < q.nthr) prob[least] = prob[least] + q.no_trough * q.cb[K0];   // no threshold above it (d' = 1, silence): no share
  }
  __syncthreads();
  const double nan = __builtin_nan("");
  const int64_t S = 2 * q.n_bins;
  T *out = q.out ? reinterpret_cast<T *>(q.out) + (clip * S) * q.frames + p : nullptr;
  double vp = 0.0;
  int occupied = 0;
  for (int b0 = 0; b0 < q.n_bins; b0 += 64) {
    const int b = b0 + lane;
    double acc = 0.0;
    if (b < q.n_bins) {
      for (int r = 0; r < R; ++r)
        if (bin[r] == b && prob[r] > 0.0) acc = acc + prob[r];
      if (out) out[(int64_t)b * q.frames] = sound ? (T)acc : (T)nan;
    }
    unsigned long long mask = __ballot(acc != 0.0);         // the bins in ascending order; a zero adds nothing
    if (q.s_value && acc != 0.0) {                          // (at most one bin per trough: occupied stays below maxr)
      const int at = occupied + __popcll(mask & behind);
      if (at < q.maxr) q.s_bin[g * q.maxr + at] = b, q.s_value[g * q.maxr + at] = acc;
    }
    occupied += __popcll(mask);
    while (mask) {
      vp = vp + __shfl(acc, __ffsll((long long)mask) - 1);
      mask &= mask - 1ull;
    }
  }
  vp = vp > 1.0 ? 1.0 : vp;
  const double rest = (1.0 - vp) / (double)q.n_bins;
  if (out)
    for (int b = lane; b < q.n_bins; b += 64) out[(int64_t)(q.n_bins + b) * q.frames] = sound ? (T)rest : (T)nan;
  if (q.s_value && lane == 0) q.s_rest[g] = rest, q.s_count[g] = occupied < q.maxr ? occupied : q.maxr;
  if (q.prob && lane == 0) reinterpret_cast<T *>(q.prob)[g] = sound ? (T)vp : (T)nan;
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

// the correlation into a.r, then yin's finish or, with `troughs`, pYIN's collection of them
template <typename T>
void launch_pitch(const char *fn, PitchArgs a, const PitchPlan &plan, hipStream_t stream, const PyinArgs *troughs = nullptr) {
  a.tile_frames = tile_frames(plan, (int)sizeof(T));
  if (a.tile_frames) {
    if constexpr (sizeof(T) == 4) {
      a.tiles = (a.frames + a.tile_frames - 1) / a.tile_frames;
      const dim3 grid(grid_x(fn, "frame tiles", a.lead * a.tiles, 256));
      a.nfull = (int)(a.W / a.hop);
      a.rest = (int)(a.W - a.nfull * a.hop);
      a.groups = (a.pmax + kLags) / kLags;
      const size_t lds = (size_t)((a.tile_frames - 1) * a.hop + a.fl + kSlack) * 4 +
                         (size_t)(a.tile_frames + a.nfull) * a.groups * kLags * 8 * (a.rest ? 2 : 1);
      SMX_LAUNCH(yin_tile_kernel, grid, dim3(256), lds, stream, a);
    }
  } else {
    SMX_LAUNCH((yin_general_kernel<T>), dim3(grid_x(fn, "frames", a.total, 256)), dim3(256), 0, stream, a);   // a workgroup per frame
  }
  SMX_HIP_CHECK(hipGetLastError());
  const dim3 waves(grid_x(fn, "frames", (a.total + 63) / 64, 64));
  if (troughs) SMX_LAUNCH((pyin_trough_kernel<T>), waves, dim3(64), 0, stream, a, *troughs);
  else SMX_LAUNCH((yin_finish_kernel<T>), waves, dim3(64), 0, stream, a);
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
  // a clip range fits the scratch and one launch of a workgroup per frame (DESIGN.md "Launch extents"); one clip that does not is refused
  const int64_t step = std::max<int64_t>(1, std::min({lead, kScratchBytes / per_clip, clips_per_launch(count, 256)}));
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

// ---- pYIN: the parameters, the host tables, the observation and the call of the decoder (pyin.hip) ------------------------------
struct PyinParams {
  int64_t sample_rate;
  double fmin, fmax;
  int64_t fl, hop, nthr;
  double a, b, lambda, resolution, rate, switch_prob, no_trough;
};

struct PyinPlan {
  PitchPlan pitch;
  PyinParams q;
  int64_t bps, n_bins, h, maxr;   // maxr: the most troughs of a frame (no two lie at adjacent lags)
};

// bins per semitone and the bin count; resolution has been checked.  A count past every cap comes back as 2^40.
void pitch_bins(double fmin, double fmax, double resolution, int64_t &bps, int64_t &n_bins) {
  const double per = std::ceil(1.0 / resolution);
  const double count = std::floor(12.0 * per * std::log2(fmax / fmin)) + 1.0;
  bps = per < 0x1p40 ? (int64_t)per : (int64_t)1 << 40;
  n_bins = count < 0x1p40 ? (int64_t)count : (int64_t)1 << 40;
}

void check_resolution(const char *fn, double resolution) {
  if (!(resolution > 0.0 && resolution < 1.0))
    throw InvalidArgument(format("%s: cannot resolve pitch to %g semitones (resolution must lie in (0, 1))", fn, resolution));
}

// h = (m bps) / 2 with m = round-half-even(max_transition_rate 12 hop / sample_rate); the parameters have been checked
int64_t half_width(const char *fn, int64_t sample_rate, int64_t hop, int64_t bps, double rate) {
  const double m = std::nearbyint(rate * 12.0 * (double)hop / (double)sample_rate);
  if (!(m * (double)bps < 0x1p31))
    throw InvalidArgument(format("%s: cannot let the pitch move by %g octaves per second (the band must span fewer than 2^31 bins)", fn, rate));
  return ((int64_t)m * bps) / 2;
}

void check_rate(const char *fn, double rate) {
  if (!(std::isfinite(rate) && rate >= 0.0))
    throw InvalidArgument(format("%s: cannot let the pitch move by %g octaves per second (max_transition_rate must be finite and not negative)", fn, rate));
}

// yin's own checks first, then pYIN's in the header's order; `decode`: the call runs the decoder
PyinPlan check_pyin(const char *fn, const PyinParams &q, bool decode) {
  PyinPlan plan{};
  plan.pitch = check_pitch(fn, q.sample_rate, q.fmin, q.fmax, q.fl, q.hop, false, 0.0);
  plan.q = q;
  if (q.nthr < 1) throw InvalidArgument(format("%s: cannot integrate over %lld thresholds (n_thresholds must be at least 1)", fn, (long long)q.nthr));
  if (!(std::isfinite(q.a) && std::isfinite(q.b) && q.a > 0.0 && q.b > 0.0))
    throw InvalidArgument(format("%s: cannot weigh the thresholds by a beta distribution with parameters %g and %g (beta_parameters must be finite and positive)",
                                 fn, q.a, q.b));
  if (!(std::isfinite(q.lambda) && q.lambda > 0.0))
    throw InvalidArgument(format("%s: cannot weigh the troughs with a Boltzmann parameter of %g (boltzmann_parameter must be finite and positive)", fn, q.lambda));
  check_resolution(fn, q.resolution);
  check_rate(fn, q.rate);
  if (!(q.switch_prob >= 0.0 && q.switch_prob <= 1.0))
    throw InvalidArgument(format("%s: cannot switch voicing with probability %g (switch_prob must lie in [0, 1])", fn, q.switch_prob));
  if (!(q.no_trough >= 0.0 && q.no_trough <= 1.0))
    throw InvalidArgument(format("%s: cannot give a frame without a trough the probability %g (no_trough_prob must lie in [0, 1])", fn, q.no_trough));
  pitch_bins(q.fmin, q.fmax, q.resolution, plan.bps, plan.n_bins);
  if (2 * plan.n_bins > 65535)
    throw InvalidArgument(format("%s: cannot decode %lld states (2 n_bins must be at most 65535)", fn, (long long)(2 * plan.n_bins)));
  plan.h = half_width(fn, q.sample_rate, q.hop, plan.bps, q.rate);
  if (decode) check_pyin_decode(fn, plan.n_bins, plan.h, q.switch_prob);
  if (q.nthr > 2147483646LL) throw Failure(format("%s: too many thresholds", fn));
  plan.maxr = (plan.pitch.pmax - plan.pitch.pmin) / 2 + 1;
  return plan;
}

// the continued fraction of the incomplete beta function (modified Lentz)
double beta_fraction(double a, double b, double x) {
  const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (std::fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 10000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < 1e-16) break;
  }
  return h;
}

// the regularised incomplete beta function I(x; a, b)
double beta_cdf(double a, double b, double x) {
  if (x <= 0.0) return 0.0;
  if (x >= 1.0) return 1.0;
  const double front = std::exp(std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x));
  return x < (a + 1.0) / (a + b + 2.0) ? front * beta_fraction(a, b, x) / a : 1.0 - front * beta_fraction(b, a, 1.0 - x) / b;
}

struct PyinTables {
  std::vector<double> thr, beta, cb, E, Z, freq, edge;     // edge[0] is not an edge (0.0); cb[K] = beta[0] + .. + beta[K - 1]
};

PyinTables pyin_tables(const PyinPlan &p) {
  PyinTables t;
  const int64_t n = p.q.nthr;
  t.thr.resize((size_t)n + 1), t.beta.resize((size_t)n), t.cb.resize((size_t)n + 1);
  for (int64_t k = 0; k <= n; ++k) t.thr[(size_t)k] = (double)k / (double)n;
  double before = beta_cdf(p.q.a, p.q.b, t.thr[0]);
  t.cb[0] = 0.0;
  for (int64_t k = 0; k < n; ++k) {
    const double here = beta_cdf(p.q.a, p.q.b, t.thr[(size_t)k + 1]);
    t.beta[(size_t)k] = here - before;
    t.cb[(size_t)k + 1] = t.cb[(size_t)k] + t.beta[(size_t)k];
    before = here;
  }
  t.E.resize((size_t)p.maxr), t.Z.resize((size_t)p.maxr + 1);
  for (int64_t q = 0; q < p.maxr; ++q) t.E[(size_t)q] = std::exp(-p.q.lambda * (double)q);
  t.Z[0] = 0.0;
  for (int64_t N = 1; N <= p.maxr; ++N) t.Z[(size_t)N] = (1.0 - std::exp(-p.q.lambda)) / (1.0 - std::exp(-p.q.lambda * (double)N));
  t.freq.resize((size_t)p.n_bins), t.edge.resize((size_t)p.n_bins);
  const double per = (double)(12 * p.bps);
  for (int64_t b = 0; b < p.n_bins; ++b) {
    t.freq[(size_t)b] = p.q.fmin * std::exp2((double)b / per);
    t.edge[(size_t)b] = b ? p.q.fmin * std::exp2(((double)b - 0.5) / per) : 0.0;
  }
  return t;
}

void band_tables(int64_t n_bins, int64_t h, double *tri, double *rs) {
  if (tri)
    for (int64_t k = 0; k <= 2 * h; ++k) tri[k] = pyin_triangle(k, h);
  if (rs) pyin_band_scale(n_bins, h, rs);
}

// thr, beta, cb, E, Z, freq, edge in one allocation, in this order
std::shared_ptr<void> pyin_device_tables(const PyinPlan &p) {
  const PyinParams &q = p.q;
  return cached_table(format("pyin|%lld|%a|%a|%lld|%lld|%lld|%a|%a|%a|%a", (long long)q.sample_rate, q.fmin, q.fmax, (long long)q.fl, (long long)q.hop,
                             (long long)q.nthr, q.a, q.b, q.lambda, q.resolution),
                      [&] {
                        const PyinTables t = pyin_tables(p);
                        std::vector<unsigned char> out;
                        for (const std::vector<double> *v : {&t.thr, &t.beta, &t.cb, &t.E, &t.Z, &t.freq, &t.edge}) {
                          const unsigned char *b = reinterpret_cast<const unsigned char *>(v->data());
                          out.insert(out.end(), b, b + v->size() * sizeof(double));
                        }
                        return out;
                      });
}

struct PyinOut {
  void *obs;                      // pyin_observation [lead; 2 n_bins; count], or null and
  void *f0, *flag, *prob;         // pyin's three [lead; count]
  bool keep_bin;
  double fill;
};

void pyin_dev(const char *fn, const PyinPlan &p, const void *d_x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride, int64_t count,
              const PyinOut &out, hipStream_t stream) {
  if (lead == 0 || count == 0) return;
  if (x_stride < n) throw Failure(format("%s: x_stride is smaller than the signal length", fn));
  const bool decode = !out.obs;
  if (!d_x || (decode && !(out.f0 && out.flag && out.prob))) throw Failure(format("%s: null device pointer", fn));
  const PitchPlan &plan = p.pitch;
  if (plan.fl > 2147483647LL / 2 || count > (int64_t)1 << 40) throw Failure(format("%s: frames too long or too many", fn));
  PitchArgs a{};
  a.n = n, a.x_stride = x_stride, a.frames = count, a.border = plan.fl / 2, a.fl = plan.fl, a.hop = plan.hop;
  a.sample_rate = (double)plan.sample_rate;
  a.W = (int)(plan.fl / 2), a.pmin = (int)plan.pmin, a.pmax = (int)plan.pmax, a.lags = a.pmax + 1;
  const int64_t S = 2 * p.n_bins, nthr = p.q.nthr, maxr = p.maxr;
  const bool in_lds = maxr * kTroughBytes <= 60 * 1024;
  // per clip: the observation's scratch (r, the troughs), the sparse observation kept for the decoder, the decoder's pointers.
  // A decode group of D clips keeps its sparse observations and its pointers, and the observation goes through it O clips at a time,
  // all within kScratchBytes: the decoder is a serial chain per clip, so a launch of fewer clips than compute units costs as much
  // as a full one, while the observation's kernels lose nothing by going range by range.
  const int64_t o_bytes = count * (a.lags * 8 + maxr * 12 + 4 + (in_lds ? 0 : maxr * kTroughBytes));
  const int64_t s_bytes = decode ? count * (maxr * 12 + 12) : 0, b_bytes = decode ? pyin_decode_scratch(count, p.n_bins, p.h) : 0;
  const int64_t D = decode ? std::max<int64_t>(1, std::min<int64_t>(lead, kScratchBytes / (s_bytes + b_bytes))) : lead;
  const int64_t O = std::max<int64_t>(1, std::min({D, (kScratchBytes - (decode ? D * (s_bytes + b_bytes) : 0)) / o_bytes, clips_per_launch(count, 256)}));
  const auto tables = pyin_device_tables(p);
  init_device_pool();
  DeviceScratch scratch, kept;
  scratch.pool((size_t)(O * o_bytes + 64), stream);
  if (decode) kept.pool((size_t)(D * s_bytes + 64), stream);
  PyinArgs q{};
  q.thr = reinterpret_cast<const double *>(tables.get());
  q.beta = q.thr + nthr + 1, q.cb = q.beta + nthr, q.E = q.cb + nthr + 1, q.Z = q.E + maxr;
  const double *freq = q.Z + maxr + 1;
  q.edge = freq + p.n_bins;
  const int64_t all = O * count, held = D * count;            // the doubles first, then the bytes, then the ints
  a.r = scratch.as<double>();
  q.tg = a.r + a.lags * all;
  unsigned char *work = reinterpret_cast<unsigned char *>(q.tg + maxr * all);
  q.tbin = reinterpret_cast<int *>(work + (in_lds ? 0 : maxr * kTroughBytes * all));
  q.tcnt = q.tbin + maxr * all;
  double *s_value = decode ? kept.as<double>() : nullptr, *s_rest = decode ? s_value + maxr * held : nullptr;
  int *s_bin = decode ? reinterpret_cast<int *>(s_rest + held) : nullptr, *s_count = decode ? s_bin + maxr * held : nullptr;
  q.frames = count, q.no_trough = p.q.no_trough;
  q.nthr = (int)nthr, q.n_bins = (int)p.n_bins, q.maxr = (int)maxr;
  q.work = in_lds ? nullptr : work;
  const size_t lds = in_lds ? (size_t)(maxr * kTroughBytes) : 0;
  for (int64_t d0 = 0; d0 < lead; d0 += D) {
    const int64_t nd = std::min(D, lead - d0);
    for (int64_t c0 = d0; c0 < d0 + nd; c0 += O) {
      a.lead = std::min(O, d0 + nd - c0);
      a.total = q.total = a.lead * count;
      a.x = (const char *)d_x + c0 * x_stride * elem_bytes;
      if (elem_bytes == 8) launch_pitch<double>(fn, a, plan, stream, &q);
      else launch_pitch<float>(fn, a, plan, stream, &q);
      const int64_t at = (c0 - d0) * count;                  // the range's first frame among the group's
      q.s_value = decode ? s_value + at * maxr : nullptr, q.s_bin = decode ? s_bin + at * maxr : nullptr;
      q.s_rest = decode ? s_rest + at : nullptr, q.s_count = decode ? s_count + at : nullptr;
      q.out = out.obs ? (char *)out.obs + c0 * S * count * elem_bytes : nullptr;
      q.prob = out.prob ? (char *)out.prob + c0 * count * elem_bytes : nullptr;
      if (elem_bytes == 8) launch_tiles(fn, pyin_observe_kernel<double>, a.total, 64, lds, stream, q);
      else launch_tiles(fn, pyin_observe_kernel<float>, a.total, 64, lds, stream, q);
    }
    if (!decode) continue;
    PyinDecodeJob job{};
    job.fn = fn;
    job.d_rest = s_rest, job.d_value = s_value, job.d_count = s_count, job.d_bin = s_bin, job.list = maxr;
    job.lead = nd, job.frames = count, job.n_bins = p.n_bins, job.half_width = p.h;
    job.switch_prob = p.q.switch_prob;
    job.elem_bytes = elem_bytes;
    job.d_f0 = (char *)out.f0 + d0 * count * elem_bytes, job.d_flag = (char *)out.flag + d0 * count * elem_bytes;
    job.d_freq = freq, job.keep_bin = out.keep_bin, job.fill = out.fill;
    job.stream = stream;
    launch_pyin_decode(job);
  }
}

void pyin_call(bool device, bool observation, const PyinParams &q, const void *x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride, PyinOut out,
               hipStream_t stream) {
  const char *fn = observation ? "pyin_observation" : "pyin";
  const PyinPlan p = check_pyin(fn, q, !observation);
  check_rank_extents(fn, lead, n);
  const int64_t count = count_frames(q.fl, q.hop, n);
  if (lead == 0 || count == 0) return;
  if (device) {
    if (observation && !out.obs) throw Failure(format("%s: null device pointer", fn));
    pyin_dev(fn, p, x, elem_bytes, lead, n, x_stride, count, out, stream);
    return;
  }
  if (!x || (observation ? !out.obs : !(out.f0 && out.flag && out.prob))) throw Failure(format("%s: null pointer", fn));
  const size_t row = (size_t)count * (size_t)elem_bytes;
  const std::vector<HostOut> outs =
      observation ? std::vector<HostOut>{HostOut{out.obs, row * (size_t)(2 * p.n_bins)}} : std::vector<HostOut>{HostOut{out.f0, row}, HostOut{out.flag, row}, HostOut{out.prob, row}};
  host_call(fn, {{x, (size_t)n * (size_t)elem_bytes}}, outs, lead, false, nullptr, [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t st) {
    PyinOut part = out;
    if (observation) part.obs = d_out[0];
    else part.f0 = d_out[0], part.flag = d_out[1], part.prob = d_out[2];
    pyin_dev(fn, p, d_in[0], elem_bytes, nc, n, n, count, part, st);
  });
}

}  // namespace
}  // namespace smx

using namespace smx;

// the parameters of the pYIN entry points, in the header's order
#define SMX_PYIN_PARAMS                                                                                                                      \
  int64_t sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop, int64_t n_thresholds, double beta_a, double beta_b,      \
      double boltzmann_parameter, double resolution, double max_transition_rate, double switch_prob, double no_trough_prob
#define SMX_PYIN_PACK \
  PyinParams { sample_rate, fmin, fmax, frame_length, hop, n_thresholds, beta_a, beta_b, boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob }

extern "C" {

// ---- pYIN ----------------------------------------------------------------------------------------------------------------------
int smx_pyin_f32(const float *x, int64_t lead, int64_t n, SMX_PYIN_PARAMS, int64_t keep_bin, double fill, float *f0, float *voiced_flag, float *voiced_prob) {
  return guarded([&] { pyin_call(false, false, SMX_PYIN_PACK, x, 4, lead, n, n, PyinOut{nullptr, f0, voiced_flag, voiced_prob, keep_bin != 0, fill}, nullptr); });
}
int smx_pyin_f64(const double *x, int64_t lead, int64_t n, SMX_PYIN_PARAMS, int64_t keep_bin, double fill, double *f0, double *voiced_flag,
                 double *voiced_prob) {
  return guarded([&] { pyin_call(false, false, SMX_PYIN_PACK, x, 8, lead, n, n, PyinOut{nullptr, f0, voiced_flag, voiced_prob, keep_bin != 0, fill}, nullptr); });
}
int smx_pyin_accel_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, SMX_PYIN_PARAMS, int64_t keep_bin, double fill, float *d_f0,
                       float *d_voiced_flag, float *d_voiced_prob, void *stream) {
  return guarded([&] {
    pyin_call(true, false, SMX_PYIN_PACK, d_x, 4, lead, n, x_stride, PyinOut{nullptr, d_f0, d_voiced_flag, d_voiced_prob, keep_bin != 0, fill},
              (hipStream_t)stream);
  });
}
int smx_pyin_observation_f32(const float *x, int64_t lead, int64_t n, SMX_PYIN_PARAMS, float *out) {
  return guarded([&] { pyin_call(false, true, SMX_PYIN_PACK, x, 4, lead, n, n, PyinOut{out, nullptr, nullptr, nullptr, false, 0.0}, nullptr); });
}
int smx_pyin_observation_f64(const double *x, int64_t lead, int64_t n, SMX_PYIN_PARAMS, double *out) {
  return guarded([&] { pyin_call(false, true, SMX_PYIN_PACK, x, 8, lead, n, n, PyinOut{out, nullptr, nullptr, nullptr, false, 0.0}, nullptr); });
}
int smx_pyin_observation_accel_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, SMX_PYIN_PARAMS, float *d_out, void *stream) {
  return guarded(
      [&] { pyin_call(true, true, SMX_PYIN_PACK, d_x, 4, lead, n, x_stride, PyinOut{d_out, nullptr, nullptr, nullptr, false, 0.0}, (hipStream_t)stream); });
}
int smx_pyin_bins(double fmin, double fmax, double resolution, int64_t *n_bins) {
  return guarded([&] {
    if (!(std::isfinite(fmin) && std::isfinite(fmax) && 0.0 < fmin && fmin < fmax))
      throw InvalidArgument(format("pyin_bins: cannot lay bins between %g and %g Hz (fmin and fmax must be finite with 0 < fmin < fmax)", fmin, fmax));
    check_resolution("pyin_bins", resolution);
    int64_t bps = 0, count = 0;
    pitch_bins(fmin, fmax, resolution, bps, count);
    if (n_bins) *n_bins = count;
  });
}
int smx_pyin_half_width(int64_t sample_rate, int64_t hop, double resolution, double max_transition_rate, int64_t *half) {
  return guarded([&] {
    const char *fn = "pyin_half_width";
    if (sample_rate < 1) throw InvalidArgument(format("%s: cannot analyse audio sampled at %lld Hz (sample_rate must be at least 1)", fn, (long long)sample_rate));
    if (hop < 1) throw InvalidArgument(format("%s: cannot advance frames by %lld samples (hop must be at least 1)", fn, (long long)hop));
    check_resolution(fn, resolution);
    check_rate(fn, max_transition_rate);
    const int64_t h = half_width(fn, sample_rate, hop, (int64_t)std::ceil(1.0 / resolution), max_transition_rate);
    if (half) *half = h;
  });
}
// thr [n + 1], beta [n], E [maxr], Z [maxr + 1] (Z[0] = 0), freq [n_bins], edge [n_bins - 1] (b = 1 ..), tri [2 h + 1], rs [n_bins] with
// maxr = (pmax - pmin) / 2 + 1; each may be null
int smx_pyin_tables(SMX_PYIN_PARAMS, double *thr, double *beta, double *E, double *Z, double *freq, double *edge, double *tri, double *rs) {
  return guarded([&] {
    const PyinPlan p = check_pyin("pyin_tables", SMX_PYIN_PACK, false);
    const PyinTables t = pyin_tables(p);
    auto copy = [](const std::vector<double> &v, double *to, size_t from = 0) {
      if (to) std::copy(v.begin() + (std::ptrdiff_t)from, v.end(), to);
    };
    copy(t.thr, thr), copy(t.beta, beta), copy(t.E, E), copy(t.Z, Z), copy(t.freq, freq), copy(t.edge, edge, 1);
    band_tables(p.n_bins, p.h, tri, rs);
  });
}

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
