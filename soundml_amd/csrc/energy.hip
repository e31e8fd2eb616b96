// Frame energy features (energy.ml): root-mean-square energy and zero-crossing rate over device-resident audio [lead; n]
// (time fastest), and the root-mean-square energy of a magnitude spectrogram [lead; bins; frames] by Parseval's identity.
//
// The grid (energy.ml:107-118): frame p covers padded positions [p hop, p hop + frame_length) of the signal extended by
// border = frame_length / 2 positions on each side, zeros for rms, copies of the first / last sample for the zero-crossing rate.
// The borders are virtual (a zero, an index clamp); border 0 is the uncentred "frames of a segment" call of the stages.
//
// The summation order of a frame's float64 sum of squares is a function of the frame's own samples:
//   1. the frame is cut into consecutive blocks of blk = min(hop, frame_length) samples from its start, the last one may be short;
//   2. a block's partial: lane l of 64 adds the squares of elements l, l + 64, ... of the block in ascending order, starting
//      from the first of them; the 64 lane sums are combined by the butterfly v += v[lane ^ d], d = 32, 16, 8, 4, 2, 1;
//   3. the frame's sum is the first block's partial, the others added to it in ascending order.
// A full block k of frame p is block 0 of frame p + k, and the short last block's lane sums are prefixes of a full block's: the
// tile kernel computes every hop block of its span once and the frames pick theirs.  Crossing counts are integers: any order.
//
//   energy_frames_kernel           a workgroup owns up to 64 consecutive frames of one clip: their span goes to LDS once, in
//                                  aligned 16-byte loads; each wave reduces hop blocks from LDS (stride-1 across lanes) and parks
//                                  the partials in LDS; one thread per frame adds that frame's partials in order
//   energy_frames_general_kernel   a wave per frame straight from memory, the same order: hop > frame_length, hop < 64, and frames
//                                  so long that a tile holds fewer of them than a frame has blocks; SMX_DISABLE_FAST=1 forces
//                                  it (tests: the same bits)
//   rms_of_spectrogram_kernel      frames across lanes, each thread walks the bins in ascending order
#include <type_traits>

#include "smx_internal.hpp"

namespace smx {
namespace {

enum EnergyOp { ENERGY_RMS = 0, ENERGY_ZCR = 1 };

constexpr int kTileBytes = 32 * 1024;   // samples of one tile in LDS (measured at 2048 / 512: 24 KB 0.149 ms, 32 KB 0.132, 48 KB 0.141)
constexpr int kTileFrames = 64;         // most frames of a tile
constexpr int kInFlight = 12;           // 16-byte loads in flight per thread while a tile is staged: a whole tile in one round
constexpr int kRows = 4;                // rows of 64 samples a wave reads from LDS at a time
constexpr int kDepth = 8;               // loads in flight per thread of the spectrogram walk

struct EnergyArgs {
  const void *x;                  // [lead; n], rows x_stride apart
  void *out;                      // [lead; frames]
  int64_t lead, n, x_stride, frames, border, fl, hop, tiles;   // tiles: workgroups per clip
  double threshold;
  int tile_frames, nfull, rest;   // the tile kernel: frames per tile, full hop blocks per frame, the short block's length
};

// the sample at signal-relative index s of the virtually extended row
template <typename T, int OP>
__device__ __forceinline__ T sample_at(const T *row, int64_t s, int64_t n) {
  if constexpr (OP == ENERGY_ZCR) return row[s < 0 ? 0 : (s >= n ? n - 1 : s)];
  return (s >= 0 && s < n) ? row[s] : (T)0;
}

// energy.ml:136-139: negative iff strictly below -threshold, compared in float64 (NaN is not)
template <typename T>
__device__ __forceinline__ bool negative(T v, double threshold) { return (double)v < -threshold; }

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

template <typename T, int OP>
__device__ __forceinline__ T frame_value(double sum, int64_t count, int64_t fl) {
  if constexpr (OP == ENERGY_RMS) return (T)sqrt(sum / (double)fl);
  return (T)((double)count / (double)fl);
}

template <typename T, int OP>
__global__ void __launch_bounds__(256) energy_frames_kernel(EnergyArgs a) {
  using Vec = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
  constexpr int kVec = 16 / (int)sizeof(T);
  extern __shared__ __align__(16) unsigned char tile_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t clip = blockIdx.x / a.tiles, p0 = (blockIdx.x % a.tiles) * a.tile_frames;
  const int nf = (int)(a.frames - p0 < a.tile_frames ? a.frames - p0 : a.tile_frames);
  const int hop = (int)a.hop, fl = (int)a.fl;
  const T *row = reinterpret_cast<const T *>(a.x) + clip * a.x_stride;
  const int64_t s0 = p0 * a.hop - a.border;                 // the tile's first padded position as a signal index
  const int span = (nf - 1) * hop + fl;
  // 16-byte groups by address: element e of the tile is signal index s0 - shift + e
  const int shift = (int)(((int64_t)(reinterpret_cast<uintptr_t>(row) / sizeof(T)) + s0) & (kVec - 1));
  const int groups = (shift + span + kVec - 1) / kVec;
  T *smp = reinterpret_cast<T *>(tile_lds);
  // the partials lie behind the samples of a full tile: 16 bytes per hop block
  const int cap = (kVec - 1 + (a.tile_frames - 1) * hop + fl + kVec - 1) / kVec;
  unsigned char *parts = tile_lds + (size_t)cap * 16;
  const int units = nf + a.nfull - 1 + (a.rest ? 1 : 0);
  const int slots = a.tile_frames + a.nfull;

  for (int g0 = threadIdx.x; g0 < groups; g0 += 256 * kInFlight) {
    Vec q[kInFlight];
    bool whole[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int g = g0 + u * 256;
      const int64_t s = s0 - shift + (int64_t)g * kVec;
      whole[u] = g < groups && s >= 0 && s + kVec <= a.n;
      if (whole[u]) q[u] = *reinterpret_cast<const Vec *>(row + s);
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int g = g0 + u * 256;
      if (g >= groups) continue;
      if (!whole[u]) {                                      // a group that meets a border: element by element
        const int64_t s = s0 - shift + (int64_t)g * kVec;
        T *e = reinterpret_cast<T *>(&q[u]);
#pragma unroll
        for (int i = 0; i < kVec; ++i) e[i] = sample_at<T, OP>(row, s + i, a.n);
      }
      reinterpret_cast<Vec *>(smp)[g] = q[u];
    }
  }
  __syncthreads();

  // hop block j of the tile starts at padded position (p0 + j) hop; the blocks behind the last frame's full ones are read for
  // their short prefix only
  for (int j = wave; j < units; j += 4) {
    const int e0 = shift + j * hop;
    const bool full = j < nf + a.nfull - 1;
    const int len = full ? hop : a.rest;
    // kRows rows of 64 positions are read from LDS before the first is used; the adds keep their ascending order
    if constexpr (OP == ENERGY_RMS) {
      double acc = 0.0, prefix = 0.0;
      for (int i0 = lane; i0 < len; i0 += 64 * kRows) {
        T v[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) v[u] = smp[e0 + (i0 + 64 * u < len ? i0 + 64 * u : 0)];
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
          const int i = i0 + 64 * u;
          if (i >= len) break;
          const double d = (double)v[u];
          acc += d * d;
          if (i < a.rest) prefix = acc;
        }
      }
      double *sum = reinterpret_cast<double *>(parts);
      if (full) acc = wave_sum(acc);
      if (a.rest) prefix = wave_sum(prefix);
      if (lane == 0) sum[j] = acc, sum[slots + j] = prefix;
    } else {
      // the flags of a row are one 64-bit mask and a crossing is a bit that differs from the bit before it.  Crossings inside
      // the block, those among its first `rest` positions, and the one at its join with the block before.
      int inner = 0, head = 0, join = 0;
      unsigned long long before = e0 > 0 && negative(smp[e0 - 1], a.threshold) ? 1ull : 0ull;   // e0 = 0: the tile's first block, whose join no frame reads
      for (int r0 = 0; r0 < len; r0 += 64 * kRows) {
        T v[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) v[u] = smp[e0 + (r0 + 64 * u + lane < len ? r0 + 64 * u + lane : 0)];
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
          const int i0 = r0 + 64 * u;
          if (i0 >= len) break;
          const unsigned long long flags = __ballot(i0 + lane < len && negative(v[u], a.threshold));
          const int width = len - i0, below = a.rest - i0;
          unsigned long long changes = flags ^ ((flags << 1) | before);
          if (width < 64) changes &= (1ull << width) - 1;
          before = flags >> 63;
          if (i0 == 0) join = (int)(changes & 1ull), changes &= ~1ull;
          inner += __popcll(changes);
          if (below > 0) head += __popcll(below < 64 ? changes & ((1ull << below) - 1) : changes);
        }
      }
      int *count = reinterpret_cast<int *>(parts);
      if (lane == 0) count[j] = inner, count[slots + j] = head, count[2 * slots + j] = join;
    }
  }
  __syncthreads();

  const int f = threadIdx.x;
  if (f >= nf) return;
  double sum = 0.0;
  int64_t crossings = 0;
  if constexpr (OP == ENERGY_RMS) {
    const double *part = reinterpret_cast<const double *>(parts);
    sum = part[f];
    for (int k = 1; k < a.nfull; ++k) sum += part[f + k];
    if (a.rest) sum += part[slots + f + a.nfull];
  } else {
    const int *count = reinterpret_cast<const int *>(parts);
    crossings = count[f];
    for (int k = 1; k < a.nfull; ++k) crossings += count[f + k] + count[2 * slots + f + k];
    if (a.rest) crossings += count[slots + f + a.nfull] + count[2 * slots + f + a.nfull];
  }
  reinterpret_cast<T *>(a.out)[clip * a.frames + p0 + f] = frame_value<T, OP>(sum, crossings, a.fl);
}

// a wave per frame, four frames per workgroup, any geometry
template <typename T, int OP>
__global__ void __launch_bounds__(256) energy_frames_general_kernel(EnergyArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t clip = blockIdx.x / a.tiles, p = (blockIdx.x % a.tiles) * 4 + (threadIdx.x >> 6);
  if (p >= a.frames) return;
  const T *row = reinterpret_cast<const T *>(a.x) + clip * a.x_stride;
  const int64_t s0 = p * a.hop - a.border;
  double sum = 0.0;
  int64_t crossings = 0;
  if constexpr (OP == ENERGY_RMS) {
    const int64_t blk = a.hop < a.fl ? a.hop : a.fl;
    for (int64_t b0 = 0; b0 < a.fl; b0 += blk) {
      const int64_t len = a.fl - b0 < blk ? a.fl - b0 : blk;
      double acc = 0.0;
      for (int64_t i = lane; i < len; i += 64) {
        const double v = (double)sample_at<T, OP>(row, s0 + b0 + i, a.n);
        acc += v * v;
      }
      acc = wave_sum(acc);
      sum = b0 == 0 ? acc : sum + acc;
    }
  } else {
    for (int64_t i = 1 + lane; i < a.fl; i += 64)
      crossings += negative(sample_at<T, OP>(row, s0 + i, a.n), a.threshold) != negative(sample_at<T, OP>(row, s0 + i - 1, a.n), a.threshold) ? 1 : 0;
    crossings = wave_sum(crossings);
  }
  if (lane == 0) reinterpret_cast<T *>(a.out)[clip * a.frames + p] = frame_value<T, OP>(sum, crossings, a.fl);
}

// energy.ml:394-421: sqrt(2 sum_k w_k s_k^2 / frame_length^2), w = 0.5 at bin 0 and (even frame_length) at the last bin
template <typename T>
__global__ void __launch_bounds__(256) rms_of_spectrogram_kernel(const T *s, T *out, int64_t bins, int64_t frames, int64_t ftiles, int even,
                                                                 double fl) {
  const int64_t clip = blockIdx.x / ftiles, t = (blockIdx.x % ftiles) * 256 + threadIdx.x;
  if (t >= frames) return;
  const T *col = s + clip * bins * frames + t;
  const int64_t half = even ? bins - 1 : -1;
  double sum = 0.0;
  auto add = [&](int64_t k, T x) {
    const double v = (double)x;
    sum += (v * v) * ((k == 0 || k == half) ? 0.5 : 1.0);
  };
  int64_t k = 0;
  for (; k + kDepth <= bins; k += kDepth) {
    T v[kDepth];
#pragma unroll
    for (int i = 0; i < kDepth; ++i) v[i] = col[(k + i) * frames];
#pragma unroll
    for (int i = 0; i < kDepth; ++i) add(k + i, v[i]);
  }
  for (; k < bins; ++k) add(k, col[k * frames]);
  const double power = (sum * 2.0) / (fl * fl);
  out[clip * frames + t] = (T)sqrt(power);
}

// ---- the host side -------------------------------------------------------------------------------------------------------------
void check_frame_length(const char *op, int64_t fl) {      // energy.ml:84-90
  if (fl < 1)
    throw InvalidArgument(format("%s: cannot analyse frames of %lld samples (frame_length must be at least 1)", op, (long long)fl));
}
void check_hop(const char *op, int64_t hop) {               // energy.ml:92-97
  if (hop < 1) throw InvalidArgument(format("%s: cannot advance frames by %lld samples (hop must be at least 1)", op, (long long)hop));
}
void check_threshold(const char *op, double threshold) {    // energy.ml:99-105
  if (!(std::isfinite(threshold) && threshold >= 0.0))
    throw InvalidArgument(format("%s: cannot clamp signs with a threshold of %g (threshold must be finite and non-negative)", op, threshold));
}

int64_t count_frames(int64_t fl, int64_t hop, int64_t n) {  // energy.ml:114-118
  if (n == 0) return 0;
  const int64_t padded = n + 2 * (fl / 2);
  return padded < fl ? 0 : 1 + (padded - fl) / hop;
}

// frames per tile of the tile kernel, or 0: the general kernel.  A function of the geometry and the sample width alone.
int tile_frames(int64_t fl, int64_t hop, int elem_bytes) {
  if (fast_path_disabled() || hop > fl || hop < 64) return 0;
  const int64_t room = kTileBytes / elem_bytes - 2 * (16 / elem_bytes) - fl;
  if (room < 0) return 0;
  const int64_t fit = std::min<int64_t>(room / hop + 1, kTileFrames);
  return fit >= (fl + hop - 1) / hop ? (int)fit : 0;        // a sample is staged less than twice
}

template <typename T, int OP>
void launch_energy(const char *fn, EnergyArgs a, hipStream_t stream) {
  a.tile_frames = tile_frames(a.fl, a.hop, (int)sizeof(T));
  const int64_t per_tile = a.tile_frames ? a.tile_frames : 4;
  a.tiles = (a.frames + per_tile - 1) / per_tile;
  // clip range by clip range where the batch exceeds one launch (DESIGN.md "Launch extents"); the clips are independent
  const int64_t lead = a.lead, per_launch = std::max<int64_t>(1, clips_per_launch(a.tiles, 256));
  const char *x = reinterpret_cast<const char *>(a.x);
  char *out = reinterpret_cast<char *>(a.out);
  if (a.tile_frames) {
    a.nfull = (int)(a.fl / a.hop);
    a.rest = (int)(a.fl - a.nfull * a.hop);
  }
  for (int64_t c0 = 0; c0 < lead; c0 += per_launch) {
    a.lead = std::min(per_launch, lead - c0);
    a.x = x + c0 * a.x_stride * (int64_t)sizeof(T);
    a.out = out + c0 * a.frames * (int64_t)sizeof(T);
    const dim3 grid(grid_x(fn, "frame tiles", a.lead * a.tiles, 256));
    if (a.tile_frames) {
      constexpr int64_t kVec = 16 / sizeof(T);
      const int64_t cap = (kVec - 1 + (a.tile_frames - 1) * a.hop + a.fl + kVec - 1) / kVec;
      const size_t lds = (size_t)cap * 16 + (size_t)(a.tile_frames + a.nfull) * 16;
      SMX_LAUNCH((energy_frames_kernel<T, OP>), grid, dim3(256), lds, stream, a);
    } else {
      SMX_LAUNCH((energy_frames_general_kernel<T, OP>), grid, dim3(256), 0, stream, a);
    }
    SMX_HIP_CHECK(hipGetLastError());
  }
}

// frames [0, count) of rows extended by `border` virtual positions on each side; the parameters are the caller's to check
void energy_dev(const char *fn, int op, double threshold, int64_t fl, int64_t hop, int64_t border, const void *d_x, int elem_bytes,
                int64_t lead, int64_t n, int64_t x_stride, int64_t count, void *d_out, hipStream_t stream) {
  if (lead == 0 || count == 0) return;
  if (x_stride < n) throw Failure(format("%s: x_stride is smaller than the signal length", fn));
  if (!d_x || !d_out) throw Failure(format("%s: null device pointer", fn));
  EnergyArgs a{};
  a.x = d_x;
  a.out = d_out;
  a.lead = lead;
  a.n = n;
  a.x_stride = x_stride;
  a.frames = count;
  a.border = border;
  a.fl = fl;
  a.hop = hop;
  a.threshold = threshold;
  if (op == ENERGY_RMS) {
    if (elem_bytes == 8) launch_energy<double, ENERGY_RMS>(fn, a, stream);
    else launch_energy<float, ENERGY_RMS>(fn, a, stream);
  } else {
    if (elem_bytes == 8) launch_energy<double, ENERGY_ZCR>(fn, a, stream);
    else launch_energy<float, ENERGY_ZCR>(fn, a, stream);
  }
}

// rms / zero_crossing_rate (energy.ml:360-388): the threshold, the frame length, the hop, then the tensor
int64_t check_centred(const char *fn, int op, double threshold, int64_t fl, int64_t hop, int64_t lead, int64_t n) {
  if (op == ENERGY_ZCR) check_threshold(fn, threshold);
  check_frame_length(fn, fl);
  check_hop(fn, hop);
  check_rank_extents(fn, lead, n);
  return count_frames(fl, hop, n);
}

const char *centred_name(int op) { return op == ENERGY_RMS ? "rms" : "zero_crossing_rate"; }

void centred_dev(int op, double threshold, int64_t fl, int64_t hop, const void *d_x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride,
                 void *d_out, hipStream_t stream) {
  const char *fn = centred_name(op);
  const int64_t count = check_centred(fn, op, threshold, fl, hop, lead, n);
  energy_dev(fn, op, threshold, fl, hop, fl / 2, d_x, elem_bytes, lead, n, x_stride, count, d_out, stream);
}

void centred_host(int op, double threshold, int64_t fl, int64_t hop, const void *x, int elem_bytes, int64_t lead, int64_t n, void *out) {
  const char *fn = centred_name(op);
  const int64_t count = check_centred(fn, op, threshold, fl, hop, lead, n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure(format("%s: null pointer", fn));
  host_call(fn, {{x, (size_t)n * (size_t)elem_bytes}}, out, (size_t)count * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              energy_dev(fn, op, threshold, fl, hop, fl / 2, d_in[0], elem_bytes, nc, n, n, count, d_out, stream);
            });
}

// the stages' call (energy.ml:157-183 `analyse`): frames [0, count) of a segment of the padded stream, no border; the parameters
// are checked as rms_stage / zero_crossing_rate_stage check theirs (energy.ml:514-525)
const char *check_segment(int op, double threshold, int64_t fl, int64_t hop, int64_t lead, int64_t n, int64_t count) {
  if (op != ENERGY_RMS && op != ENERGY_ZCR) throw Failure(format("energy_frames: unknown feature %d", op));
  const char *fn = op == ENERGY_RMS ? "rms_stage" : "zero_crossing_rate_stage";
  check_frame_length(fn, fl);
  check_hop(fn, hop);
  if (op == ENERGY_ZCR) check_threshold(fn, threshold);
  check_rank_extents(fn, lead, n);
  if (count < 0) throw Failure(format("%s: negative frame count", fn));
  if (count > 0 && (n < fl || (n - fl) / hop < count - 1))
    throw Failure(format("%s: %lld frames of %lld samples at hop %lld do not fit a segment of %lld samples", fn, (long long)count,
                         (long long)fl, (long long)hop, (long long)n));
  return fn;
}

void segment_dev(int op, double threshold, int64_t fl, int64_t hop, const void *d_x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride,
                 int64_t count, void *d_out, hipStream_t stream) {
  const char *fn = check_segment(op, threshold, fl, hop, lead, n, count);
  energy_dev(fn, op, threshold, fl, hop, 0, d_x, elem_bytes, lead, n, x_stride, count, d_out, stream);
}

void segment_host(int op, double threshold, int64_t fl, int64_t hop, const void *x, int elem_bytes, int64_t lead, int64_t n, int64_t count,
                  void *out) {
  const char *fn = check_segment(op, threshold, fl, hop, lead, n, count);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure(format("%s: null pointer", fn));
  host_call(fn, {{x, (size_t)n * (size_t)elem_bytes}}, out, (size_t)count * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              energy_dev(fn, op, threshold, fl, hop, 0, d_in[0], elem_bytes, nc, n, n, count, d_out, stream);
            });
}

// rms_of_spectrogram (energy.ml:394-421); the rank is the caller's to check between the two
void check_of_spectrogram(int64_t fl, int64_t lead, int64_t bins, int64_t frames) {
  const char *fn = "rms_of_spectrogram";
  check_frame_length(fn, fl);
  if (lead < 0 || bins < 0 || frames < 0)
    throw Failure(format("%s: negative extent (lead %lld, bins %lld, frames %lld)", fn, (long long)lead, (long long)bins, (long long)frames));
  if (bins != fl / 2 + 1)
    throw InvalidArgument(format(
        "%s: cannot read %lld frequency bins as frames of %lld samples (a magnitude spectrogram holds frame_length / 2 + 1 bins)", fn,
        (long long)bins, (long long)fl));
}

void of_spectrogram_dev(int64_t fl, const void *d_s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *d_out,
                        hipStream_t stream) {
  check_of_spectrogram(fl, lead, bins, frames);
  if (lead == 0 || frames == 0) return;
  if (!d_s || !d_out) throw Failure("rms_of_spectrogram: null device pointer");
  const int64_t ftiles = (frames + 255) / 256;
  const int even = fl % 2 == 0 ? 1 : 0;
  const int64_t per_launch = std::max<int64_t>(1, clips_per_launch(ftiles, 256));   // clip range by clip range (DESIGN.md "Launch extents")
  for (int64_t c0 = 0; c0 < lead; c0 += per_launch) {
    const int64_t nc = std::min(per_launch, lead - c0);
    const dim3 grid(grid_x("rms_of_spectrogram", "frame tiles", nc * ftiles, 256));
    const char *s = (const char *)d_s + c0 * bins * frames * elem_bytes;
    char *out = (char *)d_out + c0 * frames * elem_bytes;
    if (elem_bytes == 8)
      SMX_LAUNCH(rms_of_spectrogram_kernel<double>, grid, dim3(256), 0, stream, (const double *)s, (double *)out, bins, frames, ftiles, even,
                 (double)fl);
    else
      SMX_LAUNCH(rms_of_spectrogram_kernel<float>, grid, dim3(256), 0, stream, (const float *)s, (float *)out, bins, frames, ftiles, even,
                 (double)fl);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

void of_spectrogram_host(int64_t fl, const void *s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, void *out) {
  check_of_spectrogram(fl, lead, bins, frames);
  if (lead == 0 || frames == 0) return;
  if (!s || !out) throw Failure("rms_of_spectrogram: null pointer");
  const size_t row = (size_t)frames * (size_t)elem_bytes;
  host_call("rms_of_spectrogram", {{s, (size_t)bins * row}}, out, row, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              of_spectrogram_dev(fl, d_in[0], elem_bytes, nc, bins, frames, d_out, stream);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Energy (energy.ml) ----------------------------------------------------------------------------------------------------
int smx_rms_f32(const float *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop, float *out) {
  return guarded([&] { centred_host(ENERGY_RMS, 0.0, frame_length, hop, x, 4, lead, n, out); });
}
int smx_rms_f64(const double *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop, double *out) {
  return guarded([&] { centred_host(ENERGY_RMS, 0.0, frame_length, hop, x, 8, lead, n, out); });
}
int smx_rms_device_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t frame_length, int64_t hop, float *d_out,
                       void *stream) {
  return guarded([&] { centred_dev(ENERGY_RMS, 0.0, frame_length, hop, d_x, 4, lead, n, x_stride, d_out, (hipStream_t)stream); });
}
int smx_zero_crossing_rate_f32(const float *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop, double threshold, float *out) {
  return guarded([&] { centred_host(ENERGY_ZCR, threshold, frame_length, hop, x, 4, lead, n, out); });
}
int smx_zero_crossing_rate_f64(const double *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop, double threshold, double *out) {
  return guarded([&] { centred_host(ENERGY_ZCR, threshold, frame_length, hop, x, 8, lead, n, out); });
}
int smx_zero_crossing_rate_device_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t frame_length, int64_t hop,
                                      double threshold, float *d_out, void *stream) {
  return guarded([&] { centred_dev(ENERGY_ZCR, threshold, frame_length, hop, d_x, 4, lead, n, x_stride, d_out, (hipStream_t)stream); });
}
int smx_rms_of_spectrogram_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t frame_length, float *out) {
  return guarded([&] { of_spectrogram_host(frame_length, s, 4, lead, bins, frames, out); });
}
int smx_rms_of_spectrogram_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t frame_length, double *out) {
  return guarded([&] { of_spectrogram_host(frame_length, s, 8, lead, bins, frames, out); });
}
int smx_rms_of_spectrogram_device_f32(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t frame_length, float *d_out,
                                      void *stream) {
  return guarded([&] { of_spectrogram_dev(frame_length, d_s, 4, lead, bins, frames, d_out, (hipStream_t)stream); });
}
int smx_energy_frames_f32(int op, double threshold, int64_t frame_length, int64_t hop, const float *x, int64_t lead, int64_t n, int64_t count,
                          float *out) {
  return guarded([&] { segment_host(op, threshold, frame_length, hop, x, 4, lead, n, count, out); });
}
int smx_energy_frames_f64(int op, double threshold, int64_t frame_length, int64_t hop, const double *x, int64_t lead, int64_t n, int64_t count,
                          double *out) {
  return guarded([&] { segment_host(op, threshold, frame_length, hop, x, 8, lead, n, count, out); });
}
int smx_energy_frames_device_f32(int op, double threshold, int64_t frame_length, int64_t hop, const float *d_x, int64_t lead, int64_t n,
                                 int64_t x_stride, int64_t count, float *d_out, void *stream) {
  return guarded([&] { segment_dev(op, threshold, frame_length, hop, d_x, 4, lead, n, x_stride, count, d_out, (hipStream_t)stream); });
}

}  // extern "C"
