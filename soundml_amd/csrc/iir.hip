// Recursive filters as cascaded second-order sections (scipy.signal.sosfilt's definition; not in the reference, whose README
// lists "IIR/FIR filtering" as planned) over device-resident audio [lead; n], time fastest.
//
// One step of the cascade on a sample u, float64, every product and every sum rounded on its own (this file is built with
// -ffp-contract=off), for k = 0 .. S-1 in turn:
//     y = b0 u + z[k][0];   z[k][0] = (b1 u - a1 y) + z[k][1];   z[k][1] = b2 u - a2 y;   u = y
//
// The stated order.  The time axis is cut into blocks of B = kBlock samples counted from the first sample of the
// call (of the stream since reset).  s_b, 2S doubles in the order z[0][0], z[0][1], z[1][0], ..., is the state entering block b;
// s_0 is zi or zero.  The outputs of block b are the serial cascade run from s_b over the block's samples; w_b is the end state of
// the same cascade run over the same samples from a ZERO state; then
//     s_{b+1}[i] = (((M[i][0] s_b[0] + M[i][1] s_b[1]) + M[i][2] s_b[2]) + ... ) + w_b[i]          (ascending j, then w)
// M [2S; 2S] is built on the host: column i is the end state of B zero-input steps of the cascade from the unit state e_i.
// Outputs are rounded once, to the dtype of the result.  The running state after the last sample of a block is s_{b+1}.
//
// Every face keeps one state record per channel on the device: s_b | the partial w | the running state, 6S doubles.
//
//   iir_general_kernel   a lane per channel walks samples [i0, i1) serially from the record, both runs side by side, and applies M
//                        where a block ends: every shape, every position inside a block; SMX_DISABLE_FAST=1 forces it
//   the block route      three launches ordered by the stream, for the whole blocks of a call:
//     iir_block_w_kernel   a wave owns kSpanBlocks consecutive blocks of one channel, lane l block l, all S sections' states in
//                          registers.  The span passes through LDS kPhase samples of every block at a time (a block's piece is
//                          whole 128-byte lines of float32, so the wave's loads are coalesced; 8 KB per wave, so many waves share
//                          a compute unit and hide each other's loads), rows kPhase + 1 elements apart: an odd pitch, the lanes'
//                          walks hit distinct banks.  The run starts from zero and stores w_b
//     iir_chain_kernel     a lane per (channel, state component): s_{b+1} = M s_b + w_b along the blocks, the row of M in registers,
//                          s_b shared through the wave, w_b fetched sixteen blocks ahead; s_b replaces w_b in the scratch array
//     iir_block_y_kernel   the same staging; lane l reruns block l from s_b, writes y over its samples in LDS, and the wave
//                          flushes each piece in coalesced stores
//   A call's head (up to the next block edge of a stream) and tail (the samples behind the last whole block) take the general kernel.
//
// filtfilt is two such passes: the odd extension is virtual in the first pass's load index, the float64 intermediate lies in
// library scratch, and the reversals are virtual in the second pass's load and store indices.
#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kBlock = kIirBlock;            // B
constexpr int kSpanBlocks = kIirSpanBlocks;  // blocks per wave: one per lane
constexpr int kMaxSections = kIirMaxSections;
constexpr int kPhase = 32, kLogPhase = 5;    // samples of every block of the span that lie in LDS at a time
constexpr int kPitch = kPhase + 1;           // LDS row pitch in elements
constexpr int kAhead = 8;                    // LDS reads a lane issues before it uses the first
constexpr int kChainAhead = 16;              // blocks of w the chain fetches ahead

enum { SRC_PLAIN = 0, SRC_EXT = 1, SRC_REV = 2 };
enum { DST_PLAIN = 0, DST_REV_TRIM = 1 };
enum { ZI_ZERO = 0, ZI_CALL = 1, ZI_ROWS = 2, ZI_SCALED = 3 };

struct IirZi {
  double v[2 * kMaxSections];
};
// where a pass reads sample i of channel c and where it puts output i; the pass is m samples long
struct IirIo {
  const void *x;
  void *out;
  int64_t x_stride, out_stride;   // elements between rows
  int64_t nx, pad, m;             // SRC_EXT / DST_REV_TRIM: the signal's length and the extension on each side (m = nx + 2 pad)
  int x_bytes, out_bytes, src, dst;
};

__device__ __forceinline__ double src_raw(const IirIo &io, int64_t c, int64_t j) {
  return io.x_bytes == 4 ? (double)reinterpret_cast<const float *>(io.x)[c * io.x_stride + j]
                         : reinterpret_cast<const double *>(io.x)[c * io.x_stride + j];
}

__device__ __forceinline__ double load_src(const IirIo &io, int64_t c, int64_t i) {
  if (io.src == SRC_PLAIN) return src_raw(io, c, i);
  if (io.src == SRC_REV) return src_raw(io, c, io.m - 1 - i);
  // scipy's odd_ext: 2 x[0] - x[pad - i] | x | 2 x[n-1] - x[n-2-k], taken in float64 (the doubling is exact, one rounding)
  if (i < io.pad) return 2.0 * src_raw(io, c, 0) - src_raw(io, c, io.pad - i);
  if (i < io.pad + io.nx) return src_raw(io, c, i - io.pad);
  return 2.0 * src_raw(io, c, io.nx - 1) - src_raw(io, c, io.nx - 2 - (i - io.pad - io.nx));
}

__device__ __forceinline__ void store_dst(const IirIo &io, int64_t c, int64_t i, double y) {
  int64_t j = i;
  if (io.dst == DST_REV_TRIM) {
    j = io.m - 1 - i - io.pad;
    if (j < 0 || j >= io.nx) return;
  }
  if (io.out_bytes == 4) reinterpret_cast<float *>(io.out)[c * io.out_stride + j] = (float)y;
  else reinterpret_cast<double *>(io.out)[c * io.out_stride + j] = y;
}

// (the cascade itself is smx_internal.hpp's iir_cascade: Loudness runs it too)
template <int S>
__device__ __forceinline__ double cascade(const IirCoef &k, double u, double (&z)[2 * S]) {
  return iir_cascade<S>(k, u, z);
}

// load_src with the element type and the mode fixed at compile time and no branch around a load: the extension reads the mirrored
// sample and the edge it is mirrored about with two loads that always happen, so a whole round of them stays in flight together
template <typename X, int SRC>
__device__ __forceinline__ double load_fixed(const IirIo &io, int64_t c, int64_t i) {
  const X *row = reinterpret_cast<const X *>(io.x) + c * io.x_stride;
  if constexpr (SRC == SRC_PLAIN) return (double)row[i];
  if constexpr (SRC == SRC_REV) return (double)row[io.m - 1 - i];
  const int64_t q = i - io.pad;
  const int64_t j = q < 0 ? -q : (q >= io.nx ? 2 * io.nx - 2 - q : q);
  const int64_t edge = q < 0 ? 0 : (q >= io.nx ? io.nx - 1 : j);
  const double v = (double)row[j], about = (double)row[edge];
  return edge == j ? v : 2.0 * about - v;
}

// positions [ph kPhase, (ph + 1) kPhase) of the nblk blocks that start at sample i0 of channel c into the wave's rows: a block's
// piece is kPhase consecutive samples, so a wave's load covers whole pieces
template <typename E, typename X, int SRC>
__device__ __forceinline__ void stage_fixed(const IirIo &io, int64_t c, int64_t i0, int nblk, int ph, E *rows) {
  const int lane = threadIdx.x, count = nblk * kPhase;
  E v[kPhase];
#pragma unroll
  for (int u = 0; u < kPhase; ++u) {   // every lane loads, past the end the last valid sample again: the loads stay in flight together
    const int e = u * 64 + lane < count ? u * 64 + lane : count - 1;
    v[u] = (E)load_fixed<X, SRC>(io, c, i0 + (int64_t)(e >> kLogPhase) * kBlock + ph * kPhase + (e & (kPhase - 1)));
  }
#pragma unroll
  for (int u = 0; u < kPhase; ++u) {
    const int e = u * 64 + lane;
    if (e < count) rows[(e >> kLogPhase) * kPitch + (e & (kPhase - 1))] = v[u];
  }
}

// float32 rows hold float32 audio read as it lies; float64 rows whatever a pass of filtfilt or a float64 host array asks for
template <typename E>
__device__ __forceinline__ void stage_phase(const IirIo &io, int64_t c, int64_t i0, int nblk, int ph, E *rows) {
  if constexpr (sizeof(E) == 4) {
    stage_fixed<E, float, SRC_PLAIN>(io, c, i0, nblk, ph, rows);
  } else {
    if (io.src == SRC_EXT && io.x_bytes == 4) stage_fixed<E, float, SRC_EXT>(io, c, i0, nblk, ph, rows);
    else if (io.src == SRC_EXT) stage_fixed<E, double, SRC_EXT>(io, c, i0, nblk, ph, rows);
    else if (io.src == SRC_REV) stage_fixed<E, double, SRC_REV>(io, c, i0, nblk, ph, rows);
    else stage_fixed<E, double, SRC_PLAIN>(io, c, i0, nblk, ph, rows);
  }
}

template <typename E, int S>
__global__ void __launch_bounds__(64) iir_block_w_kernel(IirCoef k, IirIo io, int64_t first, int64_t nb, int64_t spans, double *ws) {
  extern __shared__ __align__(16) unsigned char iir_lds[];
  E *rows = reinterpret_cast<E *>(iir_lds);
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x / spans, b0 = (blockIdx.x % spans) * kSpanBlocks;
  const int nblk = (int)(nb - b0 < kSpanBlocks ? nb - b0 : kSpanBlocks);
  const E *row = rows + lane * kPitch;
  double z[2 * S];
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) z[i] = 0.0;
  for (int ph = 0; ph < kBlock / kPhase; ++ph) {
    if (ph) __syncthreads();
    stage_phase<E>(io, c, first + b0 * kBlock, nblk, ph, rows);
    __syncthreads();
    if (lane < nblk) {
      for (int t = 0; t < kPhase; t += kAhead) {
        E v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = row[t + u];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) (void)cascade<S>(k, (double)v[u], z);
      }
    }
  }
  if (lane >= nblk) return;
  double *w = ws + (c * nb + b0 + lane) * (2 * S);
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) w[i] = z[i];
}

template <typename E, int S>
__global__ void __launch_bounds__(64) iir_block_y_kernel(IirCoef k, IirIo io, int64_t first, int64_t nb, int64_t spans, const double *ws) {
  extern __shared__ __align__(16) unsigned char iir_lds[];
  E *rows = reinterpret_cast<E *>(iir_lds);
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x / spans, b0 = (blockIdx.x % spans) * kSpanBlocks;
  const int nblk = (int)(nb - b0 < kSpanBlocks ? nb - b0 : kSpanBlocks);
  const int count = nblk * kPhase;
  E *row = rows + lane * kPitch;
  const double *s = ws + (c * nb + b0 + (lane < nblk ? lane : 0)) * (2 * S);
  double z[2 * S];
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) z[i] = s[i];
  for (int ph = 0; ph < kBlock / kPhase; ++ph) {
    if (ph) __syncthreads();
    stage_phase<E>(io, c, first + b0 * kBlock, nblk, ph, rows);
    __syncthreads();
    if (lane < nblk) {
      for (int t = 0; t < kPhase; t += kAhead) {
        E v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = row[t + u];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) row[t + u] = (E)cascade<S>(k, (double)v[u], z);   // float32 results round here, once
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int e = lane; e < count; e += 64)
      store_dst(io, c, first + (b0 + (e >> kLogPhase)) * kBlock + ph * kPhase + (e & (kPhase - 1)), (double)rows[(e >> kLogPhase) * kPitch + (e & (kPhase - 1))]);
  }
}

// ws [lead; nb; 2S]: w_b on entry, s_b on return; the record gets s_nb as its block state and running state, and a zero partial
template <int S>
__global__ void __launch_bounds__(64) iir_chain_kernel(const double *M, double *st, double *ws, int64_t lead, int64_t nb) {
  constexpr int N = 2 * S, G = N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : 16;
  const int lane = threadIdx.x, i = lane % G, base = lane - i;
  const int64_t c = (int64_t)blockIdx.x * (64 / G) + lane / G;
  const bool active = c < lead && i < N;
  const int64_t cc = active ? c : 0;
  const int ii = active ? i : 0;
  double m[N];
#pragma unroll
  for (int j = 0; j < N; ++j) m[j] = M[ii * N + j];
  double s = st[cc * 3 * N + ii];
  double *wp = ws + cc * nb * N + ii;
  double w[kChainAhead];
#pragma unroll
  for (int d = 0; d < kChainAhead; ++d) w[d] = d < nb ? wp[(int64_t)d * N] : 0.0;
  // one step: s_b goes where w_b was, then s_{b+1} = M s_b + w_b
  auto advance = [&](int64_t at, double wb) {
    if (active) wp[at * N] = s;
    double acc = m[0] * __shfl(s, base);
#pragma unroll
    for (int j = 1; j < N; ++j) acc = acc + m[j] * __shfl(s, base + j);
    s = acc + wb;
  };
  int64_t b = 0;
  for (; b + kChainAhead <= nb; b += kChainAhead) {
#pragma unroll
    for (int d = 0; d < kChainAhead; ++d) {
      const double wb = w[d];
      const int64_t ahead = b + d + kChainAhead;
      w[d] = wp[(ahead < nb ? ahead : nb - 1) * N];   // always a load of a valid slot: nothing waits on a branch; past the end it is not used
      advance(b + d, wb);
    }
  }
#pragma unroll
  for (int d = 0; d < kChainAhead; ++d)
    if (b + d < nb) advance(b + d, w[d]);
  if (!active) return;
  st[c * 3 * N + i] = s;
  st[c * 3 * N + N + i] = 0.0;
  st[c * 3 * N + 2 * N + i] = s;
}

template <int S>
__global__ void __launch_bounds__(64) iir_general_kernel(IirCoef k, IirIo io, const double *M, double *st, int64_t lead, int64_t i0, int64_t i1,
                                                         int pos0) {
  constexpr int N = 2 * S;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= lead) return;
  double s[N], w[N], r[N];
  double *rec = st + c * 3 * N;
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = rec[i], w[i] = rec[N + i], r[i] = rec[2 * N + i];
  int pos = pos0;
  for (int64_t t = i0; t < i1; ++t) {
    const double u = load_src(io, c, t);
    store_dst(io, c, t, cascade<S>(k, u, r));
    (void)cascade<S>(k, u, w);
    if (++pos == kBlock) {
      double next[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        double acc = M[i * N] * s[0];
#pragma unroll
        for (int j = 1; j < N; ++j) acc = acc + M[i * N + j] * s[j];
        next[i] = acc + w[i];
      }
#pragma unroll
      for (int i = 0; i < N; ++i) s[i] = next[i], r[i] = next[i], w[i] = 0.0;
      pos = 0;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) rec[i] = s[i], rec[N + i] = w[i], rec[2 * N + i] = r[i];
}

// a fresh record per channel: s_0 = 0 | zi | zi_rows[c] | zi times the pass's first sample (filtfilt), no partial, running = s_0
__global__ void __launch_bounds__(256) iir_init_kernel(IirIo io, IirZi zi, const double *zi_rows, int mode, double *st, int64_t lead, int N) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, c = idx / N;
  const int i = (int)(idx % N);
  if (c >= lead) return;
  double v = 0.0;
  if (mode == ZI_CALL) v = zi.v[i];
  else if (mode == ZI_ROWS) v = zi_rows[c * N + i];
  else if (mode == ZI_SCALED) v = zi.v[i] * load_src(io, c, 0);
  st[c * 3 * N + i] = v;
  st[c * 3 * N + N + i] = 0.0;
  st[c * 3 * N + 2 * N + i] = v;
}

__global__ void __launch_bounds__(256) iir_state_out_kernel(const double *st, double *zf, int64_t lead, int N) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, c = idx / N;
  if (c >= lead) return;
  zf[idx] = st[c * 3 * N + 2 * N + idx % N];
}

}  // namespace

// ---- the host side -------------------------------------------------------------------------------------------------------------
struct IirCore {
  int S = 0;
  IirCoef coef{};
  std::vector<double> sos;   // [S; 6] as given
  std::vector<double> M;     // [2S; 2S] row-major
  int64_t padlen = 0;

  const double *device_matrix() const {
    int device = 0;
    SMX_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(mutex_);
    auto it = tables_.find(device);
    if (it != tables_.end()) return it->second;
    double *p = nullptr;
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p), M.size() * sizeof(double)));
    hipError_t err = hipMemcpy(p, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
      (void)hipFree(p);
      SMX_HIP_CHECK(err);
    }
    tables_[device] = p;
    return p;
  }
  ~IirCore() {
    for (auto &t : tables_) (void)hipFree(t.second);
  }

 private:
  mutable std::mutex mutex_;
  mutable std::map<int, double *> tables_;
};

namespace {

std::shared_ptr<IirCore> make_core(const double *sos, int64_t sections) {
  if (sections < 1 || sections > kMaxSections)
    throw InvalidArgument(format("create: cannot run a cascade of %lld sections (sections must lie in [1, %d])", (long long)sections, kMaxSections));
  if (!sos) throw Failure("create: null pointer");
  auto core = std::make_shared<IirCore>();
  const int S = (int)sections, N = 2 * S;
  core->S = S;
  core->sos.assign(sos, sos + 6 * S);
  int64_t b2_zero = 0, a2_zero = 0;
  for (int s = 0; s < S; ++s) {
    const double *row = sos + 6 * s;
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(row[i]))
        throw InvalidArgument(format("create: cannot use the coefficient %g of section %d (coefficients must be finite)", row[i], s));
    if (row[3] != 1.0)
      throw InvalidArgument(format("create: cannot run section %d with a0 = %g (sections must be normalised: a0 must be exactly 1)", s, row[3]));
    const double c[5] = {row[0], row[1], row[2], row[4], row[5]};
    for (int i = 0; i < 5; ++i) core->coef.c[s][i] = c[i];
    b2_zero += row[2] == 0.0 ? 1 : 0;
    a2_zero += row[5] == 0.0 ? 1 : 0;
  }
  core->padlen = 3 * (2 * S + 1 - std::min(b2_zero, a2_zero));
  // column i of M: kBlock zero-input steps from the unit state e_i, the filter's own arithmetic (this file has no contraction,
  // and the host target no fused multiply-add)
  core->M.assign((size_t)N * N, 0.0);
  for (int i = 0; i < N; ++i) {
    double z[2 * kMaxSections] = {};
    z[i] = 1.0;
    for (int t = 0; t < kBlock; ++t) {
      double u = 0.0;
      for (int s = 0; s < S; ++s) {
        const double y = core->coef.c[s][0] * u + z[2 * s];
        z[2 * s] = (core->coef.c[s][1] * u - core->coef.c[s][3] * y) + z[2 * s + 1];
        z[2 * s + 1] = core->coef.c[s][2] * u - core->coef.c[s][4] * y;
        u = y;
      }
    }
    for (int j = 0; j < N; ++j) core->M[(size_t)j * N + i] = z[j];
  }
  return core;
}

// the unit-step steady state in closed form: g = (b0 + b1 + b2) / (1 + a1 + a2), z1 = g - b0, z2 = b2 - a2 g, both scaled by
// the product of the earlier sections' g
void steady_state(const IirCore &core, double *zi) {
  double scale = 1.0;
  for (int s = 0; s < core.S; ++s) {
    const double *k = core.coef.c[s];
    const double den = (1.0 + k[3]) + k[4];
    if (den == 0.0)
      throw InvalidArgument(format("zi: cannot settle section %d on a unit step (1 + a1 + a2 is zero: a pole at z = 1)", s));
    const double g = ((k[0] + k[1]) + k[2]) / den;
    zi[2 * s] = scale * (g - k[0]);
    zi[2 * s + 1] = scale * (k[2] - k[4] * g);
    scale = scale * g;
  }
}

template <int S>
void launch_general(const char *fn, const IirCore &core, const IirIo &io, double *st, int64_t lead, int64_t i0, int64_t i1, int pos0,
                    hipStream_t stream) {
  SMX_LAUNCH((iir_general_kernel<S>), dim3(grid_x(fn, "workgroups", (lead + 63) / 64, 64)), dim3(64), 0, stream, core.coef, io, core.device_matrix(), st, lead,
             i0, i1, pos0);
  SMX_HIP_CHECK(hipGetLastError());
}

// the zero-state pass and the chain: ws [lead; nb; 2S] leaves with s_b
template <typename E, int S>
void launch_block_states(const char *fn, const IirCore &core, const IirIo &io, double *st, int64_t lead, int64_t first, int64_t nb, double *ws,
                         hipStream_t stream) {
  constexpr int N = 2 * S, G = N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : 16;
  const int64_t spans = (nb + kSpanBlocks - 1) / kSpanBlocks;
  const size_t lds = (size_t)kSpanBlocks * kPitch * sizeof(E);   // 8.25 KB of float32, 16.5 KB of float64
  launch_tiles(fn, iir_block_w_kernel<E, S>, lead * spans, 64, lds, stream, core.coef, io, first, nb, spans, ws);
  SMX_LAUNCH((iir_chain_kernel<S>), dim3(grid_x(fn, "workgroups", (lead + 64 / G - 1) / (64 / G), 64)), dim3(64), 0, stream, core.device_matrix(), st, ws, lead, nb);
  SMX_HIP_CHECK(hipGetLastError());
}

template <typename E, int S>
void launch_blocks(const char *fn, const IirCore &core, const IirIo &io, double *st, int64_t lead, int64_t first, int64_t nb, hipStream_t stream) {
  constexpr int N = 2 * S;
  const int64_t spans = (nb + kSpanBlocks - 1) / kSpanBlocks;
  grid_x(fn, "block spans", lead * spans, 64);                // refused before the scratch is taken
  const size_t lds = (size_t)kSpanBlocks * kPitch * sizeof(E);
  DeviceScratch ws;
  ws.pool((size_t)lead * (size_t)nb * N * sizeof(double), stream);
  launch_block_states<E, S>(fn, core, io, st, lead, first, nb, ws.as<double>(), stream);
  launch_tiles(fn, iir_block_y_kernel<E, S>, lead * spans, 64, lds, stream, core.coef, io, first, nb, spans, (const double *)ws.as<double>());
}

// samples [0, m) of a pass whose first sample lies pos0 samples into a block, from and into the records st
template <int S>
void run_pass(const char *fn, const IirCore &core, const IirIo &io, double *st, int64_t lead, int64_t m, int pos0, hipStream_t stream) {
  if (lead == 0 || m == 0) return;
  const int64_t head = pos0 ? std::min<int64_t>(m, kBlock - pos0) : 0;
  const int64_t nb = fast_path_disabled() ? 0 : (m - head) / kBlock;
  if (nb == 0) {
    launch_general<S>(fn, core, io, st, lead, 0, m, pos0, stream);
    return;
  }
  if (head) launch_general<S>(fn, core, io, st, lead, 0, head, pos0, stream);
  if (io.x_bytes == 4 && io.out_bytes == 4 && io.src == SRC_PLAIN && io.dst == DST_PLAIN) launch_blocks<float, S>(fn, core, io, st, lead, head, nb, stream);
  else if (io.x_bytes == 4 && io.src != SRC_EXT) throw Failure(format("%s: no block kernel reads float32 samples this way", fn));   // (no face asks for it)
  else launch_blocks<double, S>(fn, core, io, st, lead, head, nb, stream);
  if (head + nb * kBlock < m) launch_general<S>(fn, core, io, st, lead, head + nb * kBlock, m, 0, stream);
}

void run_pass(const char *fn, const IirCore &core, const IirIo &io, double *st, int64_t lead, int64_t m, int pos0, hipStream_t stream) {
  switch (core.S) {
    case 1: return run_pass<1>(fn, core, io, st, lead, m, pos0, stream);
    case 2: return run_pass<2>(fn, core, io, st, lead, m, pos0, stream);
    case 3: return run_pass<3>(fn, core, io, st, lead, m, pos0, stream);
    case 4: return run_pass<4>(fn, core, io, st, lead, m, pos0, stream);
    case 5: return run_pass<5>(fn, core, io, st, lead, m, pos0, stream);
    case 6: return run_pass<6>(fn, core, io, st, lead, m, pos0, stream);
    case 7: return run_pass<7>(fn, core, io, st, lead, m, pos0, stream);
    case 8: return run_pass<8>(fn, core, io, st, lead, m, pos0, stream);
    default: throw Failure(format("%s: a cascade of %d sections has no kernel", fn, core.S));
  }
}

void init_records(const char *fn, const IirCore &core, const IirIo &io, int mode, const double *zi, const double *d_zi_rows, double *st, int64_t lead,
                  hipStream_t stream) {
  const int N = 2 * core.S;
  IirZi v{};
  if (zi) std::copy(zi, zi + N, v.v);
  SMX_LAUNCH(iir_init_kernel, dim3(grid_x(fn, "workgroups", (lead * N + 255) / 256, 256)), dim3(256), 0, stream, io, v, d_zi_rows, mode, st, lead, N);
  SMX_HIP_CHECK(hipGetLastError());
}

IirIo plain_io(const void *d_x, int x_bytes, int64_t x_stride, void *d_out, int out_bytes, int64_t out_stride, int64_t m) {
  IirIo io{};
  io.x = d_x, io.out = d_out, io.x_stride = x_stride, io.out_stride = out_stride, io.nx = m, io.m = m, io.x_bytes = x_bytes, io.out_bytes = out_bytes;
  return io;
}

void check_signal(const char *fn, int64_t lead, int64_t n, int64_t x_stride) {
  check_rank_extents(fn, lead, n);
  if (x_stride < n) throw Failure(format("%s: x_stride is smaller than the signal length", fn));
}

// zi: host [S; 2] or null; d_zi_rows: device [lead; S; 2] or null (at most one of them); d_zf: device [lead; S; 2] or null
void apply_dev(const IirCore &core, const void *d_x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride, const double *zi,
               const double *d_zi_rows, void *d_out, double *d_zf, hipStream_t stream) {
  const char *fn = "apply";
  check_signal(fn, lead, n, x_stride);
  if (zi && d_zi_rows) throw Failure("apply: an initial state per call and one per channel were both given");
  if (lead == 0 || (n == 0 && !d_zf)) return;
  if (n && (!d_x || !d_out)) throw Failure("apply: null device pointer");
  const int N = 2 * core.S;
  DeviceScratch st;
  st.pool((size_t)lead * 3 * N * sizeof(double), stream);
  const IirIo io = plain_io(d_x, elem_bytes, x_stride, d_out, elem_bytes, n, n);
  init_records(fn, core, io, zi ? ZI_CALL : d_zi_rows ? ZI_ROWS : ZI_ZERO, zi, d_zi_rows, st.as<double>(), lead, stream);
  run_pass(fn, core, io, st.as<double>(), lead, n, 0, stream);
  if (d_zf) {
    SMX_LAUNCH(iir_state_out_kernel, dim3(grid_x(fn, "workgroups", (lead * N + 255) / 256, 256)), dim3(256), 0, stream, (const double *)st.as<double>(), d_zf, lead, N);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

void apply_host(const IirCore &core, const void *x, int elem_bytes, int64_t lead, int64_t n, const double *zi, int zi_rows, void *out, double *zf) {
  const char *fn = "apply";
  check_rank_extents(fn, lead, n);
  if (lead == 0) return;
  const int N = 2 * core.S;
  if (n == 0) {   // nothing runs: the state handed back is the state given
    for (int64_t i = 0; zf && i < lead * N; ++i) zf[i] = zi ? zi[zi_rows ? i : i % N] : 0.0;
    return;
  }
  if (!x || !out) throw Failure("apply: null pointer");
  const size_t row = (size_t)n * (size_t)elem_bytes, rec = (size_t)N * sizeof(double);
  host_call(fn, {{x, row}, {zi && zi_rows ? zi : nullptr, rec}}, {HostOut{out, row}, HostOut{zf, rec}}, lead, false, nullptr,
            [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t stream) {
              apply_dev(core, d_in[0], elem_bytes, nc, n, n, zi && !zi_rows ? zi : nullptr, reinterpret_cast<const double *>(d_in[1]), d_out[0],
                        reinterpret_cast<double *>(d_out[1]), stream);
            });
}

void filtfilt_dev(const IirCore &core, const void *d_x, int elem_bytes, int64_t lead, int64_t n, int64_t x_stride, void *d_out, hipStream_t stream) {
  const char *fn = "filtfilt";
  check_signal(fn, lead, n, x_stride);
  double zi[2 * kMaxSections];
  steady_state(core, zi);
  const int64_t p = core.padlen, m = n + 2 * p;
  if (n <= p)
    throw InvalidArgument(format("filtfilt: cannot extend a signal of %lld samples by %lld on each side (n must exceed padlen = %lld)", (long long)n,
                                 (long long)p, (long long)p));
  if (lead == 0) return;
  if (!d_x || !d_out) throw Failure("filtfilt: null device pointer");
  const int N = 2 * core.S;
  DeviceScratch st, mid;
  st.pool((size_t)lead * 3 * N * sizeof(double), stream);
  mid.pool((size_t)lead * (size_t)m * sizeof(double), stream);
  IirIo fwd = plain_io(d_x, elem_bytes, x_stride, mid.ptr, 8, m, m);
  fwd.src = SRC_EXT, fwd.nx = n, fwd.pad = p;
  init_records(fn, core, fwd, ZI_SCALED, zi, nullptr, st.as<double>(), lead, stream);
  run_pass(fn, core, fwd, st.as<double>(), lead, m, 0, stream);
  IirIo back = plain_io(mid.ptr, 8, m, d_out, elem_bytes, n, m);
  back.src = SRC_REV, back.dst = DST_REV_TRIM, back.nx = n, back.pad = p;
  init_records(fn, core, back, ZI_SCALED, zi, nullptr, st.as<double>(), lead, stream);
  run_pass(fn, core, back, st.as<double>(), lead, m, 0, stream);
}

void filtfilt_host(const IirCore &core, const void *x, int elem_bytes, int64_t lead, int64_t n, void *out) {
  filtfilt_dev(core, nullptr, elem_bytes, 0, n, n, nullptr, nullptr);   // the checks, before a device is asked for
  check_rank_extents("filtfilt", lead, n);
  if (lead == 0) return;
  if (!x || !out) throw Failure("filtfilt: null pointer");
  const size_t row = (size_t)n * (size_t)elem_bytes;
  host_call("filtfilt", {{x, row}}, out, row, lead, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
    filtfilt_dev(core, d_in[0], elem_bytes, nc, n, n, d_out, stream);
  });
}

template <int S>
void block_states(const char *fn, const IirCore &core, const IirIo &io, double *st, int64_t lead, int64_t first, int64_t nb, double *ws, hipStream_t stream) {
  if (io.x_bytes == 4) launch_block_states<float, S>(fn, core, io, st, lead, first, nb, ws, stream);
  else launch_block_states<double, S>(fn, core, io, st, lead, first, nb, ws, stream);
}

}  // namespace

// ---- what smx_internal.hpp offers the modules built on the block route ------------------------------------------------------------
std::shared_ptr<IirCore> iir_make_core(const double *sos, int64_t sections) { return make_core(sos, sections); }
const IirCoef &iir_coef(const IirCore &core) { return core.coef; }
const double *iir_device_matrix(const IirCore &core) { return core.device_matrix(); }

void iir_block_states(const char *fn, const IirCore &core, const void *d_x, int x_bytes, int64_t x_stride, double *st, int64_t lead, int64_t first,
                      int64_t nb, double *ws, hipStream_t stream) {
  if (lead == 0 || nb == 0) return;
  const IirIo io = plain_io(d_x, x_bytes, x_stride, nullptr, x_bytes, 0, first + nb * kBlock);
  switch (core.S) {
    case 1: return block_states<1>(fn, core, io, st, lead, first, nb, ws, stream);
    case 2: return block_states<2>(fn, core, io, st, lead, first, nb, ws, stream);
    case 3: return block_states<3>(fn, core, io, st, lead, first, nb, ws, stream);
    case 4: return block_states<4>(fn, core, io, st, lead, first, nb, ws, stream);
    case 5: return block_states<5>(fn, core, io, st, lead, first, nb, ws, stream);
    case 6: return block_states<6>(fn, core, io, st, lead, first, nb, ws, stream);
    case 7: return block_states<7>(fn, core, io, st, lead, first, nb, ws, stream);
    case 8: return block_states<8>(fn, core, io, st, lead, first, nb, ws, stream);
    default: throw Failure(format("%s: a cascade of %d sections has no kernel", fn, core.S));
  }
}

}  // namespace smx

struct smx_iir {
  std::shared_ptr<smx::IirCore> core;
};

// Iir.Kernel: the records of `channels` channels on the device, the position since reset on the host
struct smx_iir_kernel {
  std::shared_ptr<smx::IirCore> core;
  int64_t channels = 0, position = 0;
  int device = 0;
  double *st = nullptr;
  bool fresh = true, drained = false;
  ~smx_iir_kernel() {
    if (st) (void)hipFree(st);
  }
};

namespace smx {
namespace {

void kernel_step_dev(smx_iir_kernel &k, const void *d_x, int elem_bytes, int64_t m, int64_t x_stride, void *d_out, hipStream_t stream) {
  const char *fn = "step";
  if (k.drained) throw InvalidArgument("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)");
  if (m < 0) throw Failure("step: negative chunk length");
  if (x_stride < m) throw Failure("step: x_stride is smaller than the chunk length");
  if (m == 0) return;
  if (!d_x || !d_out) throw Failure("step: null device pointer");
  const IirCore &core = *k.core;
  if (!k.st) {
    SMX_HIP_CHECK(hipGetDevice(&k.device));
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&k.st), (size_t)k.channels * 6 * core.S * sizeof(double)));
  }
  const IirIo io = plain_io(d_x, elem_bytes, x_stride, d_out, elem_bytes, m, m);
  if (k.fresh) init_records(fn, core, io, ZI_ZERO, nullptr, nullptr, k.st, k.channels, stream);
  k.fresh = false;
  run_pass(fn, core, io, k.st, k.channels, m, (int)(k.position % kBlock), stream);
  k.position += m;
}

void kernel_step_host(smx_iir_kernel &k, const void *x, int elem_bytes, int64_t m, void *out) {
  if (k.drained || m <= 0) return kernel_step_dev(k, nullptr, elem_bytes, m, m, nullptr, nullptr);
  if (!x || !out) throw Failure("step: null pointer");
  const size_t row = (size_t)m * (size_t)elem_bytes;
  host_call("step", {{x, row}}, out, row, k.channels, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t, hipStream_t stream) {
    kernel_step_dev(k, d_in[0], elem_bytes, m, m, d_out, stream);
  });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Iir -------------------------------------------------------------------------------------------------------------------
int smx_iir_create(const double *sos, int64_t sections, smx_iir **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null result pointer");
    auto core = make_core(sos, sections);
    *out = new smx_iir{core};
  });
}
void smx_iir_destroy(smx_iir *c) { delete c; }
int64_t smx_iir_block(void) { return kBlock; }
int64_t smx_iir_span_blocks(void) { return kSpanBlocks; }
int64_t smx_iir_max_sections(void) { return kMaxSections; }
int64_t smx_iir_sections(const smx_iir *c) { return c ? c->core->S : 0; }
int64_t smx_iir_padlen(const smx_iir *c) { return c ? c->core->padlen : 0; }
int smx_iir_matrix(const smx_iir *c, double *m) {
  return guarded([&] {
    check_config(c, "matrix");
    if (!m) throw Failure("matrix: null pointer");
    std::copy(c->core->M.begin(), c->core->M.end(), m);
  });
}
int smx_iir_zi(const smx_iir *c, double *zi) {
  return guarded([&] {
    check_config(c, "zi");
    if (!zi) throw Failure("zi: null pointer");
    steady_state(*c->core, zi);
  });
}
int smx_iir_apply_f32(const smx_iir *c, const float *x, int64_t lead, int64_t n, const double *zi, int zi_rows, float *out, double *zf) {
  return guarded([&] {
    check_config(c, "apply");
    apply_host(*c->core, x, 4, lead, n, zi, zi_rows, out, zf);
  });
}
int smx_iir_apply_f64(const smx_iir *c, const double *x, int64_t lead, int64_t n, const double *zi, int zi_rows, double *out, double *zf) {
  return guarded([&] {
    check_config(c, "apply");
    apply_host(*c->core, x, 8, lead, n, zi, zi_rows, out, zf);
  });
}
int smx_iir_apply_card_f32(const smx_iir *c, void *stream, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, const double *zi,
                           const double *d_zi_rows, float *d_out, double *d_zf) {
  return guarded([&] {
    check_config(c, "apply");
    apply_dev(*c->core, d_x, 4, lead, n, x_stride, zi, d_zi_rows, d_out, d_zf, (hipStream_t)stream);
  });
}
int smx_iir_filtfilt_f32(const smx_iir *c, const float *x, int64_t lead, int64_t n, float *out) {
  return guarded([&] {
    check_config(c, "filtfilt");
    filtfilt_host(*c->core, x, 4, lead, n, out);
  });
}
int smx_iir_filtfilt_f64(const smx_iir *c, const double *x, int64_t lead, int64_t n, double *out) {
  return guarded([&] {
    check_config(c, "filtfilt");
    filtfilt_host(*c->core, x, 8, lead, n, out);
  });
}
int smx_iir_filtfilt_card_f32(const smx_iir *c, void *stream, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, float *d_out) {
  return guarded([&] {
    check_config(c, "filtfilt");
    filtfilt_dev(*c->core, d_x, 4, lead, n, x_stride, d_out, (hipStream_t)stream);
  });
}
int smx_iir_kernel_prepare(const smx_iir *c, int64_t channels, smx_iir_kernel **out) {
  return guarded([&] {
    check_config(c, "prepare");
    if (!out) throw Failure("prepare: null result pointer");
    if (channels < 1)
      throw InvalidArgument(format("prepare: cannot keep the state of %lld channels (channels must be at least 1)", (long long)channels));
    auto *k = new smx_iir_kernel;
    k->core = c->core;
    k->channels = channels;
    *out = k;
  });
}
void smx_iir_kernel_destroy(smx_iir_kernel *k) { delete k; }
int smx_iir_kernel_reset(smx_iir_kernel *k) {
  return guarded([&] {
    check_config(k, "reset");
    k->position = 0, k->fresh = true, k->drained = false;
  });
}
int smx_iir_kernel_flush(smx_iir_kernel *k) {
  return guarded([&] {
    check_config(k, "flush");
    k->drained = true;
  });
}
int64_t smx_iir_kernel_position(const smx_iir_kernel *k) { return k ? k->position : 0; }
int smx_iir_kernel_step_f32(smx_iir_kernel *k, const float *x, int64_t m, float *out) {
  return guarded([&] {
    check_config(k, "step");
    kernel_step_host(*k, x, 4, m, out);
  });
}
int smx_iir_kernel_step_f64(smx_iir_kernel *k, const double *x, int64_t m, double *out) {
  return guarded([&] {
    check_config(k, "step");
    kernel_step_host(*k, x, 8, m, out);
  });
}
int smx_iir_kernel_step_card_f32(smx_iir_kernel *k, void *stream, const float *d_x, int64_t m, int64_t x_stride, float *d_out) {
  return guarded([&] {
    check_config(k, "step");
    kernel_step_dev(*k, d_x, 4, m, x_stride, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
