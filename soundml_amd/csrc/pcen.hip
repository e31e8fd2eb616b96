// Per-channel energy normalisation (PCEN; Wang et al. 2017, Lostanlen et al. 2019; librosa.pcen with max_size = 1; not in the
// reference) over a device-resident non-negative spectrogram [rows; frames], frames fastest.  A row is one (leading index, band).
//
// The definition, float64 inside, every product and every sum rounded on its own (this file is built with
// -ffp-contract=off and nothing here says fma), one rounding to the dtype of the input at the end:
//     u[t] = scale * (double)S[t]
//     M[t] = a * M[t-1] + s * u[t]            the two products, then the sum; a = 1 - s from the host; M[-1] = zi, or u[0]
//     sm   = exp(-gain * (log(eps) + log1p(M[t] / eps)))                                  log(eps) from the host
//     out  = log1p(u * sm / bias)                                 power == 0
//          = exp(power * (log(u) + log(sm))), 0 where u == 0      bias == 0
//          = bias^power * expm1(power * log1p(u * sm / bias))     otherwise; bias^power from the host
// Time is not cut into blocks: the order is the plain recurrence and a stream carries one double per row.  pcen_compress is the one
// statement of the compression; both kernels call it, so the device library's exp / log / log1p / expm1 give the same bits on
// either route.
//
//   pcen_general_kernel   a lane per row walks the frames serially: every geometry; short chunks and SMX_DISABLE_FAST=1.  Its loads
//                         across a wave are strided
//   pcen_tile_kernel      a workgroup of four waves owns 64 consecutive rows and walks the frames in tiles of 64.  A tile comes to
//                         LDS in coalesced loads (rows kTile + 1 elements apart: an odd pitch, a lane per row walks distinct
//                         banks); wave 0 runs the 64 recurrences over it, a lane per row, and leaves M as doubles in LDS; all four
//                         waves compress the tile's cells, a lane per frame, and store them coalesced.  The next tile's samples are
//                         fetched into registers before the compression starts, so their latency hides behind it; the recurrence
//                         (64 dependent steps between two barriers; with loads, staging and stores 15 to 19 % of the kernel's time,
//                         profiles/pcen/NOTES.md) runs while the waves of the other workgroups on the compute unit compress.  Partial row groups, a partial last tile and a row pitch larger than
//                         `frames` are handled here.  Rows may start at any 4-byte position: the loads are one element per lane
//
// The module's checks and extern "C" entries close the file.
#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kRows = 64;            // rows of a workgroup: one per lane of the recurrence wave
constexpr int kTile = 64;            // frames of a tile
constexpr int kPitch = kTile + 1;    // LDS row pitch in elements
constexpr int kThreads = 256;
constexpr int kPerThread = kRows * kTile / kThreads;
constexpr int kTileMinFrames = 16;   // the tile kernel serves calls of at least this many frames

enum { FORM_LOG = 0, FORM_NO_BIAS = 1, FORM_GENERAL = 2 };

struct PcenParams {
  double a, s, scale, eps, log_eps, gain, bias, power, bias_pow;
  int form;
};

// the compression of one cell, the operations in the stated order
__device__ __forceinline__ double pcen_compress(const PcenParams &p, double u, double M) {
  const double sm = exp(-p.gain * (p.log_eps + log1p(M / p.eps)));
  if (p.form == FORM_LOG) return log1p(u * sm / p.bias);
  if (p.form == FORM_NO_BIAS) return u == 0.0 ? 0.0 : exp(p.power * (log(u) + log(sm)));
  return p.bias_pow * expm1(p.power * log1p(u * sm / p.bias));
}

// one step of the smoother
__device__ __forceinline__ double pcen_smooth(const PcenParams &p, double M, double u) {
  const double keep = p.a * M, take = p.s * u;
  return keep + take;
}

template <typename E>
__global__ void __launch_bounds__(64) pcen_general_kernel(PcenParams p, const E *x, int64_t x_stride, E *out, int64_t rows, int64_t frames,
                                                          const double *zi, double *zf, int smooth_only) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  const E *row = x + r * x_stride;
  E *o = out + r * frames;
  double M = zi ? zi[r] : p.scale * (double)row[0];
  for (int64_t t = 0; t < frames; ++t) {
    const double u = p.scale * (double)row[t];
    M = pcen_smooth(p, M, u);
    o[t] = (E)(smooth_only ? M : pcen_compress(p, u, M));
  }
  if (zf) zf[r] = M;
}

template <typename E>
__global__ void __launch_bounds__(kThreads) pcen_tile_kernel(PcenParams p, const E *x, int64_t x_stride, E *out, int64_t rows, int64_t frames,
                                                             const double *zi, double *zf, int smooth_only) {
  extern __shared__ __align__(16) unsigned char pcen_lds[];
  double *s_m = reinterpret_cast<double *>(pcen_lds);                  // [kRows][kPitch]
  E *s_x = reinterpret_cast<E *>(s_m + kRows * kPitch);                // [kRows][kPitch]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kRows;
  const int nrows = (int)(rows - r0 < kRows ? rows - r0 : kRows);
  const int64_t ntiles = (frames + kTile - 1) / kTile;

  // cell i of this thread in a tile: row (i * kThreads + tid) / kTile = i * 4 + wave, frame lane
  E v[kPerThread];
  auto fetch = [&](int64_t tile) {
    const int64_t t = tile * kTile + lane;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int rr = i * (kThreads / kTile) + wave;
      v[i] = rr < nrows && t < frames ? x[(r0 + rr) * x_stride + t] : (E)0;
    }
  };
  fetch(0);
  double M = 0.0;
  if (wave == 0 && lane < nrows) M = zi ? zi[r0 + lane] : p.scale * (double)x[(r0 + lane) * x_stride];
  for (int64_t tile = 0; tile < ntiles; ++tile) {
    const int64_t t0 = tile * kTile;
    const int width = (int)(frames - t0 < kTile ? frames - t0 : kTile);
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) s_x[(i * (kThreads / kTile) + wave) * kPitch + lane] = v[i];
    __syncthreads();
    if (tile + 1 < ntiles) fetch(tile + 1);            // in flight while this tile is smoothed and compressed
    if (wave == 0 && lane < nrows) {
      const E *xr = s_x + lane * kPitch;
      double *mr = s_m + lane * kPitch;
      for (int t = 0; t < width; ++t) {
        M = pcen_smooth(p, M, p.scale * (double)xr[t]);
        mr[t] = M;
      }
    }
    __syncthreads();
    if (lane < width) {
#pragma unroll 2
      for (int i = 0; i < kPerThread; ++i) {
        const int rr = i * (kThreads / kTile) + wave;
        if (rr < nrows) {
          const double m = s_m[rr * kPitch + lane];
          const double u = p.scale * (double)s_x[rr * kPitch + lane];
          out[(r0 + rr) * frames + t0 + lane] = (E)(smooth_only ? m : pcen_compress(p, u, m));
        }
      }
    }
    __syncthreads();                                   // the tile is read: the next one may take its place
  }
  if (zf && wave == 0 && lane < nrows) zf[r0 + lane] = M;
}

}  // namespace

// ---- the host side -------------------------------------------------------------------------------------------------------------
struct PcenCore {
  PcenParams p{};   // the coefficient and the constants the host computes once, as the kernels take them
};

namespace {

std::shared_ptr<PcenCore> make_core(int64_t sr, int64_t hop, double gain, double bias, double power, double time_constant, double eps, bool has_b,
                                    double b, double scale) {
  const struct {
    const char *name;
    double v;
  } all[] = {{"gain", gain}, {"bias", bias}, {"power", power}, {"time_constant", time_constant}, {"eps", eps}, {"b", has_b ? b : 0.0}, {"scale", scale}};
  for (const auto &q : all)
    if (!std::isfinite(q.v)) throw InvalidArgument(format("create: cannot use the parameter %s = %g (parameters must be finite)", q.name, q.v));
  if (gain < 0.0) throw InvalidArgument(format("create: cannot use a gain of %g (gain must be at least 0)", gain));
  if (bias < 0.0) throw InvalidArgument(format("create: cannot use a bias of %g (bias must be at least 0)", bias));
  if (power < 0.0) throw InvalidArgument(format("create: cannot use a power of %g (power must be at least 0)", power));
  if (eps <= 0.0) throw InvalidArgument(format("create: cannot use an eps of %g (eps must be positive)", eps));
  if (time_constant <= 0.0) throw InvalidArgument(format("create: cannot use a time constant of %g (time_constant must be positive)", time_constant));
  if (sr <= 0) throw InvalidArgument(format("create: cannot use a sample rate of %lld (sr must be at least 1)", (long long)sr));
  if (hop <= 0) throw InvalidArgument(format("create: cannot advance frames by %lld samples (hop must be at least 1)", (long long)hop));
  if (has_b && !(b >= 0.0 && b <= 1.0)) throw InvalidArgument(format("create: cannot smooth with the coefficient b = %g (b must lie in [0, 1])", b));
  if (scale <= 0.0) throw InvalidArgument(format("create: cannot scale by %g (scale must be positive)", scale));
  if (power == 0.0 && bias == 0.0)
    throw InvalidArgument("create: cannot take the logarithm form without a bias (power == 0 needs bias > 0)");
  auto core = std::make_shared<PcenCore>();
  double s = b;
  if (!has_b) {
    const double T = time_constant * (double)sr / (double)hop;
    const double TT = T * T;
    s = (std::sqrt(1.0 + 4.0 * TT) - 1.0) / (2.0 * TT);
  }
  PcenParams &p = core->p;
  p.s = s, p.a = 1.0 - s, p.scale = scale, p.eps = eps, p.log_eps = std::log(eps), p.gain = gain, p.bias = bias, p.power = power;
  p.bias_pow = std::pow(bias, power);
  p.form = power == 0.0 ? FORM_LOG : bias == 0.0 ? FORM_NO_BIAS : FORM_GENERAL;
  return core;
}

void check_rows(const char *fn, int64_t rows, int64_t frames, int64_t x_stride) {
  if (rows < 0 || frames < 0) throw Failure(format("%s: negative extent", fn));
  if (x_stride < frames) throw Failure(format("%s: x_stride is smaller than the number of frames", fn));
}

template <typename E>
void launch_rows(const char *fn, const PcenParams &p, const void *d_x, int64_t x_stride, void *d_out, int64_t rows, int64_t frames, const double *d_zi,
                 double *d_zf, int smooth_only, hipStream_t stream) {
  const E *x = reinterpret_cast<const E *>(d_x);
  E *out = reinterpret_cast<E *>(d_out);
  // (the row count cannot reach the launch limit within device memory: grid_x words the refusal, no range loop is needed)
  if (frames >= kTileMinFrames && !fast_path_disabled()) {
    const size_t lds = (size_t)kRows * kPitch * (sizeof(double) + sizeof(E));   // 48.75 KB of float32, 65 KB of float64
    const unsigned grid = grid_x(fn, "row groups", (rows + kRows - 1) / kRows, kThreads);
    SMX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(pcen_tile_kernel<E>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SMX_LAUNCH((pcen_tile_kernel<E>), dim3(grid), dim3(kThreads), lds, stream, p, x, x_stride, out, rows, frames, d_zi, d_zf, smooth_only);
  } else {
    SMX_LAUNCH((pcen_general_kernel<E>), dim3(grid_x(fn, "row groups", (rows + 63) / 64, 64)), dim3(64), 0, stream, p, x, x_stride, out, rows, frames, d_zi,
               d_zf, smooth_only);
  }
  SMX_HIP_CHECK(hipGetLastError());
}

// d_zi: device [rows] or null (M[-1] = u[0]); d_zf: device [rows] or null; both may be the same array
void rows_dev(const char *fn, const PcenCore &core, const void *d_x, int elem_bytes, int64_t rows, int64_t frames, int64_t x_stride, const double *d_zi,
              void *d_out, double *d_zf, int smooth_only, hipStream_t stream) {
  check_rows(fn, rows, frames, x_stride);
  if (rows == 0) return;
  if (frames == 0) {   // nothing runs: the state handed back is the state given, or zero
    if (d_zf && d_zi && d_zf != d_zi) SMX_HIP_CHECK(hipMemcpyAsync(d_zf, d_zi, (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, stream));
    else if (d_zf && !d_zi) SMX_HIP_CHECK(hipMemsetAsync(d_zf, 0, (size_t)rows * sizeof(double), stream));
    return;
  }
  if (!d_x || !d_out) throw Failure(format("%s: null device pointer", fn));
  if (elem_bytes == 4) launch_rows<float>(fn, core.p, d_x, x_stride, d_out, rows, frames, d_zi, d_zf, smooth_only, stream);
  else launch_rows<double>(fn, core.p, d_x, x_stride, d_out, rows, frames, d_zi, d_zf, smooth_only, stream);
}

void rows_host(const char *fn, const PcenCore &core, const void *x, int elem_bytes, int64_t rows, int64_t frames, const double *zi, void *out, double *zf,
               int smooth_only) {
  check_rows(fn, rows, frames, frames);
  if (rows == 0) return;
  if (frames == 0) {
    for (int64_t i = 0; zf && i < rows; ++i) zf[i] = zi ? zi[i] : 0.0;
    return;
  }
  if (!x || !out) throw Failure(format("%s: null pointer", fn));
  const size_t row = (size_t)frames * (size_t)elem_bytes;
  host_call(fn, {{x, row}, {zi, sizeof(double)}}, {HostOut{out, row}, HostOut{zf, sizeof(double)}}, rows, false, nullptr,
            [&](const void *const *d_in, void *const *d_out, int64_t nr, hipStream_t stream) {
              rows_dev(fn, core, d_in[0], elem_bytes, nr, frames, frames, reinterpret_cast<const double *>(d_in[1]), d_out[0],
                       reinterpret_cast<double *>(d_out[1]), smooth_only, stream);
            });
}

// pcen of mel_spectrogram(power = 1) of audio [lead; n]: the mel spectrogram lies in stream-ordered scratch and never leaves the device
void of_audio_dev(const PcenCore &core, const smx_stft_config &sc, const smx_mel_config &mc, const void *d_x, int elem_bytes, int64_t lead, int64_t n,
                  int64_t x_stride, void *d_out, hipStream_t stream) {
  const char *fn = "pcen";
  check_rank_extents(fn, lead, n);
  if (x_stride < n) throw Failure("pcen: x_stride is smaller than the signal length");
  mel_spectrogram_dev(sc, mc, nullptr, elem_bytes, 0, n, n, 1.0, nullptr, stream);   // the configurations' own check, in mel_spectrogram's words
  if (lead == 0) return;
  const int64_t count = sc.frames(n);
  DeviceScratch mel;
  if (count > 0) mel.pool((size_t)lead * (size_t)mc.n_mels * (size_t)count * (size_t)elem_bytes, stream);
  mel_spectrogram_dev(sc, mc, d_x, elem_bytes, lead, n, x_stride, 1.0, mel.ptr, stream);
  if (count == 0) return;
  rows_dev(fn, core, mel.ptr, elem_bytes, lead * mc.n_mels, count, count, nullptr, d_out, nullptr, 0, stream);
}

void of_audio_host(const PcenCore &core, const smx_stft_config &sc, const smx_mel_config &mc, const void *x, int elem_bytes, int64_t lead, int64_t n,
                   void *out) {
  of_audio_dev(core, sc, mc, nullptr, elem_bytes, 0, n, n, nullptr, nullptr);   // the checks, before a device is asked for
  check_rank_extents("pcen", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure("pcen: null pointer");
  host_call("pcen", {{x, (size_t)n * (size_t)elem_bytes}}, out, (size_t)mc.n_mels * (size_t)count * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              of_audio_dev(core, sc, mc, d_in[0], elem_bytes, nc, n, n, d_out, stream);
            });
}

}  // namespace
}  // namespace smx

struct smx_pcen {
  std::shared_ptr<smx::PcenCore> core;
};

// Pcen.Kernel: one double per row on the device (M at the last frame fed), whether the stream has started on the host.  The state
// is allocated by the first step, on that step's device, and is both input and output of every later launch: one kernel belongs to
// one device and to one stream at a time (steps on different streams are the caller's to order)
struct smx_pcen_kernel {
  std::shared_ptr<smx::PcenCore> core;
  int64_t rows = 0;
  int device = -1;
  double *state = nullptr;
  bool started = false, drained = false;
  ~smx_pcen_kernel() {
    if (state) (void)hipFree(state);
  }
};

namespace smx {
namespace {

void kernel_step_dev(smx_pcen_kernel &k, const void *d_x, int elem_bytes, int64_t m, int64_t x_stride, void *d_out, hipStream_t stream) {
  if (k.drained) throw InvalidArgument("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)");
  if (m < 0) throw Failure("step: negative chunk length");
  if (x_stride < m) throw Failure("step: x_stride is smaller than the chunk length");
  if (m == 0) return;
  if (!d_x || !d_out) throw Failure("step: null device pointer");
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  if (!k.state) {
    SMX_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&k.state), (size_t)k.rows * sizeof(double)));
    k.device = device;
  }
  if (device != k.device)
    throw InvalidArgument(format("step: cannot continue on device %d a stream whose state lies on device %d (a kernel belongs to one device)", device, k.device));
  rows_dev("step", *k.core, d_x, elem_bytes, k.rows, m, x_stride, k.started ? k.state : nullptr, d_out, k.state, 0, stream);
  k.started = true;
}

void kernel_step_host(smx_pcen_kernel &k, const void *x, int elem_bytes, int64_t m, void *out) {
  if (k.drained || m <= 0) return kernel_step_dev(k, nullptr, elem_bytes, m, m, nullptr, nullptr);
  if (!x || !out) throw Failure("step: null pointer");
  const size_t row = (size_t)m * (size_t)elem_bytes;
  host_call("step", {{x, row}}, out, row, k.rows, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t, hipStream_t stream) {
    kernel_step_dev(k, d_in[0], elem_bytes, m, m, d_out, stream);
  });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Pcen ------------------------------------------------------------------------------------------------------------------
int smx_pcen_create(int64_t sr, int64_t hop, double gain, double bias, double power, double time_constant, double eps, int has_b, double b, double scale,
                    smx_pcen **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null result pointer");
    auto core = make_core(sr, hop, gain, bias, power, time_constant, eps, has_b != 0, b, scale);
    *out = new smx_pcen{core};
  });
}
void smx_pcen_destroy(smx_pcen *c) { delete c; }
double smx_pcen_coefficient(const smx_pcen *c) { return c ? c->core->p.s : 0.0; }
int64_t smx_pcen_tile_min_frames(void) { return kTileMinFrames; }
int smx_pcen_apply_f32(const smx_pcen *c, const float *x, int64_t rows, int64_t frames, const double *zi, float *out, double *zf) {
  return guarded([&] {
    check_config(c, "apply");
    rows_host("apply", *c->core, x, 4, rows, frames, zi, out, zf, 0);
  });
}
int smx_pcen_apply_f64(const smx_pcen *c, const double *x, int64_t rows, int64_t frames, const double *zi, double *out, double *zf) {
  return guarded([&] {
    check_config(c, "apply");
    rows_host("apply", *c->core, x, 8, rows, frames, zi, out, zf, 0);
  });
}
int smx_pcen_apply_card_f32(const smx_pcen *c, void *stream, const float *d_x, int64_t rows, int64_t frames, int64_t x_stride, const double *d_zi,
                            float *d_out, double *d_zf) {
  return guarded([&] {
    check_config(c, "apply");
    rows_dev("apply", *c->core, d_x, 4, rows, frames, x_stride, d_zi, d_out, d_zf, 0, (hipStream_t)stream);
  });
}
int smx_pcen_smooth_f32(const smx_pcen *c, const float *x, int64_t rows, int64_t frames, const double *zi, float *out) {
  return guarded([&] {
    check_config(c, "smooth");
    rows_host("smooth", *c->core, x, 4, rows, frames, zi, out, nullptr, 1);
  });
}
int smx_pcen_smooth_f64(const smx_pcen *c, const double *x, int64_t rows, int64_t frames, const double *zi, double *out) {
  return guarded([&] {
    check_config(c, "smooth");
    rows_host("smooth", *c->core, x, 8, rows, frames, zi, out, nullptr, 1);
  });
}
int smx_pcen_smooth_card_f32(const smx_pcen *c, void *stream, const float *d_x, int64_t rows, int64_t frames, int64_t x_stride, const double *d_zi,
                             float *d_out) {
  return guarded([&] {
    check_config(c, "smooth");
    rows_dev("smooth", *c->core, d_x, 4, rows, frames, x_stride, d_zi, d_out, nullptr, 1, (hipStream_t)stream);
  });
}
int smx_pcen_of_audio_f32(const smx_pcen *c, const smx_stft_config *sc, const smx_mel_config *mc, const float *x, int64_t lead, int64_t n, float *out) {
  return guarded([&] {
    check_config(c, "pcen");
    check_config(sc, "pcen");
    check_config(mc, "pcen");
    of_audio_host(*c->core, *sc, *mc, x, 4, lead, n, out);
  });
}
int smx_pcen_of_audio_f64(const smx_pcen *c, const smx_stft_config *sc, const smx_mel_config *mc, const double *x, int64_t lead, int64_t n, double *out) {
  return guarded([&] {
    check_config(c, "pcen");
    check_config(sc, "pcen");
    check_config(mc, "pcen");
    of_audio_host(*c->core, *sc, *mc, x, 8, lead, n, out);
  });
}
int smx_pcen_of_audio_card_f32(const smx_pcen *c, void *stream, const smx_stft_config *sc, const smx_mel_config *mc, const float *d_x, int64_t lead,
                               int64_t n, int64_t x_stride, float *d_out) {
  return guarded([&] {
    check_config(c, "pcen");
    check_config(sc, "pcen");
    check_config(mc, "pcen");
    of_audio_dev(*c->core, *sc, *mc, d_x, 4, lead, n, x_stride, d_out, (hipStream_t)stream);
  });
}
int smx_pcen_kernel_prepare(const smx_pcen *c, int64_t rows, smx_pcen_kernel **out) {
  return guarded([&] {
    check_config(c, "prepare");
    if (!out) throw Failure("prepare: null result pointer");
    if (rows < 1) throw InvalidArgument(format("prepare: cannot keep the state of %lld rows (rows must be at least 1)", (long long)rows));
    auto *k = new smx_pcen_kernel;
    k->core = c->core;
    k->rows = rows;
    *out = k;
  });
}
void smx_pcen_kernel_destroy(smx_pcen_kernel *k) { delete k; }
int smx_pcen_kernel_reset(smx_pcen_kernel *k) {
  return guarded([&] {
    check_config(k, "reset");
    k->started = false, k->drained = false;
  });
}
int smx_pcen_kernel_flush(smx_pcen_kernel *k) {
  return guarded([&] {
    check_config(k, "flush");
    k->drained = true;
  });
}
int smx_pcen_kernel_step_f32(smx_pcen_kernel *k, const float *x, int64_t m, float *out) {
  return guarded([&] {
    check_config(k, "step");
    kernel_step_host(*k, x, 4, m, out);
  });
}
int smx_pcen_kernel_step_f64(smx_pcen_kernel *k, const double *x, int64_t m, double *out) {
  return guarded([&] {
    check_config(k, "step");
    kernel_step_host(*k, x, 8, m, out);
  });
}
int smx_pcen_kernel_step_card_f32(smx_pcen_kernel *k, void *stream, const float *d_x, int64_t m, int64_t x_stride, float *d_out) {
  return guarded([&] {
    check_config(k, "step");
    kernel_step_dev(*k, d_x, 4, m, x_stride, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
