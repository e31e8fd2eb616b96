// Cqt.transform / Cqt.power_spectrum (cqt.ml:615-692) and Chroma.of_cqt / Soundml.chroma_cqt (chroma.ml:371-385) on the device.
//
//   cqt_project_kernel   one octave: z[c, first + b, p] = sum_{n < n_fft} src(c, p hop - n_fft / 2 + n) g[b, n], the frame of
//                        Stft's centered rectangular analysis projected against the time-domain taps of the octave's
//                        half-spectrum kernel (cqt_plan.cpp) -- no transform on the device.  float32 samples widened, float64
//                        taps, float64 sums (v_fma_f64), the octave's gain and the bin's `scale` divisor applied, ONE rounding
//                        to complex64 or to |z|^power in float32, written into the octave's rows of [lead; n_bins; frames].
//
// A workgroup owns 128 frames x 16 bins of one clip and walks the taps in tiles of 32: the tile's taps ([32][16] double2) and
// the samples its frames read are staged in LDS once per tile.  Where hop < 32 the frames' tiles overlap and ONE span of
// (frames - 1) hop + 32 samples serves all of them (the bottom octaves: hop 8 under n_fft 256); where hop >= 32 every frame
// gets its own 32 samples in a row padded to 33 doubles.  A thread holds 4 frames x 2 bins (16 float64 sums): per tap 2
// ds_read_b128 + 4 ds_read_b64 feed 16 v_fma_f64.  The taps of an octave (36 x 512 x 16 B and more) never sit in LDS whole:
// every workgroup streams the same tiles, which L2 serves.  profiles/cqt/NOTES.md has the reasoning and the measurements.
//
// The octave recursion keeps the UNSCALED decimated signals u_i = decimate^i(x) and folds the recursion's scalars (sqrt(2^early),
// once more without `scale`; 1 / sqrt(1/2) per halving) into the octave's gain: the decimator is linear, so this is the
// reference's composition with one float32 rounding fewer per stage, and no elementwise pass over the signal.
#include <cfloat>

#include "cqt_project.hpp"

namespace smx {
namespace {

constexpr int kTapTile = kCqtTapTile, kFrameTile = kCqtFrameTile, kBinTile = kCqtBinTile, kRowPad = kCqtRowPad;   // cqt_project.hpp

struct CqtArgs {
  const float *x;
  int64_t n, x_stride;
  const double2 *taps;
  const double *divisors;
  int64_t count, n_fft, hop;
  int pad;
  double pad_value, gain;
  int64_t first, n_bins, frames, ftiles;
  int mode;
  double power;
  void *out;
};

__global__ void __launch_bounds__(256) cqt_project_kernel(CqtArgs a) {
  __shared__ double2 s_taps[kTapTile * kBinTile];   // [tap][bin]
  __shared__ double s_x[kFrameTile * kRowPad];
  const int tid = threadIdx.x;
  const int64_t clip = blockIdx.x / a.ftiles, tile = blockIdx.x % a.ftiles;
  const int64_t b0 = (int64_t)blockIdx.y * kBinTile, p0 = tile * kFrameTile;
  const int nf = (int)(a.frames - p0 < kFrameTile ? a.frames - p0 : kFrameTile);
  const float *x = a.x + clip * a.x_stride;
  const bool shared_span = a.hop < kTapTile;
  const int fs = shared_span ? (int)a.hop : kRowPad;
  const int bl = tid & 7, fg = tid >> 3;   // this thread: bins b0 + bl, b0 + bl + 8; frames p0 + fg + 32 r
  const int64_t origin = p0 * a.hop - a.n_fft / 2;   // signal position of tap 0 of the tile's first frame
  double re[4][2] = {}, im[4][2] = {};
  for (int64_t n0 = 0; n0 < a.n_fft; n0 += kTapTile) {
    const int tn = (int)(a.n_fft - n0 < kTapTile ? a.n_fft - n0 : kTapTile);
    for (int i = tid; i < kTapTile * kBinTile; i += 256) {
      const int b = i / kTapTile, j = i % kTapTile;
      double2 v = make_double2(0.0, 0.0);
      if (b0 + b < a.count && j < tn) v = a.taps[(b0 + b) * a.n_fft + n0 + j];
      s_taps[j * kBinTile + b] = v;
    }
    if (shared_span) {
      const int span = (nf - 1) * (int)a.hop + tn;
      for (int i = tid; i < span; i += 256) s_x[i] = fetch_sample(x, a.n, origin + n0 + i, a.pad, a.pad_value);
    } else {
      for (int i = tid; i < nf * kTapTile; i += 256) {
        const int f = i / kTapTile, j = i % kTapTile;
        if (j < tn) s_x[f * kRowPad + j] = fetch_sample(x, a.n, origin + f * a.hop + n0 + j, a.pad, a.pad_value);
      }
    }
    __syncthreads();
    cqt_tile_fma(s_taps, s_x + fg * fs, fs, tn, bl, re, im);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int f = fg + 32 * r;
    if (f >= nf) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t b = b0 + bl + 8 * h;
      if (b >= a.count) continue;
      const int64_t at = (clip * a.n_bins + a.first + b) * a.frames + p0 + f;
      cqt_finish(re[r][h], im[r][h], a.gain, a.divisors, b, a.mode, a.power, a.out, at);
    }
  }
}

double *upload_doubles(const std::vector<double> &host) {
  double *dev = nullptr;
  SMX_HIP_CHECK(hipMalloc((void **)&dev, host.size() * sizeof(double) + 16));
  const hipError_t err = hipMemcpy(dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    (void)hipFree(dev);
    SMX_HIP_CHECK(err);
  }
  return dev;
}

void check_status(int code) {
  if (code == SMX_OK) return;
  if (code == SMX_INVALID_ARGUMENT) throw InvalidArgument(smx_last_error());
  throw Failure(smx_last_error());
}

void check_cqt(const smx_cqt_config *c, const char *op, int64_t lead, int64_t n) {
  if (!c) throw Failure(format("%s: configuration handle is null", op));
  if (lead < 0 || n < 0) throw Failure(format("%s: negative extent (lead %lld, n %lld)", op, (long long)lead, (long long)n));
}

// cqt.ml:615-667 on device-resident float32 audio: out [lead; n_bins; frames] complex64, or |z|^power float32
void cqt_dev(const smx_cqt_config &c, const char *op, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, OutMode mode,
             double power, void *d_out, hipStream_t stream) {
  check_cqt(&c, op, lead, n);
  const int64_t count = c.frames(n);
  if (lead == 0 || count == 0) return;
  if (x_stride < n) throw Failure(format("%s: x_stride is smaller than the signal length", op));
  if (!d_x || !d_out) throw Failure(format("%s: null device pointer", op));
  const smx_cqt_config::Tables &tables = c.tables();
  init_device_pool();
  DeviceScratch ping, pong;   // the decimated signals, alternating
  const float *cur = d_x;
  int64_t cur_n = n, cur_stride = x_stride, stages = 0;
  auto decimate = [&] {
    const int64_t half_n = (cur_n + 1) / 2;
    DeviceScratch &next = stages % 2 == 0 ? ping : pong;
    if (!next.ptr) next.pool(std::max<size_t>(16, (size_t)lead * (size_t)((n + 1) / 2) * sizeof(float)), stream);
    check_status(smx_resample_apply_f32_dev(c.half, cur, lead, cur_n, cur_stride, next.as<float>(), half_n, stream));
    cur = next.as<float>();
    cur_n = cur_stride = half_n;
    ++stages;
  };
  double gain = 1.0;
  if (c.early > 0) {   // cqt.ml:630-640
    for (int64_t e = 0; e < c.early; ++e) decimate();
    const double factor = std::sqrt((double)(int64_t(1) << c.early));
    gain = factor;
    if (!c.scale) gain *= factor;
  }
  const int64_t last = (int64_t)c.octaves.size() - 1;
  for (int64_t i = 0; i <= last; ++i) {
    const smx_cqt_config::Octave &o = c.octaves[(size_t)i];
    CqtProjectJob job;
    job.x = cur; job.lead = lead; job.n = cur_n; job.x_stride = cur_stride;
    job.taps = tables.octaves[(size_t)i];
    job.divisors = c.scale ? job.taps + o.count * o.n_fft * 2 : nullptr;
    job.count = o.count; job.n_fft = o.n_fft; job.hop = o.hop;
    job.pad = c.pad; job.pad_value = c.pad_value / gain;   // the reference pads the scaled signal
    job.gain = gain;
    job.first = o.first; job.n_bins = c.n_bins; job.frames = count;
    job.mode = mode; job.power = power; job.out = d_out; job.stream = stream;
    launch_cqt_project(job);
    if (i < last && o.hop % 2 == 0) {   // halve (cqt.ml:594, 650)
      decimate();
      gain /= std::sqrt(0.5);
    }
  }
}

void cqt_host(const smx_cqt_config *c, const char *op, const float *x, int64_t lead, int64_t n, OutMode mode, double power, void *out) {
  check_cqt(c, op, lead, n);
  const int64_t count = c->frames(n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure(format("%s: null pointer", op));
  host_call(op, {{x, (size_t)n * sizeof(float)}}, out, (size_t)c->n_bins * (size_t)count * (mode == OUT_COMPLEX ? 8 : 4), lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              cqt_dev(*c, op, reinterpret_cast<const float *>(d_in[0]), nc, n, n, mode, power, d_out, stream);
            });
}

// ---- Chroma.of_cqt / Soundml.chroma_cqt --------------------------------------------------------------------------------
// the conditions of chroma.ml:371-381 in the reference's order; true when there is something to compute
bool check_of_cqt(const smx_cqt_config *c, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma, int norm, double norm_p) {
  if (!c) throw Failure("of_cqt: configuration handle is null");
  check_chroma_norm("of_cqt", norm, norm_p);
  (void)cqt_fold_matrix("of_cqt", *c, n_chroma);
  if (lead < 0 || bins < 0 || frames < 0) throw Failure("of_cqt: negative extent");
  if (bins != c->n_bins)
    throw InvalidArgument(format("of_cqt: cannot project %lld constant-Q bins through a configuration of %lld bins", (long long)bins,
                                 (long long)c->n_bins));
  return lead > 0 && frames > 0;
}

void of_cqt_dev(const smx_cqt_config &c, const void *d_s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                int norm, double norm_p, void *d_out, hipStream_t stream) {
  if (!check_of_cqt(&c, lead, bins, frames, n_chroma, norm, norm_p)) return;
  if (!d_s || !d_out) throw Failure("of_cqt: null device pointer");
  ChromaJob job;
  job.weights_t = c.fold(n_chroma);
  job.bins = c.n_bins;
  job.n_chroma = n_chroma;
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

void of_cqt_host(const smx_cqt_config *c, const void *s, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                 int norm, double norm_p, void *out) {
  if (!check_of_cqt(c, lead, bins, frames, n_chroma, norm, norm_p)) return;
  if (!s || !out) throw Failure("of_cqt: null pointer");
  const size_t row = (size_t)frames * (size_t)elem_bytes;
  host_call("of_cqt", {{s, (size_t)bins * row}}, out, (size_t)n_chroma * row, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              of_cqt_dev(*c, d_in[0], elem_bytes, nc, bins, frames, n_chroma, norm, norm_p, d_out, stream);
            });
}

// of_cqt of power_spectrum ~power:1; the magnitudes live in scratch on the device
void chroma_cqt_dev(const smx_cqt_config &c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t n_chroma, int norm,
                    double norm_p, float *d_out, hipStream_t stream) {
  check_cqt(&c, "chroma_cqt", lead, n);
  check_chroma_norm("of_cqt", norm, norm_p);
  (void)cqt_fold_matrix("of_cqt", c, n_chroma);
  const int64_t count = c.frames(n);
  if (lead == 0 || count == 0) return;
  if (!d_x || !d_out) throw Failure("chroma_cqt: null device pointer");
  init_device_pool();
  DeviceScratch magnitudes;
  magnitudes.pool((size_t)lead * (size_t)c.n_bins * (size_t)count * sizeof(float), stream);
  cqt_dev(c, "power_spectrum", d_x, lead, n, x_stride, OUT_POWER, 1.0, magnitudes.ptr, stream);
  of_cqt_dev(c, magnitudes.ptr, 4, lead, c.n_bins, count, n_chroma, norm, norm_p, d_out, stream);
}

}  // namespace

void launch_cqt_project(const CqtProjectJob &job) {
  if (job.lead <= 0 || job.count <= 0 || job.frames <= 0) return;
  if (job.n_fft < 1 || job.hop < 1 || job.n < 1 || job.first < 0 || job.first + job.count > job.n_bins)
    throw Failure("cqt: invalid projection geometry");
  CqtArgs a{};
  a.x = job.x; a.n = job.n; a.x_stride = job.x_stride;
  a.taps = reinterpret_cast<const double2 *>(job.taps);
  a.divisors = job.divisors;
  a.count = job.count; a.n_fft = job.n_fft; a.hop = job.hop;
  a.pad = job.pad; a.pad_value = job.pad_value; a.gain = job.gain;
  a.first = job.first; a.n_bins = job.n_bins; a.frames = job.frames;
  a.ftiles = (job.frames + kFrameTile - 1) / kFrameTile;
  a.mode = (int)job.mode; a.power = job.power; a.out = job.out;
  const int64_t btiles = (job.count + kBinTile - 1) / kBinTile;
  if (btiles > kMaxGridYZ) throw Failure("cqt: too many tiles for one launch");
  SMX_LAUNCH(cqt_project_kernel, dim3(grid_x("cqt", "tiles", job.lead * a.ftiles, 256), (unsigned)btiles), dim3(256), 0, job.stream, a);
  SMX_HIP_CHECK(hipGetLastError());
}

}  // namespace smx

const smx_cqt_config::Tables &smx_cqt_config::tables() const {
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(mutex_);
  auto it = tables_.find(device);
  if (it != tables_.end()) return it->second;
  Tables t;
  try {
    for (const Octave &o : octaves) {   // taps [count; n_fft] (re, im), then the octave's divisors [count]
      std::vector<double> host(o.taps);
      host.insert(host.end(), divisors.begin() + o.first, divisors.begin() + o.first + o.count);
      t.octaves.push_back(smx::upload_doubles(host));
    }
  } catch (...) {
    for (double *p : t.octaves) (void)hipFree(p);
    throw;
  }
  return tables_.emplace(device, std::move(t)).first->second;
}

const double *smx_cqt_config::fold(int64_t n_chroma) const {
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(mutex_);
  auto it = folds_.find({device, n_chroma});
  if (it != folds_.end()) return it->second;
  // transposed [n_bins; rows_pad], rows padded with zeros to a multiple of 12: the layout launch_chroma reads
  const std::vector<double> w = smx::cqt_fold_matrix("of_cqt", *this, n_chroma);
  const int64_t rows_pad = (n_chroma + 11) / 12 * 12;
  std::vector<double> wt((size_t)(n_bins * rows_pad), 0.0);
  for (int64_t ch = 0; ch < n_chroma; ++ch)
    for (int64_t k = 0; k < n_bins; ++k) wt[(size_t)(k * rows_pad + ch)] = w[(size_t)(ch * n_bins + k)];
  double *dev = smx::upload_doubles(wt);
  folds_.emplace(std::make_pair(device, n_chroma), dev);
  return dev;
}

smx_cqt_config::~smx_cqt_config() {
  for (auto &kv : tables_)
    for (double *p : kv.second.octaves) (void)hipFree(p);
  for (auto &kv : folds_) (void)hipFree(kv.second);
  smx_resample_config_destroy(half);
}

using namespace smx;

extern "C" {

int smx_cqt_config_create(int64_t n_bins, int64_t sample_rate, double fmin, int64_t bins_per_octave, int gamma, double gamma_value,
                          double tuning, double filter_scale, double norm, int window, double window_param, int scale, int64_t hop,
                          int pad, double pad_value, smx_cqt_config **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null output handle");
    *out = cqt_config_create(n_bins, sample_rate, fmin, bins_per_octave, gamma, gamma_value, tuning, filter_scale, norm, window,
                             window_param, scale != 0, hop, pad, pad_value);
  });
}
void smx_cqt_config_destroy(smx_cqt_config *c) { delete c; }
int64_t smx_cqt_config_n_bins(const smx_cqt_config *c) { return c ? c->n_bins : -1; }
int64_t smx_cqt_config_bins_per_octave(const smx_cqt_config *c) { return c ? c->bins_per_octave : -1; }
int64_t smx_cqt_config_sample_rate(const smx_cqt_config *c) { return c ? c->sample_rate : -1; }
int64_t smx_cqt_config_hop(const smx_cqt_config *c) { return c ? c->hop : -1; }
int64_t smx_cqt_config_n_octaves(const smx_cqt_config *c) { return c ? c->n_octaves : -1; }
int64_t smx_cqt_config_early(const smx_cqt_config *c) { return c ? c->early : -1; }
int64_t smx_cqt_config_latency(const smx_cqt_config *c) { return c ? c->latency() : -1; }
double smx_cqt_config_cutoff(const smx_cqt_config *c) { return c ? c->cutoff : -1.0; }
int smx_cqt_frequencies(const smx_cqt_config *c, double *out) {
  return guarded([&] {
    if (!c || !out) throw Failure("frequencies: null argument");
    std::copy(c->freqs.begin(), c->freqs.end(), out);
  });
}
int smx_cqt_filter_lengths(const smx_cqt_config *c, double *out) {
  return guarded([&] {
    if (!c || !out) throw Failure("filter_lengths: null argument");
    std::copy(c->lengths.begin(), c->lengths.end(), out);
  });
}
int smx_cqt_frames(const smx_cqt_config *c, int64_t n, int64_t *frames) {
  return guarded([&] {
    if (!c || !frames) throw Failure("frames: null argument");
    *frames = c->frames(n);
  });
}
int smx_cqt_config_octave(const smx_cqt_config *c, int64_t i, int64_t *first, int64_t *count, int64_t *n_fft, int64_t *hop,
                          int64_t *halvings) {
  return guarded([&] {
    if (!c || i < 0 || i >= (int64_t)c->octaves.size()) throw Failure("octave: no such octave");
    const smx_cqt_config::Octave &o = c->octaves[(size_t)i];
    if (first) *first = o.first;
    if (count) *count = o.count;
    if (n_fft) *n_fft = o.n_fft;
    if (hop) *hop = o.hop;
    if (halvings) *halvings = o.halvings;
  });
}
int smx_cqt_config_taps(const smx_cqt_config *c, int64_t i, double *out) {
  return guarded([&] {
    if (!c || !out || i < 0 || i >= (int64_t)c->octaves.size()) throw Failure("taps: no such octave");
    const std::vector<double> &taps = c->octaves[(size_t)i].taps;
    std::copy(taps.begin(), taps.end(), out);
  });
}
int smx_cqt_config_divisors(const smx_cqt_config *c, double *out) {
  return guarded([&] {
    if (!c || !out) throw Failure("divisors: null argument");
    std::copy(c->divisors.begin(), c->divisors.end(), out);
  });
}

int smx_cqt_transform_f32(const smx_cqt_config *c, const float *x, int64_t lead, int64_t n, float *out_c64) {
  return guarded([&] { cqt_host(c, "transform", x, lead, n, OUT_COMPLEX, 2.0, out_c64); });
}
int smx_cqt_transform_f32_dev(const smx_cqt_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, float *d_out_c64,
                              void *stream) {
  return guarded([&] {
    check_cqt(c, "transform", lead, n);
    cqt_dev(*c, "transform", d_x, lead, n, x_stride, OUT_COMPLEX, 2.0, d_out_c64, (hipStream_t)stream);
  });
}
int smx_cqt_power_spectrum_f32(const smx_cqt_config *c, const float *x, int64_t lead, int64_t n, double power, float *out) {
  return guarded([&] { cqt_host(c, "power_spectrum", x, lead, n, OUT_POWER, power, out); });
}
int smx_cqt_power_spectrum_f32_dev(const smx_cqt_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, double power,
                                   float *d_out, void *stream) {
  return guarded([&] {
    check_cqt(c, "power_spectrum", lead, n);
    cqt_dev(*c, "power_spectrum", d_x, lead, n, x_stride, OUT_POWER, power, d_out, (hipStream_t)stream);
  });
}

int smx_debug_cqt_project_f32_dev(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, const double *d_taps,
                                  const double *d_divisors, int64_t count, int64_t n_fft, int64_t hop, int pad, double pad_value,
                                  int64_t first, int64_t n_bins, int64_t frames, int as_power, double power, void *d_out,
                                  void *stream) {
  return guarded([&] {
    if (lead < 0 || count < 0 || frames < 0) throw Failure("cqt_project: negative extent");
    if (lead == 0 || count == 0 || frames == 0) return;
    if (!d_x || !d_taps || !d_out) throw Failure("cqt_project: null device pointer");
    if (x_stride < n) throw Failure("cqt_project: x_stride is smaller than the signal length");
    if (pad < SMX_PAD_REFLECT || pad > SMX_PAD_EDGE) throw Failure("cqt_project: unknown pad mode");
    CqtProjectJob job;
    job.x = d_x; job.lead = lead; job.n = n; job.x_stride = x_stride;
    job.taps = d_taps; job.divisors = d_divisors;
    job.count = count; job.n_fft = n_fft; job.hop = hop;
    job.pad = pad; job.pad_value = pad_value;
    job.first = first; job.n_bins = n_bins; job.frames = frames;
    job.mode = as_power ? OUT_POWER : OUT_COMPLEX; job.power = power; job.out = d_out; job.stream = (hipStream_t)stream;
    launch_cqt_project(job);
  });
}

int smx_chroma_cqt_projection(const smx_cqt_config *c, int64_t n_chroma, double *out) {
  return guarded([&] {
    if (!c || !out) throw Failure("cqt_projection: null argument");
    const std::vector<double> w = cqt_fold_matrix("cqt_projection", *c, n_chroma);
    std::copy(w.begin(), w.end(), out);
  });
}
int smx_chroma_of_cqt_f32(const smx_cqt_config *c, const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                          int norm, double norm_p, float *out) {
  return guarded([&] { of_cqt_host(c, s, 4, lead, bins, frames, n_chroma, norm, norm_p, out); });
}
int smx_chroma_of_cqt_f64(const smx_cqt_config *c, const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                          int norm, double norm_p, double *out) {
  return guarded([&] { of_cqt_host(c, s, 8, lead, bins, frames, n_chroma, norm, norm_p, out); });
}
int smx_chroma_of_cqt_f32_dev(const smx_cqt_config *c, const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                              int norm, double norm_p, float *d_out, void *stream) {
  return guarded([&] {
    if (!c) throw Failure("of_cqt: configuration handle is null");
    of_cqt_dev(*c, d_s, 4, lead, bins, frames, n_chroma, norm, norm_p, d_out, (hipStream_t)stream);
  });
}
int smx_chroma_cqt_f32(const smx_cqt_config *c, const float *x, int64_t lead, int64_t n, int64_t n_chroma, int norm, double norm_p,
                       float *out) {
  return guarded([&] {
    check_cqt(c, "chroma_cqt", lead, n);
    check_chroma_norm("of_cqt", norm, norm_p);
    (void)cqt_fold_matrix("of_cqt", *c, n_chroma);
    const int64_t count = c->frames(n);
    if (lead == 0 || count == 0) return;
    if (!x || !out) throw Failure("chroma_cqt: null pointer");
    host_call("chroma_cqt", {{x, (size_t)n * sizeof(float)}}, out, (size_t)n_chroma * (size_t)count * sizeof(float), lead, false, nullptr,
              [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
                chroma_cqt_dev(*c, reinterpret_cast<const float *>(d_in[0]), nc, n, n, n_chroma, norm, norm_p,
                               reinterpret_cast<float *>(d_out), stream);
              });
  });
}
int smx_chroma_cqt_f32_dev(const smx_cqt_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t n_chroma,
                           int norm, double norm_p, float *d_out, void *stream) {
  return guarded([&] {
    check_cqt(c, "chroma_cqt", lead, n);
    if (x_stride < n) throw Failure("chroma_cqt: x_stride is smaller than the signal length");
    chroma_cqt_dev(*c, d_x, lead, n, x_stride, n_chroma, norm, norm_p, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
