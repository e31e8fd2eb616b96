// Cqt.Kernel (cqt.ml:694-1012, cqt.mli:317-413): the streaming constant-Q transform, one state for all channels.
//
// The state joins what exists: one streaming 2:1 decimator (smx_resample_stream_*, resample_direct.hip) per early decimation
// and per halving octave, the plan and its latency (cqt_plan.cpp), and the projection arithmetic of cqt.hip (cqt_project.hpp).
// Per octave it keeps a device ring of the octave's UNSCALED float32 stream u_i, the host counters seen_i (samples of u_i so
// far) and produced_i (frames projected), and all octaves write finished columns -- scaled, divided, rounded -- into one
// column ring [channels; n_bins; cap], from which the columns every octave has produced leave by a copy.
//
//   cqt_stream_append_kernel    the step's new samples of every octave into the octaves' rings: ONE launch
//   cqt_stream_project_kernel   every frame that became ready, of every octave: ONE launch over a small job table.  A
//                               workgroup's 128 frame slots are filled with (channel, frame) pairs of one octave across channels
//                               (256 channels and one ready frame fill two tiles), bin tiles as in cqt_project_kernel.  Each
//                               slot stages its own 32 samples per tap tile; the taps, the fma chain per (frame, bin) and the
//                               epilogue are cqt_project.hpp's, so a column has the bits Cqt.transform gives it.
//   cqt_stream_emit_kernel      columns [emitted, min_i produced_i) out of the ring: ONE launch
//
// A frame of octave i is projected in the step that brings seen_i to its last sample (cqt_plan.cpp: cqt_octave_ready); the
// boundary rule is fetch_sample_of on the frame's logical positions with n = seen_i, mapped into the ring.  Before the flush
// that n is not final, and need not be: a ready frame reads nothing at or past seen_i, and what it reads before sample 0 does
// not depend on n once seen_i > n_fft / 2 (the Reflect rule of cqt_octave_ready).  All counters are host integers and nothing
// here synchronises: a step on device chunks is enqueued on the caller's stream.
#include "cqt_project.hpp"

struct smx_cqt_kernel {
  struct Octave {
    int64_t level = 0;       // u_i = decimate^level(x): early + halvings
    int64_t cap = 0;         // ring capacity, a power of two: sample s of u_i lives at s & (cap - 1)
    int64_t seen = 0, produced = 0;
    float *history = nullptr;   // [channels][cap]
    double gain = 1.0, pad_value = 0.0;
  };
  const smx_cqt_config *config = nullptr;   // borrowed: outlives the kernel
  int64_t channels = 0, max_block = 0, fed = 0, emitted = 0, ring_cap = 0;
  smx::OutMode mode = smx::OUT_COMPLEX;
  double power = 2.0;
  bool drained = false;
  int device = 0;
  std::vector<smx_resample_stream *> stages;   // stage j: level j -> level j + 1
  std::vector<float *> fresh;                  // fresh[j], j >= 1: what stage j - 1 emitted this step, [channels][fresh_cap[j]]
  std::vector<int64_t> fresh_cap;              // most samples level j gains in one step or flush
  std::vector<Octave> octaves;
  void *ring = nullptr;                        // [channels; n_bins; ring_cap] complex64, or float32 under a power
  ~smx_cqt_kernel() {
    for (smx_resample_stream *s : stages) smx_resample_stream_destroy(s);
    for (float *p : fresh) if (p) (void)hipFree(p);
    for (Octave &o : octaves) if (o.history) (void)hipFree(o.history);
    if (ring) (void)hipFree(ring);
  }
};

namespace smx {
namespace {

constexpr int kMaxOctaves = 16;   // the job tables travel as kernel arguments

struct AppendJob {
  const float *src;
  int64_t src_stride;
  float *history;
  int64_t cap, seen, count;
};
struct AppendArgs {
  AppendJob jobs[kMaxOctaves];
  int64_t xtiles;
};

__global__ void __launch_bounds__(256) cqt_stream_append_kernel(AppendArgs a) {
  const AppendJob &job = a.jobs[blockIdx.y];
  const int64_t ch = blockIdx.x / a.xtiles, i = (blockIdx.x % a.xtiles) * 256 + threadIdx.x;
  if (i < job.count) job.history[ch * job.cap + ((job.seen + i) & (job.cap - 1))] = job.src[ch * job.src_stride + i];
}

struct StreamJob {
  const double2 *taps;
  const double *divisors;
  const float *history;
  int64_t cap, seen, n_fft, hop, frame0;   // frames frame0 .. frame0 + nframes - 1 of the signal u_i[0, seen)
  double gain, pad_value;
  int count, first, nframes, ftiles, tile0;   // tiles tile0 .. of the launch are this octave's, frame tiles fastest
};
struct StreamArgs {
  StreamJob jobs[kMaxOctaves];
  int njobs, channels, pad, mode;
  double power;
  int64_t n_bins, ring_cap;
  void *ring;
};

// the octave's stream as fetch_sample_of indexes it: sample s at s modulo the ring's capacity
struct RingView {
  const float *base;
  int64_t mask;
  __device__ float operator[](int64_t s) const { return base[s & mask]; }
};

__global__ void __launch_bounds__(256) cqt_stream_project_kernel(StreamArgs a) {
  __shared__ double2 s_taps[kCqtTapTile * kCqtBinTile];   // [tap][bin]
  __shared__ double s_x[kCqtFrameTile * kCqtRowPad];
  __shared__ int64_t s_origin[kCqtFrameTile];             // position in u_i of tap 0 of the slot's frame
  __shared__ int s_channel[kCqtFrameTile], s_frame[kCqtFrameTile];
  const int tid = threadIdx.x;
  int which = 0;
  while (which + 1 < a.njobs && (int)blockIdx.x >= a.jobs[which + 1].tile0) ++which;
  const StreamJob &o = a.jobs[which];
  const int tile = (int)blockIdx.x - o.tile0;
  const int64_t b0 = (int64_t)(tile / o.ftiles) * kCqtBinTile, q0 = (int64_t)(tile % o.ftiles) * kCqtFrameTile;
  const int64_t pairs = (int64_t)a.channels * o.nframes;
  const int nf = (int)(pairs - q0 < kCqtFrameTile ? pairs - q0 : kCqtFrameTile);
  if (tid < nf) {   // slot tid: pair q0 + tid, channels outermost
    const int64_t q = q0 + tid, p = o.frame0 + q % o.nframes;
    s_channel[tid] = (int)(q / o.nframes);
    s_frame[tid] = (int)(p % a.ring_cap);
    s_origin[tid] = p * o.hop - o.n_fft / 2;
  }
  __syncthreads();
  const int bl = tid & 7, fg = tid >> 3;   // this thread: bins b0 + bl, b0 + bl + 8; slots fg + 32 r
  double re[4][2] = {}, im[4][2] = {};
  for (int64_t n0 = 0; n0 < o.n_fft; n0 += kCqtTapTile) {
    const int tn = (int)(o.n_fft - n0 < kCqtTapTile ? o.n_fft - n0 : kCqtTapTile);
    for (int i = tid; i < kCqtTapTile * kCqtBinTile; i += 256) {
      const int b = i / kCqtTapTile, j = i % kCqtTapTile;
      double2 v = make_double2(0.0, 0.0);
      if (b0 + b < o.count && j < tn) v = o.taps[(b0 + b) * o.n_fft + n0 + j];
      s_taps[j * kCqtBinTile + b] = v;
    }
    for (int i = tid; i < nf * kCqtTapTile; i += 256) {
      const int f = i / kCqtTapTile, j = i % kCqtTapTile;
      if (j < tn) {
        const RingView u{o.history + (int64_t)s_channel[f] * o.cap, o.cap - 1};
        s_x[f * kCqtRowPad + j] = fetch_sample_of(u, o.seen, s_origin[f] + n0 + j, a.pad, o.pad_value);
      }
    }
    __syncthreads();
    cqt_tile_fma(s_taps, s_x + fg * kCqtRowPad, kCqtRowPad, tn, bl, re, im);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int f = fg + 32 * r;
    if (f >= nf) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t b = b0 + bl + 8 * h;
      if (b >= o.count) continue;
      const int64_t at = ((int64_t)s_channel[f] * a.n_bins + o.first + b) * a.ring_cap + s_frame[f];
      cqt_finish(re[r][h], im[r][h], o.gain, o.divisors, b, a.mode, a.power, a.ring, at);
    }
  }
}

// columns first .. first + columns - 1 of every row of the ring into out [rows; out_stride]
template <typename T>
__global__ void __launch_bounds__(256) cqt_stream_emit_kernel(const T *ring, int64_t ring_cap, int64_t first, int64_t columns, int64_t rows,
                                                              T *out, int64_t out_stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * columns) return;
  const int64_t row = i / columns, col = i % columns;
  out[row * out_stride + col] = ring[row * ring_cap + (first + col) % ring_cap];
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
int64_t pow2_at_least(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

void check_status(int code) {
  if (code == SMX_OK) return;
  if (code == SMX_INVALID_ARGUMENT) throw InvalidArgument(smx_last_error());
  throw Failure(smx_last_error());
}

void kernel_check(const smx_cqt_kernel *k, const char *op) {
  if (!k || !k->config) throw Failure(format("%s: null kernel", op));
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  if (device != k->device) throw Failure(format("%s: the kernel was prepared on another device", op));
}

int64_t element_bytes(const smx_cqt_kernel &k) { return k.mode == OUT_COMPLEX ? 8 : 4; }

int64_t columns_after(const smx_cqt_kernel &k, int64_t n) {
  if (k.drained || n <= 0 || n > k.max_block) return 0;
  return cqt_columns_ready(*k.config, k.fed + n) - k.emitted;
}
int64_t columns_pending(const smx_cqt_kernel &k) { return k.drained ? 0 : k.config->frames(k.fed) - k.emitted; }

// the new samples of every level (count[j] of them at src[j], rows src_stride[j] apart) into the rings of the octaves at that level
void append(smx_cqt_kernel &k, const std::vector<const float *> &src, const std::vector<int64_t> &src_stride,
            const std::vector<int64_t> &count, hipStream_t stream) {
  AppendArgs a{};
  int64_t jobs = 0, longest = 0;
  for (smx_cqt_kernel::Octave &o : k.octaves) {
    const int64_t got = count[(size_t)o.level];
    if (got <= 0) continue;
    if (got > k.fresh_cap[(size_t)o.level]) throw Failure("cqt_kernel: a step brought more samples than the history was sized for");
    a.jobs[jobs++] = AppendJob{src[(size_t)o.level], src_stride[(size_t)o.level], o.history, o.cap, o.seen, got};
    longest = std::max(longest, got);
    o.seen += got;
  }
  if (jobs == 0) return;
  a.xtiles = ceil_div(longest, 256);
  SMX_LAUNCH(cqt_stream_append_kernel, dim3(grid_x("cqt_kernel", "channels", a.xtiles * k.channels, 256), (unsigned)jobs), dim3(256), 0, stream, a);
  SMX_HIP_CHECK(hipGetLastError());
}

// frames [produced_i, target_i) of every octave into the column ring
void project(smx_cqt_kernel &k, const std::vector<int64_t> &target, hipStream_t stream) {
  const smx_cqt_config &c = *k.config;
  const smx_cqt_config::Tables &tables = c.tables();
  StreamArgs a{};
  int64_t tiles = 0;
  for (size_t i = 0; i < k.octaves.size(); ++i) {
    smx_cqt_kernel::Octave &s = k.octaves[i];
    const smx_cqt_config::Octave &o = c.octaves[i];
    const int64_t nframes = target[i] - s.produced;
    if (nframes <= 0) continue;
    if (target[i] - k.emitted > k.ring_cap) throw Failure("cqt_kernel: an octave ran further ahead than the column ring holds");
    StreamJob &job = a.jobs[a.njobs++];
    const double *taps = tables.octaves[i];
    job.taps = reinterpret_cast<const double2 *>(taps);
    job.divisors = c.scale ? taps + o.count * o.n_fft * 2 : nullptr;
    job.history = s.history;
    job.cap = s.cap; job.seen = s.seen; job.n_fft = o.n_fft; job.hop = o.hop; job.frame0 = s.produced;
    job.gain = s.gain; job.pad_value = s.pad_value;
    const int64_t ftiles = ceil_div(k.channels * nframes, kCqtFrameTile), btiles = ceil_div(o.count, kCqtBinTile);
    grid_x("cqt_kernel", "tiles", tiles + ftiles * btiles, 256);   // (before the int fields below take their share of it)
    job.count = (int)o.count; job.first = (int)o.first; job.nframes = (int)nframes;
    job.ftiles = (int)ftiles; job.tile0 = (int)tiles;
    tiles += ftiles * btiles;
    s.produced = target[i];
  }
  if (a.njobs == 0) return;
  a.channels = (int)k.channels; a.pad = c.pad; a.mode = (int)k.mode; a.power = k.power;
  a.n_bins = c.n_bins; a.ring_cap = k.ring_cap; a.ring = k.ring;
  SMX_LAUNCH(cqt_stream_project_kernel, dim3(grid_x("cqt_kernel", "tiles", tiles, 256)), dim3(256), 0, stream, a);
  SMX_HIP_CHECK(hipGetLastError());
}

// columns [emitted, upto) leave: d_out [channels; n_bins; out_stride]
int64_t emit(smx_cqt_kernel &k, int64_t upto, void *d_out, int64_t out_stride, hipStream_t stream) {
  const int64_t columns = upto - k.emitted;
  if (columns <= 0) return 0;
  const int64_t rows = k.channels * k.config->n_bins;
  const unsigned blocks = grid_x("cqt_kernel", "columns", ceil_div(rows * columns, 256), 256);
  if (k.mode == OUT_COMPLEX)
    SMX_LAUNCH(cqt_stream_emit_kernel<float2>, dim3(blocks), dim3(256), 0, stream, (const float2 *)k.ring, k.ring_cap, k.emitted,
               columns, rows, (float2 *)d_out, out_stride);
  else
    SMX_LAUNCH(cqt_stream_emit_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float *)k.ring, k.ring_cap, k.emitted,
               columns, rows, (float *)d_out, out_stride);
  SMX_HIP_CHECK(hipGetLastError());
  k.emitted = upto;
  return columns;
}

void check_room(int64_t columns, const void *d_out, int64_t out_stride, const char *op) {
  if (columns > 0 && (!d_out || out_stride < columns)) throw Failure(format("%s: null output or stride smaller than the emitted columns", op));
}

int64_t step_dev(smx_cqt_kernel &k, const float *d_x, int64_t n, int64_t x_stride, void *d_out, int64_t out_stride, hipStream_t stream) {
  if (k.drained) throw InvalidArgument("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)");
  if (n < 0) throw Failure("step: negative extent");
  if (n > k.max_block)
    throw InvalidArgument(format("step: cannot feed a %lld-sample chunk (max_block is %lld)", (long long)n, (long long)k.max_block));
  if (n == 0) return 0;
  if (!d_x || x_stride < n) throw Failure("step: null chunk or stride smaller than the chunk");
  check_room(columns_after(k, n), d_out, out_stride, "step");
  const size_t levels = k.stages.size() + 1;
  std::vector<const float *> src(levels, nullptr);
  std::vector<int64_t> stride(levels, 0), count(levels, 0);
  src[0] = d_x; stride[0] = x_stride; count[0] = n;
  for (size_t j = 0; j + 1 < levels && count[j] > 0; ++j) {   // the chain, front to back
    src[j + 1] = k.fresh[j + 1]; stride[j + 1] = k.fresh_cap[j + 1];
    check_status(smx_resample_stream_step_f32_dev(k.stages[j], src[j], count[j], stride[j], k.fresh[j + 1], k.fresh_cap[j + 1],
                                                  &count[j + 1], stream));
  }
  append(k, src, stride, count, stream);
  k.fed += n;
  std::vector<int64_t> target(k.octaves.size());
  int64_t least = INT64_MAX;
  for (size_t i = 0; i < k.octaves.size(); ++i) {
    target[i] = cqt_octave_ready(*k.config, k.config->octaves[i], k.octaves[i].seen);
    least = std::min(least, target[i]);
  }
  project(k, target, stream);
  return emit(k, least, d_out, out_stride, stream);
}

int64_t flush_dev(smx_cqt_kernel &k, void *d_out, int64_t out_stride, hipStream_t stream) {
  if (k.drained) return 0;   // a second flush has nothing (cqt.mli:402-409)
  const smx_cqt_config &c = *k.config;
  const int64_t total = c.frames(k.fed);
  check_room(total - k.emitted, d_out, out_stride, "flush");
  k.drained = true;
  const size_t levels = k.stages.size() + 1;
  std::vector<const float *> src(levels, nullptr);
  std::vector<int64_t> stride(levels, 0), count(levels, 0);
  for (size_t j = 0; j + 1 < levels; ++j) {   // drain the chain front to back (cqt.ml:958-999): what level j gained, then stage j's own tail
    src[j + 1] = k.fresh[j + 1]; stride[j + 1] = k.fresh_cap[j + 1];
    int64_t head = 0, tail = 0;
    if (count[j] > 0)
      check_status(smx_resample_stream_step_f32_dev(k.stages[j], src[j], count[j], stride[j], k.fresh[j + 1], k.fresh_cap[j + 1], &head, stream));
    if (head + smx_resample_stream_pending(k.stages[j]) > k.fresh_cap[j + 1])
      throw Failure("flush: a decimator's tail is longer than the history was sized for");
    check_status(smx_resample_stream_flush_f32_dev(k.stages[j], k.fresh[j + 1] + head, k.fresh_cap[j + 1], &tail, stream));
    count[j + 1] = head + tail;
  }
  append(k, src, stride, count, stream);
  std::vector<int64_t> target(k.octaves.size(), total);   // every octave has at least `total` frames: frames is their minimum
  for (size_t i = 0; i < k.octaves.size(); ++i) {
    const int64_t d = int64_t(1) << k.octaves[i].level;
    if (k.octaves[i].seen != ceil_div(k.fed, d)) throw Failure("flush: an octave's stream did not drain to its length");
    target[i] = std::max(total, k.octaves[i].produced);
  }
  project(k, target, stream);
  return emit(k, total, d_out, out_stride, stream);
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_cqt_config_columns_ready(const smx_cqt_config *c, int64_t fed, int64_t *columns) {
  return guarded([&] {
    if (!c || !columns) throw Failure("columns_ready: null argument");
    if (fed < 0) throw Failure("columns_ready: negative sample count");
    *columns = cqt_columns_ready(*c, fed);
  });
}
int smx_cqt_config_column_bound(const smx_cqt_config *c, int64_t max_block, int64_t *bound) {
  return guarded([&] {
    if (!c || !bound) throw Failure("column_bound: null argument");
    if (max_block < 1) throw Failure("column_bound: max_block must be at least 1");
    *bound = cqt_column_bound(*c, max_block);
  });
}
int smx_cqt_config_run_ahead(const smx_cqt_config *c, int64_t *columns) {
  return guarded([&] {
    if (!c || !columns) throw Failure("run_ahead: null argument");
    *columns = cqt_run_ahead(*c);
  });
}

int smx_cqt_kernel_prepare(const smx_cqt_config *c, int64_t channels, int64_t max_block, int has_power, double power, smx_cqt_kernel **out) {
  return guarded([&] {
    if (!out) throw Failure("prepare: null output handle");
    if (!c) throw Failure("prepare: configuration handle is null");
    if (channels < 1)
      throw InvalidArgument(format("prepare: cannot analyse %lld channels (channels must be at least 1)", (long long)channels));
    if (max_block < 1)
      throw InvalidArgument(format("prepare: cannot accept blocks of %lld samples (max_block must be at least 1)", (long long)max_block));
    // Cqt.transform halves through smx_resample_apply_f32_dev, which runs the direct executor for this plan; the streaming
    // decimator below is that executor's.  Another executor would not give the same bits.
    if (smx_resample_config_executor(c->half) != SMX_RESAMPLE_DIRECT)
      throw Failure("prepare: the 2:1 plan does not run on the direct executor, so its streaming face would not equal Cqt.transform");
    if ((int64_t)c->octaves.size() > kMaxOctaves)
      throw Failure(format("prepare: this path streams plans of up to %d octaves (the plan has %lld)", kMaxOctaves, (long long)c->octaves.size()));
    require_device();
    auto k = std::make_unique<smx_cqt_kernel>();
    k->config = c;
    k->channels = channels;
    k->max_block = max_block;
    k->mode = has_power ? OUT_POWER : OUT_COMPLEX;
    k->power = power;
    SMX_HIP_CHECK(hipGetDevice(&k->device));
    const int64_t lag = smx_resample_config_latency(c->half);
    const int64_t stages = c->early + c->octaves.back().halvings;
    // what level j gains at most: in a step, the decimator's out_bound of the level above; at the flush, half of what the level
    // above gains plus the decimator's own tail of at most (lag + 1) / 2 + 1
    k->fresh_cap.assign((size_t)stages + 1, max_block);
    k->fresh.assign((size_t)stages + 1, nullptr);
    int64_t in_step = max_block, at_flush = 0;
    for (int64_t j = 0; j < stages; ++j) {
      smx_resample_stream *s = nullptr;
      check_status(smx_resample_stream_prepare(c->half, channels, k->fresh_cap[(size_t)j], &s));
      k->stages.push_back(s);
      in_step = ceil_div(in_step, 2) + 1;
      at_flush = (at_flush + lag + 1) / 2 + 2;
      k->fresh_cap[(size_t)j + 1] = std::max(in_step, at_flush);
      SMX_HIP_CHECK(hipMalloc((void **)&k->fresh[(size_t)j + 1], (size_t)channels * (size_t)k->fresh_cap[(size_t)j + 1] * sizeof(float)));
    }
    double gain = 1.0;   // as cqt_dev folds it (cqt.ml:630-640, 650)
    if (c->early > 0) {
      const double factor = std::sqrt((double)(int64_t(1) << c->early));
      gain = factor;
      if (!c->scale) gain *= factor;
    }
    const int64_t last = (int64_t)c->octaves.size() - 1;
    for (int64_t i = 0; i <= last; ++i) {
      const smx_cqt_config::Octave &o = c->octaves[(size_t)i];
      smx_cqt_kernel::Octave s;
      s.level = c->early + o.halvings;
      s.gain = gain;
      s.pad_value = c->pad_value / gain;   // the reference pads the scaled signal
      // the oldest frame not yet projected starts less than n_fft samples before seen_i (one more under Reflect), and the right
      // boundary rule reads no further back; then one step's burst
      s.cap = pow2_at_least(o.n_fft + 2 + k->fresh_cap[(size_t)s.level]);
      k->octaves.push_back(s);
      SMX_HIP_CHECK(hipMalloc((void **)&k->octaves.back().history, (size_t)channels * (size_t)s.cap * sizeof(float)));
      if (i < last && o.hop % 2 == 0) gain /= std::sqrt(0.5);
    }
    k->ring_cap = cqt_run_ahead(*c) + cqt_column_bound(*c, max_block);
    SMX_HIP_CHECK(hipMalloc(&k->ring, (size_t)channels * (size_t)c->n_bins * (size_t)k->ring_cap * (size_t)element_bytes(*k)));
    (void)c->tables();
    *out = k.release();
  });
}
void smx_cqt_kernel_destroy(smx_cqt_kernel *k) { delete k; }
int smx_cqt_kernel_reset(smx_cqt_kernel *k) {
  return guarded([&] {
    kernel_check(k, "reset");
    SMX_HIP_CHECK(hipDeviceSynchronize());   // steps on other streams may still read the rings
    for (smx_resample_stream *s : k->stages) check_status(smx_resample_stream_reset(s));
    for (smx_cqt_kernel::Octave &o : k->octaves) o.seen = o.produced = 0;
    k->fed = k->emitted = 0;
    k->drained = false;
  });
}
int64_t smx_cqt_kernel_columns_after(const smx_cqt_kernel *k, int64_t n) { return k && k->config ? columns_after(*k, n) : -1; }
int64_t smx_cqt_kernel_pending(const smx_cqt_kernel *k) { return k && k->config ? columns_pending(*k) : -1; }

int smx_cqt_kernel_step_f32_dev(smx_cqt_kernel *k, const float *d_x, int64_t n, int64_t x_stride, void *d_out, int64_t out_stride,
                                int64_t *columns, void *stream) {
  return guarded([&] {
    kernel_check(k, "step");
    const int64_t got = step_dev(*k, d_x, n, x_stride, d_out, out_stride, (hipStream_t)stream);
    if (columns) *columns = got;
  });
}
int smx_cqt_kernel_flush_f32_dev(smx_cqt_kernel *k, void *d_out, int64_t out_stride, int64_t *columns, void *stream) {
  return guarded([&] {
    kernel_check(k, "flush");
    const int64_t got = flush_dev(*k, d_out, out_stride, (hipStream_t)stream);
    if (columns) *columns = got;
  });
}

// the host forms of step and flush are not batch calls (strided rows, a column count known only after the run): no host_call
int smx_cqt_kernel_step_f32(smx_cqt_kernel *k, const float *x, int64_t n, int64_t x_stride, void *out, int64_t out_stride, int64_t *columns) {
  return guarded([&] {
    kernel_check(k, "step");
    if (columns) *columns = 0;
    if (n <= 0 || n > k->max_block || k->drained) {   // the checks and their messages live in one place
      (void)step_dev(*k, nullptr, n, x_stride, nullptr, 0, nullptr);
      return;
    }
    if (!x || x_stride < n) throw Failure("step: null chunk or stride smaller than the chunk");
    const int64_t expect = columns_after(*k, n), rows = k->channels * k->config->n_bins, bytes = element_bytes(*k);
    check_room(expect, out, out_stride, "step");
    DeviceScratch d_x((size_t)k->channels * (size_t)n * sizeof(float)), d_out((size_t)rows * (size_t)std::max<int64_t>(expect, 1) * (size_t)bytes);
    SMX_HIP_CHECK(hipMemcpy2D(d_x.ptr, (size_t)n * sizeof(float), x, (size_t)x_stride * sizeof(float), (size_t)n * sizeof(float),
                              (size_t)k->channels, hipMemcpyHostToDevice));
    const int64_t got = step_dev(*k, d_x.as<float>(), n, n, d_out.ptr, expect, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (got > 0)
      SMX_HIP_CHECK(hipMemcpy2D(out, (size_t)(out_stride * bytes), d_out.ptr, (size_t)(expect * bytes), (size_t)(got * bytes), (size_t)rows,
                                hipMemcpyDeviceToHost));
    if (columns) *columns = got;
  });
}
int smx_cqt_kernel_flush_f32(smx_cqt_kernel *k, void *out, int64_t out_stride, int64_t *columns) {
  return guarded([&] {
    kernel_check(k, "flush");
    if (columns) *columns = 0;
    const int64_t expect = columns_pending(*k), rows = k->channels * k->config->n_bins, bytes = element_bytes(*k);
    check_room(expect, out, out_stride, "flush");
    DeviceScratch d_out((size_t)rows * (size_t)std::max<int64_t>(expect, 1) * (size_t)bytes);
    const int64_t got = flush_dev(*k, d_out.ptr, expect, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (got > 0)
      SMX_HIP_CHECK(hipMemcpy2D(out, (size_t)(out_stride * bytes), d_out.ptr, (size_t)(expect * bytes), (size_t)(got * bytes), (size_t)rows,
                                hipMemcpyDeviceToHost));
    if (columns) *columns = got;
  });
}

}  // extern "C"
