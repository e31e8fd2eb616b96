// Stft.Kernel and Stft.Synthesis: the streaming analysis and synthesis state machines and their extern "C" entry points.
// The state lives in device memory; every step runs the offline kernels (launch_stft, launch_istft) over [carry ++ chunk].
#include "smx_internal.hpp"

using namespace smx;

// ---- Stft.Synthesis (stft.ml:1029-1298): incremental least-squares synthesis ---------------------------------------------
// The reference keeps the last blocks - 1 WINDOWED frames; here the state is the last blocks - 1 SPECTRA (device,
// [channels; bins; blocks - 1], frames fastest) and a step runs the offline synthesis kernels over [history ++ new frames]
// with the envelope of the whole stream (IstftJob::env_q0 / env_open): a frame is inverted by the code that inverts it
// offline and a position sums its taps in the offline order, so any chunking of a stream totals Stft.invert bit for bit
// (the reference's law, soundml/test/istft/istft_law.ml) at the price of re-inverting blocks - 1 frames per step.
// The held quotients (`carry`, stft.ml:1063) and the head-trim counter are as in the reference; absent frames before the
// stream are zero spectra, whose frames are the exact zeros the reference's overlap-add pads with.
struct smx_stft_synthesis {
  const smx_stft_config *cfg = nullptr;
  int z_bytes = 8;                     // 8 = complex64 in / float32 out, 16 = complex128 / float64
  int64_t channels = 0, max_block = 0;
  int64_t left = 0, hold = 0, blocks = 0;
  int64_t fed = 0, drop = 0;
  bool drained = false;
  void *d_hist = nullptr;              // [channels; bins; blocks - 1] complex
  void *d_local = nullptr;             // [channels; bins; blocks - 1 + cap] complex
  void *d_quot = nullptr;              // [channels; cap * hop] real
  void *d_carry = nullptr;             // [channels; hold] real (valid when carry_len == hold)
  void *d_stage = nullptr;             // host-pointer steps: the chunk and the released samples
  int64_t cap = 0, carry_len = 0, stage_bytes = 0;
  hipStream_t last_stream = nullptr;   // the stream of the latest step / flush: reset orders its memset behind it
  int64_t elem() const { return z_bytes / 2; }
  ~smx_stft_synthesis() {
    (void)hipFree(d_hist); (void)hipFree(d_local); (void)hipFree(d_quot); (void)hipFree(d_carry); (void)hipFree(d_stage);
  }
};

// =============================== Stft.Kernel ==================================
// Streaming analysis (stft.ml:366-622).  The state machine is the reference's:
// a prelude until the left extension is computable, the pending padded suffix,
// the last right+1 raw samples, and `skip` when hop > fft.  The carry (pending
// suffix, tail) lives in DEVICE memory; each step uploads only the new chunk and
// runs the same analysis kernels over [pending ++ extension ++ chunk].
struct smx_stft_kernel {
  const smx_stft_config *cfg = nullptr;
  int dtype_bytes = 4;
  int64_t channels = 0, max_block = 0;
  int64_t left = 0, right = 0;
  bool started = false, drained = false;
  int64_t received = 0;
  int64_t skip = 0;
  // the small carried pieces live on the device too (prelude and tail are at most left + 1 / right + 1 samples per
  // channel), so a step on a device-resident chunk moves nothing over the host link
  void *d_prelude = nullptr;            // [channels][prelude_cap], prelude_len valid
  int64_t prelude_len = 0, prelude_cap = 0;
  void *d_tail = nullptr;               // [channels][right + 1], tail_len valid
  int64_t tail_len = 0;
  void *d_stream = nullptr;             // device [channels][cap]: pending ++ new padded samples
  int64_t cap = 0;
  int64_t pending_len = 0;
  void *d_out = nullptr;
  int64_t out_cap = 0;                  // frames
  // what a step emits: the complex spectrum (Stft.Kernel / Stft.stage) or |.|^power of it in the chunk's dtype
  // (Stft.power_stage, stft.ml:1364-1409)
  OutMode mode = OUT_COMPLEX;
  double power = 2.0;
  int64_t values() const { return mode == OUT_COMPLEX ? 2 : 1; }   // scalars per emitted element
  ~smx_stft_kernel() {
    (void)hipFree(d_stream);
    (void)hipFree(d_out);
    (void)hipFree(d_prelude);
    (void)hipFree(d_tail);
  }
};

namespace smx {
namespace {

int64_t frame_bound(const smx_stft_config &c, int64_t max_block) {  // stft.ml:1316-1317 + :1307-1308
  int64_t lat = c.alignment == SMX_ALIGN_CENTERED ? c.fft_size / 2 : 0;
  if (c.pad == SMX_PAD_REFLECT && c.left_width() > lat) lat = c.left_width();
  return (max_block + lat + c.hop - 1) / c.hop + 1;
}

// (the copy into the grown buffer runs on the caller's stream, behind the previous step's asynchronous move of the pending
// suffix; the old buffer is released only once that copy has run)
void ensure_stream(smx_stft_kernel &k, int64_t need, hipStream_t stream) {
  if (need <= k.cap) return;
  int64_t cap = k.cap ? k.cap : 1024;
  while (cap < need) cap *= 2;
  void *fresh = nullptr;
  const size_t es = (size_t)k.dtype_bytes;
  SMX_HIP_CHECK(hipMalloc(&fresh, (size_t)k.channels * (size_t)cap * es));
  if (k.d_stream && k.pending_len > 0)
    SMX_HIP_CHECK(hipMemcpy2DAsync(fresh, (size_t)cap * es, k.d_stream, (size_t)k.cap * es,
                                   (size_t)k.pending_len * es, (size_t)k.channels, hipMemcpyDeviceToDevice, stream));
  SMX_HIP_CHECK(hipStreamSynchronize(stream));
  (void)hipFree(k.d_stream);
  k.d_stream = fresh;
  k.cap = cap;
}

// One row-wise copy between device arrays: len elements per channel from src[ch][src_off ..] to dst[ch][dst_off ..]
// (strides in elements).  Ranges of one array may not overlap.
void rows_copy(void *dst, int64_t dst_stride, int64_t dst_off, const void *src, int64_t src_stride, int64_t src_off, int64_t len,
               int64_t channels, size_t es, hipStream_t stream) {
  if (len <= 0 || channels <= 0) return;
  SMX_HIP_CHECK(hipMemcpy2DAsync(reinterpret_cast<unsigned char *>(dst) + (size_t)dst_off * es, (size_t)dst_stride * es,
                                 reinterpret_cast<const unsigned char *>(src) + (size_t)src_off * es, (size_t)src_stride * es,
                                 (size_t)len * es, (size_t)channels, hipMemcpyDeviceToDevice, stream));
}

// The three border gathers of the state machine, on the device (kind 0: the left extension at install, stft.ml:457-471
// `left_pad`: reflect reads x[left - j], edge x[0]; kind 1: `pad_signal` of a stream that never reached the install
// threshold, stft.ml:318-338; kind 2: the right extension at the drain, stft.ml:506-519 `right_pad`: reflect reads
// tail[len - 2 - i], edge tail[len - 1]); constant padding writes the value.
template <typename T>
__global__ void __launch_bounds__(256) stream_pad_kernel(T *dst, int64_t dst_stride, int64_t count, const T *src, int64_t src_stride,
                                                         int64_t src_len, int kind, int pad, T value, int64_t left) {
  const int64_t ch = blockIdx.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += (int64_t)gridDim.x * 256) {
    int64_t idx = -1;
    if (pad != SMX_PAD_CONSTANT) {
      if (kind == 0) idx = pad == SMX_PAD_REFLECT ? left - j : 0;
      else if (kind == 2) idx = pad == SMX_PAD_REFLECT ? src_len - 2 - j : src_len - 1;
      else {
        const int64_t q = j - left;
        if (q >= 0 && q < src_len) idx = q;
        else if (pad == SMX_PAD_REFLECT) {
          if (src_len == 1) idx = 0;
          else {
            const int64_t period = 2 * (src_len - 1);
            const int64_t m = ((q % period) + period) % period;
            idx = m < src_len ? m : period - m;
          }
        } else idx = q < 0 ? 0 : src_len - 1;
      }
    } else if (kind == 1) {
      const int64_t q = j - left;
      if (q >= 0 && q < src_len) idx = q;
    }
    dst[ch * dst_stride + j] = idx < 0 ? value : src[ch * src_stride + idx];
  }
}

void stream_pad(smx_stft_kernel &k, void *dst, int64_t dst_stride, int64_t count, const void *src, int64_t src_stride, int64_t src_len,
                int kind, hipStream_t stream) {
  if (count <= 0) return;
  if (k.channels > 65535) throw Failure("step: more than 65535 channels in one stream");
  dim3 grid((unsigned)std::min<int64_t>((count + 255) / 256, 256), (unsigned)k.channels);
  if (k.dtype_bytes == 4)
    SMX_LAUNCH(stream_pad_kernel<float>, grid, dim3(256), 0, stream, reinterpret_cast<float *>(dst), dst_stride, count,
               reinterpret_cast<const float *>(src), src_stride, src_len, kind, k.cfg->pad, (float)k.cfg->pad_value, k.left);
  else
    SMX_LAUNCH(stream_pad_kernel<double>, grid, dim3(256), 0, stream, reinterpret_cast<double *>(dst), dst_stride, count,
               reinterpret_cast<const double *>(src), src_stride, src_len, kind, k.cfg->pad, (double)k.cfg->pad_value, k.left);
  SMX_HIP_CHECK(hipGetLastError());
}

// where a call's frames go: the caller's window [channels; bins; capacity], in host or device memory
struct StreamOut {
  void *ptr;
  int64_t capacity;
  bool on_device;
};

// stft.ml:415-442 `process`: append `extra` (device rows, extra_stride apart, from element extra_off) to the pending padded
// stream and emit every frame that became complete.
int64_t process(smx_stft_kernel &k, const void *extra, int64_t extra_stride, int64_t extra_off, int64_t extra_len, const StreamOut &out,
                hipStream_t stream) {
  const smx_stft_config &c = *k.cfg;
  const int64_t fft = c.fft_size, hop = c.hop;
  const size_t es = (size_t)k.dtype_bytes;
  const int64_t total = k.pending_len + extra_len;
  ensure_stream(k, total, stream);
  rows_copy(k.d_stream, k.cap, k.pending_len, extra, extra_stride, extra_off, extra_len, k.channels, es, stream);
  const int64_t count = total < fft ? 0 : 1 + (total - fft) / hop;
  if (count == 0) {
    k.pending_len = total;
    return 0;
  }
  if (count > out.capacity)
    throw Failure(format("step: %lld frames do not fit the caller's %lld-frame output window",
                         (long long)count, (long long)out.capacity));
  const int64_t bins = c.bins();
  if (count > k.out_cap) {
    SMX_HIP_CHECK(hipStreamSynchronize(stream));
    (void)hipFree(k.d_out);
    k.d_out = nullptr;
    int64_t cap = k.out_cap ? k.out_cap : 16;
    while (cap < count) cap *= 2;
    SMX_HIP_CHECK(hipMalloc(&k.d_out, (size_t)k.channels * (size_t)bins * (size_t)cap * 2 * es));   // sized for either face
    k.out_cap = cap;
  }
  StftJob job = stft_job(c, k.d_stream, k.dtype_bytes, k.channels, total, k.cap, 0, count, k.mode, k.power, k.d_out, stream);
  job.left = 0;                 // the stream is already padded
  job.pad = SMX_PAD_CONSTANT;
  job.pad_value = 0.0;
  launch_stft(job);
  // [channels; bins; count] (dense) -> caller's [channels; bins; capacity] window
  const size_t vs = (size_t)k.values() * es;
  if (out.on_device) {
    SMX_HIP_CHECK(hipMemcpy2DAsync(out.ptr, (size_t)out.capacity * vs, k.d_out, (size_t)count * vs, (size_t)count * vs,
                                   (size_t)(k.channels * bins), hipMemcpyDeviceToDevice, stream));
  } else {
    SMX_HIP_CHECK(hipStreamSynchronize(stream));
    SMX_HIP_CHECK(hipMemcpy2D(out.ptr, (size_t)out.capacity * vs, k.d_out, (size_t)count * vs, (size_t)count * vs,
                              (size_t)(k.channels * bins), hipMemcpyDeviceToHost));
  }
  const int64_t next_start = count * hop;
  if (next_start >= total) {
    k.skip += next_start - total;
    k.pending_len = 0;
  } else {
    const int64_t keep = total - next_start;
    // move the suffix to the front (rows are independent; overlapping ranges -> staged copy)
    void *tmp = nullptr;
    SMX_HIP_CHECK(smx::pool_malloc_async(&tmp, (size_t)k.channels * (size_t)keep * es, stream));
    rows_copy(tmp, keep, 0, k.d_stream, k.cap, next_start, keep, k.channels, es, stream);
    rows_copy(k.d_stream, k.cap, 0, tmp, keep, 0, keep, k.channels, es, stream);
    SMX_HIP_CHECK(smx::pool_free_async(tmp, stream));
    k.pending_len = keep;
  }
  return count;
}

int64_t install_threshold(const smx_stft_config &c) {  // stft.ml:447-452
  return c.pad == SMX_PAD_REFLECT ? c.left_width() + 1 : 1;
}

// the last `right + 1` samples of [old tail ++ chunk] (stft.ml:492-502 `update_tail`; stft.ml:480-483 at install)
void update_tail(smx_stft_kernel &k, const void *chunk, int64_t chunk_stride, int64_t m, hipStream_t stream) {
  const size_t es = (size_t)k.dtype_bytes;
  const int64_t keep = k.right + 1;
  if (!k.d_tail) SMX_HIP_CHECK(hipMalloc(&k.d_tail, (size_t)k.channels * (size_t)keep * es));
  if (m >= keep) {
    rows_copy(k.d_tail, keep, 0, chunk, chunk_stride, m - keep, keep, k.channels, es, stream);
    k.tail_len = keep;
    return;
  }
  const int64_t cm = k.tail_len + m, start = cm - keep > 0 ? cm - keep : 0, kept_old = k.tail_len - start;
  if (start > 0 && kept_old > 0) {   // shift the surviving part of the old tail to the front (staged: the ranges overlap)
    void *tmp = nullptr;
    SMX_HIP_CHECK(smx::pool_malloc_async(&tmp, (size_t)k.channels * (size_t)kept_old * es, stream));
    rows_copy(tmp, kept_old, 0, k.d_tail, keep, start, kept_old, k.channels, es, stream);
    rows_copy(k.d_tail, keep, 0, tmp, kept_old, 0, kept_old, k.channels, es, stream);
    SMX_HIP_CHECK(smx::pool_free_async(tmp, stream));
  }
  const int64_t old = kept_old > 0 ? kept_old : 0;
  // (start >= tail_len cannot happen: then m >= keep)
  rows_copy(k.d_tail, keep, old, chunk, chunk_stride, 0, m, k.channels, es, stream);
  k.tail_len = old + m;
}

// stft.ml:476-488 `install`: x = [prelude ++ chunk] (device rows, x_stride apart), n samples
int64_t install(smx_stft_kernel &k, const void *x, int64_t x_stride, int64_t n, const StreamOut &out, hipStream_t stream) {
  const size_t es = (size_t)k.dtype_bytes;
  if (k.right > 0) {
    k.tail_len = 0;
    const int64_t keep = k.right + 1 < n ? k.right + 1 : n;
    if (!k.d_tail) SMX_HIP_CHECK(hipMalloc(&k.d_tail, (size_t)k.channels * (size_t)(k.right + 1) * es));
    rows_copy(k.d_tail, k.right + 1, 0, x, x_stride, n - keep, keep, k.channels, es, stream);
    k.tail_len = keep;
  }
  k.started = true;
  k.prelude_len = 0;
  if (k.left == 0) return process(k, x, x_stride, 0, n, out, stream);
  void *both = nullptr;   // [left extension ++ x]
  const int64_t bl = k.left + n;
  SMX_HIP_CHECK(smx::pool_malloc_async(&both, (size_t)k.channels * (size_t)bl * es, stream));
  stream_pad(k, both, bl, k.left, x, x_stride, n, 0, stream);
  rows_copy(both, bl, k.left, x, x_stride, 0, n, k.channels, es, stream);
  const int64_t emitted = process(k, both, bl, 0, bl, out, stream);
  SMX_HIP_CHECK(smx::pool_free_async(both, stream));
  return emitted;
}

// Kernel.step on a device-resident chunk [channels][m] (rows chunk_stride apart): stft.ml:521-559
int64_t step_core(smx_stft_kernel &k, const void *chunk, int64_t chunk_stride, int64_t m, const StreamOut &out, hipStream_t stream) {
  if (k.drained)
    throw InvalidArgument("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)");
  if (m < 0) throw Failure("step: negative chunk length");
  if (m == 0) return 0;
  if (!chunk) throw Failure("step: null chunk");
  const size_t es = (size_t)k.dtype_bytes;
  k.received += m;
  if (!k.started) {
    const int64_t n = k.prelude_len + m;
    if (k.received >= install_threshold(*k.cfg)) {
      if (k.prelude_len == 0) return install(k, chunk, chunk_stride, m, out, stream);
      void *x = nullptr;
      SMX_HIP_CHECK(smx::pool_malloc_async(&x, (size_t)k.channels * (size_t)n * es, stream));
      rows_copy(x, n, 0, k.d_prelude, k.prelude_cap, 0, k.prelude_len, k.channels, es, stream);
      rows_copy(x, n, k.prelude_len, chunk, chunk_stride, 0, m, k.channels, es, stream);
      const int64_t emitted = install(k, x, n, n, out, stream);
      SMX_HIP_CHECK(smx::pool_free_async(x, stream));
      return emitted;
    }
    if (n > k.prelude_cap) {   // below the install threshold: at most left samples ever wait here
      const int64_t cap = std::max<int64_t>(n, k.left + 1);
      void *fresh = nullptr;
      SMX_HIP_CHECK(hipMalloc(&fresh, (size_t)k.channels * (size_t)cap * es));
      rows_copy(fresh, cap, 0, k.d_prelude, k.prelude_cap, 0, k.prelude_len, k.channels, es, stream);
      SMX_HIP_CHECK(hipStreamSynchronize(stream));
      (void)hipFree(k.d_prelude);
      k.d_prelude = fresh;
      k.prelude_cap = cap;
    }
    rows_copy(k.d_prelude, k.prelude_cap, k.prelude_len, chunk, chunk_stride, 0, m, k.channels, es, stream);
    k.prelude_len = n;
    return 0;
  }
  if (k.right > 0) update_tail(k, chunk, chunk_stride, m, stream);
  if (k.skip >= m) {
    k.skip -= m;
    return 0;
  }
  const int64_t dropped = k.skip;
  k.skip = 0;
  return process(k, chunk, chunk_stride, dropped, m - dropped, out, stream);
}

// Kernel.flush: stft.ml:561-595
int64_t flush_core(smx_stft_kernel &k, const StreamOut &out, hipStream_t stream) {
  if (k.drained) return 0;
  k.drained = true;
  const size_t es = (size_t)k.dtype_bytes;
  int64_t emitted = 0;
  if (!k.started) {
    if (k.received != 0) {   // the whole stream sits in the prelude: pad_signal, stft.ml:318-338
      const int64_t n = k.prelude_len, pl = k.left + n + k.right;
      void *padded = nullptr;
      SMX_HIP_CHECK(smx::pool_malloc_async(&padded, (size_t)k.channels * (size_t)pl * es, stream));
      stream_pad(k, padded, pl, pl, k.d_prelude, k.prelude_cap, n, 1, stream);
      k.started = true;
      k.prelude_len = 0;
      emitted = process(k, padded, pl, 0, pl, out, stream);
      SMX_HIP_CHECK(smx::pool_free_async(padded, stream));
    }
  } else if (k.right > 0) {
    const int64_t r = k.right;
    if (k.skip >= r) {
      k.skip -= r;
    } else {
      void *rp = nullptr;   // stft.ml:506-519 right_pad
      SMX_HIP_CHECK(smx::pool_malloc_async(&rp, (size_t)k.channels * (size_t)r * es, stream));
      stream_pad(k, rp, r, r, k.d_tail, k.right + 1, k.tail_len, 2, stream);
      const int64_t dropped = k.skip;
      k.skip = 0;
      emitted = process(k, rp, r, dropped, r - dropped, out, stream);
      SMX_HIP_CHECK(smx::pool_free_async(rp, stream));
    }
  }
  k.pending_len = 0;
  return emitted;
}

}  // namespace
}  // namespace smx

extern "C" {

int smx_stft_kernel_prepare(const smx_stft_config *c, int dtype_bytes, int64_t channels,
                            int64_t max_block, smx_stft_kernel **out) {
  return guarded([&] {
    check_config(c, "prepare");
    if (channels < 1)  // stft.ml:604-608
      throw InvalidArgument(format(
          "prepare: cannot analyse %lld channels (channels must be at least 1)", (long long)channels));
    if (max_block < 1)  // stft.ml:609-614
      throw InvalidArgument(format(
          "prepare: cannot accept blocks of %lld samples (max_block must be at least 1)",
          (long long)max_block));
    if (dtype_bytes != 4 && dtype_bytes != 8) throw Failure("prepare: dtype_bytes must be 4 or 8");
    if (!out) throw Failure("prepare: null output handle");
    require_device();
    auto k = std::make_unique<smx_stft_kernel>();
    k->cfg = c;
    k->dtype_bytes = dtype_bytes;
    k->channels = channels;
    k->max_block = max_block;
    k->left = c->left_width();
    k->right = c->right_width();
    *out = k.release();
  });
}

int smx_stft_kernel_prepare_power(const smx_stft_config *c, int dtype_bytes, int64_t channels, int64_t max_block,
                                  double power, smx_stft_kernel **out) {
  const int status = smx_stft_kernel_prepare(c, dtype_bytes, channels, max_block, out);
  if (status == SMX_OK) {
    (*out)->mode = OUT_POWER;
    (*out)->power = power;
  }
  return status;
}

int64_t smx_stft_stage_latency(const smx_stft_config *c) {   // max (Config.latency c) (install_threshold c - 1)
  if (!c) return -1;
  int64_t lat = c->alignment == SMX_ALIGN_CENTERED ? c->fft_size / 2 : 0;
  if (c->pad == SMX_PAD_REFLECT && c->left_width() > lat) lat = c->left_width();
  return lat;
}
int64_t smx_stft_frame_bound(const smx_stft_config *c, int64_t max_items) { return c ? frame_bound(*c, max_items) : -1; }

void smx_stft_kernel_destroy(smx_stft_kernel *k) { delete k; }

int smx_stft_kernel_frame_bound(const smx_stft_kernel *k, int64_t *out) {
  return guarded([&] {
    if (!k) throw Failure("frame_bound: null kernel");
    *out = frame_bound(*k->cfg, k->max_block);
  });
}

int smx_stft_kernel_channels(const smx_stft_kernel *k, int64_t *out) {
  return guarded([&] {
    if (!k || !out) throw Failure("channels: null argument");
    *out = k->channels;
  });
}

const smx_stft_config *smx_stft_kernel_config(const smx_stft_kernel *k) { return k ? k->cfg : nullptr; }

int smx_stft_kernel_set_channels(smx_stft_kernel *k, int64_t channels) {
  return guarded([&] {
    if (!k) throw Failure("set_channels: null kernel");
    if (channels < 1)  // stft.ml:604-608
      throw InvalidArgument(format(
          "prepare: cannot analyse %lld channels (channels must be at least 1)", (long long)channels));
    if (channels == k->channels) return;
    if (k->received != 0 || k->started || k->drained)
      throw InvalidArgument(format("step: cannot feed %lld channels to a stream of %lld (the chunks of one stream share their "
                                   "leading shape; reset before changing it)", (long long)channels, (long long)k->channels));
    // nothing carried yet: the device buffers are sized on first use
    SMX_HIP_CHECK(hipFree(k->d_stream));
    SMX_HIP_CHECK(hipFree(k->d_out));
    SMX_HIP_CHECK(hipFree(k->d_prelude));
    SMX_HIP_CHECK(hipFree(k->d_tail));
    k->d_stream = k->d_out = k->d_prelude = k->d_tail = nullptr;
    k->cap = k->out_cap = k->prelude_cap = 0;
    k->channels = channels;
  });
}

int smx_stft_kernel_reset(smx_stft_kernel *k) {  // stft.ml:401-409
  return guarded([&] {
    if (!k) throw Failure("reset: null kernel");
    k->started = k->drained = false;
    k->received = k->skip = 0;
    k->prelude_len = 0;
    k->tail_len = 0;
    k->pending_len = 0;
  });
}

// host chunk [channels; m] -> frames in the caller's host window [channels; bins; capacity]; not a batch call (the window's rows
// are strided and the frame count is known only after the run), so the copies stay here instead of host_call
int smx_stft_kernel_step(smx_stft_kernel *k, const void *chunk, int64_t m, void *out, int64_t capacity,
                         int64_t *emitted) {
  return guarded([&] {  // stft.ml:521-559
    if (!k || !emitted) throw Failure("step: null argument");
    *emitted = 0;
    if (m > 0 && !chunk) throw Failure("step: null chunk");
    if (m <= 0 || k->drained) {   // nothing to move: the core states the error or the empty result
      *emitted = step_core(*k, chunk, m, m, StreamOut{out, capacity, false}, nullptr);
      return;
    }
    DeviceScratch d((size_t)k->channels * (size_t)m * (size_t)k->dtype_bytes);
    copy_to_device(d.ptr, chunk, (size_t)k->channels * (size_t)m * (size_t)k->dtype_bytes);
    *emitted = step_core(*k, d.ptr, m, m, StreamOut{out, capacity, false}, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}

int smx_stft_kernel_flush(smx_stft_kernel *k, void *out, int64_t capacity, int64_t *emitted) {
  return guarded([&] {  // stft.ml:561-595
    if (!k || !emitted) throw Failure("flush: null argument");
    *emitted = 0;
    *emitted = flush_core(*k, StreamOut{out, capacity, false}, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}

// the same on a device-resident chunk (rows x_stride samples apart) and a device-resident window: nothing crosses the host link
int smx_stft_kernel_step_dev(smx_stft_kernel *k, const void *d_chunk, int64_t m, int64_t x_stride, void *d_out, int64_t capacity,
                             int64_t *emitted, void *stream) {
  return guarded([&] {
    if (!k || !emitted) throw Failure("step: null argument");
    *emitted = 0;
    if (m > 0 && x_stride < m) throw Failure("step: stride smaller than the chunk length");
    *emitted = step_core(*k, d_chunk, x_stride, m, StreamOut{d_out, capacity, true}, (hipStream_t)stream);
  });
}

int smx_stft_kernel_flush_dev(smx_stft_kernel *k, void *d_out, int64_t capacity, int64_t *emitted, void *stream) {
  return guarded([&] {
    if (!k || !emitted) throw Failure("flush: null argument");
    *emitted = 0;
    *emitted = flush_core(*k, StreamOut{d_out, capacity, true}, (hipStream_t)stream);
  });
}

}  // extern "C"

// =============================== Stft.Synthesis (stft.ml:1029-1298) ============
namespace smx {
namespace {

void synth_grow(smx_stft_synthesis &s, int64_t k) {
  if (k <= s.cap) return;
  const int64_t cap = std::max<int64_t>(k, std::max<int64_t>(s.max_block, s.blocks));
  const int64_t bins = s.cfg->bins();
  SMX_HIP_CHECK(hipFree(s.d_local));
  SMX_HIP_CHECK(hipFree(s.d_quot));
  s.d_local = s.d_quot = nullptr;
  SMX_HIP_CHECK(hipMalloc(&s.d_local, (size_t)s.channels * (size_t)bins * (size_t)(2 * s.blocks + cap) * (size_t)s.z_bytes));
  SMX_HIP_CHECK(hipMalloc(&s.d_quot, (size_t)s.channels * (size_t)(cap * s.cfg->hop + s.cfg->fft_size) * (size_t)s.elem()));
  s.cap = cap;
}

void synth_clear(smx_stft_synthesis &s, hipStream_t stream) {   // stft.ml:1091-1096 `synthesis_reset`
  s.fed = 0;
  s.drop = s.left;
  s.drained = false;
  s.carry_len = 0;
  if (s.blocks > 1)   // absent frames before the stream: zero spectra
    SMX_HIP_CHECK(hipMemsetAsync(s.d_hist, 0, (size_t)s.channels * (size_t)s.cfg->bins() * (size_t)(s.blocks - 1) * (size_t)s.z_bytes, stream));
}

// quotients of the array's hops [blocks - 1, blocks - 1 + count_out / hop) -> d_quot, released through the carry into d_out
int64_t synth_emit(smx_stft_synthesis &s, int64_t frames_local, int64_t nq, int64_t env_count, bool open_end, int64_t keep, void *d_out,
                   int64_t capacity, hipStream_t stream) {
  const smx_stft_config &c = *s.cfg;
  IstftJob job;
  job.cfg = &c;
  job.z = s.d_local;
  job.z_bytes = s.z_bytes;
  job.interior = s.z_bytes == 16 ? SMX_INTERIOR_F64 : interior();
  job.lead = s.channels;
  job.frames = frames_local;
  job.count = frames_local;
  job.out_len = nq;
  job.out = s.d_quot;
  job.stream = stream;
  job.left = (s.blocks - 1) * c.hop;
  job.env_q0 = (s.fed - (s.blocks - 1)) * c.hop;
  job.env_count = env_count;
  job.env_open = open_end;
  const int64_t total = s.carry_len + nq, release = total - keep;
  const int64_t dropped = std::min<int64_t>(s.drop, release);
  const int64_t emit = release - dropped;
  // checked before anything is launched or the head trim is consumed: a retry with a larger buffer starts from the same state
  if (emit > capacity) throw Failure("synthesis: output capacity below the samples this call releases");
  launch_istft(job);
  s.drop -= dropped;
  void *carry_next = nullptr;
  if (keep > 0) SMX_HIP_CHECK(smx::pool_malloc_async(&carry_next, (size_t)s.channels * (size_t)s.hold * (size_t)s.elem(), stream));
  launch_synthesis_release(s.d_carry, s.carry_len, s.d_quot, nq, s.channels, dropped, release, s.hold > 0 ? s.hold : 1, d_out, capacity,
                           carry_next, (int)s.elem(), stream);
  if (keep > 0) {
    SMX_HIP_CHECK(hipMemcpyAsync(s.d_carry, carry_next, (size_t)s.channels * (size_t)s.hold * (size_t)s.elem(), hipMemcpyDeviceToDevice, stream));
    SMX_HIP_CHECK(smx::pool_free_async(carry_next, stream));
  }
  s.carry_len = keep;
  return emit;
}

int64_t synth_step_dev(smx_stft_synthesis &s, const void *d_z, int64_t bins, int64_t k, void *d_out, int64_t capacity, hipStream_t stream) {
  const smx_stft_config &c = *s.cfg;
  if (s.drained)   // stft.ml:1182-1186
    throw InvalidArgument("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)");
  if (bins != c.bins())   // check_frames "step", stft.ml:753-766
    throw InvalidArgument(format("step: cannot invert %lld frequency bins of a %lld-point transform (the bin axis must hold "
                                 "fft_size / 2 + 1 = %lld values)", (long long)bins, (long long)c.fft_size, (long long)c.bins()));
  if (k < 0) throw Failure("step: negative frame count");
  if (k == 0) return 0;
  if (!d_z || !d_out) throw Failure("step: null device pointer");
  synth_grow(s, k);
  const int64_t b = s.blocks, rows = s.channels * c.bins();
  const size_t zb = (size_t)s.z_bytes, lpitch = (size_t)(b - 1 + k) * zb;
  if (b > 1)
    SMX_HIP_CHECK(hipMemcpy2DAsync(s.d_local, lpitch, s.d_hist, (size_t)(b - 1) * zb, (size_t)(b - 1) * zb, (size_t)rows, hipMemcpyDeviceToDevice, stream));
  SMX_HIP_CHECK(hipMemcpy2DAsync(reinterpret_cast<unsigned char *>(s.d_local) + (size_t)(b - 1) * zb, lpitch, d_z, (size_t)k * zb, (size_t)k * zb,
                                 (size_t)rows, hipMemcpyDeviceToDevice, stream));
  const int64_t emit = synth_emit(s, b - 1 + k, k * c.hop, 2 * b + 2, true, s.hold, d_out, capacity, stream);
  if (b > 1)   // the last blocks - 1 spectra of [history ++ chunk]
    SMX_HIP_CHECK(hipMemcpy2DAsync(s.d_hist, (size_t)(b - 1) * zb, reinterpret_cast<unsigned char *>(s.d_local) + (size_t)k * zb, lpitch,
                                   (size_t)(b - 1) * zb, (size_t)rows, hipMemcpyDeviceToDevice, stream));
  s.fed += k;
  return emit;
}

int64_t synth_flush_dev(smx_stft_synthesis &s, void *d_out, int64_t capacity, hipStream_t stream) {   // stft.ml:1243-1269
  if (s.drained) return 0;
  s.drained = true;
  const smx_stft_config &c = *s.cfg;
  const int64_t b = s.blocks, cut = std::max<int64_t>(0, c.fft_size - c.hop - c.right_width());
  s.carry_len = 0;   // a held tail is a tail the trim discards
  if (s.fed == 0 || cut == 0) return 0;
  if (!d_out) throw Failure("flush: null device pointer");
  synth_grow(s, b);
  const int64_t rows = s.channels * c.bins();
  const size_t zb = (size_t)s.z_bytes, lpitch = (size_t)(2 * (b - 1)) * zb;
  SMX_HIP_CHECK(hipMemsetAsync(s.d_local, 0, lpitch * (size_t)rows, stream));
  SMX_HIP_CHECK(hipMemcpy2DAsync(s.d_local, lpitch, s.d_hist, (size_t)(b - 1) * zb, (size_t)(b - 1) * zb, (size_t)rows, hipMemcpyDeviceToDevice, stream));
  return synth_emit(s, 2 * (b - 1), cut, s.fed, false, 0, d_out, capacity, stream);
}

}  // namespace
}  // namespace smx

extern "C" {

int smx_stft_synthesis_prepare(const smx_stft_config *c, int dtype_bytes, int64_t channels, int64_t max_block, smx_stft_synthesis **out) {
  return guarded([&] {
    check_config(c, "prepare");
    if (channels < 1)   // stft.ml:1278-1283
      throw InvalidArgument(format("prepare: cannot synthesise %lld channels (channels must be at least 1)", (long long)channels));
    if (max_block < 1)  // stft.ml:1284-1289
      throw InvalidArgument(format("prepare: cannot accept blocks of %lld frames (max_block must be at least 1)", (long long)max_block));
    if (!stft_nola(*c))  // check_invertible "prepare", stft.ml:742-749
      throw InvalidArgument(format(
          "prepare: cannot invert a %lld-point window advanced by %lld samples inside a %lld-point frame (the "
          "overlap-added squared window must stay above 1e-10 of its largest value at every position)",
          (long long)c->win_length, (long long)c->hop, (long long)c->fft_size));
    if (dtype_bytes != 4 && dtype_bytes != 8) throw Failure("prepare: dtype_bytes must be 4 or 8");
    if (!out) throw Failure("prepare: null output handle");
    require_device();
    auto s = std::make_unique<smx_stft_synthesis>();
    s->cfg = c;
    s->z_bytes = 2 * dtype_bytes;
    s->channels = channels;
    s->max_block = max_block;
    s->left = c->left_width();
    s->hold = std::max<int64_t>(0, c->hop + c->right_width() - c->fft_size);   // stft.ml:1073
    s->blocks = (c->fft_size + c->hop - 1) / c->hop;
    if (s->blocks > 1)
      SMX_HIP_CHECK(hipMalloc(&s->d_hist, (size_t)channels * (size_t)c->bins() * (size_t)(s->blocks - 1) * (size_t)s->z_bytes));
    if (s->hold > 0) SMX_HIP_CHECK(hipMalloc(&s->d_carry, (size_t)channels * (size_t)s->hold * (size_t)s->elem()));
    synth_clear(*s, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = s.release();
  });
}

void smx_stft_synthesis_destroy(smx_stft_synthesis *s) { delete s; }

int64_t smx_stft_synthesis_latency(const smx_stft_config *c) {   // Config.synthesis_latency, stft.ml:152-153
  return c ? c->left_width() + std::max<int64_t>(0, c->hop + c->right_width() - c->fft_size) : -1;
}

int smx_stft_synthesis_sample_bound(const smx_stft_synthesis *s, int64_t *out) {   // synthesis_stage's out_format, stft.ml:1421-1427
  return guarded([&] {
    if (!s || !out) throw Failure("sample_bound: null argument");
    *out = std::max<int64_t>(s->max_block * s->cfg->hop, s->cfg->fft_size - s->cfg->hop);
  });
}

int smx_stft_synthesis_reset(smx_stft_synthesis *s) {
  return guarded([&] {
    if (!s) throw Failure("reset: null kernel");
    // on the stream the kernel last ran on (a non-blocking side stream is not ordered with the null stream), then drained:
    // the next step may come on any stream
    synth_clear(*s, s->last_stream);
    SMX_HIP_CHECK(hipStreamSynchronize(s->last_stream));
  });
}

int smx_stft_synthesis_step_dev(smx_stft_synthesis *s, const void *d_z, int64_t bins, int64_t k, void *d_out, int64_t capacity,
                                int64_t *emitted, void *stream) {
  return guarded([&] {
    if (!s || !emitted) throw Failure("step: null argument");
    *emitted = 0;
    s->last_stream = (hipStream_t)stream;
    *emitted = synth_step_dev(*s, d_z, bins, k, d_out, capacity, (hipStream_t)stream);
  });
}

int smx_stft_synthesis_flush_dev(smx_stft_synthesis *s, void *d_out, int64_t capacity, int64_t *emitted, void *stream) {
  return guarded([&] {
    if (!s || !emitted) throw Failure("flush: null argument");
    *emitted = 0;
    s->last_stream = (hipStream_t)stream;
    *emitted = synth_flush_dev(*s, d_out, capacity, (hipStream_t)stream);
  });
}

// host chunks: [channels; bins; k] complex in, [channels; capacity] real out (row stride = capacity); not a batch call (the
// sample count is known only after the run), so step and flush keep their own copies instead of host_call
int smx_stft_synthesis_step(smx_stft_synthesis *s, const void *z, int64_t bins, int64_t k, void *out, int64_t capacity, int64_t *emitted) {
  return guarded([&] {
    if (!s || !emitted) throw Failure("step: null argument");
    *emitted = 0;
    if (k > 0 && (!z || !out)) throw Failure("step: null pointer");
    if (k <= 0 || bins != s->cfg->bins() || s->drained) {   // nothing to move: the device entry states the error or the empty result
      *emitted = synth_step_dev(*s, z, bins, k, out, capacity, nullptr);
      return;
    }
    const size_t zb = (size_t)s->channels * (size_t)bins * (size_t)k * (size_t)s->z_bytes;
    const size_t ob = (size_t)s->channels * (size_t)capacity * (size_t)s->elem();
    DeviceScratch dz(zb), dout(ob);
    copy_to_device(dz.ptr, z, zb);
    *emitted = synth_step_dev(*s, dz.ptr, bins, k, dout.ptr, capacity, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (*emitted > 0) copy_to_host(out, dout.ptr, ob);
  });
}

int smx_stft_synthesis_flush(smx_stft_synthesis *s, void *out, int64_t capacity, int64_t *emitted) {
  return guarded([&] {
    if (!s || !emitted) throw Failure("flush: null argument");
    *emitted = 0;
    const size_t ob = (size_t)s->channels * (size_t)std::max<int64_t>(capacity, 1) * (size_t)s->elem();
    DeviceScratch dout(ob);
    *emitted = synth_flush_dev(*s, dout.ptr, capacity, nullptr);
    SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (*emitted > 0) {
      if (!out) throw Failure("flush: null pointer");
      copy_to_host(out, dout.ptr, ob);
    }
  });
}

}  // extern "C"
