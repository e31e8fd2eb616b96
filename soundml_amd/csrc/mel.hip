// Mel filterbank product, the one dense contraction of the path:
//   Mel.apply c s = cast dtype (matmul W_f64 (cast f64 s))        mel.ml:202-231
// out[l][m][t] = sum_b W[m][b] * S[l][b][t], W = [n_mels; bins] triangular filters.
//
// float32: v_mfma_f32_32x32x2_f32 (exact f32 FMA chain, 64 FLOP/clk/SIMD).  A
// wave owns a 32-mel x 64-frame output block (two 32x32 accumulators sharing
// the A operand).  The filters are banded (each mel row touches a contiguous
// bin range), so every 32-mel block only walks the union of its rows' supports:
// for 128 mels over 1025 bins that is ~1/3.8 of the dense K loop.
// float64 (and float32 audio with the float64 interior): VALU dot products over
// the band, float64 accumulation, one rounding -- the reference's arithmetic.
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
#ifndef SMX_MEL_DEPTH
#define SMX_MEL_DEPTH 2   // k-steps whose operands are fetched together (C3: 1: 0.34 ms, 2: 0.29, 4: 0.30; next trip prefetched: 0.35)
#endif

struct MelArgs {
  const void *s;
  void *out;
  const float *w_block;  // [n_mels_pad / 32][k_pad / 2][64]: weights in MFMA A-operand order
  const int *block_lo, *block_hi;
  const double *w64;     // [n_mels][bins]
  const int *band_lo, *band_hi;
  int64_t lead, frames;
  int n_mels, n_mels_pad, bins, k_pad;
  int mel_blocks, frame_tiles;
};

// BY_BLOCK = false: grid = lead * frame_tiles workgroups of 4 waves; wave w walks mel blocks w, w+4, ...
// BY_BLOCK = true: a workgroup's 4 waves take 4 neighbouring frame tiles of ONE mel block (equal work per wave), and
// the blocks are dealt longest band first (the highest mels), so the launch ends on the short ones.
template <bool BY_BLOCK>
__global__ void __launch_bounds__(256) mel_apply_mfma_kernel(MelArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t tile = blockIdx.x;
  int mb_first = wave, mb_step = 4, mb_end = a.mel_blocks;
  if (BY_BLOCK) {
    const int64_t groups = (a.lead * a.frame_tiles + 3) / 4;
    mb_first = a.mel_blocks - 1 - (int)(blockIdx.x / groups);
    mb_end = mb_first + 1;
    mb_step = 1;
    tile = (blockIdx.x % groups) * 4 + wave;
    if (tile >= a.lead * a.frame_tiles) return;
  }
  const int64_t clip = tile / a.frame_tiles;
  const int64_t t0 = (tile % a.frame_tiles) * 64;
  const float *S = reinterpret_cast<const float *>(a.s) + clip * (int64_t)a.bins * a.frames;
  float *O = reinterpret_cast<float *>(a.out) + clip * (int64_t)a.n_mels * a.frames;
  const int col = lane & 31, half = lane >> 5;
  const int64_t ta = t0 + col, tb = t0 + 32 + col;
  const int64_t ta_c = ta < a.frames ? ta : a.frames - 1;
  const int64_t tb_c = tb < a.frames ? tb : a.frames - 1;
  for (int mb = mb_first; mb < mb_end; mb += mb_step) {
    // the block's band (host-built, wave-uniform) and its weights in operand order: one 256-byte run per k-step
    const int klo = __builtin_amdgcn_readfirstlane(a.block_lo[mb]) & ~7;
    const int khi = __builtin_amdgcn_readfirstlane(a.block_hi[mb]);
    f32x16 acc0 = {0}, acc1 = {0};
    const float *wb = a.w_block + (int64_t)mb * (a.k_pad / 2) * 64 + lane;
    // four k-steps (8 bins) per trip, every operand fetched before the first multiply-add; trips may run past the
    // band (W is zero there; k_pad is a multiple of 32) but never past the spectrogram's last bin: whole trips walk a
    // uniform row pointer with no guards and no 64-bit multiplies, the one trip that can cross the last bin is guarded
    const int whole_end = khi < (a.bins & ~7) ? khi : (a.bins & ~7);
    const int64_t lane_a = (int64_t)half * a.frames + ta_c, lane_b = (int64_t)half * a.frames + tb_c;
    const int64_t two_rows = 2 * a.frames;
    const float *rows = S + (int64_t)klo * a.frames;     // wave-uniform
    int k = klo;
    for (; k + 8 <= whole_end; k += 8, rows += 4 * two_rows) {
#pragma unroll
      for (int h = 0; h < 4; h += SMX_MEL_DEPTH) {
        float av[SMX_MEL_DEPTH], b0[SMX_MEL_DEPTH], b1[SMX_MEL_DEPTH];
#pragma unroll
        for (int j = 0; j < SMX_MEL_DEPTH; ++j) {
          av[j] = wb[(int64_t)(k / 2 + h + j) * 64];
          b0[j] = rows[(h + j) * two_rows + lane_a];
          b1[j] = rows[(h + j) * two_rows + lane_b];
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the first multiply-add
#pragma unroll
        for (int j = 0; j < SMX_MEL_DEPTH; ++j) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b0[j], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b1[j], acc1, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    for (; k < khi; k += 8) {
      float av[4], b0[4], b1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = k + 2 * j + half;
        av[j] = wb[(int64_t)(k / 2 + j) * 64];                     // W[m0 + col][k + 2 j + half]
        const bool ok = kk < a.bins;
        const int64_t row = (int64_t)(ok ? kk : 0) * a.frames;
        b0[j] = ok ? S[row + ta_c] : 0.0f;                         // S[kk][t0 + col]
        b1[j] = ok ? S[row + tb_c] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b0[j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b1[j], acc1, 0, 0, 0);
      }
    }
    // C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = mb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
      if (m < a.n_mels) {
        if (ta < a.frames) O[(int64_t)m * a.frames + ta] = acc0[reg];
        if (tb < a.frames) O[(int64_t)m * a.frames + tb] = acc1[reg];
      }
    }
  }
}

// float64 accumulation over the band; Tio = float (f64 interior on f32 data) or double
template <typename Tio>
__global__ void __launch_bounds__(256) mel_apply_f64_kernel(MelArgs a) {
  const int64_t clip = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.frames) return;
  const Tio *S = reinterpret_cast<const Tio *>(a.s) + clip * (int64_t)a.bins * a.frames;
  Tio *O = reinterpret_cast<Tio *>(a.out) + clip * (int64_t)a.n_mels * a.frames;
  for (int m = 0; m < a.n_mels; ++m) {
    const double *w = a.w64 + (int64_t)m * a.bins;
    double acc = 0.0;
    for (int b = a.band_lo[m]; b < a.band_hi[m]; ++b) acc += w[b] * (double)S[(int64_t)b * a.frames + t];
    O[(int64_t)m * a.frames + t] = (Tio)acc;
  }
}

}  // namespace

void launch_mel_apply(const MelJob &job) {
  if (job.lead <= 0 || job.frames <= 0) return;
  const smx_mel_config &c = *job.cfg;
  const smx_mel_config::Tables &t = c.tables();
  MelArgs a{};
  a.s = job.s;
  a.out = job.out;
  a.w_block = t.w_block;
  a.block_lo = t.block_lo;
  a.block_hi = t.block_hi;
  a.w64 = t.w_f64;
  a.band_lo = t.band_lo;
  a.band_hi = t.band_hi;
  a.lead = job.lead;
  a.frames = job.frames;
  a.n_mels = (int)c.n_mels;
  a.n_mels_pad = (int)t.n_mels_pad;
  a.bins = (int)c.bins();
  a.k_pad = (int)t.k_pad;
  a.mel_blocks = (int)(t.n_mels_pad / 32);
  a.frame_tiles = (int)((job.frames + 63) / 64);
  const bool f64_interior = job.elem_bytes == 8 || smx_get_interior() == SMX_INTERIOR_F64;
  if (!f64_interior) {
    static const bool by_tile = diag_flag("SMX_MEL_APPLY_BY_TILE") == 1;   // diagnostic: all blocks in one workgroup
    if (by_tile) {
      SMX_LAUNCH(mel_apply_mfma_kernel<false>, dim3(grid_x("apply", "frame tiles", job.lead * a.frame_tiles, 256)), dim3(256), 0, job.stream, a);
    } else {
      const int64_t blocks = (job.lead * a.frame_tiles + 3) / 4 * a.mel_blocks;
      SMX_LAUNCH(mel_apply_mfma_kernel<true>, dim3(grid_x("apply", "frame tiles", blocks, 256)), dim3(256), 0, job.stream, a);
    }
  } else {
    const unsigned ftiles = grid_x("apply", "frame tiles", (job.frames + 255) / 256, 256);
    for (int64_t c0 = 0; c0 < job.lead; c0 += kMaxGridYZ) {        // the slices sit on grid.y: 65535 at a time (DESIGN.md "Launch extents")
      a.lead = std::min(kMaxGridYZ, job.lead - c0);
      a.s = (const char *)job.s + c0 * a.bins * job.frames * job.elem_bytes;
      a.out = (char *)job.out + c0 * a.n_mels * job.frames * job.elem_bytes;
      const dim3 grid(ftiles, (unsigned)a.lead);
      if (job.elem_bytes == 8)
        SMX_LAUNCH(mel_apply_f64_kernel<double>, grid, dim3(256), 0, job.stream, a);
      else
        SMX_LAUNCH(mel_apply_f64_kernel<float>, grid, dim3(256), 0, job.stream, a);
    }
  }
  SMX_HIP_CHECK(hipGetLastError());
}

}  // namespace smx

// ---- the C ABI's side: Mel.Config, Mel.apply, Soundml.mel_spectrogram ------------------------------------------------------
namespace smx {
namespace {

void check_mel_shape(const smx_mel_config &c, int64_t lead, int64_t bins, int64_t frames) {
  if (lead < 0 || frames < 0 || bins < 0) throw Failure("apply: negative extent");
  if (bins != c.bins())  // mel.ml:210-218
    throw InvalidArgument(format(
        "apply: cannot project %lld frequency bins through a filterbank built for an FFT of size %lld "
        "(%lld bins)",
        (long long)bins, (long long)c.fft_size, (long long)c.bins()));
}

void mel_apply_dev(const smx_mel_config &c, const void *d_s, int elem_bytes, int64_t lead, int64_t bins,
                   int64_t frames, void *d_out, hipStream_t stream) {
  check_mel_shape(c, lead, bins, frames);
  if (lead == 0 || frames == 0) return;  // mel.ml:220-226: nothing to reduce over
  if (!d_s || !d_out) throw Failure("apply: null device pointer");
  MelJob job;
  job.cfg = &c;
  job.s = d_s;
  job.elem_bytes = elem_bytes;
  job.lead = lead;
  job.frames = frames;
  job.out = d_out;
  job.stream = stream;
  launch_mel_apply(job);
}

void mel_apply_host(const smx_mel_config &c, const void *s, int elem_bytes, int64_t lead, int64_t bins,
                    int64_t frames, void *out) {
  check_mel_shape(c, lead, bins, frames);
  if (lead == 0 || frames == 0) return;
  if (!s || !out) throw Failure("apply: null pointer");
  host_call("mel_apply", {{s, (size_t)bins * (size_t)frames * (size_t)elem_bytes}}, out, (size_t)c.n_mels * (size_t)frames * (size_t)elem_bytes,
            lead, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              mel_apply_dev(c, d_in[0], elem_bytes, nc, bins, frames, d_out, stream);
            });
}

void check_fft_sizes(const smx_stft_config &sc, const smx_mel_config &mc) {  // soundml.ml:12-20
  if (sc.fft_size != mc.fft_size)
    throw InvalidArgument(format(
        "mel_spectrogram: cannot project a %lld-point STFT through a filterbank built for an FFT of "
        "size %lld (the two configurations must agree on fft_size)",
        (long long)sc.fft_size, (long long)mc.fft_size));
}

}  // namespace

// Soundml.mel_spectrogram on device-resident audio.  The fused kernel keeps the
// power tile on chip; other geometries run power_spectrum into a scratch
// spectrogram followed by Mel.apply (the reference's own composition).
void mel_spectrogram_dev(const smx_stft_config &sc, const smx_mel_config &mc, const void *d_x,
                         int in_bytes, int64_t lead, int64_t n, int64_t x_stride, double power,
                         void *d_out, hipStream_t stream) {
  check_fft_sizes(sc, mc);
  check_rank_extents("mel_spectrogram", lead, n);
  if (x_stride < n) throw Failure("mel_spectrogram: x_stride is smaller than the signal length");
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!d_x || !d_out) throw Failure("mel_spectrogram: null device pointer");
  MelSpecJob job;
  job.stft = stft_job(sc, d_x, in_bytes, lead, n, x_stride, 0, count, OUT_POWER, power, nullptr, stream);
  job.mel = &mc;
  job.out = d_out;
  if (launch_mel_spectrogram_fused(job)) return;
  // two-step form; scratch is stream-ordered
  void *scratch = nullptr;
  const size_t bytes = (size_t)lead * (size_t)sc.bins() * (size_t)count * (size_t)in_bytes;
  SMX_HIP_CHECK(smx::pool_malloc_async(&scratch, bytes, stream));
  job.stft.out = scratch;
  launch_stft(job.stft);
  mel_apply_dev(mc, scratch, in_bytes, lead, sc.bins(), count, d_out, stream);
  SMX_HIP_CHECK(smx::pool_free_async(scratch, stream));
}

namespace {

// Soundml.mel_spectrogram from host memory: the current device, or the device list's clip ranges side by side (soundml.mli:85-101:
// leading axes broadcast; mel_props.ml:136-155 tests the slices)
void mel_spectrogram_host(const smx_stft_config &sc, const smx_mel_config &mc, const void *x, int in_bytes,
                          int64_t lead, int64_t n, double power, void *out) {
  check_fft_sizes(sc, mc);
  check_rank_extents("mel_spectrogram", lead, n);
  const int64_t count = sc.frames(n);
  if (lead == 0 || count == 0) return;
  if (!x || !out) throw Failure("mel_spectrogram: null pointer");
  host_call("mel_spectrogram", {{x, (size_t)n * (size_t)in_bytes}}, out, (size_t)mc.n_mels * (size_t)count * (size_t)in_bytes, lead, true,
            nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              mel_spectrogram_dev(sc, mc, d_in[0], in_bytes, nc, n, n, power, d_out, stream);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_mel_config_create(int64_t n_mels, int64_t sample_rate, int64_t fft_size, double f_min,
                          int has_f_max, double f_max, int scale, int norm, smx_mel_config **out) {
  return guarded([&] {
    if (!out) throw Failure("create: null output handle");
    *out = mel_config_create(n_mels, sample_rate, fft_size, f_min, has_f_max != 0, f_max, scale, norm);
  });
}
int smx_mel_config_from_weights(int64_t rows, int64_t fft_size, const double *weights, smx_mel_config **out) {
  return guarded([&] {
    if (!out || !weights) throw Failure("from_weights: null pointer");
    if (rows < 1) throw InvalidArgument(format("from_weights: cannot build %lld filters (rows must be at least 1)", (long long)rows));
    if (fft_size < 1)
      throw InvalidArgument(format("from_weights: cannot use an FFT of size %lld (fft_size must be at least 1)", (long long)fft_size));
    smx_mel_config *c = new smx_mel_config();
    c->n_mels = rows;
    c->fft_size = fft_size;
    c->weights.assign(weights, weights + (size_t)rows * (size_t)(fft_size / 2 + 1));
    *out = c;
  });
}
void smx_mel_config_destroy(smx_mel_config *c) { delete c; }
int64_t smx_mel_config_n_mels(const smx_mel_config *c) { return c ? c->n_mels : -1; }
int64_t smx_mel_config_bins(const smx_mel_config *c) { return c ? c->bins() : -1; }
int64_t smx_mel_config_fft_size(const smx_mel_config *c) { return c ? c->fft_size : -1; }
double smx_mel_config_f_max(const smx_mel_config *c) { return c ? c->f_max : -1.0; }
int smx_mel_filterbank(const smx_mel_config *c, double *out) {
  return guarded([&] {
    check_config(c, "filterbank");
    std::memcpy(out, c->weights.data(), c->weights.size() * sizeof(double));
  });
}
int smx_mel_apply_f32(const smx_mel_config *c, const float *s, int64_t lead, int64_t bins,
                      int64_t frames, float *out) {
  return guarded([&] {
    check_config(c, "apply");
    mel_apply_host(*c, s, 4, lead, bins, frames, out);
  });
}
int smx_mel_apply_f64(const smx_mel_config *c, const double *s, int64_t lead, int64_t bins,
                      int64_t frames, double *out) {
  return guarded([&] {
    check_config(c, "apply");
    mel_apply_host(*c, s, 8, lead, bins, frames, out);
  });
}
int smx_mel_apply_f32_dev(const smx_mel_config *c, const float *d_s, int64_t lead, int64_t bins,
                          int64_t frames, float *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "apply");
    mel_apply_dev(*c, d_s, 4, lead, bins, frames, d_out, (hipStream_t)stream);
  });
}
int smx_mel_apply_f64_dev(const smx_mel_config *c, const double *d_s, int64_t lead, int64_t bins,
                          int64_t frames, double *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "apply");
    mel_apply_dev(*c, d_s, 8, lead, bins, frames, d_out, (hipStream_t)stream);
  });
}
int smx_mel_spectrogram_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *x,
                            int64_t lead, int64_t n, double power, float *out) {
  return guarded([&] {
    check_config(sc, "mel_spectrogram");
    check_config(mc, "mel_spectrogram");
    mel_spectrogram_host(*sc, *mc, x, 4, lead, n, power, out);
  });
}
int smx_mel_spectrogram_f64(const smx_stft_config *sc, const smx_mel_config *mc, const double *x,
                            int64_t lead, int64_t n, double power, double *out) {
  return guarded([&] {
    check_config(sc, "mel_spectrogram");
    check_config(mc, "mel_spectrogram");
    mel_spectrogram_host(*sc, *mc, x, 8, lead, n, power, out);
  });
}
int smx_mel_spectrogram_f32_dev(const smx_stft_config *sc, const smx_mel_config *mc, const float *d_x,
                                int64_t lead, int64_t n, int64_t x_stride, double power, float *d_out,
                                void *stream) {
  return guarded([&] {
    check_config(sc, "mel_spectrogram");
    check_config(mc, "mel_spectrogram");
    mel_spectrogram_dev(*sc, *mc, d_x, 4, lead, n, x_stride, power, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
