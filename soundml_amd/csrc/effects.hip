// Effects.phase_vocoder (effects.ml:184-274): complex [lead; bins; frames] -> [lead; bins; count] on the device.
//
// The phases are a recurrence whose accumulator is never reduced (about 1600 rad per frame at the top bin of fft 2048 / hop 512),
// and the reference meets librosa only because both perform the same float64 operations in the same order.  So whatever the
// spectrum's dtype and whatever the library's interior, everything here is float64: hypot, atan2 (correctly rounded, as the
// reference's libm rounds it: atan2_dd.hpp), the interpolation, the
// recurrence and the closing sincos, each bracketed as the reference brackets it, and the result rounded once into the
// spectrum's dtype.  This file is built with -ffp-contract=off (Makefile): a fused multiply-add would round differently.
//
// Every (signal, bin) chain is walked in frame order; nothing is scanned or reassociated.  The parallelism is signals x bins.
#include "smx_internal.hpp"
#include "atan2_dd.hpp"

namespace smx {
namespace {

constexpr double kTwoPi = 2.0 * 3.14159265358979323846;

// effects.ml:66-79: x reduced to the interval of width 2 pi centred at zero; rint rounds ties to even
__device__ __forceinline__ double principal(double x) { return x - (kTwoPi * rint(x / kTwoPi)); }

// effects.ml:83-86
__device__ __forceinline__ double advance_of(const double hop, const double step, int64_t k) { return hop * ((double)k * step); }

template <typename Z> struct Parts;
template <> struct Parts<float2> { using Real = float; };
template <> struct Parts<double2> { using Real = double; };

struct PvocArgs {
  const void *z;
  void *out;
  int64_t bins, frames, count;
  double rate, hop, step;
  int oc;   // independent mode: output frames per chunk
};

// magnitude and argument of one analysis cell; rows `frames` and `frames + 1` are the reference's two zero rows (effects.ml:245-248)
template <typename Z>
__device__ __forceinline__ void polar(const Z *row, int64_t frame, int64_t frames, double &m, double &a) {
  m = 0.0;
  a = 0.0;
  if (frame < frames) {
    const Z v = row[frame];
    m = hypot((double)v.x, (double)v.y);
    a = dd::atan2_rounded((double)v.y, (double)v.x);   // rounds as glibc's does (atan2_dd.hpp); arg(-0 + 0i) = pi
  }
}

// ---- independent phases ----------------------------------------------------------------------------------------------------
// A workgroup owns one signal, kBins bins and the whole frame axis, in chunks of `oc` output frames.  A chunk reads the analysis
// frames [i0(first), i0(last) + 2): at most kIn of them, by the launcher's choice of oc.  Global memory is touched with lanes along
// frames only; the chains are walked with lanes along bins on LDS tiles (pitches odd: no bank conflicts).
constexpr int kBins = 32, kOut = 32, kIn = 48, kThreads = 256;
constexpr int kInPitch = kIn + 1, kOutPitch = kOut + 1;

template <typename Z>
__global__ __launch_bounds__(kThreads) void pvoc_independent_kernel(PvocArgs a) {
  __shared__ double s_mag[kBins * kInPitch], s_ang[kBins * kInPitch], s_dev[kBins * kInPitch], s_phi[kBins * kOutPitch];
  using Real = typename Parts<Z>::Real;
  const int tid = threadIdx.x;
  const int64_t per_signal = (a.bins + kBins - 1) / kBins;
  const int64_t signal = blockIdx.x / per_signal, b0 = (blockIdx.x % per_signal) * kBins;
  const int nb = a.bins - b0 < kBins ? (int)(a.bins - b0) : kBins;
  const Z *z = reinterpret_cast<const Z *>(a.z) + (signal * a.bins + b0) * a.frames;
  Z *out = reinterpret_cast<Z *>(a.out) + (signal * a.bins + b0) * a.count;
  const double omega = advance_of(a.hop, a.step, b0 + tid);   // the walking lanes' own bin
  double phi = 0.0;
  for (int64_t o0 = 0; o0 < a.count; o0 += a.oc) {
    const int oc = a.count - o0 < a.oc ? (int)(a.count - o0) : a.oc;
    const int64_t in_lo = (int64_t)((double)o0 * a.rate);
    const int span = (int)((int64_t)((double)(o0 + oc - 1) * a.rate) + 2 - in_lo);
    if (span > kIn) return;   // (never: launch_pvoc sizes oc so that the span fits; uniform over the workgroup)
    // 1. magnitude and argument once per analysis cell, lanes along frames
    for (int c = tid; c < nb * span; c += kThreads) {
      const int b = c / span, f = c % span;
      double m, g;
      polar(z + (int64_t)b * a.frames, in_lo + f, a.frames, m, g);
      s_mag[b * kInPitch + f] = m;
      s_ang[b * kInPitch + f] = g;
    }
    __syncthreads();
    // the heterodyned increment between consecutive analysis frames depends on i0 alone
    for (int c = tid; c < nb * (span - 1); c += kThreads) {
      const int b = c / (span - 1), f = c % (span - 1);
      s_dev[b * kInPitch + f] = principal(s_ang[b * kInPitch + f + 1] - s_ang[b * kInPitch + f] - advance_of(a.hop, a.step, b0 + b));
    }
    if (o0 == 0 && tid < nb) phi = s_ang[tid * kInPitch];   // the accumulator starts at the argument of frame 0
    __syncthreads();
    // 2. the chains, lanes along bins, in frame order: phi + (omega + deviation)
    if (tid < nb) {
      for (int j = 0; j < oc; ++j) {
        s_phi[tid * kOutPitch + j] = phi;
        const int64_t i = o0 + j;
        if (i + 1 < a.count) {
          const int f = (int)((int64_t)((double)i * a.rate) - in_lo);
          phi = phi + (omega + s_dev[tid * kInPitch + f]);
        }
      }
    }
    __syncthreads();
    // 3. amplitude and phasor, lanes along output frames
    for (int c = tid; c < nb * oc; c += kThreads) {
      const int b = c / oc, j = c % oc;
      const int64_t i = o0 + j;
      const double position = (double)i * a.rate;
      const int64_t i0 = (int64_t)position;
      const double alpha = position - (double)i0;
      const int f = (int)(i0 - in_lo);
      const double amp = ((1.0 - alpha) * s_mag[b * kInPitch + f]) + (alpha * s_mag[b * kInPitch + f + 1]);
      double sn, cs;
      sincos(s_phi[b * kOutPitch + j], &sn, &cs);
      Z y;
      y.x = (Real)(amp * cs);
      y.y = (Real)(amp * sn);
      out[(int64_t)b * a.count + i] = y;
    }
    __syncthreads();
  }
}

// ---- identity phase locking (effects.ml:146-182) -----------------------------------------------------------------------------
// A frame's bins are coupled and the locked phases are what the next frame accumulates from, so one workgroup holds every bin of
// one signal and steps through the output frames.  The float64 magnitude and argument rows of analysis frames i0 and i0 + 1 live in
// LDS (slot = frame & 1; a row is computed when the walk first reaches it), with the accumulator row and one bit per bin for the
// peak set of frame i0.
constexpr int kLockThreads = 512;

size_t locked_lds_bytes(int64_t bins) { return (size_t)(5 * bins + (bins + 63) / 64) * 8; }

template <typename Z>
__global__ __launch_bounds__(kLockThreads) void pvoc_locked_kernel(PvocArgs a) {
  extern __shared__ double s_lock[];
  using Real = typename Parts<Z>::Real;
  const int tid = threadIdx.x;
  const int bins = (int)a.bins, words = (bins + 63) / 64;
  double *s_mag = s_lock, *s_ang = s_lock + 2 * bins, *s_phi = s_lock + 4 * bins;
  unsigned long long *s_peak = reinterpret_cast<unsigned long long *>(s_lock + 5 * bins);
  const Z *z = reinterpret_cast<const Z *>(a.z) + (int64_t)blockIdx.x * a.bins * a.frames;
  Z *out = reinterpret_cast<Z *>(a.out) + (int64_t)blockIdx.x * a.bins * a.count;
  int64_t held0 = -1, held1 = -1;   // the analysis frame each slot holds
  for (int64_t i = 0; i < a.count; ++i) {
    const double position = (double)i * a.rate;
    const int64_t i0 = (int64_t)position;
    const double alpha = position - (double)i0;
    __syncthreads();   // the previous step's readers are done with the slot that is replaced
    for (int64_t frame = i0; frame <= i0 + 1; ++frame) {
      const int slot = (int)(frame & 1);
      if ((slot ? held1 : held0) == frame) continue;
      for (int k = tid; k < bins; k += kLockThreads) polar(z + (int64_t)k * a.frames, frame, a.frames, s_mag[slot * bins + k], s_ang[slot * bins + k]);
      if (slot) held1 = frame;
      else held0 = frame;
    }
    if (i == 0)
      for (int k = tid; k < bins; k += kLockThreads) s_phi[k] = s_ang[k];   // frame 0 sits in slot 0; a lane reads what it wrote
    __syncthreads();
    const double *m0 = s_mag + (int)(i0 & 1) * bins, *a0 = s_ang + (int)(i0 & 1) * bins;
    const double *m1 = s_mag + (int)((i0 + 1) & 1) * bins, *a1 = s_ang + (int)((i0 + 1) & 1) * bins;
    // peaks_of: strictly above each of the up to four neighbours a bin has; one ballot word per 64 bins
    for (int base = 0; base < words * 64; base += kLockThreads) {
      const int k = base + tid;
      bool peak = false;
      if (k < bins) {
        const double v = m0[k];
        peak = (k < 2 || v > m0[k - 2]) && (k < 1 || v > m0[k - 1]) && (k + 1 >= bins || v > m0[k + 1]) && (k + 2 >= bins || v > m0[k + 2]);
      }
      const unsigned long long word = __ballot(peak);
      if ((tid & 63) == 0 && k < words * 64) s_peak[k >> 6] = word;
    }
    __syncthreads();
    for (int k = tid; k < bins; k += kLockThreads) {
      // lock: a bin that is no peak takes its region's peak phase plus the analysis phase difference; regions split at
      // (kp + kp_next + 1) / 2, the first region starts at bin 0 and the last ends at the top; no peaks: left alone.  Only
      // peaks' accumulators are read here and only the others' are written.
      const int w = k >> 6, bit = k & 63;
      if (!((s_peak[w] >> bit) & 1ull)) {
        int below = -1, above = -1;
        unsigned long long lo = s_peak[w] & ((1ull << bit) - 1ull);
        for (int v = w; v >= 0; --v) {
          if (lo) {
            below = v * 64 + 63 - __clzll((long long)lo);
            break;
          }
          if (v > 0) lo = s_peak[v - 1];
        }
        unsigned long long hi = s_peak[w] & ~((1ull << bit) - 1ull);
        for (int v = w; v < words; ++v) {
          if (hi) {
            above = v * 64 + __ffsll((unsigned long long)hi) - 1;
            break;
          }
          if (v + 1 < words) hi = s_peak[v + 1];
        }
        int owner = -1;
        if (below >= 0 && above >= 0) owner = k < (below + above + 1) / 2 ? below : above;
        else if (below >= 0) owner = below;
        else if (above >= 0) owner = above;
        if (owner >= 0) s_phi[k] = s_phi[owner] + (a0[k] - a0[owner]);
      }
    }
    __syncthreads();   // the peaks' accumulators advance only after every bin of their regions has read them
    for (int k = tid; k < bins; k += kLockThreads) {
      const double amp = ((1.0 - alpha) * m0[k]) + (alpha * m1[k]);
      const double phi = s_phi[k];
      double sn, cs;
      sincos(phi, &sn, &cs);
      Z y;
      y.x = (Real)(amp * cs);
      y.y = (Real)(amp * sn);
      out[(int64_t)k * a.count + i] = y;
      if (i + 1 < a.count) {
        const double omega = advance_of(a.hop, a.step, k);
        s_phi[k] = phi + (omega + principal(a1[k] - a0[k] - omega));
      }
    }
  }
}

template <typename Z>
void launch_typed(const PvocJob &job, PvocArgs a) {
  if (job.locked) {
    const size_t lds = locked_lds_bytes(job.bins);
    if (lds > (size_t)160 * 1024)
      throw Failure(format("phase_vocoder: the locked phase mode holds a frame's %lld bins in LDS, which has room for %d",
                           (long long)job.bins, (int)((160 * 1024 / 8 - 64) / 5)));
    launch_tiles("phase_vocoder", pvoc_locked_kernel<Z>, job.lead, kLockThreads, lds, job.stream, a);
    return;
  }
  const int64_t per_signal = (job.bins + kBins - 1) / kBins;
  SMX_LAUNCH(pvoc_independent_kernel<Z>, dim3(grid_x("phase_vocoder", "bin blocks", per_signal * job.lead, kThreads)), dim3(kThreads), 0, job.stream, a);
  SMX_HIP_CHECK(hipGetLastError());
}

}  // namespace

static double pvoc_advance_step(int64_t fft_size) { return 1.0 / ((double)fft_size * (1.0 / kTwoPi)); }

void launch_pvoc(const PvocJob &job) {
  if (job.lead <= 0 || job.bins <= 0 || job.count <= 0) return;
  PvocArgs a;
  a.z = job.z;
  a.out = job.out;
  a.bins = job.bins;
  a.frames = job.frames;
  a.count = job.count;
  a.rate = job.rate;
  a.hop = (double)job.hop;
  a.step = pvoc_advance_step(job.fft_size);
  // a chunk of oc output frames reads at most (oc - 1) * rate + 3 analysis frames (i0 truncates, and i0 + 1 is read too); one
  // more for the rounding of the products
  a.oc = (int)std::max(1.0, std::min((double)kOut, std::floor((double)(kIn - 4) / job.rate) + 1.0));
  if (job.elem_bytes == 8) launch_typed<double2>(job, a);
  else launch_typed<float2>(job, a);
}

}  // namespace smx

// ---- the C ABI's side: Effects ---------------------------------------------------------------------------------------------
namespace smx {
namespace {

// ---- Effects (effects.ml:96-123, 285-334): checks in the reference's order and words, then the launches ---------------------
bool pvoc_locked(const char *fn, int phase) {
  if (phase != SMX_PHASE_INDEPENDENT && phase != SMX_PHASE_LOCKED) throw Failure(format("%s: unknown phase mode %d", fn, phase));
  return phase == SMX_PHASE_LOCKED;
}

// check_rate, check_spectrum (effects.ml:96-117; the rank is what the entry point's signature states); the output frame count
int64_t check_vocoder(const smx_stft_config *c, double rate, int phase, int64_t lead, int64_t bins, int64_t frames) {
  check_stretch_rate("phase_vocoder", rate);
  check_config(c, "phase_vocoder");
  if (lead < 0 || bins < 0 || frames < 0)
    throw Failure(format("phase_vocoder: negative extent (lead %lld, bins %lld, frames %lld)", (long long)lead, (long long)bins,
                         (long long)frames));
  if (bins != c->bins())
    throw InvalidArgument(format("phase_vocoder: cannot vocode %lld frequency bins of a %lld-point transform (the bin axis must hold "
                                 "fft_size / 2 + 1 = %lld values)", (long long)bins, (long long)c->fft_size, (long long)c->bins()));
  pvoc_locked("phase_vocoder", phase);
  return pvoc_out_frames(frames, rate);
}

void vocoder_dev(const smx_stft_config &c, const void *d_z, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, double rate,
                 int phase, void *d_out, hipStream_t stream) {
  const int64_t count = check_vocoder(&c, rate, phase, lead, bins, frames);
  if (lead == 0 || count == 0) return;   // a spectrum with no frames is a spectrum with no frames
  if (!d_z || !d_out) throw Failure("phase_vocoder: null device pointer");
  PvocJob job;
  job.z = d_z;
  job.elem_bytes = elem_bytes;
  job.lead = lead;
  job.bins = bins;
  job.frames = frames;
  job.count = count;
  job.fft_size = c.fft_size;
  job.hop = c.hop;
  job.rate = rate;
  job.locked = phase == SMX_PHASE_LOCKED;
  job.out = d_out;
  job.stream = stream;
  launch_pvoc(job);
}

void vocoder_host(const smx_stft_config *c, const void *z, int elem_bytes, int64_t lead, int64_t bins, int64_t frames, double rate,
                  int phase, void *out) {
  const int64_t count = check_vocoder(c, rate, phase, lead, bins, frames);
  if (lead == 0 || count == 0) return;
  if (!z || !out) throw Failure("phase_vocoder: null pointer");
  const size_t cell = 2 * (size_t)elem_bytes;
  host_call("phase_vocoder", {{z, (size_t)bins * (size_t)frames * cell}}, out, (size_t)bins * (size_t)count * cell, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              vocoder_dev(*c, d_in[0], elem_bytes, nc, bins, frames, rate, phase, d_out, stream);
            });
}

// `time_stretch` (effects.ml:291-298): rate, rank (the signature's), then what Stft.invert checks for the length it will be asked for
struct StretchPlan {
  int64_t frames = 0, count = 0, length = 0;
};
StretchPlan check_stretch(const smx_stft_config *c, double rate, int phase, int64_t lead, int64_t n) {
  check_stretch_rate("time_stretch", rate);
  check_config(c, "time_stretch");
  check_rank_extents("time_stretch", lead, n);
  pvoc_locked("time_stretch", phase);
  StretchPlan p;
  p.length = stretch_length(n, rate);
  check_synthesis("invert", *c, c->bins(), p.length, true);
  p.frames = c->frames(n);
  p.count = pvoc_out_frames(p.frames, rate);
  return p;
}

// Stft.transform -> vocoder -> Stft.invert ~length inside the library, bit for bit those three calls.  The two complex stacks live
// in scratch and the batch goes through in clip chunks that keep them bounded (every clip is stretched on its own).  float64 audio,
// and float32 audio under the float64 interior (widened first, the result rounded once: effects.ml:291-298), keep complex128
// spectra between the stages.
void stretch_dev(const smx_stft_config &c, const void *d_x, int in_bytes, int64_t lead, int64_t n, double rate, int phase, void *d_y,
                 hipStream_t stream) {
  const StretchPlan p = check_stretch(&c, rate, phase, lead, n);
  if (lead == 0 || p.length == 0) return;
  if (!d_y || (n > 0 && !d_x)) throw Failure("time_stretch: null device pointer");
  if (p.count == 0) {   // no analysis frame: silence
    SMX_HIP_CHECK(hipMemsetAsync(d_y, 0, (size_t)lead * (size_t)p.length * (size_t)in_bytes, stream));
    return;
  }
  const int work = in_bytes == 8 || interior() == SMX_INTERIOR_F64 ? 8 : 4;
  const bool widen = work != in_bytes;
  const int64_t bins = c.bins();
  const size_t cell = 2 * (size_t)work;
  const size_t plane = (size_t)bins * (size_t)std::max(p.frames, p.count) * cell;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(lead, (int64_t)(((size_t)256 << 20) / std::max<size_t>(plane, 1))));
  init_device_pool();
  DeviceScratch z, stretched, wide_x, wide_y;
  z.pool(std::max<size_t>(16, (size_t)chunk * (size_t)bins * (size_t)p.frames * cell), stream);
  stretched.pool(std::max<size_t>(16, (size_t)chunk * (size_t)bins * (size_t)p.count * cell), stream);
  if (widen) {
    wide_x.pool(std::max<size_t>(16, (size_t)chunk * (size_t)n * 8), stream);
    wide_y.pool(std::max<size_t>(16, (size_t)chunk * (size_t)p.length * 8), stream);
  }
  for (int64_t c0 = 0; c0 < lead; c0 += chunk) {
    const int64_t nc = std::min(chunk, lead - c0);
    const void *src = reinterpret_cast<const unsigned char *>(d_x) + (size_t)c0 * (size_t)n * (size_t)in_bytes;
    void *dst = reinterpret_cast<unsigned char *>(d_y) + (size_t)c0 * (size_t)p.length * (size_t)in_bytes;
    if (widen) {
      launch_gl_widen(reinterpret_cast<const float *>(src), wide_x.as<double>(), nc * n, stream);
      src = wide_x.ptr;
    }
    stft_range_dev(c, src, work, nc, n, n, 0, p.frames, OUT_COMPLEX, 2.0, z.ptr, stream);
    vocoder_dev(c, z.ptr, work, nc, bins, p.frames, rate, phase, stretched.ptr, stream);
    invert_dev(c, stretched.ptr, 2 * work, nc, bins, p.count, 1, p.length, widen ? wide_y.ptr : dst, stream);
    if (widen) launch_gl_narrow(wide_y.as<double>(), reinterpret_cast<float *>(dst), nc * p.length, stream);
  }
}

void stretch_host(const smx_stft_config *c, const void *x, int in_bytes, int64_t lead, int64_t n, double rate, int phase, void *y) {
  const StretchPlan p = check_stretch(c, rate, phase, lead, n);
  if (lead == 0 || p.length == 0) return;
  if (!y || (n > 0 && !x)) throw Failure("time_stretch: null pointer");
  host_call("time_stretch", {{x, (size_t)n * (size_t)in_bytes}}, y, (size_t)p.length * (size_t)in_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) { stretch_dev(*c, d_in[0], in_bytes, nc, n, rate, phase, d_out, stream); });
}

// `pitch_shift` (effects.ml:324-334): time_stretch at den / num (this very quotient: the vocoder is chaotic in its rate), the
// resampler built for num -> den, then the cut or zero-extension to n; the stretched signal stays on the device between the
// stages.  DEVIATION: Resample.apply is float32 here, so float64 audio is stretched in float64 and converted in float32.
struct ShiftPlan {
  double rate = 1.0;
  StretchPlan stretch;
  int64_t resampled = 0;
};
ShiftPlan check_shift(const smx_stft_config *c, const smx_resample_config *r, int phase, int64_t lead, int64_t n) {
  check_config(c, "pitch_shift");
  check_config(r, "pitch_shift");
  check_rank_extents("pitch_shift", lead, n);
  ShiftPlan p;
  p.rate = (double)smx_resample_config_target(r) / (double)smx_resample_config_sample_rate(r);
  p.stretch = check_stretch(c, p.rate, phase, lead, n);
  if (smx_resample_config_output_frames(r, p.stretch.length, &p.resampled) != SMX_OK) throw InvalidArgument(smx_last_error());
  return p;
}

void shift_dev(const smx_stft_config &c, const smx_resample_config &r, int phase, const void *d_x, int in_bytes, int64_t lead, int64_t n,
               void *d_y, hipStream_t stream) {
  const ShiftPlan p = check_shift(&c, &r, phase, lead, n);
  if (lead == 0 || n == 0) return;
  if (!d_x || !d_y) throw Failure("pitch_shift: null device pointer");
  const int64_t length = p.stretch.length, kept = std::min(n, p.resampled);
  init_device_pool();
  DeviceScratch stretched, resampled, wide, fixed;
  stretched.pool(std::max<size_t>(16, (size_t)lead * (size_t)length * 4), stream);
  resampled.pool(std::max<size_t>(16, (size_t)lead * (size_t)p.resampled * 4), stream);
  if (in_bytes == 8) {
    wide.pool(std::max<size_t>(16, (size_t)lead * (size_t)length * 8), stream);
    fixed.pool((size_t)lead * (size_t)n * 4, stream);
    stretch_dev(c, d_x, 8, lead, n, p.rate, phase, wide.ptr, stream);
    if (length > 0) launch_gl_narrow(wide.as<double>(), stretched.as<float>(), lead * length, stream);
  } else {
    stretch_dev(c, d_x, 4, lead, n, p.rate, phase, stretched.ptr, stream);
  }
  if (p.resampled > 0) {
    const int code = smx_resample_apply_f32_dev(&r, stretched.as<float>(), lead, length, length, resampled.as<float>(), p.resampled, stream);
    if (code != SMX_OK) {
      if (code == SMX_INVALID_ARGUMENT) throw InvalidArgument(smx_last_error());
      throw Failure(smx_last_error());
    }
  }
  float *out = in_bytes == 8 ? fixed.as<float>() : reinterpret_cast<float *>(d_y);   // fix_length, effects.ml:302-314
  if (kept < n) SMX_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)lead * (size_t)n * 4, stream));
  if (kept > 0)
    SMX_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)n * 4, resampled.ptr, (size_t)p.resampled * 4, (size_t)kept * 4, (size_t)lead,
                                   hipMemcpyDeviceToDevice, stream));
  if (in_bytes == 8) launch_gl_widen(fixed.as<float>(), reinterpret_cast<double *>(d_y), lead * n, stream);
}

void shift_host(const smx_stft_config *c, const smx_resample_config *r, int phase, const void *x, int in_bytes, int64_t lead, int64_t n,
                void *y) {
  check_shift(c, r, phase, lead, n);
  if (lead == 0 || n == 0) return;
  if (!x || !y) throw Failure("pitch_shift: null pointer");
  const size_t row = (size_t)n * (size_t)in_bytes;
  host_call("pitch_shift", {{x, row}}, y, row, lead, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
    shift_dev(*c, *r, phase, d_in[0], in_bytes, nc, n, d_out, stream);
  });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Effects (effects.ml) ---------------------------------------------------------------------------
int smx_phase_vocoder_c64(const smx_stft_config *c, const float *z, int64_t lead, int64_t bins, int64_t frames, double rate, int phase,
                          float *out) {
  return guarded([&] { vocoder_host(c, z, 4, lead, bins, frames, rate, phase, out); });
}
int smx_phase_vocoder_c128(const smx_stft_config *c, const double *z, int64_t lead, int64_t bins, int64_t frames, double rate, int phase,
                           double *out) {
  return guarded([&] { vocoder_host(c, z, 8, lead, bins, frames, rate, phase, out); });
}
int smx_phase_vocoder_c64_dev(const smx_stft_config *c, const float *d_z, int64_t lead, int64_t bins, int64_t frames, double rate,
                              int phase, float *d_out, void *stream) {
  return guarded([&] {
    check_vocoder(c, rate, phase, lead, bins, frames);
    vocoder_dev(*c, d_z, 4, lead, bins, frames, rate, phase, d_out, (hipStream_t)stream);
  });
}
int smx_phase_vocoder_c128_dev(const smx_stft_config *c, const double *d_z, int64_t lead, int64_t bins, int64_t frames, double rate,
                               int phase, double *d_out, void *stream) {
  return guarded([&] {
    check_vocoder(c, rate, phase, lead, bins, frames);
    vocoder_dev(*c, d_z, 8, lead, bins, frames, rate, phase, d_out, (hipStream_t)stream);
  });
}
int smx_time_stretch_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, double rate, int phase, float *y) {
  return guarded([&] { stretch_host(c, x, 4, lead, n, rate, phase, y); });
}
int smx_time_stretch_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, double rate, int phase, double *y) {
  return guarded([&] { stretch_host(c, x, 8, lead, n, rate, phase, y); });
}
int smx_time_stretch_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, double rate, int phase, float *d_y,
                             void *stream) {
  return guarded([&] {
    check_stretch(c, rate, phase, lead, n);
    stretch_dev(*c, d_x, 4, lead, n, rate, phase, d_y, (hipStream_t)stream);
  });
}
int smx_pitch_shift_f32(const smx_stft_config *c, const smx_resample_config *r, int phase, const float *x, int64_t lead, int64_t n,
                        float *y) {
  return guarded([&] { shift_host(c, r, phase, x, 4, lead, n, y); });
}
int smx_pitch_shift_f64(const smx_stft_config *c, const smx_resample_config *r, int phase, const double *x, int64_t lead, int64_t n,
                        double *y) {
  return guarded([&] { shift_host(c, r, phase, x, 8, lead, n, y); });
}
int smx_pitch_shift_f32_dev(const smx_stft_config *c, const smx_resample_config *r, int phase, const float *d_x, int64_t lead, int64_t n,
                            float *d_y, void *stream) {
  return guarded([&] {
    check_shift(c, r, phase, lead, n);
    shift_dev(*c, *r, phase, d_x, 4, lead, n, d_y, (hipStream_t)stream);
  });
}

}  // extern "C"
