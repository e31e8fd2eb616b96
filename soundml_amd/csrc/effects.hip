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
  if (per_signal > 2147483647LL / job.lead) throw Failure("phase_vocoder: too many bin blocks for one launch");
  SMX_LAUNCH(pvoc_independent_kernel<Z>, dim3((unsigned)(per_signal * job.lead)), dim3(kThreads), 0, job.stream, a);
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
