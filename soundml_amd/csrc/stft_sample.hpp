// Device helpers shared by the generic STFT kernels (stft_generic.hip) and the constant-Q projection (cqt.hip): the ONE
// statement of the boundary rule of Stft's padded signal, and of |z|^p in the reference's rounding order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/soundml_amd.h"

namespace smx {

// sample s of the signal x[0, n) extended by `pad` (stft.ml:300-338), widened to double.  `x` is anything indexed by sample
// position: a pointer, or a view of a signal that does not lie flat in memory (the history ring of cqt_stream.hip)
template <typename Src>
__device__ inline double fetch_sample_of(Src x, int64_t n, int64_t s, int pad, double pad_value) {
  using Tin = std::decay_t<decltype(x[0])>;
  if (s >= 0 && s < n) return (double)x[s];
  if (pad == SMX_PAD_REFLECT) {  // stft.ml:300-305
    if (n == 1) return (double)x[0];
    const int64_t period = 2 * (n - 1);
    int64_t m = s % period;
    if (m < 0) m += period;
    return (double)x[m < n ? m : period - m];
  }
  if (pad == SMX_PAD_EDGE) return (double)x[s < 0 ? 0 : n - 1];
  return (double)(Tin)pad_value;   // the padded signal is built in the input dtype (stft.ml:318-338), then widened
}

template <typename Tin>
__device__ inline double fetch_sample(const Tin *x, int64_t n, int64_t s, int pad, double pad_value) {
  return fetch_sample_of(x, n, s, pad, pad_value);
}

// |z|^p with the reference's rounding order (stft.ml:670-674): the spectrum is
// rounded to the storage component type first, the magnitude is taken in the
// real dtype, then squared / kept / raised.
// kept out of line: the general power is rare and long, and the callers are unrolled 16 times
__device__ __noinline__ static float general_power_f32(float p2, float half_power) { return powf(p2, half_power); }

template <typename Tacc, typename Tout>
__device__ inline Tout magnitude_pow(Tacc re, Tacc im, double power) {
  if constexpr (sizeof(Tacc) == 4) {
    const float p2 = re * re + im * im;
    if (power == 2.0) return (Tout)p2;
    if (power == 1.0) return (Tout)sqrtf(p2);
    return (Tout)general_power_f32(p2, (float)(0.5 * power));
  } else {
    const Tout r = (Tout)re, i = (Tout)im;
    const Tout m = (Tout)sqrt((double)r * (double)r + (double)i * (double)i);
    if (power == 2.0) return m * m;
    if (power == 1.0) return m;
    return (Tout)pow((double)m, power);
  }
}

}  // namespace smx
