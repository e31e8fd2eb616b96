// What the offline projection (cqt.hip: cqt_project_kernel) and the streaming one (cqt_stream.hip:
// cqt_stream_project_kernel) share, stated ONCE: the tile geometry, the tap loop and the epilogue.  Per (frame, bin) the
// result is one fixed chain -- sums from 0, fma(sample, tap, sum) over the taps in ascending order, * gain, / divisor, one
// rounding -- so the two kernels give the same bits whatever tile a frame lands in.
#pragma once

#include "smx_internal.hpp"
#include "stft_sample.hpp"

namespace smx {

constexpr int kCqtTapTile = 32;                  // taps per LDS tile
constexpr int kCqtFrameTile = 128;               // frame slots per workgroup: 32 thread groups x 4
constexpr int kCqtBinTile = 16;                  // bins per workgroup: 8 thread lanes x 2
constexpr int kCqtRowPad = kCqtTapTile + 1;      // doubles per frame row where frames do not share samples (33: conflict-free reads)

// One staged tile of `tn` taps into the thread's 4 frames x 2 bins.  s_taps is [tap][bin]; the thread's frame r reads
// sx[r * 32 * fs + j], bins bl and bl + 8.
__device__ __forceinline__ void cqt_tile_fma(const double2 *s_taps, const double *sx, int fs, int tn, int bl, double (&re)[4][2],
                                             double (&im)[4][2]) {
  auto tap = [&](int j) {
    const double2 t0 = s_taps[j * kCqtBinTile + bl], t1 = s_taps[j * kCqtBinTile + bl + 8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = sx[r * 32 * fs + j];
      re[r][0] = fma(v, t0.x, re[r][0]);
      im[r][0] = fma(v, t0.y, im[r][0]);
      re[r][1] = fma(v, t1.x, re[r][1]);
      im[r][1] = fma(v, t1.y, im[r][1]);
    }
  };
  if (tn == kCqtTapTile) {
#pragma unroll 8
    for (int j = 0; j < kCqtTapTile; ++j) tap(j);
  } else {
    for (int j = 0; j < tn; ++j) tap(j);
  }
}

// the octave's gain, the bin's `scale` divisor, then ONE rounding: complex64, or |z|^power of the rounded value in float32
__device__ __forceinline__ void cqt_finish(double zr, double zi, double gain, const double *divisors, int64_t b, int mode, double power,
                                           void *out, int64_t at) {
  zr *= gain;
  zi *= gain;
  if (divisors) {
    const double d = divisors[b];
    zr /= d;
    zi /= d;
  }
  if (mode == OUT_COMPLEX) reinterpret_cast<float2 *>(out)[at] = make_float2((float)zr, (float)zi);
  else reinterpret_cast<float *>(out)[at] = magnitude_pow<double, float>(zr, zi, power);
}

}  // namespace smx
