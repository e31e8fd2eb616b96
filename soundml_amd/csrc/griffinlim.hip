// Elementwise steps of Stft.griffin_lim (stft.ml:941-1017); the transforms between them are the library's own
// synthesis and analysis launches (griffin_lim_dev below strings them together on the caller's stream):
//   z      = S * angles                                   spectrum handed to the synthesis
//   angles = unit (c_k - a c_{k-1}),  unit e = e / (|e| + tiny)   (tiny: the smallest positive normal number,
//            which makes the map total: an exactly vanishing bin gives 0, not NaN -- stft.ml:957-960)
#include "smx_internal.hpp"

#include <cfloat>

namespace smx {
namespace {

template <typename T> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<double> { using type = double2; };

template <typename T>
__global__ void __launch_bounds__(256) gl_init_kernel(const T *phase, typename Vec2<T>::type *angles, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    typename Vec2<T>::type a;
    if (phase) {
      a.x = (T)cos((double)phase[i]);   // the reference evaluates cos / sin in float64 (stft.ml:987-988)
      a.y = (T)sin((double)phase[i]);
    } else {
      a.x = (T)1;
      a.y = (T)0;
    }
    angles[i] = a;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) gl_apply_kernel(const T *mag, const typename Vec2<T>::type *angles,
                                                       typename Vec2<T>::type *z, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const T m = mag[i];
    typename Vec2<T>::type a = angles[i];
    a.x *= m;
    a.y *= m;
    z[i] = a;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) gl_update_kernel(const typename Vec2<T>::type *rebuilt,
                                                        const typename Vec2<T>::type *previous, T beta,
                                                        typename Vec2<T>::type *angles, int64_t total) {
  const T tiny = sizeof(T) == 8 ? (T)DBL_MIN : (T)FLT_MIN;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    typename Vec2<T>::type e = rebuilt[i];
    if (previous) {
      const typename Vec2<T>::type p = previous[i];
      e.x -= beta * p.x;
      e.y -= beta * p.y;
    }
    const T m = (T)hypot((double)e.x, (double)e.y) + tiny;
    e.x /= m;
    e.y /= m;
    angles[i] = e;
  }
}

template <typename Ta, typename Tb>
__global__ void __launch_bounds__(256) gl_convert_kernel(const Ta *src, Tb *dst, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) dst[i] = (Tb)src[i];
}

// [lead][bins][frames] -> [lead][rows][pitch] (frame-major, rows >= frames, pitch >= bins): Griffin-Lim's own layout for the
// fft-2048 pipelines (griffin_lim_dev); 32 x 32 tiles through LDS, both sides coalesced
template <typename T>
__global__ void __launch_bounds__(256) gl_to_frame_major_kernel(const T *src, T *dst, int64_t bins, int64_t frames, int64_t rows, int64_t pitch) {
  __shared__ T tile[32][33];
  const int64_t clip = blockIdx.z;
  const int64_t f0 = (int64_t)blockIdx.x * 32, b0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const T *s = src + clip * bins * frames;
  T *d = dst + clip * rows * pitch;
  for (int r = ty; r < 32; r += 8)
    if (b0 + r < bins && f0 + tx < frames) tile[r][tx] = s[(b0 + r) * frames + f0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (f0 + r < frames && b0 + tx < bins) d[(f0 + r) * pitch + b0 + tx] = tile[tx][r];
}

unsigned grid_for(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 16384); }

}  // namespace

void launch_gl_widen(const float *src, double *dst, int64_t total, hipStream_t stream) {
  if (total <= 0) return;
  SMX_LAUNCH((gl_convert_kernel<float, double>), dim3(grid_for(total)), dim3(256), 0, stream, src, dst, total);
  SMX_HIP_CHECK(hipGetLastError());
}
void launch_gl_narrow(const double *src, float *dst, int64_t total, hipStream_t stream) {
  if (total <= 0) return;
  SMX_LAUNCH((gl_convert_kernel<double, float>), dim3(grid_for(total)), dim3(256), 0, stream, src, dst, total);
  SMX_HIP_CHECK(hipGetLastError());
}

void launch_gl_to_frame_major(const void *src, void *dst, int64_t lead, int64_t bins, int64_t frames, int64_t rows, int64_t pitch, int elem_bytes,
                              hipStream_t stream) {
  if (lead <= 0 || bins <= 0 || frames <= 0) return;
  if ((bins + 31) / 32 > kMaxGridYZ) throw Failure("griffin_lim: too many bins for the frame-major transposition");
  const unsigned ftiles = grid_x("griffin_lim", "frame tiles", (frames + 31) / 32, 256);
  for (int64_t c0 = 0; c0 < lead; c0 += kMaxGridYZ) {            // a clip per blockIdx.z: 65535 at a time (DESIGN.md "Launch extents")
    const dim3 grid(ftiles, (unsigned)((bins + 31) / 32), (unsigned)std::min(kMaxGridYZ, lead - c0));
    const char *s = (const char *)src + c0 * bins * frames * elem_bytes;
    char *d = (char *)dst + c0 * rows * pitch * elem_bytes;
    if (elem_bytes == 8)
      SMX_LAUNCH(gl_to_frame_major_kernel<float2>, grid, dim3(256), 0, stream, (const float2 *)s, (float2 *)d, bins, frames, rows, pitch);
    else
      SMX_LAUNCH(gl_to_frame_major_kernel<float>, grid, dim3(256), 0, stream, (const float *)s, (float *)d, bins, frames, rows, pitch);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

void launch_gl_init(const void *phase, void *angles, int64_t total, int elem_bytes, hipStream_t stream) {
  if (total <= 0) return;
  if (elem_bytes == 8)
    SMX_LAUNCH(gl_init_kernel<double>, dim3(grid_for(total)), dim3(256), 0, stream, (const double *)phase, (double2 *)angles, total);
  else
    SMX_LAUNCH(gl_init_kernel<float>, dim3(grid_for(total)), dim3(256), 0, stream, (const float *)phase, (float2 *)angles, total);
  SMX_HIP_CHECK(hipGetLastError());
}

void launch_gl_apply(const void *mag, const void *angles, void *z, int64_t total, int elem_bytes, hipStream_t stream) {
  if (total <= 0) return;
  if (elem_bytes == 8)
    SMX_LAUNCH(gl_apply_kernel<double>, dim3(grid_for(total)), dim3(256), 0, stream, (const double *)mag, (const double2 *)angles, (double2 *)z, total);
  else
    SMX_LAUNCH(gl_apply_kernel<float>, dim3(grid_for(total)), dim3(256), 0, stream, (const float *)mag, (const float2 *)angles, (float2 *)z, total);
  SMX_HIP_CHECK(hipGetLastError());
}

void launch_gl_update(const void *rebuilt, const void *previous, double beta, void *angles, int64_t total,
                      int elem_bytes, hipStream_t stream) {
  if (total <= 0) return;
  if (elem_bytes == 8)
    SMX_LAUNCH(gl_update_kernel<double>, dim3(grid_for(total)), dim3(256), 0, stream, (const double2 *)rebuilt, (const double2 *)previous, beta, (double2 *)angles, total);
  else
    SMX_LAUNCH(gl_update_kernel<float>, dim3(grid_for(total)), dim3(256), 0, stream, (const float2 *)rebuilt, (const float2 *)previous, (float)beta, (float2 *)angles, total);
  SMX_HIP_CHECK(hipGetLastError());
}

}  // namespace smx

// ---- the C ABI's side: Stft.griffin_lim ------------------------------------------------------------------------------------
namespace smx {
namespace {

// Stft.griffin_lim (stft.ml:961-1017) on device-resident data: the reference's loop, its transforms replaced by
// this library's synthesis and analysis launches, everything on `stream`.
void griffin_lim_dev(const smx_stft_config &c, const void *d_s, int elem_bytes, int64_t lead, int64_t bins,
                     int64_t frames, int64_t n_iter, double momentum, const void *d_phase, int has_length,
                     int64_t length, void *d_out, hipStream_t stream) {
  if (lead < 0 || frames < 0) throw Failure("griffin_lim: negative extent");
  check_synthesis("griffin_lim", c, bins, length, has_length != 0);   // (stft.ml:963), then the loop's own preconditions
  if (n_iter < 1)
    throw InvalidArgument(format("griffin_lim: cannot run %lld iterations (n_iter must be at least 1)", (long long)n_iter));
  if (momentum < 0.0)
    throw InvalidArgument(format("griffin_lim: cannot use a momentum of %g (momentum must be non-negative)", momentum));
  const int64_t natural = stft_output_length(c, frames);
  const int64_t out_len = has_length ? length : natural;
  if (lead == 0 || out_len == 0) return;
  if (!d_out || (frames > 0 && !d_s)) throw Failure("griffin_lim: null device pointer");
  const int64_t total = lead * bins * frames;
  if (elem_bytes == 4 && interior() == SMX_INTERIOR_F64) {
    // the reference's loop is float64 throughout whatever the dtype of s (stft.ml:977, 1017): widen, run, narrow
    double *s64 = nullptr, *p64 = nullptr, *o64 = nullptr;
    const size_t n64 = (size_t)std::max<int64_t>(total, 1) * sizeof(double);
    SMX_HIP_CHECK(smx::pool_malloc_async((void **)&s64, n64, stream));
    launch_gl_widen((const float *)d_s, s64, total, stream);
    if (d_phase) {
      SMX_HIP_CHECK(smx::pool_malloc_async((void **)&p64, n64, stream));
      launch_gl_widen((const float *)d_phase, p64, total, stream);
    }
    SMX_HIP_CHECK(smx::pool_malloc_async((void **)&o64, (size_t)lead * (size_t)out_len * sizeof(double), stream));
    griffin_lim_dev(c, s64, 8, lead, bins, frames, n_iter, momentum, p64, has_length, length, o64, stream);
    launch_gl_narrow(o64, (float *)d_out, lead * out_len, stream);
    for (void *ptr : {(void *)s64, (void *)p64, (void *)o64})
      if (ptr) SMX_HIP_CHECK(smx::pool_free_async(ptr, stream));
    return;
  }
  const int z_bytes = 2 * elem_bytes;
  void *zbuf = nullptr;
  const size_t cbytes = (size_t)std::max<int64_t>(total, 1) * (size_t)z_bytes;
  auto make_job = [&](const void *z, int has_len, int64_t len, void *out, int64_t olen) {
    IstftJob job;
    job.cfg = &c;
    job.z = z;
    job.z_bytes = z_bytes;
    job.interior = elem_bytes == 8 ? SMX_INTERIOR_F64 : interior();
    job.lead = lead;
    job.frames = frames;
    job.count = has_len ? std::min<int64_t>(frames, (len + c.left_width() + c.hop - 1) / c.hop) : frames;
    job.out_len = olen;
    job.out = out;
    job.stream = stream;
    return job;
  };
  // S * angles: multiplied in by the fused synthesis kernel as it stages the spectrum, or materialised for the others
  auto synth = [&](const void *angles_in, int has_len, int64_t len, void *out, int64_t olen) {
    IstftJob job = make_job(angles_in, has_len, len, out, olen);
    if (istft_takes_factors(job)) {
      job.mag = d_s;
    } else {
      if (!zbuf) SMX_HIP_CHECK(smx::pool_malloc_async(&zbuf, cbytes, stream));
      launch_gl_apply(d_s, angles_in, zbuf, total, elem_bytes, stream);
      job.z = zbuf;
    }
    launch_istft(job);
  };
  void *angles = nullptr, *rebuilt = nullptr, *previous = nullptr, *signal = nullptr;
  const bool iterate = natural > 0 && frames > 0;   // stft.ml:993-996
  const double beta = momentum / (1.0 + momentum);
  const bool folded = iterate && istft_takes_factors(make_job(nullptr, 0, 0, nullptr, natural));
  // Round 5 (late): the loop's spectra FRAME-MAJOR where both fft-2048 pipelines take them so -- c_k never leaves the library, so its
  // layout is free: the analysis stores a frame's bins straight from its registers (no output tile, no flush, waves that never
  // wait for each other: stft2048_complex_fm_kernel) and the synthesis stages whole rows (istft2048_pipe_kernel<.., true>).  The
  // arithmetic of every value is that of the reference-layout kernels: same bits.  SMX_GL_FRAME_MAJOR=0: the reference layout.
  bool frame_major = false;
  const int64_t fm_rows = (frames + 15) / 16 * 16, fm_pitch = 1032;   // (rows of 8256 bytes: whole 64-byte blocks)
  auto fm_analysis_job = [&](const void *x, void *out) {
    return stft_job(c, x, 4, lead, natural, natural, 0, frames, OUT_COMPLEX, 0.0, out, stream);
  };
  if (folded && elem_bytes == 4 && env_flag("SMX_GL_FRAME_MAJOR") != 0 && c.frames(natural) == frames && lead <= kMaxGridYZ) {   // (the fft-2048 analysis takes at most 65535 clips: fast_eligible)
    IstftJob probe = make_job(nullptr, 0, 0, nullptr, natural);
    probe.fm_pitch = fm_pitch;
    probe.fm_rows = fm_rows;
    frame_major = istft_frame_major_ok(probe) && launch_stft_complex_fm(fm_analysis_job(nullptr, nullptr), nullptr, 2 * fm_pitch, fm_rows, /*only_ask=*/true);
  }
  if (!frame_major || d_phase) {   // the initial angles in the reference layout (the frame-major loop without a phase fills its own)
    SMX_HIP_CHECK(smx::pool_malloc_async(&angles, cbytes, stream));
    launch_gl_init(d_phase, angles, total, elem_bytes, stream);
  }
  if (frame_major) {
    const size_t fm_elems = (size_t)lead * (size_t)fm_rows * (size_t)fm_pitch;
    void *mag_fm = nullptr, *a_fm = nullptr, *b_fm = nullptr, *c_fm = nullptr;
    SMX_HIP_CHECK(smx::pool_malloc_async(&mag_fm, fm_elems * 4, stream));
    SMX_HIP_CHECK(smx::pool_malloc_async(&a_fm, fm_elems * 8, stream));
    SMX_HIP_CHECK(smx::pool_malloc_async(&b_fm, fm_elems * 8, stream));
    SMX_HIP_CHECK(smx::pool_malloc_async(&c_fm, fm_elems * 8, stream));
    SMX_HIP_CHECK(smx::pool_malloc_async(&signal, (size_t)lead * (size_t)natural * 4, stream));
    launch_gl_to_frame_major(d_s, mag_fm, lead, bins, frames, fm_rows, fm_pitch, 4, stream);
    if (d_phase) launch_gl_to_frame_major(angles, a_fm, lead, bins, frames, fm_rows, fm_pitch, 8, stream);
    else launch_gl_init(nullptr, a_fm, (int64_t)fm_elems, 4, stream);   // (1, 0) everywhere
    auto synth_fm = [&](const void *z, const void *prev, bool unit, int has_len, int64_t len, void *out, int64_t olen) {
      IstftJob job = make_job(z, has_len, len, out, olen);
      job.mag = mag_fm;
      job.unit = unit;
      job.prev = prev;
      job.beta = beta;
      job.fm_pitch = fm_pitch;
      job.fm_rows = fm_rows;
      launch_istft(job);
    };
    void *cur = nullptr, *old = nullptr;          // c_k, c_(k-1)
    void *spare[2] = {b_fm, c_fm};
    for (int64_t k = 0; k < n_iter; ++k) {
      if (!cur) synth_fm(a_fm, nullptr, false, 0, 0, signal, natural);
      else synth_fm(cur, old, true, 0, 0, signal, natural);
      void *target = !cur ? spare[0] : (old ? old : spare[1]);
      if (!launch_stft_complex_fm(fm_analysis_job(signal, target), target, 2 * fm_pitch, fm_rows)) throw Failure("griffin_lim: the frame-major analysis refused a job it had accepted");
      old = cur;
      cur = target;
    }
    synth_fm(cur, old, true, has_length, length, d_out, out_len);
    for (void *ptr : {mag_fm, a_fm, b_fm, c_fm})
      SMX_HIP_CHECK(smx::pool_free_async(ptr, stream));
  } else if (folded) {
    // fused fft-2048 kernels: neither S * angles nor the angles themselves are materialised after the first pass --
    // the synthesis kernel forms S * unit(c_k - beta c_(k-1)) from the two latest rebuilt spectra as it stages them
    // (stft.ml:1003-1012), and the analysis of iteration k + 1 overwrites c_(k-1), which nothing reads any more
    SMX_HIP_CHECK(smx::pool_malloc_async(&rebuilt, cbytes, stream));
    SMX_HIP_CHECK(smx::pool_malloc_async(&previous, cbytes, stream));
    SMX_HIP_CHECK(smx::pool_malloc_async(&signal, (size_t)lead * (size_t)natural * (size_t)elem_bytes, stream));
    void *cur = nullptr, *old = nullptr;          // c_k, c_(k-1)
    auto synth_unit = [&](int has_len, int64_t len, void *out, int64_t olen) {
      IstftJob job = make_job(cur, has_len, len, out, olen);
      job.mag = d_s;
      job.unit = true;
      job.prev = old;
      job.beta = beta;
      launch_istft(job);
    };
    for (int64_t k = 0; k < n_iter; ++k) {
      if (!cur) synth(angles, 0, 0, signal, natural);
      else synth_unit(0, 0, signal, natural);
      void *target = !cur ? rebuilt : (old ? old : previous);
      stft_range_dev(c, signal, elem_bytes, lead, natural, natural, 0, frames, OUT_COMPLEX, 0.0, target, stream);
      old = cur;
      cur = target;
    }
    synth_unit(has_length, length, d_out, out_len);
  } else {
    if (iterate) {
      SMX_HIP_CHECK(smx::pool_malloc_async(&rebuilt, cbytes, stream));
      SMX_HIP_CHECK(smx::pool_malloc_async(&previous, cbytes, stream));
      SMX_HIP_CHECK(smx::pool_malloc_async(&signal, (size_t)lead * (size_t)natural * (size_t)elem_bytes, stream));
      bool has_prev = false;
      for (int64_t k = 0; k < n_iter; ++k) {
        synth(angles, 0, 0, signal, natural);
        stft_range_dev(c, signal, elem_bytes, lead, natural, natural, 0, frames, OUT_COMPLEX, 0.0, rebuilt, stream);
        launch_gl_update(rebuilt, has_prev ? previous : nullptr, beta, angles, total, elem_bytes, stream);
        std::swap(rebuilt, previous);   // previous <- rebuilt
        has_prev = true;
      }
    }
    synth(angles, has_length, length, d_out, out_len);
  }
  for (void *ptr : {angles, zbuf, rebuilt, previous, signal})
    if (ptr) SMX_HIP_CHECK(smx::pool_free_async(ptr, stream));
}

void griffin_lim_host(const smx_stft_config &c, const void *s, int elem_bytes, int64_t lead, int64_t bins,
                      int64_t frames, int64_t n_iter, double momentum, const void *phase, int has_length,
                      int64_t length, void *out) {
  if (lead < 0 || frames < 0) throw Failure("griffin_lim: negative extent");
  const int64_t out_len = has_length ? length : (frames >= 0 ? stft_output_length(c, frames) : 0);
  const bool run = lead > 0 && out_len > 0 && bins == c.bins() && stft_nola(c) && n_iter >= 1 && momentum >= 0.0 &&
                   !(has_length && length < 0);
  if (!run) {   // the checks (and nothing else) run without a device
    griffin_lim_dev(c, nullptr, elem_bytes, 0, bins, frames, n_iter, momentum, nullptr, has_length, length, nullptr, nullptr);
    return;
  }
  if (!out || (frames > 0 && !s)) throw Failure("griffin_lim: null pointer");
  const size_t s_clip = (size_t)bins * (size_t)frames * (size_t)elem_bytes;
  host_call("griffin_lim", {{s, s_clip}, {phase, s_clip}}, out, (size_t)out_len * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              griffin_lim_dev(c, d_in[0], elem_bytes, nc, bins, frames, n_iter, momentum, d_in[1], has_length, length, d_out, stream);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Stft.griffin_lim (stft.ml:961-1017) -----------------------------------------------------------
int smx_stft_griffin_lim_f32(const smx_stft_config *c, const float *s, int64_t lead, int64_t bins, int64_t frames,
                             int64_t n_iter, double momentum, const float *init_phase, int has_length,
                             int64_t length, float *out) {
  return guarded([&] {
    check_config(c, "griffin_lim");
    griffin_lim_host(*c, s, 4, lead, bins, frames, n_iter, momentum, init_phase, has_length, length, out);
  });
}
int smx_stft_griffin_lim_f64(const smx_stft_config *c, const double *s, int64_t lead, int64_t bins, int64_t frames,
                             int64_t n_iter, double momentum, const double *init_phase, int has_length,
                             int64_t length, double *out) {
  return guarded([&] {
    check_config(c, "griffin_lim");
    griffin_lim_host(*c, s, 8, lead, bins, frames, n_iter, momentum, init_phase, has_length, length, out);
  });
}
int smx_stft_griffin_lim_f32_dev(const smx_stft_config *c, const float *d_s, int64_t lead, int64_t bins,
                                 int64_t frames, int64_t n_iter, double momentum, const float *d_init_phase,
                                 int has_length, int64_t length, float *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "griffin_lim");
    griffin_lim_dev(*c, d_s, 4, lead, bins, frames, n_iter, momentum, d_init_phase, has_length, length, d_out,
                    (hipStream_t)stream);
  });
}

}  // extern "C"
