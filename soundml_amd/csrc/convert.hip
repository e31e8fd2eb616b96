// The rest of Soundml.Convert (convert.ml:58-68, 104-115):
//   db_to_power / db_to_amplitude   reference * 10^(db / gain), gain 10 / 20: float64 inside, one rounding to the data's dtype
//   hz_to_midi / midi_to_hz / frames_to_time / time_to_frames   host maps over float64 values
#include "smx_internal.hpp"

namespace smx {
namespace {

// Every element is read and written by the same lane, so out may be db.
template <typename T>
__global__ void __launch_bounds__(256) from_db_kernel(const T *db, T *out, int64_t total, double gain, double reference) {
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += nthreads)
    out[i] = (T)(reference * pow(10.0, (double)db[i] / gain));
}

}  // namespace

void launch_from_db(const FromDbJob &job) {
  if (job.total <= 0) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((job.total + 255) / 256, 8192);
  if (job.elem_bytes == 8)
    SMX_LAUNCH(from_db_kernel<double>, dim3(blocks), dim3(256), 0, job.stream, (const double *)job.db, (double *)job.out, job.total,
               job.gain, job.reference);
  else
    SMX_LAUNCH(from_db_kernel<float>, dim3(blocks), dim3(256), 0, job.stream, (const float *)job.db, (float *)job.out, job.total,
               job.gain, job.reference);
  SMX_HIP_CHECK(hipGetLastError());
}

namespace {

void from_db_check(const char *fn, double reference) {   // convert.ml:3-6
  if (!(std::isfinite(reference) && reference > 0.0))
    throw InvalidArgument(format("Soundml.Convert.%s: reference must be finite and positive", fn));
}

void from_db_dev(bool amplitude, const void *d_db, int elem_bytes, int64_t total, double reference, void *d_out, hipStream_t stream) {
  const char *fn = amplitude ? "db_to_amplitude" : "db_to_power";
  from_db_check(fn, reference);
  if (total < 0) throw Failure(format("%s: negative extent", fn));
  if (total == 0) return;
  if (!d_db || !d_out) throw Failure(format("%s: null device pointer", fn));
  FromDbJob job;
  job.db = d_db;
  job.out = d_out;
  job.elem_bytes = elem_bytes;
  job.total = total;
  job.gain = amplitude ? 20.0 : 10.0;
  job.reference = reference;
  job.stream = stream;
  launch_from_db(job);
}

// in place on one device array, as to_db_host (mfcc.hip)
void from_db_host(bool amplitude, const void *db, int elem_bytes, int64_t total, double reference, void *out) {
  from_db_check(amplitude ? "db_to_amplitude" : "db_to_power", reference);
  if (total <= 0) return;
  if (!db || !out) throw Failure("from_db: null pointer");
  require_device();
  const size_t bytes = (size_t)total * (size_t)elem_bytes;
  DeviceScratch d(bytes);
  copy_to_device(d.ptr, db, bytes);
  from_db_dev(amplitude, d.ptr, elem_bytes, total, reference, d.ptr, nullptr);
  SMX_HIP_CHECK(hipStreamSynchronize(nullptr));
  copy_to_host(out, d.ptr, bytes);
}

void check_grid(const char *fn, int64_t sample_rate, int64_t hop) {   // convert.ml:18-20
  if (sample_rate < 1) throw InvalidArgument(format("Soundml.Convert.%s: sample_rate must be positive", fn));
  if (hop < 1) throw InvalidArgument(format("Soundml.Convert.%s: hop must be positive", fn));
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_db_to_power_f32(const float *db, int64_t total, double reference, float *out) {
  return guarded([&] { from_db_host(false, db, 4, total, reference, out); });
}
int smx_db_to_power_f64(const double *db, int64_t total, double reference, double *out) {
  return guarded([&] { from_db_host(false, db, 8, total, reference, out); });
}
int smx_db_to_power_f32_dev(const float *d_db, int64_t total, double reference, float *d_out, void *stream) {
  return guarded([&] { from_db_dev(false, d_db, 4, total, reference, d_out, (hipStream_t)stream); });
}
int smx_db_to_power_f64_dev(const double *d_db, int64_t total, double reference, double *d_out, void *stream) {
  return guarded([&] { from_db_dev(false, d_db, 8, total, reference, d_out, (hipStream_t)stream); });
}
int smx_db_to_amplitude_f32(const float *db, int64_t total, double reference, float *out) {
  return guarded([&] { from_db_host(true, db, 4, total, reference, out); });
}
int smx_db_to_amplitude_f64(const double *db, int64_t total, double reference, double *out) {
  return guarded([&] { from_db_host(true, db, 8, total, reference, out); });
}
int smx_db_to_amplitude_f32_dev(const float *d_db, int64_t total, double reference, float *d_out, void *stream) {
  return guarded([&] { from_db_dev(true, d_db, 4, total, reference, d_out, (hipStream_t)stream); });
}
int smx_db_to_amplitude_f64_dev(const double *d_db, int64_t total, double reference, double *d_out, void *stream) {
  return guarded([&] { from_db_dev(true, d_db, 8, total, reference, d_out, (hipStream_t)stream); });
}

// Convert.hz_to_midi / midi_to_hz (convert.ml:104-106)
int smx_hz_to_midi(const double *f, int64_t n, double *out) {
  return guarded([&] {
    if (n > 0 && (!f || !out)) throw Failure("hz_to_midi: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = std::log2(f[i] / 440.0) * 12.0 + 69.0;
  });
}
int smx_midi_to_hz(const double *m, int64_t n, double *out) {
  return guarded([&] {
    if (n > 0 && (!m || !out)) throw Failure("midi_to_hz: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = std::exp2((m[i] - 69.0) / 12.0) * 440.0;
  });
}
// Convert.frames_to_time / time_to_frames (convert.ml:108-115)
int smx_frames_to_time(int64_t sample_rate, int64_t hop, const double *frames, int64_t n, double *out) {
  return guarded([&] {
    check_grid("frames_to_time", sample_rate, hop);
    if (n > 0 && (!frames || !out)) throw Failure("frames_to_time: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = frames[i] * (double)hop / (double)sample_rate;
  });
}
int smx_time_to_frames(int64_t sample_rate, int64_t hop, const double *times, int64_t n, double *out) {
  return guarded([&] {
    check_grid("time_to_frames", sample_rate, hop);
    if (n > 0 && (!times || !out)) throw Failure("time_to_frames: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = std::floor(times[i] * (double)sample_rate / (double)hop);
  });
}

}  // extern "C"
