// pYIN's decoder: a banded Viterbi recursion over 2 n_bins states (voiced bin b = state b, unvoiced = n_bins + b) and frames, in the
// probability domain (include/soundml_amd.h words the definition).  Only *, < and a scaling by a power of two occur:
//   B = obs > FLOOR ? obs : FLOOR                          (FLOOR = 2^-200; a NaN is the floor)
//   delta_0 = p_init B_0, p_init = 1 / n_bins on the unvoiced states and 0 on the voiced
//   per frame: u[i] = (delta[i] 2^-e) rs[i], e the binary exponent of the greatest delta;  M_v(j) the greatest u_v[i] tri[j - i + h]
//   over the band's i in ascending order (strictly greater replaces: the smallest i wins ties);  a = M_v(j) (1 - switch_prob),
//   b = M_{1-v}(j) switch_prob, b taken only if b > a;  delta_t(v, j) = taken B_t(v, j), the back pointer the taken (v', i)
//   the end: the smallest state of the greatest delta_{T-1}; the walk back follows the pointers
// The observation is dense (pyin_decode: float32 or float64 [2 n_bins; frames]) or pyin's sparse float64 one: per frame the unvoiced
// states' value and the occupied voiced bins, which the workgroup scatters into a double-buffered LDS row of floors and takes out again.
//
//   pyin_decode_kernel<J>   a workgroup per clip.  delta and u in LDS, u with a halo of NaN on both sides (a NaN candidate is never
//                           greater, so neither the halo nor a lag outside the band needs an index test); a lane owns J consecutive
//                           bins of both voicings and slides them across the sources from registers: per source one LDS read of
//                           u_0[i] and u_1[i] serves 2 J candidates, and the triangle's value is the same in every lane (a scalar).
//                           The frame's greatest delta is one workgroup reduction, carried into the next frame's scale.  Back pointers
//                           go to stream-ordered scratch, 8 bits (offset in the band and a switch bit) where 2 h + 1 <= 128, else the
//                           16-bit source state.  Every loop's trip count is fixed by the shapes; ordering is __syncthreads() only.
//   pyin_path_kernel        a wave per clip: blocks of frames of the pointers staged in LDS by the whole wave, lane 0 walks a block,
//                           then the wave writes that block's results
// The kernel's LDS (6 n_bins + 4 min(h, n_bins - 1) + 8 doubles) caps the shapes it takes: past it the call is an argument error.
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kMaxRun = 3;                       // most consecutive bins of a lane: the LDS cap keeps n_bins below 3 x 1024
constexpr int kPad = 4;                          // NaNs on each side of the band's triangle: kMaxRun of them are read
constexpr int64_t kDecodeLds = 160 * 1024 - 16 * 1024;   // dynamic LDS of the decoder; the rest is its reduction's
constexpr int64_t kScratchBytes = 512ll << 20;   // back pointers of one launch; larger calls go clip range by clip range
constexpr int kStageBytes = 64 * 1024;           // back pointers of one block of the walk back
constexpr double kFloor = 0x1p-200;

struct DecodeArgs {
  const void *obs;
  const double *ext, *rs;                        // tri[k], k = h - heff - kPad .. h + heff + kPad (NaN outside [0, 2 h]); rs[i]
  unsigned char *back;                           // [clip][frame][pitch bytes]
  int *end;                                      // [clip]
  int64_t clip_stride, state_stride, frame_stride, frames, back_clip, back_pitch;
  double sp, keep;                               // switch_prob, 1 - switch_prob
  int obs_bytes, n_bins, h, heff, wide;          // wide: 16-bit pointers
  const double *rest, *value;                    // obs null: the sparse observation, frame f = clip frames + t: rest[f], count[f] and
  const int *count, *bin;                        // bin / value [f list + k]
  int64_t list;
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double other = __shfl_xor(v, o);
    v = other > v ? other : v;
  }
  return v;
}

template <int J>
__global__ void __launch_bounds__(1024) pyin_decode_kernel(DecodeArgs a) {
  extern __shared__ __align__(16) unsigned char decode_lds[];
  __shared__ double wmax[16], redv[1024];
  __shared__ int redi[1024];
  const int tid = threadIdx.x, nt = blockDim.x, nb = a.n_bins, S = 2 * nb, heff = a.heff, LU = nb + 2 * heff + kPad;
  const int64_t clip = blockIdx.x;
  double *d = reinterpret_cast<double *>(decode_lds), *U0 = d + S, *U1 = U0 + LU;   // u_v[i] at U_v[i + heff]
  double *Bv = U1 + LU;                                     // sparse: the voiced observation of frame t in Bv[(t & 1) nb ..]
  const bool sparse = a.obs == nullptr;
  auto floored = [](double v) { return v > kFloor ? v : kFloor; };
  auto B = [&](int s, int64_t t) {
    const int64_t at = clip * a.clip_stride + (int64_t)s * a.state_stride + t * a.frame_stride;
    const double v = a.obs_bytes == 8 ? reinterpret_cast<const double *>(a.obs)[at] : (double)reinterpret_cast<const float *>(a.obs)[at];
    return floored(v);
  };
  const double nan = __builtin_nan("");
  for (int i = tid; i < 2 * LU; i += nt) U0[i] = nan;
  if (sparse)
    for (int i = tid; i < S; i += nt) Bv[i] = kFloor;
  const double p_init = 1.0 / (double)nb;
  double local = 0.0;                                       // no delta is negative
  for (int s = tid; s < S; s += nt) {
    const double v = (s < nb ? 0.0 : p_init) * (sparse ? floored(a.rest[clip * a.frames]) : B(s, 0));
    d[s] = v;
    local = v > local ? v : local;
  }
  local = wave_max(local);
  if ((tid & 63) == 0) wmax[tid >> 6] = local;
  __syncthreads();

  for (int64_t t = 1; t < a.frames; ++t) {
    double m = wmax[0];
    for (int wv = 1; wv < (nt >> 6); ++wv) m = wmax[wv] > m ? wmax[wv] : m;
    int e = 0;
    (void)frexp(m, &e);
    const double scale = ldexp(1.0, -e);
    for (int s = tid; s < S; s += nt) {
      const int i = s < nb ? s : s - nb;
      (s < nb ? U0 : U1)[i + heff] = (d[s] * scale) * a.rs[i];
    }
    const double *cur = Bv + (t & 1) * nb;
    double rest = 0.0;
    if (sparse) {
      // this frame's occupied bins into its buffer; the frame before's out of the other one, which nobody reads any more
      const int64_t f = clip * a.frames + t;
      rest = floored(a.rest[f]);
      if (t >= 2) {
        const int64_t n0 = a.count[f - 1] < a.list ? a.count[f - 1] : a.list;
        for (int64_t k = tid; k < n0; k += nt) Bv[((t - 1) & 1) * nb + a.bin[(f - 1) * a.list + k]] = kFloor;
      }
      const int64_t n1 = a.count[f] < a.list ? a.count[f] : a.list;
      for (int64_t k = tid; k < n1; k += nt) Bv[(t & 1) * nb + a.bin[f * a.list + k]] = floored(a.value[f * a.list + k]);
    }
    __syncthreads();                                        // u is whole, and wmax has been read by everyone

    unsigned char *row = a.back + clip * a.back_clip + t * a.back_pitch;
    local = 0.0;
    for (int j0 = tid * J; j0 < nb; j0 += nt * J) {
      double b0[J], b1[J], w[J], B0[J], B1[J];
      int a0[J], a1[J];
#pragma unroll
      for (int jj = 0; jj < J; ++jj) {
        const int j = j0 + jj < nb ? j0 + jj : nb - 1;
        B0[jj] = sparse ? cur[j] : B(j, t);
        B1[jj] = sparse ? rest : B(nb + j, t);
        b0[jj] = b1[jj] = -HUGE_VAL;
        a0[jj] = a1[jj] = j;
        w[jj] = a.ext[jj + 2 * heff + kPad];                // source j0 - heff: k = jj + heff + h
      }
      const double *u0 = U0 + j0, *u1 = U1 + j0;
      for (int step = 0; step < J + 2 * heff; ++step) {     // source i = j0 - heff + step
        const double x0 = u0[step], x1 = u1[step];
        const int i = j0 - heff + step;
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
          const double c0 = x0 * w[jj], c1 = x1 * w[jj];
          if (c0 > b0[jj]) b0[jj] = c0, a0[jj] = i;
          if (c1 > b1[jj]) b1[jj] = c1, a1[jj] = i;
        }
#pragma unroll
        for (int jj = J - 1; jj >= 1; --jj) w[jj] = w[jj - 1];
        w[0] = a.ext[2 * heff + kPad - 1 - step];
      }
#pragma unroll
      for (int jj = 0; jj < J; ++jj) {
        const int j = j0 + jj;
        if (j >= nb) break;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const double stay = (v ? b1[jj] : b0[jj]) * a.keep, change = (v ? b0[jj] : b1[jj]) * a.sp;
          const bool sw = change > stay;
          const int from = sw ? (v ? a0[jj] : a1[jj]) : (v ? a1[jj] : a0[jj]), fv = sw ? 1 - v : v;
          const double dv = (sw ? change : stay) * (v ? B1[jj] : B0[jj]);
          const int s = v * nb + j;
          d[s] = dv;
          local = dv > local ? dv : local;
          if (a.wide) reinterpret_cast<unsigned short *>(row)[s] = (unsigned short)(fv * nb + from);
          else row[s] = (unsigned char)((from - j + a.h) | (sw ? 0x80 : 0));
        }
      }
    }
    local = wave_max(local);
    if ((tid & 63) == 0) wmax[tid >> 6] = local;
    __syncthreads();                                        // delta is whole
  }

  // the smallest state of the greatest delta
  double best = d[tid < S ? tid : 0];
  int at = tid < S ? tid : S;
  if (tid >= S) best = -HUGE_VAL;
  for (int s = tid + nt; s < S; s += nt)
    if (d[s] > best) best = d[s], at = s;
  redv[tid] = best;
  redi[tid] = at;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < nt; ++k)
      if (redv[k] > best || (redv[k] == best && redi[k] < at)) best = redv[k], at = redi[k];
    a.end[clip] = at;
  }
}

struct PathArgs {
  const unsigned char *back;
  const int *end;
  const double *freq;
  void *states, *f0, *flag;
  int64_t frames, back_clip, back_pitch;
  double fill;
  int n_bins, h, wide, block, keep_bin;          // block: frames per staged block
};

template <typename T>
__global__ void __launch_bounds__(64) pyin_path_kernel(PathArgs a) {
  extern __shared__ __align__(16) unsigned char path_lds[];
  const int lane = threadIdx.x, nb = a.n_bins, S = 2 * nb;
  const int64_t clip = blockIdx.x;
  uint4 *rows = reinterpret_cast<uint4 *>(path_lds);
  int *path = reinterpret_cast<int *>(path_lds + (size_t)a.block * a.back_pitch);
  int s = a.end[clip];                                      // lane 0 carries it from block to block
  s = s < 0 ? 0 : s >= S ? S - 1 : s;
  for (int64_t hi = a.frames; hi > 0; hi -= a.block) {
    const int64_t lo = hi > a.block ? hi - a.block : 0;
    const int count = (int)(hi - lo);
    __syncthreads();
    // frame 0 has no pointers: its row is not read
    const int64_t first = lo > 1 ? lo : 1;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.back + clip * a.back_clip + first * a.back_pitch);
    const int64_t vecs = (hi - first) * (a.back_pitch / 16), skip = (first - lo) * (a.back_pitch / 16);
    for (int64_t v = lane; v < vecs; v += 64) rows[skip + v] = src[v];
    __syncthreads();
    if (lane == 0) {
      for (int64_t t = hi - 1; t >= lo; --t) {
        path[t - lo] = s;
        if (t == 0) break;
        const unsigned char *row = path_lds + (size_t)(t - lo) * a.back_pitch;
        if (a.wide) {
          s = reinterpret_cast<const unsigned short *>(row)[s];
        } else {
          const int code = row[s], v = s >= nb ? 1 : 0, j = s - v * nb;
          s = ((code >> 7) ? 1 - v : v) * nb + j + (code & 0x7f) - a.h;
        }
        s = s < 0 ? 0 : s >= S ? S - 1 : s;                 // (a pointer written by the decoder is in range)
      }
    }
    __syncthreads();
    for (int k = lane; k < count; k += 64) {
      const int st = path[k];
      const int64_t o = clip * a.frames + lo + k;
      if (a.states) {
        reinterpret_cast<T *>(a.states)[o] = (T)st;
      } else {
        const bool voiced = st < nb;
        const double f = a.freq[voiced ? st : st - nb];
        reinterpret_cast<T *>(a.f0)[o] = voiced || a.keep_bin ? (T)f : (T)a.fill;
        reinterpret_cast<T *>(a.flag)[o] = voiced ? (T)1 : (T)0;
      }
    }
  }
}

int64_t effective_width(int64_t n_bins, int64_t h) { return std::min(h, n_bins - 1); }
int64_t pointer_pitch(int64_t n_bins, int64_t h) { return ((2 * n_bins * (2 * h + 1 <= 128 ? 1 : 2) + 15) / 16) * 16; }

// tri around the band with NaNs outside it, then rs
std::shared_ptr<void> decode_table(int64_t n_bins, int64_t h) {
  return cached_table(format("pyin_decode|%lld|%lld", (long long)n_bins, (long long)h), [&] {
    const int64_t heff = effective_width(n_bins, h), m = 2 * heff + 1 + 2 * kPad;
    std::vector<double> all((size_t)(m + n_bins));
    for (int64_t i = 0; i < m; ++i) all[(size_t)i] = i >= kPad && i < m - kPad ? pyin_triangle(i - kPad + (h - heff), h) : std::nan("");
    pyin_band_scale(n_bins, h, all.data() + m);
    std::vector<unsigned char> out(all.size() * sizeof(double));
    std::memcpy(out.data(), all.data(), out.size());
    return out;
  });
}

// the run of a lane: the shortest that covers the bins with one workgroup of 1024 lanes.  More waves beat longer runs: at 602 bins and
// h = 50 a run of 1 (10 waves) decodes 256 clips x 431 frames in 6.3 ms, a run of 3 (4 waves, one per SIMD, nothing to hide the LDS
// reads behind) in 12.8 ms (profiles/pitch/NOTES.md).  SMX_DISABLE_FAST=1: always 1, the same bits (tests).
int choose_run(int64_t n_bins) {
  if (fast_path_disabled()) return 1;
  return (int)std::min<int64_t>(kMaxRun, (n_bins + 1023) / 1024);
}

}  // namespace

double pyin_triangle(int64_t k, int64_t h) { return 1.0 - std::fabs((double)(k - h)) / (double)(h + 1); }

void pyin_band_scale(int64_t n_bins, int64_t h, double *rs) {
  for (int64_t i = 0; i < n_bins; ++i) {
    double sum = 0.0;
    for (int64_t j = std::max<int64_t>(0, i - h); j <= std::min(n_bins - 1, i + h); ++j) sum = sum + pyin_triangle(j - i + h, h);
    rs[i] = 1.0 / sum;
  }
}

void check_pyin_decode(const char *fn, int64_t n_bins, int64_t half_width, double switch_prob) {
  if (half_width < 0)
    throw InvalidArgument(format("%s: cannot decode with a transition half-width of %lld bins (half_width must not be negative)", fn, (long long)half_width));
  if (!(switch_prob >= 0.0 && switch_prob <= 1.0))
    throw InvalidArgument(format("%s: cannot switch voicing with probability %g (switch_prob must lie in [0, 1])", fn, switch_prob));
  if (n_bins < 1) return;
  if (2 * n_bins > 65535)
    throw InvalidArgument(format("%s: cannot decode %lld states (2 n_bins must be at most 65535)", fn, (long long)(2 * n_bins)));
  const int64_t cap = kDecodeLds / 16 - 4;
  if (3 * n_bins + 2 * effective_width(n_bins, half_width) > cap)
    throw InvalidArgument(format("%s: cannot decode %lld pitch bins with a transition half-width of %lld (3 n_bins + 2 min(half_width, n_bins - 1) must be at most %lld)",
                                 fn, (long long)n_bins, (long long)half_width, (long long)cap));
}

int64_t pyin_decode_scratch(int64_t frames, int64_t n_bins, int64_t half_width) { return frames * pointer_pitch(n_bins, half_width) + 16; }

void launch_pyin_decode(const PyinDecodeJob &job) {
  if (job.lead == 0 || job.frames == 0) return;
  const int64_t nb = job.n_bins, h = job.half_width, heff = effective_width(nb, h), pitch = pointer_pitch(nb, h);
  if (job.frames > (int64_t)1 << 40) throw Failure(format("%s: too many frames or clips", job.fn));
  const auto table = decode_table(nb, h);
  const int64_t per_clip = job.frames * pitch + 16;
  const int64_t step = std::max<int64_t>(1, std::min({job.lead, kScratchBytes / per_clip, clips_per_launch(1, 1024)}));   // a workgroup of at most 1024 per clip
  init_device_pool();
  DeviceScratch scratch;
  scratch.pool((size_t)(step * per_clip), job.stream);
  DecodeArgs a{};
  a.ext = reinterpret_cast<const double *>(table.get());
  a.rs = a.ext + 2 * heff + 1 + 2 * kPad;
  a.back = scratch.as<unsigned char>();
  a.end = reinterpret_cast<int *>(a.back + step * job.frames * pitch);
  a.clip_stride = job.clip_stride, a.state_stride = job.state_stride, a.frame_stride = job.frame_stride;
  a.frames = job.frames, a.back_clip = job.frames * pitch, a.back_pitch = pitch;
  a.sp = job.switch_prob, a.keep = 1.0 - job.switch_prob;
  a.obs_bytes = job.obs_bytes, a.n_bins = (int)nb, a.h = (int)std::min<int64_t>(h, 1 << 20), a.heff = (int)heff, a.wide = 2 * h + 1 <= 128 ? 0 : 1;
  const int J = choose_run(nb);
  const int64_t runs = (nb + J - 1) / J;
  const int threads = (int)std::min<int64_t>(1024, ((runs + 63) / 64) * 64);
  const size_t lds = (size_t)(4 * nb + 2 * (nb + 2 * heff + kPad)) * sizeof(double);
  PathArgs p{};
  p.back = a.back, p.end = a.end, p.freq = job.d_freq;
  p.frames = job.frames, p.back_clip = a.back_clip, p.back_pitch = pitch;
  p.fill = job.fill;
  p.n_bins = (int)nb, p.h = a.h, p.wide = a.wide, p.keep_bin = job.keep_bin ? 1 : 0;
  p.block = (int)std::max<int64_t>(1, std::min<int64_t>(job.frames, kStageBytes / pitch));
  const size_t path_lds = (size_t)p.block * (size_t)pitch + (size_t)p.block * sizeof(int);
  for (int64_t c0 = 0; c0 < job.lead; c0 += step) {
    const int64_t nc = std::min(step, job.lead - c0);
    a.obs = job.d_obs ? (const char *)job.d_obs + c0 * job.clip_stride * job.obs_bytes : nullptr;
    if (!job.d_obs) {
      a.rest = job.d_rest + c0 * job.frames, a.count = job.d_count + c0 * job.frames;
      a.value = job.d_value + c0 * job.frames * job.list, a.bin = job.d_bin + c0 * job.frames * job.list;
      a.list = job.list;
    }
    switch (J) {
      case 1: launch_tiles(job.fn, pyin_decode_kernel<1>, nc, threads, lds, job.stream, a); break;
      case 2: launch_tiles(job.fn, pyin_decode_kernel<2>, nc, threads, lds, job.stream, a); break;
      default: launch_tiles(job.fn, pyin_decode_kernel<3>, nc, threads, lds, job.stream, a); break;
    }
    const int64_t o = c0 * job.frames * job.elem_bytes;
    p.states = job.d_states ? (char *)job.d_states + o : nullptr;
    p.f0 = job.d_f0 ? (char *)job.d_f0 + o : nullptr;
    p.flag = job.d_flag ? (char *)job.d_flag + o : nullptr;
    if (job.elem_bytes == 8) launch_tiles(job.fn, pyin_path_kernel<double>, nc, 64, path_lds, job.stream, p);
    else launch_tiles(job.fn, pyin_path_kernel<float>, nc, 64, path_lds, job.stream, p);
  }
}

namespace {

void decode_call(bool device, const void *obs, int elem_bytes, int64_t lead, int64_t states, int64_t frames, int64_t clip_stride, int64_t half_width,
                 double switch_prob, void *out, hipStream_t stream) {
  const char *fn = "pyin_decode";
  const bool probe = !obs && lead == 0 && states == 0 && frames == 0;   // null data and zero extents: the parameters only
  if (!probe && (states < 2 || states % 2))
    throw InvalidArgument(format("%s: cannot decode a state axis of %lld (the state axis must be even and positive)", fn, (long long)states));
  check_pyin_decode(fn, states / 2, half_width, switch_prob);
  if (lead < 0 || frames < 0) throw Failure(format("%s: negative extent", fn));
  if (lead == 0 || frames == 0) return;
  if (device && clip_stride < states * frames) throw Failure(format("%s: clip_stride is smaller than a clip's observation", fn));
  if (!obs || !out) throw Failure(format("%s: null pointer", fn));
  PyinDecodeJob job{};
  job.fn = fn;
  job.obs_bytes = job.elem_bytes = elem_bytes;
  job.state_stride = frames, job.frame_stride = 1;
  job.frames = frames, job.n_bins = states / 2, job.half_width = half_width;
  job.switch_prob = switch_prob;
  if (device) {
    job.d_obs = obs, job.clip_stride = clip_stride, job.lead = lead, job.d_states = out, job.stream = stream;
    launch_pyin_decode(job);
    return;
  }
  host_call(fn, {{obs, (size_t)states * (size_t)frames * (size_t)elem_bytes}}, out, (size_t)frames * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t st) {
              PyinDecodeJob part = job;
              part.d_obs = d_in[0], part.clip_stride = states * frames, part.lead = nc, part.d_states = d_out, part.stream = st;
              launch_pyin_decode(part);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_pyin_decode_f32(const float *obs, int64_t lead, int64_t states, int64_t frames, int64_t half_width, double switch_prob, float *out) {
  return guarded([&] { decode_call(false, obs, 4, lead, states, frames, states * frames, half_width, switch_prob, out, nullptr); });
}
int smx_pyin_decode_f64(const double *obs, int64_t lead, int64_t states, int64_t frames, int64_t half_width, double switch_prob, double *out) {
  return guarded([&] { decode_call(false, obs, 8, lead, states, frames, states * frames, half_width, switch_prob, out, nullptr); });
}
int smx_pyin_decode_accel_f32(const float *d_obs, int64_t lead, int64_t states, int64_t frames, int64_t clip_stride, int64_t half_width,
                              double switch_prob, float *d_out, void *stream) {
  return guarded([&] { decode_call(true, d_obs, 4, lead, states, frames, clip_stride, half_width, switch_prob, d_out, (hipStream_t)stream); });
}

}  // extern "C"
