// Mel.invert (DESIGN.md "Mel inversion"): per frame the non-negative spectrum s that approaches min |W s - m|_2,
// by n_iter rounds of accelerated projected gradient from s = y = 0, in the data's own dtype T:
//   r_j  = fma chain over the row's band, ascending bins, from -m_j          (W_T y - m)
//   g_k  = W_T[j0,k] r_j0, then fma (W_T[j1,k], r_j1, .) when a second row touches the bin   (W_T^T r)
//   s+_k = max (0, fma (-eta, g_k, y_k)),   y+_k = fma (beta, s+_k - s_k, s+_k)
// eta = 1 / L rounded to T, L = max_j sum_i |(W W^T)_ji| (Gershgorin) over the float64 weights; beta_k from
// t_0 = 1, t_{k+1} = (1 + sqrt (1 + 4 t_k^2)) / 2, beta_k = (t_k - 1) / t_{k+1}, float64 on the host, rounded to T.
// A bin of Config.create's triangles lies in at most two filters, so W^T r is two terms per bin and W y walks 2 nnz(W) / n
// values per row; every round is ~4 bins words of LDS traffic and no memory traffic at all.
//
// Two kernels of one contract (the same bits: both call row_residual / bin_update on the same tables):
//   wave kernel     one wave per frame, eight frames per workgroup.  s, y and the bin's two weights in registers, bin
//                   b * 64 + lane in slot b; y mirrored in LDS for the rows' gathers, r left in LDS for the bins; the
//                   tables (row weights lane-interleaved, row list, 256 betas at a time) in LDS, shared by the eight
//                   frames.  m is read once, s written once through an LDS transposition (8 frames contiguous per bin row).
//                   30.7 ms for 110 336 frames x 200 rounds at fft 2048 / 128 mels, bound by the vector instruction issue
//                   (profiles/inversion/NOTES.md).
//   general kernel  one workgroup per frame, s / y / r in a scratch array, tables read from memory: any bin count,
//                   any mel count.  SMX_DISABLE_FAST selects it.
// The file is built with contraction off: a product and a sum fuse only where the source says fma.
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

template <typename T> struct BinItem {
  T w0, w1;
  int j0, j1;   // j0 = -1: no filter touches the bin; j1 = -1: one filter
};

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// w: the row's weights 64 words apart (the tables are lane-interleaved).  Eight weights and eight values are requested together,
// then their multiply-adds run in order: the chain waits for one round trip per eight terms, and the requests of a batch are one
// base address with constant offsets.  A batch may reach up to kGatherSlack - 1 terms past the row's band; both tables are
// readable there (the slots' weights are padded to whole batches, y is followed by kGatherSlack words) and nothing read there is
// used.  (One term at a time, clamped indices: 42.6 and 42.3 ms on 256 clips x 431 frames x 200 rounds.)
constexpr int kGatherSlack = 8;
template <typename T>
__device__ __forceinline__ T row_residual(const T *w, const T *y, int len, T m) {
  constexpr int U = kGatherSlack;
  T acc = -m;
  for (int q0 = 0; q0 < len; q0 += U) {
    T wv[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      wv[u] = w[(q0 + u) * 64];
      yv[u] = y[q0 + u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (q0 + u < len) acc = fma_t(wv[u], yv[u], acc);
  }
  return acc;
}

template <typename T>
__device__ __forceinline__ void bin_update(T w0, T w1, T r0, T r1, bool two, T eta, T beta, T &s, T &y) {
  T g = w0 * r0;
  if (two) g = fma_t(w1, r1, g);
  T sn = fma_t(-eta, g, y);
  sn = sn > (T)0 ? sn : (T)0;
  y = fma_t(beta, sn - s, sn);
  s = sn;
}

enum { ROOT_NONE = 0, ROOT_SQRT = 1, ROOT_POW = 2 };
template <typename T>
__device__ __forceinline__ T rooted(T s, int mode, double inv_root) {
  if (mode == ROOT_NONE) return s;
  if (mode == ROOT_SQRT) return (T)sqrt((double)s);
  return (T)pow((double)s, inv_root);
}

struct InvArgs {
  const void *m;
  void *out;
  const void *w_rows;
  const int4 *rows;
  const void *bins;
  const void *beta;     // T [n_iter]
  void *scratch;        // general kernel: T [launch frames][2 nbins + n_mels + kGatherSlack]: y | s | r
  int64_t frames, total, first;   // total = lead * frames; first: the launch's first frame (general kernel)
  int n_mels, nbins, slots, nnz, n_iter;
  double eta;
  int root_mode;
  double inv_root;
};

constexpr int kFrames = 8;         // frames (waves) per workgroup of the wave kernel
constexpr int kBetaChunk = 256;
constexpr int kYPad = 8;           // the transposed read of the final store: 8 frames x 8 bins on 64 different banks; >= kGatherSlack

// LDS of the wave kernel, in bytes from the start: rows | w | beta | y [8][ypitch] | m [8][n_mels] | r [8][n_mels]
struct WaveLds {
  size_t w, beta, y, m, r, bytes;
  int ypitch;
};
template <typename T>
__host__ __device__ inline WaveLds wave_lds(int slots, int nnz, int n_mels, int nb) {
  WaveLds l;
  l.ypitch = 64 * nb + kYPad;
  l.w = (size_t)slots * 64 * sizeof(int4);
  l.beta = l.w + (size_t)((nnz + 3) & ~3) * sizeof(T);
  l.y = l.beta + kBetaChunk * sizeof(T);
  l.m = l.y + (size_t)kFrames * l.ypitch * sizeof(T);
  l.r = l.m + (size_t)kFrames * n_mels * sizeof(T);
  l.bytes = l.r + (size_t)kFrames * n_mels * sizeof(T);
  return l;
}

// the lanes of ONE wave exchange y and r through LDS: the wave's LDS operations execute in order, the fences keep the
// compiler from moving them across the exchange
__device__ __forceinline__ void wave_exchange() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, int NB>
__global__ void __launch_bounds__(64 * kFrames) mel_invert_wave_kernel(InvArgs a) {
  extern __shared__ int4 lds_raw[];
  char *lds = reinterpret_cast<char *>(lds_raw);
  const WaveLds l = wave_lds<T>(a.slots, a.nnz, a.n_mels, NB);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 *rows_s = lds_raw;
  T *w_s = reinterpret_cast<T *>(lds + l.w);
  T *beta_s = reinterpret_cast<T *>(lds + l.beta);
  T *y_all = reinterpret_cast<T *>(lds + l.y);
  T *y_s = y_all + wave * l.ypitch;
  T *m_s = reinterpret_cast<T *>(lds + l.m) + wave * a.n_mels;
  T *r_s = reinterpret_cast<T *>(lds + l.r) + wave * a.n_mels;

  for (int i = tid; i < a.slots * 64; i += 64 * kFrames) rows_s[i] = a.rows[i];
  for (int i = tid; i < a.nnz; i += 64 * kFrames) w_s[i] = reinterpret_cast<const T *>(a.w_rows)[i];
  // this wave's frame (a wave past the last frame works on the last one and stores nothing)
  const int64_t g0 = (int64_t)blockIdx.x * kFrames;
  {
    const int64_t g = g0 + wave < a.total ? g0 + wave : a.total - 1;
    const int64_t clip = g / a.frames, t = g - clip * a.frames;
    const T *m = reinterpret_cast<const T *>(a.m) + clip * a.n_mels * a.frames + t;
    for (int j = lane; j < a.n_mels; j += 64) m_s[j] = m[(int64_t)j * a.frames];
    for (int k = lane; k < l.ypitch; k += 64) y_s[k] = (T)0;
  }
  T s[NB], y[NB], w0[NB], w1[NB];
  int j0[NB], j1[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int k = b * 64 + lane;
    s[b] = y[b] = w0[b] = w1[b] = (T)0;
    j0[b] = j1[b] = -1;
    if (k < a.nbins) {
      const BinItem<T> it = reinterpret_cast<const BinItem<T> *>(a.bins)[k];
      w0[b] = it.w0;
      w1[b] = it.w1;
      j0[b] = it.j0;
      j1[b] = it.j1;
    }
  }
  const T eta = (T)a.eta;
  for (int k0 = 0; k0 < a.n_iter; k0 += kBetaChunk) {
    __syncthreads();   // the tables are in place; every wave is done with the previous betas
    if (tid < kBetaChunk && k0 + tid < a.n_iter) beta_s[tid] = reinterpret_cast<const T *>(a.beta)[k0 + tid];
    __syncthreads();
    const int kn = a.n_iter - k0 < kBetaChunk ? a.n_iter - k0 : kBetaChunk;
    for (int kk = 0; kk < kn; ++kk) {
      const T beta = beta_s[kk];
      for (int i = 0; i < a.slots; ++i) {   // lanes over mel rows
        const int4 rw = rows_s[i * 64 + lane];
        if (rw.x >= 0) r_s[rw.x] = row_residual<T>(w_s + rw.w, y_s + rw.y, rw.z, m_s[rw.x]);
      }
      wave_exchange();
#pragma unroll
      for (int b = 0; b < NB; ++b)          // lanes over their own bins
        if (j0[b] >= 0) {
          const T r0 = r_s[j0[b]];
          const T r1 = j1[b] >= 0 ? r_s[j1[b]] : (T)0;
          bin_update<T>(w0[b], w1[b], r0, r1, j1[b] >= 0, eta, beta, s[b], y[b]);
          y_s[b * 64 + lane] = y[b];
        }
      wave_exchange();
    }
  }
  // the result through the y mirror: a bin row's eight frames leave together
#pragma unroll
  for (int b = 0; b < NB; ++b) y_s[b * 64 + lane] = rooted<T>(s[b], a.root_mode, a.inv_root);
  __syncthreads();
  const int f = tid & (kFrames - 1);
  const int64_t g = g0 + f;
  if (g >= a.total) return;
  const int64_t clip = g / a.frames, t = g - clip * a.frames;
  T *out = reinterpret_cast<T *>(a.out) + clip * a.nbins * a.frames + t;
  for (int k = tid / kFrames; k < a.nbins; k += 64) out[(int64_t)k * a.frames] = y_all[f * l.ypitch + k];
}

template <typename T>
__global__ void __launch_bounds__(256) mel_invert_general_kernel(InvArgs a) {
  const int tid = threadIdx.x;
  const int64_t g = a.first + blockIdx.x;
  const int64_t clip = g / a.frames, t = g - clip * a.frames;
  const T *m = reinterpret_cast<const T *>(a.m) + clip * a.n_mels * a.frames + t;
  T *out = reinterpret_cast<T *>(a.out) + clip * a.nbins * a.frames + t;
  T *y = reinterpret_cast<T *>(a.scratch) + (int64_t)blockIdx.x * (2 * (int64_t)a.nbins + a.n_mels + kGatherSlack);
  T *s = y + a.nbins, *r = s + a.nbins;
  const T *w = reinterpret_cast<const T *>(a.w_rows);
  const BinItem<T> *bins = reinterpret_cast<const BinItem<T> *>(a.bins);
  for (int k = tid; k < a.nbins; k += 256) y[k] = s[k] = (T)0;
  __syncthreads();
  const T eta = (T)a.eta;
  for (int it = 0; it < a.n_iter; ++it) {
    const T beta = reinterpret_cast<const T *>(a.beta)[it];
    for (int e = tid; e < a.slots * 64; e += 256) {
      const int4 rw = a.rows[e];
      if (rw.x >= 0) r[rw.x] = row_residual<T>(w + rw.w, y + rw.y, rw.z, m[(int64_t)rw.x * a.frames]);
    }
    __syncthreads();
    for (int k = tid; k < a.nbins; k += 256) {
      const BinItem<T> b = bins[k];
      if (b.j0 >= 0) {
        T sk = s[k], yk = y[k];
        bin_update<T>(b.w0, b.w1, r[b.j0], b.j1 >= 0 ? r[b.j1] : (T)0, b.j1 >= 0, eta, beta, sk, yk);
        s[k] = sk;
        y[k] = yk;
      }
    }
    __syncthreads();
  }
  for (int k = tid; k < a.nbins; k += 256) out[(int64_t)k * a.frames] = rooted<T>(s[k], a.root_mode, a.inv_root);
}

// beta_k rounded to T, device resident, as many as any call has asked for (they depend on k alone)
struct BetaTable {
  void *dev = nullptr;
  int64_t count = 0;
};
std::mutex g_beta_mutex;
std::map<std::pair<int, int>, BetaTable> g_beta;   // (device, element bytes)

const void *beta_table(int elem_bytes, int64_t n_iter) {
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_beta_mutex);
  BetaTable &t = g_beta[{device, elem_bytes}];
  if (t.count >= n_iter && t.dev) return t.dev;
  const int64_t count = std::max<int64_t>(1024, 2 * n_iter);
  std::vector<double> beta((size_t)count);
  double tk = 1.0;
  for (int64_t k = 0; k < count; ++k) {
    const double next = (1.0 + std::sqrt(1.0 + 4.0 * tk * tk)) / 2.0;
    beta[(size_t)k] = (tk - 1.0) / next;
    tk = next;
  }
  void *dev = nullptr;
  SMX_HIP_CHECK(hipMalloc(&dev, (size_t)count * (size_t)elem_bytes));
  if (elem_bytes == 4) {
    std::vector<float> b32(beta.begin(), beta.end());
    SMX_HIP_CHECK(hipMemcpy(dev, b32.data(), b32.size() * sizeof(float), hipMemcpyHostToDevice));
  } else {
    SMX_HIP_CHECK(hipMemcpy(dev, beta.data(), beta.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (t.dev) (void)hipFree(t.dev);   // (waits for the launches that read the shorter table)
  t.dev = dev;
  t.count = count;
  return dev;
}

template <typename T>
void build_plan(const smx_mel_config &c, MelInvertPlan &p) {
  const int64_t nm = c.n_mels, nb = c.bins();
  const std::vector<double> &w = c.weights;
  std::vector<int> lo((size_t)nm, 0), len((size_t)nm, 0);
  std::vector<BinItem<T>> items((size_t)nb);
  for (auto &it : items) it = BinItem<T>{(T)0, (T)0, -1, -1};
  for (int64_t j = 0; j < nm; ++j) {
    int first = -1, last = -1;
    for (int64_t k = 0; k < nb; ++k) {
      const double v = w[(size_t)(j * nb + k)];
      if (v == 0.0) continue;
      if (first < 0) first = (int)k;
      last = (int)k;
      BinItem<T> &it = items[(size_t)k];
      if (it.j0 < 0) {
        it.j0 = (int)j;
        it.w0 = (T)v;
      } else if (it.j1 < 0) {
        it.j1 = (int)j;
        it.w1 = (T)v;
      } else {
        throw InvalidArgument(format("invert: cannot invert through a filterbank whose bin %lld lies in more than two filters "
                                     "(the solver relies on the two-filters-per-bin structure of Config.create's triangles)",
                                     (long long)k));
      }
    }
    if (first >= 0) {
      lo[(size_t)j] = first;
      len[(size_t)j] = last + 1 - first;
    }
  }
  // Gershgorin: the largest absolute row sum of W W^T in float64
  double lipschitz = 0.0;
  for (int64_t j = 0; j < nm; ++j) {
    double sum = 0.0;
    for (int64_t i = 0; i < nm; ++i) {
      const int a0 = std::max(lo[(size_t)j], lo[(size_t)i]);
      const int a1 = std::min(lo[(size_t)j] + len[(size_t)j], lo[(size_t)i] + len[(size_t)i]);
      double dot = 0.0;
      for (int k = a0; k < a1; ++k) dot += w[(size_t)(j * nb + k)] * w[(size_t)(i * nb + k)];
      sum += std::fabs(dot);
    }
    lipschitz = std::max(lipschitz, sum);
  }
  // the rows dealt to lanes, longest bands first, 64 to a slot: the rows of one slot are of similar length (the wave walks the
  // longest).  A slot's weights lie lane-interleaved, term q of lane l at (slot base + q) * 64 + l: a wave's read of one term is 64
  // neighbouring words.  The values it gathers lie where the bands put them, so the rows of a slot go to the half-wave in which
  // fewer rows start on the same LDS bank.
  std::vector<int> order((size_t)nm);
  for (int64_t j = 0; j < nm; ++j) order[(size_t)j] = (int)j;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return len[(size_t)x] > len[(size_t)y]; });
  const int slots = (int)((nm + 63) / 64);
  std::vector<int64_t> slot_base((size_t)slots + 1, 0);
  for (int i = 0; i < slots; ++i) slot_base[(size_t)i + 1] = slot_base[(size_t)i] + (len[(size_t)order[(size_t)i * 64]] + kGatherSlack - 1) / kGatherSlack * kGatherSlack;
  const int64_t terms = slot_base[(size_t)slots] * 64;
  if (terms > 0x3fffffff) throw Failure("invert: the filterbank is too large");
  std::vector<int4> rows((size_t)slots * 64, make_int4(-1, 0, 0, 0));
  std::vector<T> wr((size_t)terms, (T)0);
  for (int i = 0; i < slots; ++i) {
    int used[2] = {0, 0}, starts[2][32] = {};
    for (int64_t e = (int64_t)i * 64; e < std::min<int64_t>(nm, (int64_t)i * 64 + 64); ++e) {
      const int j = order[(size_t)e], bank = lo[(size_t)j] & 31;
      int h = starts[0][bank] != starts[1][bank] ? (starts[0][bank] < starts[1][bank] ? 0 : 1) : (used[0] <= used[1] ? 0 : 1);
      if (used[h] == 32) h ^= 1;
      const int lane = h * 32 + used[h]++;
      ++starts[h][bank];
      const int64_t at = slot_base[(size_t)i] * 64 + lane;
      rows[(size_t)i * 64 + lane] = make_int4(j, lo[(size_t)j], len[(size_t)j], (int)at);
      for (int q = 0; q < len[(size_t)j]; ++q) wr[(size_t)(at + (int64_t)q * 64)] = (T)w[(size_t)(j * nb + lo[(size_t)j] + q)];
    }
  }
  const size_t rows_bytes = rows.size() * sizeof(int4), w_bytes = (wr.size() + 4) * sizeof(T), bin_bytes = items.size() * sizeof(BinItem<T>);
  const size_t w_at = rows_bytes, bin_at = (w_at + w_bytes + 15) & ~(size_t)15;
  std::vector<char> host(bin_at + bin_bytes, 0);
  std::memcpy(host.data(), rows.data(), rows_bytes);
  std::memcpy(host.data() + w_at, wr.data(), wr.size() * sizeof(T));
  std::memcpy(host.data() + bin_at, items.data(), bin_bytes);
  void *dev = nullptr;
  SMX_HIP_CHECK(hipMalloc(&dev, host.size()));
  SMX_HIP_CHECK(hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice));
  p.buf = dev;
  p.rows = reinterpret_cast<const int4 *>(dev);
  p.w_rows = reinterpret_cast<const char *>(dev) + w_at;
  p.bins = reinterpret_cast<const char *>(dev) + bin_at;
  p.slots = slots;
  p.nnz = terms;
  p.lipschitz = lipschitz;
}

constexpr size_t kWaveLdsLimit = 150 * 1024;   // of the 160 KB a workgroup can hold
constexpr int64_t kGeneralScratch = 256ll << 20;

template <typename T, int NB>
void launch_wave(const InvArgs &a, size_t lds, hipStream_t stream) {
  launch_tiles("invert", mel_invert_wave_kernel<T, NB>, (a.total + kFrames - 1) / kFrames, 64 * kFrames, lds, stream, a);
}

template <typename T>
void run_invert(const MelInvertJob &job, InvArgs a) {
  const int need = (a.nbins + 63) / 64;
  static const int widths[] = {1, 2, 3, 4, 5, 9, 17};
  int nb = 0;
  for (int w : widths)
    if (w >= need) {
      nb = w;
      break;
    }
  if (nb && a.slots <= 8 && !fast_path_disabled()) {
    const size_t lds = wave_lds<T>(a.slots, a.nnz, a.n_mels, nb).bytes;
    if (lds <= kWaveLdsLimit) {
      switch (nb) {
        case 1: launch_wave<T, 1>(a, lds, job.stream); break;
        case 2: launch_wave<T, 2>(a, lds, job.stream); break;
        case 3: launch_wave<T, 3>(a, lds, job.stream); break;
        case 4: launch_wave<T, 4>(a, lds, job.stream); break;
        case 5: launch_wave<T, 5>(a, lds, job.stream); break;
        case 9: launch_wave<T, 9>(a, lds, job.stream); break;
        default: launch_wave<T, 17>(a, lds, job.stream); break;
      }
      return;
    }
  }
  // one workgroup per frame, at most kGeneralScratch bytes of s / y / r at a time
  const int64_t per_frame = (2 * (int64_t)a.nbins + a.n_mels + kGatherSlack) * (int64_t)sizeof(T);
  const int64_t chunk = std::min<int64_t>(std::max<int64_t>(1, kGeneralScratch / per_frame), std::min<int64_t>(a.total, clips_per_launch(1, 256)));
  DeviceScratch scratch;
  scratch.pool((size_t)(chunk * per_frame), job.stream);
  a.scratch = scratch.ptr;
  for (int64_t first = 0; first < a.total; first += chunk) {
    a.first = first;
    const int64_t count = std::min(chunk, a.total - first);
    SMX_LAUNCH(mel_invert_general_kernel<T>, dim3(grid_x("invert", "frames", count, 256)), dim3(256), 0, job.stream, a);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace

void launch_mel_invert(const MelInvertJob &job) {
  if (job.lead <= 0 || job.frames <= 0) return;
  const smx_mel_config &c = *job.cfg;
  const MelInvertPlan &p = c.invert_plan(job.elem_bytes);
  InvArgs a{};
  a.m = job.m;
  a.out = job.out;
  a.w_rows = p.w_rows;
  a.rows = p.rows;
  a.bins = p.bins;
  a.beta = job.n_iter > 0 ? beta_table(job.elem_bytes, job.n_iter) : nullptr;
  a.frames = job.frames;
  a.total = job.lead * job.frames;
  a.n_mels = (int)c.n_mels;
  a.nbins = (int)c.bins();
  a.slots = p.slots;
  a.nnz = (int)p.nnz;
  if (job.n_iter > 0x7fffffff) throw Failure("invert: too many iterations for one launch");
  a.n_iter = (int)job.n_iter;
  const double step = p.lipschitz > 0.0 ? 1.0 / p.lipschitz : 0.0;
  a.eta = job.elem_bytes == 4 ? (double)(float)step : step;
  a.root_mode = job.root == 1.0 ? ROOT_NONE : job.root == 2.0 ? ROOT_SQRT : ROOT_POW;
  a.inv_root = 1.0 / job.root;
  if (job.elem_bytes == 8) run_invert<double>(job, a);
  else run_invert<float>(job, a);
}

}  // namespace smx

const smx::MelInvertPlan &smx_mel_config::invert_plan(int elem_bytes) const {
  smx::init_device_pool();
  int device = 0;
  SMX_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(mutex_);
  const std::pair<int, int> key(device, elem_bytes);
  auto it = invert_.find(key);
  if (it != invert_.end()) return it->second;
  smx::MelInvertPlan p;
  if (elem_bytes == 8) smx::build_plan<double>(*this, p);
  else smx::build_plan<float>(*this, p);
  return invert_.emplace(key, p).first->second;
}

// ---- the C ABI's side: Mel.invert, and mel_to_stft's root in the same launch ------------------------------------------------
namespace smx {
namespace {

void check_invert(const smx_mel_config &c, int64_t lead, int64_t n_mels, int64_t frames, int64_t n_iter, double power) {
  if (lead < 0 || frames < 0 || n_mels < 0) throw Failure("invert: negative extent");
  if (c.sample_rate < 1)   // Config.from_weights
    throw InvalidArgument(
        "invert: cannot invert through a filterbank built from caller-supplied weights (only the triangular filters of "
        "Config.create have the two-filters-per-bin structure the solver uses)");
  if (n_mels != c.n_mels)
    throw InvalidArgument(format("invert: cannot invert %lld mel bands through a filterbank of %lld filters (the mel axis must hold "
                                 "n_mels values)",
                                 (long long)n_mels, (long long)c.n_mels));
  if (n_iter < 0)
    throw InvalidArgument(format("invert: cannot run %lld iterations (n_iter must be non-negative)", (long long)n_iter));
  if (!(std::isfinite(power) && power > 0.0))
    throw InvalidArgument(format("mel_to_stft: cannot take magnitudes of a spectrogram raised to %g (power must be finite and positive)", power));
}

void mel_invert_dev(const smx_mel_config &c, const void *d_m, int elem_bytes, int64_t lead, int64_t n_mels, int64_t frames,
                    int64_t n_iter, double power, void *d_out, hipStream_t stream) {
  check_invert(c, lead, n_mels, frames, n_iter, power);
  if (lead == 0 || frames == 0) return;
  if (!d_m || !d_out) throw Failure("invert: null device pointer");
  MelInvertJob job;
  job.cfg = &c;
  job.m = d_m;
  job.elem_bytes = elem_bytes;
  job.lead = lead;
  job.frames = frames;
  job.n_iter = n_iter;
  job.root = power;
  job.out = d_out;
  job.stream = stream;
  launch_mel_invert(job);
}

void mel_invert_host(const smx_mel_config &c, const void *m, int elem_bytes, int64_t lead, int64_t n_mels, int64_t frames,
                     int64_t n_iter, double power, void *out) {
  check_invert(c, lead, n_mels, frames, n_iter, power);
  if (lead == 0 || frames == 0) return;
  if (!m || !out) throw Failure("invert: null pointer");
  host_call("mel_invert", {{m, (size_t)n_mels * (size_t)frames * (size_t)elem_bytes}}, out,
            (size_t)c.bins() * (size_t)frames * (size_t)elem_bytes, lead, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t stream) {
              mel_invert_dev(c, d_in[0], elem_bytes, nc, n_mels, frames, n_iter, power, d_out, stream);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_mel_invert_f32(const smx_mel_config *c, const float *m, int64_t lead, int64_t n_mels, int64_t frames, int64_t n_iter,
                       double power, float *out) {
  return guarded([&] {
    check_config(c, "invert");
    mel_invert_host(*c, m, 4, lead, n_mels, frames, n_iter, power, out);
  });
}
int smx_mel_invert_f64(const smx_mel_config *c, const double *m, int64_t lead, int64_t n_mels, int64_t frames, int64_t n_iter,
                       double power, double *out) {
  return guarded([&] {
    check_config(c, "invert");
    mel_invert_host(*c, m, 8, lead, n_mels, frames, n_iter, power, out);
  });
}
int smx_mel_invert_f32_dev(const smx_mel_config *c, const float *d_m, int64_t lead, int64_t n_mels, int64_t frames, int64_t n_iter,
                           double power, float *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "invert");
    mel_invert_dev(*c, d_m, 4, lead, n_mels, frames, n_iter, power, d_out, (hipStream_t)stream);
  });
}
int smx_mel_invert_f64_dev(const smx_mel_config *c, const double *d_m, int64_t lead, int64_t n_mels, int64_t frames, int64_t n_iter,
                           double power, double *d_out, void *stream) {
  return guarded([&] {
    check_config(c, "invert");
    mel_invert_dev(*c, d_m, 8, lead, n_mels, frames, n_iter, power, d_out, (hipStream_t)stream);
  });
}

}  // extern "C"
