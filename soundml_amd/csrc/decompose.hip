// Decompose: non-negative matrix factorisation V ~ W H by multiplicative updates (Lee & Seung 2001; Fevotte & Idier 2011) over a
// device-resident V [clips; F; T] (frames fastest), W [clips; F; K] and H [clips; K; T].  include/soundml_amd.h words the
// definition and DESIGN.md 4.8i the orders and budgets.
//
// Every inner product is ONE chain of fused multiply-adds from 0.0 whose order is a function of (F, T, K) only:
//   over f or t   32-block after 32-block; inside a block the offsets run perm32(0..31) = 0 4 1 5 2 6 3 7 | 8 12 9 13 ... (pairs
//                 rho, rho + 4 with rho = (r & 3) + 8 (r >> 2), r = 0..15): the order in which a 32 x 32 accumulator tile hands its
//                 rows to the next v_mfma_f32_32x32x2_f32 as an operand.  The last block is padded with terms fma(0, 0, acc)
//   over k        ascending, padded to an even count with one term fma(0, 0, acc)
// (a pad term changes nothing but the sign of a zero sum).  The matrix instruction is bit for bit such a chain, k = 0 then k = 1, so
// the tile kernels and the general kernels give the same bits.  The file is built with -ffp-contract=off: the products with the old
// factor, the divisions and the objective's terms round one after the other.
//
// Ordering between the launches of a round is the launch order on the one stream and nothing else: no flag in memory is polled, no
// wave waits on another workgroup, every loop's trip count is fixed by the shapes.
//
//   copy_kernel        the initial factors into the results, which every round then updates in place
//   gram_kernel        a thread per cell of G [K; K + 1]: G[k][k'] = sum W[f, k] W[f, k'] over f (the H update) or
//                      sum H[k, t] H[k', t] over t (the W update); column K holds sum W[f, k] 1 (sum H[k, t] 1): the KL denominator
//   h_tile_kernel      float32, K <= 64: one wave per (clip, 32 columns t) walks all of f once.  Per 32 rows: V's tile as the B
//                      operand [k = l >> 5][j = l & 31] (rows arrive as 128-byte runs); KL forms W H on the tile with K / 2 products,
//                      takes V / floor(.) in the accumulator layout and hands it on as the B operand of W^T R.  The numerator stays
//                      in registers over the walk; the epilogue forms (W^T W) H by K / 2 products and updates H's block in place
//   w_tile_kernel      the transpose: one wave per (clip, 32 rows f) walks t; the tile is (W H)^T, rows t in the registers, f on
//                      the lanes
//   ratio / denom / update_kernel   the general route: a thread per cell, the same chains from memory through scratch
//                      (R [F; T] for KL, the denominator [K; T] / [F; K] for Frobenius): any K <= 1024, float64, SMX_DISABLE_FAST=1
//   reconstruct_kernel a thread per cell of W H, components outside the mask entering as fma(0, 0, acc); as_mask: over floor(all)
//   divergence_rows_kernel / divergence_end_kernel   the objective in float64: a thread per row chains over t, one thread per clip
//                      chains over the rows
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

constexpr int kTileK = 64;                         // the tile route's cap on K: two 32-blocks of accumulators
constexpr int64_t kMaxK = 1024;
constexpr int64_t kScratchBytes = 512ll << 20;     // scratch of one launch group; larger batches go clip range by clip range
constexpr int64_t kMaxExtent = 1ll << 24;          // F and T
constexpr int kWords = (int)(kMaxK / 64);

using f32x16 = __attribute__((ext_vector_type(16))) float;

__host__ __device__ constexpr int perm32(int i) { return ((i >> 1) & 3) + 8 * (i >> 3) + 4 * (i & 1); }

__device__ __forceinline__ float fma_t(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return fma(a, b, c); }
template <typename T>
__device__ __forceinline__ T floor_eps(T x) {
  const T eps = (T)1.1920928955078125e-07;         // 2^-23; a NaN stays a NaN
  return x < eps ? eps : x;
}

struct Args {
  const void *V;                  // [clips; F; T]: clips vs apart, rows vp apart
  void *W, *H;                    // [clips; F; K] ws apart (0: one dictionary for every clip, read only), [clips; K; T] hs apart
  void *G;                        // [clips; K; K + 1]
  void *R;                        // general route, KL: [clips; F; T]
  void *D;                        // general route, Frobenius: [clips; max(K T, F K)]
  int64_t vs, vp, ws, hs, ds;
  int64_t F, T, K;
  int beta;
};

// the chain over n = F or T: x(i) and y(i) are read only where i < n
template <typename T, typename X, typename Y>
__device__ __forceinline__ T chain32(int64_t n, X x, Y y) {
  T acc = (T)0;
  for (int64_t b = 0; b < n; b += 32) {
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {
      const int64_t idx = b + perm32(i);
      const bool in = idx < n;
      acc = fma_t(in ? x(idx) : (T)0, in ? y(idx) : (T)0, acc);
    }
  }
  return acc;
}

// the chain over k: x(k), y(k) for k < K
template <typename T, typename X, typename Y>
__device__ __forceinline__ T chain_k(int64_t K, X x, Y y) {
  T acc = (T)0;
  for (int64_t k = 0; k < K; ++k) acc = fma_t(x(k), y(k), acc);
  if (K & 1) acc = fma_t((T)0, (T)0, acc);
  return acc;
}

// side 0: G = W^T W over f; side 1: G = H H^T over t.  sums_only (KL): column K alone
template <typename T>
__global__ void __launch_bounds__(256) gram_kernel(Args a, int side, int sums_only, int64_t clips) {
  const int64_t K = a.K, cols = sums_only ? 1 : K + 1, cells = K * cols;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= clips * cells) return;
  const int64_t c = id / cells, cell = id - c * cells, k = cell / cols, k2 = sums_only ? K : cell - k * cols;
  T acc;
  if (side == 0) {
    const T *W = (const T *)a.W + c * a.ws;
    acc = chain32<T>(a.F, [&](int64_t f) { return W[f * K + k]; }, [&](int64_t f) { return k2 < K ? W[f * K + k2] : (T)1; });
  } else {
    const T *H = (const T *)a.H + c * a.hs;
    acc = chain32<T>(a.T, [&](int64_t t) { return H[k * a.T + t]; }, [&](int64_t t) { return k2 < K ? H[k2 * a.T + t] : (T)1; });
  }
  ((T *)a.G)[c * K * (K + 1) + k * (K + 1) + k2] = acc;
}

// cells values of each of clips rows, src_stride / dst_stride apart
template <typename T>
__global__ void __launch_bounds__(256) copy_kernel(const T *src, int64_t src_stride, T *dst, int64_t dst_stride, int64_t cells, int64_t clips) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= clips * cells) return;
  const int64_t c = id / cells, cell = id - c * cells;
  dst[c * dst_stride + cell] = src[c * src_stride + cell];
}

// ---- the general route -------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) ratio_kernel(Args a, int64_t clips) {
  const int64_t cells = a.F * a.T;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= clips * cells) return;
  const int64_t c = id / cells, cell = id - c * cells, f = cell / a.T, t = cell - f * a.T;
  const T *W = (const T *)a.W + c * a.ws + f * a.K, *H = (const T *)a.H + c * a.hs + t;
  const T x = chain_k<T>(a.K, [&](int64_t k) { return W[k]; }, [&](int64_t k) { return H[k * a.T]; });
  ((T *)a.R)[c * cells + cell] = ((const T *)a.V)[c * a.vs + f * a.vp + t] / floor_eps(x);
}

// side 0: D [K; T] = G H; side 1: D [F; K] = W G
template <typename T>
__global__ void __launch_bounds__(256) denom_kernel(Args a, int side, int64_t clips) {
  const int64_t K = a.K, cells = side == 0 ? K * a.T : a.F * K;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= clips * cells) return;
  const int64_t c = id / cells, cell = id - c * cells;
  const T *G = (const T *)a.G + c * K * (K + 1);
  T acc;
  if (side == 0) {
    const int64_t k = cell / a.T, t = cell - k * a.T;
    const T *H = (const T *)a.H + c * a.hs + t;
    acc = chain_k<T>(K, [&](int64_t j) { return G[k * (K + 1) + j]; }, [&](int64_t j) { return H[j * a.T]; });
  } else {
    const int64_t f = cell / K, k = cell - f * K;
    const T *W = (const T *)a.W + c * a.ws + f * K;
    acc = chain_k<T>(K, [&](int64_t j) { return G[k * (K + 1) + j]; }, [&](int64_t j) { return W[j]; });
  }
  ((T *)a.D)[c * a.ds + cell] = acc;
}

// side 0: H[k, t]; side 1: W[f, k].  In place: a cell reads no other cell of the factor it writes
template <typename T>
__global__ void __launch_bounds__(256) update_kernel(Args a, int side, int64_t clips) {
  const int64_t K = a.K, cells = side == 0 ? K * a.T : a.F * K;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= clips * cells) return;
  const int64_t c = id / cells, cell = id - c * cells;
  const bool kl = a.beta == SMX_NMF_KULLBACK_LEIBLER;
  const T *S = kl ? (const T *)a.R + c * a.F * a.T : (const T *)a.V + c * a.vs;   // what the factors are multiplied against
  const int64_t sp = kl ? a.T : a.vp;
  const T *G = (const T *)a.G + c * K * (K + 1);
  const T *W = (const T *)a.W + c * a.ws, *H = (const T *)a.H + c * a.hs;
  T num, *dst;
  int64_t k;
  if (side == 0) {
    k = cell / a.T;
    const int64_t t = cell - k * a.T;
    num = chain32<T>(a.F, [&](int64_t f) { return W[f * K + k]; }, [&](int64_t f) { return S[f * sp + t]; });
    dst = (T *)a.H + c * a.hs + cell;
  } else {
    const int64_t f = cell / K;
    k = cell - f * K;
    num = chain32<T>(a.T, [&](int64_t t) { return H[k * a.T + t]; }, [&](int64_t t) { return S[f * sp + t]; });
    dst = (T *)a.W + c * a.ws + cell;
  }
  const T den = kl ? G[k * (K + 1) + K] : ((const T *)a.D)[c * a.ds + cell];
  const T prod = *dst * num;
  *dst = prod / floor_eps(den);
}

// ---- the tile route ----------------------------------------------------------------------------------------------------------------
// KB: 32-blocks of k (K <= 32 KB).  A wave is a workgroup; lane l: j = l & 31 is its column of every tile, h = l >> 5 its half.
// Register r of a 32 x 32 accumulator tile is row rho(r) + 4 h, column j.
__device__ __forceinline__ int rho(int r) { return (r & 3) + 8 * (r >> 2); }

template <int KB, bool KL>
__global__ void __launch_bounds__(64) h_tile_kernel(Args a, int64_t tblocks) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  const int64_t c = blockIdx.x / tblocks, t = (blockIdx.x - c * tblocks) * 32 + j;
  const int64_t F = a.F, T = a.T, K = a.K;
  const bool t_in = t < T;
  const float *V = (const float *)a.V + c * a.vs, *W = (const float *)a.W + c * a.ws, *G = (const float *)a.G + c * K * (K + 1);
  float *H = (float *)a.H + c * a.hs;
  // H's block as the B operand of every product over k: step s holds rows 2 s + h
  float hb[16 * KB];
#pragma unroll
  for (int s = 0; s < 16 * KB; ++s) hb[s] = (t_in && 2 * s + h < K) ? H[(int64_t)(2 * s + h) * T + t] : 0.0f;
  f32x16 num[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) num[kb][r] = 0.0f;

  for (int64_t fb = 0; fb < F; fb += 32) {
    f32x16 x;
    if (KL) {                                                              // (W H) on the tile: rows f, column t
#pragma unroll
      for (int r = 0; r < 16; ++r) x[r] = 0.0f;
      const bool f_in = fb + j < F;
      const float *wrow = W + (fb + j) * K;
#pragma unroll
      for (int s = 0; s < 16 * KB; ++s)
        if (2 * s < K) x = __builtin_amdgcn_mfma_f32_32x32x2f32((f_in && 2 * s + h < K) ? wrow[2 * s + h] : 0.0f, hb[s], x, 0, 0, 0);
    }
    float rt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t f = fb + rho(r) + 4 * h;
      const bool in = f < F && t_in;
      const float v = in ? V[f * a.vp + t] : 0.0f;
      rt[r] = KL ? (in ? v / floor_eps(x[r]) : 0.0f) : v;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t f = fb + rho(r) + 4 * h;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int k = kb * 32 + j;
        num[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32((f < F && k < K) ? W[f * K + k] : 0.0f, rt[r], num[kb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    f32x16 den;
    if (!KL) {                                                             // (W^T W) H on the block
#pragma unroll
      for (int r = 0; r < 16; ++r) den[r] = 0.0f;
      const int k = kb * 32 + j;
#pragma unroll
      for (int s = 0; s < 16 * KB; ++s)
        if (2 * s < K) den = __builtin_amdgcn_mfma_f32_32x32x2f32((k < K && 2 * s + h < K) ? G[k * (K + 1) + 2 * s + h] : 0.0f, hb[s], den, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = kb * 32 + rho(r) + 4 * h;
      if (k < K && t_in) {
        const float d = KL ? G[k * (K + 1) + K] : den[r];
        const float prod = H[k * T + t] * num[kb][r];
        H[k * T + t] = prod / floor_eps(d);
      }
    }
  }
}

template <int KB, bool KL>
__global__ void __launch_bounds__(64) w_tile_kernel(Args a, int64_t fblocks) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  const int64_t c = blockIdx.x / fblocks, f = (blockIdx.x - c * fblocks) * 32 + j;
  const int64_t F = a.F, T = a.T, K = a.K;
  const bool f_in = f < F;
  const float *V = (const float *)a.V + c * a.vs, *H = (const float *)a.H + c * a.hs, *G = (const float *)a.G + c * K * (K + 1);
  float *W = (float *)a.W + c * a.ws;
  // W's block as the B operand of every product over k: step s holds columns 2 s + h of row f
  float wb[16 * KB];
#pragma unroll
  for (int s = 0; s < 16 * KB; ++s) wb[s] = (f_in && 2 * s + h < K) ? W[f * K + 2 * s + h] : 0.0f;
  f32x16 num[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) num[kb][r] = 0.0f;

  for (int64_t tb = 0; tb < T; tb += 32) {
    f32x16 x;
    if (KL) {                                                              // (W H)^T on the tile: rows t, column f
#pragma unroll
      for (int r = 0; r < 16; ++r) x[r] = 0.0f;
      const bool t_in = tb + j < T;
#pragma unroll
      for (int s = 0; s < 16 * KB; ++s)
        if (2 * s < K) x = __builtin_amdgcn_mfma_f32_32x32x2f32((t_in && 2 * s + h < K) ? H[(int64_t)(2 * s + h) * T + tb + j] : 0.0f, wb[s], x, 0, 0, 0);
    }
    float rt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = tb + rho(r) + 4 * h;
      const bool in = t < T && f_in;
      const float v = in ? V[f * a.vp + t] : 0.0f;
      rt[r] = KL ? (in ? v / floor_eps(x[r]) : 0.0f) : v;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = tb + rho(r) + 4 * h;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int k = kb * 32 + j;
        num[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32((t < T && k < K) ? H[(int64_t)k * T + t] : 0.0f, rt[r], num[kb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    f32x16 den;
    if (!KL) {                                                             // (W (H H^T))^T on the block
#pragma unroll
      for (int r = 0; r < 16; ++r) den[r] = 0.0f;
      const int k = kb * 32 + j;
#pragma unroll
      for (int s = 0; s < 16 * KB; ++s)
        if (2 * s < K) den = __builtin_amdgcn_mfma_f32_32x32x2f32((k < K && 2 * s + h < K) ? G[k * (K + 1) + 2 * s + h] : 0.0f, wb[s], den, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = kb * 32 + rho(r) + 4 * h;
      if (k < K && f_in) {
        const float d = KL ? G[k * (K + 1) + K] : den[r];
        const float prod = W[f * K + k] * num[kb][r];
        W[f * K + k] = prod / floor_eps(d);
      }
    }
  }
}

// ---- reconstruction and the objective ----------------------------------------------------------------------------------------------
struct Mask {
  unsigned long long word[kWords];
};

struct ReconstructArgs {
  const void *W, *H;
  void *out;                      // [clips; F; T]: clips os apart, rows op apart
  int64_t ws, hs, os, op, F, T, K;
  int as_mask;                    // the selected components' sum over floor(the sum of all)
  Mask mask;
};

template <typename T>
__global__ void __launch_bounds__(256) reconstruct_kernel(ReconstructArgs a, int64_t clips) {
  const int64_t cells = a.F * a.T;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= clips * cells) return;
  const int64_t c = id / cells, cell = id - c * cells, f = cell / a.T, t = cell - f * a.T;
  const T *W = (const T *)a.W + c * a.ws + f * a.K, *H = (const T *)a.H + c * a.hs + t;
  const T x = chain_k<T>(
      a.K, [&](int64_t k) { return (a.mask.word[k >> 6] >> (k & 63)) & 1 ? W[k] : (T)0; },
      [&](int64_t k) { return (a.mask.word[k >> 6] >> (k & 63)) & 1 ? H[k * a.T] : (T)0; });
  T *out = (T *)a.out + c * a.os + f * a.op + t;
  if (!a.as_mask) {
    *out = x;
    return;
  }
  const T all = chain_k<T>(a.K, [&](int64_t k) { return W[k]; }, [&](int64_t k) { return H[k * a.T]; });
  *out = x / floor_eps(all);
}

struct DivergenceArgs {
  const void *V, *W, *H;
  double *rows;                   // [clips; 3; F]
  void *out;                      // [clips]
  int64_t vs, vp, ws, hs, F, T, K;
  int beta;
};

// per row f, ascending over t, X = W H an ascending chain over k of products and sums rounded one after the other in float64:
// Frobenius: sum (V - X)^2, sum V^2; KL: sum over V > 0 of V log(V / X), sum V, sum X
template <typename T>
__global__ void __launch_bounds__(64) divergence_rows_kernel(DivergenceArgs a, int64_t clips) {
  const int64_t id = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (id >= clips * a.F) return;
  const int64_t c = id / a.F, f = id - c * a.F;
  const T *V = (const T *)a.V + c * a.vs + f * a.vp, *W = (const T *)a.W + c * a.ws + f * a.K, *H = (const T *)a.H + c * a.hs;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t t = 0; t < a.T; ++t) {
    double x = 0.0;
    for (int64_t k = 0; k < a.K; ++k) x = x + (double)W[k] * (double)H[k * a.T + t];
    const double v = (double)V[t];
    if (a.beta == SMX_NMF_FROBENIUS) {
      const double d = v - x;
      s0 = s0 + d * d;
      s1 = s1 + v * v;
    } else {
      if (v > 0.0) s0 = s0 + v * log(v / x);
      s1 = s1 + v;
      s2 = s2 + x;
    }
  }
  double *rows = a.rows + c * 3 * a.F;
  rows[f] = s0, rows[a.F + f] = s1, rows[2 * a.F + f] = s2;
}

template <typename T>
__global__ void __launch_bounds__(64) divergence_end_kernel(DivergenceArgs a, int64_t clips) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= clips) return;
  const double *rows = a.rows + c * 3 * a.F;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t f = 0; f < a.F; ++f) s0 = s0 + rows[f], s1 = s1 + rows[a.F + f], s2 = s2 + rows[2 * a.F + f];
  const double d = a.beta == SMX_NMF_FROBENIUS ? sqrt(s0 / s1) : ((s0 - s1) + s2) / s1;
  ((T *)a.out)[c] = (T)d;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct Shape {
  int64_t F, T, K;
};

// the checks of every entry, in the header's order, before any pointer is looked at
void check_shape(const char *fn, int64_t F, int64_t T, int64_t K) {
  if (K < 1) throw InvalidArgument(format("%s: n_components is %lld (at least 1)", fn, (long long)K));
  if (K > kMaxK) throw InvalidArgument(format("%s: n_components is %lld (at most %lld)", fn, (long long)K, (long long)kMaxK));
  if (F < 1 || T < 1) throw InvalidArgument(format("%s: V is %lld x %lld (at least 1 x 1)", fn, (long long)F, (long long)T));
  if (F > kMaxExtent || T > kMaxExtent)
    throw InvalidArgument(format("%s: V is %lld x %lld (at most %lld either way)", fn, (long long)F, (long long)T, (long long)kMaxExtent));
}
void check_beta(const char *fn, int beta) {
  if (beta != SMX_NMF_FROBENIUS && beta != SMX_NMF_KULLBACK_LEIBLER)
    throw InvalidArgument(format("%s: unknown beta %d (0: frobenius, 1: kullback-leibler)", fn, beta));
}
void check_rounds(const char *fn, int64_t n_iter) {
  if (n_iter < 0) throw InvalidArgument(format("%s: n_iter is %lld (at least 0)", fn, (long long)n_iter));
}
void check_clips(const char *fn, int64_t clips) {
  if (clips < 0) throw InvalidArgument(format("%s: %lld clips (at least 0)", fn, (long long)clips));
}
void check_stride(const char *fn, const char *what, int64_t stride, int64_t least, bool zero_allowed = false) {
  if (zero_allowed && stride == 0) return;
  if (stride < least) throw InvalidArgument(format("%s: %s is %lld (at least %lld)", fn, what, (long long)stride, (long long)least));
}

bool takes_tiles(int64_t K, int elem_bytes) { return elem_bytes == 4 && K <= kTileK && !fast_path_disabled(); }

template <bool KL>
void launch_tiles_of(const char *fn, const Args &a, int side, int64_t clips, hipStream_t stream) {
  const int64_t blocks = side == 0 ? (a.T + 31) / 32 : (a.F + 31) / 32;
  const unsigned grid = grid_x(fn, "cells", clips * blocks, 64);
  if (side == 0) {
    if (a.K <= 32) SMX_LAUNCH((h_tile_kernel<1, KL>), dim3(grid), dim3(64), 0, stream, a, blocks);
    else SMX_LAUNCH((h_tile_kernel<2, KL>), dim3(grid), dim3(64), 0, stream, a, blocks);
  } else {
    if (a.K <= 32) SMX_LAUNCH((w_tile_kernel<1, KL>), dim3(grid), dim3(64), 0, stream, a, blocks);
    else SMX_LAUNCH((w_tile_kernel<2, KL>), dim3(grid), dim3(64), 0, stream, a, blocks);
  }
  SMX_HIP_CHECK(hipGetLastError());
}

template <typename T>
void update_general(const char *fn, const Args &a, int side, int64_t clips, hipStream_t stream) {
  const int64_t cells = side == 0 ? a.K * a.T : a.F * a.K;
  if (a.beta == SMX_NMF_KULLBACK_LEIBLER) SMX_LAUNCH((ratio_kernel<T>), dim3(grid_x(fn, "cells", (clips * a.F * a.T + 255) / 256, 256)), dim3(256), 0, stream, a, clips);
  else SMX_LAUNCH((denom_kernel<T>), dim3(grid_x(fn, "cells", (clips * cells + 255) / 256, 256)), dim3(256), 0, stream, a, side, clips);
  SMX_HIP_CHECK(hipGetLastError());
  SMX_LAUNCH((update_kernel<T>), dim3(grid_x(fn, "cells", (clips * cells + 255) / 256, 256)), dim3(256), 0, stream, a, side, clips);
  SMX_HIP_CHECK(hipGetLastError());
}

// n_iter rounds in place on d_W (with_w) and d_H, which hold the initial factors
void nmf_dev(const char *fn, const Shape &s, int elem_bytes, int beta, int64_t n_iter, bool with_w, const void *d_V, int64_t vs, int64_t vp, void *d_W, int64_t ws,
             void *d_H, int64_t hs, int64_t clips, hipStream_t stream) {
  if (clips == 0 || n_iter == 0) return;
  const bool tiles = takes_tiles(s.K, elem_bytes), kl = beta == SMX_NMF_KULLBACK_LEIBLER;
  const int64_t eb = elem_bytes;
  const int64_t g_bytes = (s.K * (s.K + 1) * eb + 15) / 16 * 16;
  const int64_t ds = std::max(s.K * s.T, s.F * s.K);
  const int64_t r_bytes = tiles ? 0 : ((kl ? s.F * s.T : ds) * eb + 15) / 16 * 16;
  const int64_t per_clip = g_bytes + r_bytes;
  const int64_t step = std::max<int64_t>(1, std::min<int64_t>(clips, kScratchBytes / per_clip));
  init_device_pool();
  DeviceScratch scratch;
  scratch.pool((size_t)(step * per_clip), stream);
  char *base = scratch.as<char>();
  for (int64_t c0 = 0; c0 < clips; c0 += step) {                           // clips are independent: a range runs all its rounds
    const int64_t nc = std::min(step, clips - c0);
    Args a{};
    a.V = (const char *)d_V + c0 * vs * eb, a.W = (char *)d_W + c0 * ws * eb, a.H = (char *)d_H + c0 * hs * eb;
    a.G = base, a.R = kl ? base + step * g_bytes : nullptr, a.D = kl ? nullptr : base + step * g_bytes;
    a.vs = vs, a.vp = vp, a.ws = ws, a.hs = hs, a.ds = ds, a.F = s.F, a.T = s.T, a.K = s.K, a.beta = beta;
    const unsigned gram_grid = grid_x(fn, "cells", (nc * s.K * (kl ? 1 : s.K + 1) + 255) / 256, 256);
    for (int64_t it = 0; it < n_iter; ++it) {
      for (int side = 0; side < (with_w ? 2 : 1); ++side) {
        // G of the factor that stays fixed in this update
        if (elem_bytes == 4) SMX_LAUNCH((gram_kernel<float>), dim3(gram_grid), dim3(256), 0, stream, a, side, kl ? 1 : 0, nc);
        else SMX_LAUNCH((gram_kernel<double>), dim3(gram_grid), dim3(256), 0, stream, a, side, kl ? 1 : 0, nc);
        SMX_HIP_CHECK(hipGetLastError());
        if (tiles) {
          if (kl) launch_tiles_of<true>(fn, a, side, nc, stream);
          else launch_tiles_of<false>(fn, a, side, nc, stream);
        } else if (elem_bytes == 4) {
          update_general<float>(fn, a, side, nc, stream);
        } else {
          update_general<double>(fn, a, side, nc, stream);
        }
      }
    }
  }
}

void copy_factor(void *dst, int64_t dst_stride, const void *src, int64_t src_stride, int64_t cells, int64_t clips, int elem_bytes, hipStream_t stream) {
  if (dst == src && dst_stride == src_stride) return;
  const unsigned grid = grid_x("nmf", "cells", (clips * cells + 255) / 256, 256);
  if (elem_bytes == 4) SMX_LAUNCH((copy_kernel<float>), dim3(grid), dim3(256), 0, stream, (const float *)src, src_stride, (float *)dst, dst_stride, cells, clips);
  else SMX_LAUNCH((copy_kernel<double>), dim3(grid), dim3(256), 0, stream, (const double *)src, src_stride, (double *)dst, dst_stride, cells, clips);
  SMX_HIP_CHECK(hipGetLastError());
}

// nmf (with_w) and nmf_activations
void nmf_call(const char *fn, bool device, bool with_w, int elem_bytes, const void *V, int64_t vs, int64_t vp, const void *W0, int64_t w0s, const void *H0,
              int64_t h0s, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta, void *W, int64_t ws, void *H, int64_t hs,
              hipStream_t stream) {
  check_shape(fn, F, T, K);
  check_beta(fn, beta);
  check_rounds(fn, n_iter);
  check_clips(fn, clips);
  check_stride(fn, "V's row pitch", vp, T);
  check_stride(fn, "V's clip stride", vs, (F - 1) * vp + T);
  check_stride(fn, "W0's clip stride", w0s, F * K, !with_w);
  check_stride(fn, "H0's clip stride", h0s, K * T);
  if (with_w) check_stride(fn, "W's clip stride", ws, F * K);
  check_stride(fn, "H's clip stride", hs, K * T);
  if (clips == 0) return;
  if (!V || !W0 || !H0 || (with_w && !W) || !H) throw Failure(format("%s: null pointer", fn));
  const Shape s{F, T, K};
  if (device) {
    if (with_w) copy_factor(W, ws, W0, w0s, F * K, clips, elem_bytes, stream);
    copy_factor(H, hs, H0, h0s, K * T, clips, elem_bytes, stream);
    nmf_dev(fn, s, elem_bytes, beta, n_iter, with_w, V, vs, vp, with_w ? W : const_cast<void *>(W0), with_w ? ws : w0s, H, hs, clips, stream);
    return;
  }
  const size_t eb = (size_t)elem_bytes;
  const std::vector<HostIn> in{{V, (size_t)(F * T) * eb}, {W0, (size_t)(F * K) * eb}, {H0, (size_t)(K * T) * eb}};
  if (with_w) {
    host_call(fn, in, {HostOut{W, (size_t)(F * K) * eb}, HostOut{H, (size_t)(K * T) * eb}}, clips, false, nullptr,
              [&](const void *const *d_in, void *const *d_out, int64_t nc, hipStream_t st) {
                copy_factor(d_out[0], F * K, d_in[1], F * K, F * K, nc, elem_bytes, st);
                copy_factor(d_out[1], K * T, d_in[2], K * T, K * T, nc, elem_bytes, st);
                nmf_dev(fn, s, elem_bytes, beta, n_iter, true, d_in[0], F * T, T, d_out[0], F * K, d_out[1], K * T, nc, st);
              });
  } else {
    host_call(fn, in, H, (size_t)(K * T) * eb, clips, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t st) {
      copy_factor(d_out, K * T, d_in[2], K * T, K * T, nc, elem_bytes, st);
      nmf_dev(fn, s, elem_bytes, beta, n_iter, false, d_in[0], F * T, T, const_cast<void *>(d_in[1]), F * K, d_out, K * T, nc, st);
    });
  }
}

void reconstruct_dev(const char *fn, const Shape &s, int elem_bytes, const Mask &mask, int as_mask, const void *d_W, int64_t ws, const void *d_H, int64_t hs, int64_t clips,
                     void *d_out, int64_t os, int64_t op, hipStream_t stream) {
  ReconstructArgs a{};
  a.W = d_W, a.H = d_H, a.out = d_out, a.ws = ws, a.hs = hs, a.os = os, a.op = op, a.F = s.F, a.T = s.T, a.K = s.K, a.as_mask = as_mask, a.mask = mask;
  const unsigned grid = grid_x(fn, "cells", (clips * s.F * s.T + 255) / 256, 256);
  if (elem_bytes == 4) SMX_LAUNCH((reconstruct_kernel<float>), dim3(grid), dim3(256), 0, stream, a, clips);
  else SMX_LAUNCH((reconstruct_kernel<double>), dim3(grid), dim3(256), 0, stream, a, clips);
  SMX_HIP_CHECK(hipGetLastError());
}

void reconstruct_call(bool device, int elem_bytes, const void *W, int64_t ws, const void *H, int64_t hs, int64_t clips, int64_t F, int64_t T, int64_t K,
                      const int64_t *components, int64_t n_components, int as_mask, void *out, int64_t os, int64_t op, hipStream_t stream) {
  const char *fn = as_mask ? "nmf_mask" : "nmf_reconstruct";
  check_shape(fn, F, T, K);
  check_clips(fn, clips);
  Mask mask{};
  if (components) {
    if (n_components < 0) throw InvalidArgument(format("%s: %lld components (at least 0)", fn, (long long)n_components));
    for (int64_t i = 0; i < n_components; ++i) {
      const int64_t k = components[i];
      if (k < 0 || k >= K) throw InvalidArgument(format("%s: component %lld is outside [0, %lld)", fn, (long long)k, (long long)K));
      mask.word[k >> 6] |= 1ull << (k & 63);
    }
  } else {
    for (int64_t k = 0; k < K; ++k) mask.word[k >> 6] |= 1ull << (k & 63);
  }
  check_stride(fn, "W's clip stride", ws, F * K, true);
  check_stride(fn, "H's clip stride", hs, K * T);
  check_stride(fn, "the output's row pitch", op, T);
  check_stride(fn, "the output's clip stride", os, (F - 1) * op + T);
  if (clips == 0) return;
  if (!W || !H || !out) throw Failure(format("%s: null pointer", fn));
  const Shape s{F, T, K};
  if (device) {
    reconstruct_dev(fn, s, elem_bytes, mask, as_mask, W, ws, H, hs, clips, out, os, op, stream);
    return;
  }
  const size_t eb = (size_t)elem_bytes;
  host_call(fn, {{W, (size_t)(F * K) * eb}, {H, (size_t)(K * T) * eb}}, out, (size_t)(F * T) * eb, clips, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t st) {
              reconstruct_dev(fn, s, elem_bytes, mask, as_mask, d_in[0], F * K, d_in[1], K * T, nc, d_out, F * T, T, st);
            });
}

void divergence_dev(const char *fn, const Shape &s, int elem_bytes, int beta, const void *d_V, int64_t vs, int64_t vp, const void *d_W, int64_t ws,
                    const void *d_H, int64_t hs, int64_t clips, void *d_out, hipStream_t stream) {
  init_device_pool();
  DeviceScratch scratch;
  scratch.pool((size_t)(clips * 3 * s.F * 8), stream);
  DivergenceArgs a{};
  a.V = d_V, a.W = d_W, a.H = d_H, a.rows = scratch.as<double>(), a.out = d_out;
  a.vs = vs, a.vp = vp, a.ws = ws, a.hs = hs, a.F = s.F, a.T = s.T, a.K = s.K, a.beta = beta;
  const unsigned rows_grid = grid_x(fn, "cells", (clips * s.F + 63) / 64, 64), end_grid = grid_x(fn, "cells", (clips + 63) / 64, 64);
  if (elem_bytes == 4) {
    SMX_LAUNCH((divergence_rows_kernel<float>), dim3(rows_grid), dim3(64), 0, stream, a, clips);
    SMX_LAUNCH((divergence_end_kernel<float>), dim3(end_grid), dim3(64), 0, stream, a, clips);
  } else {
    SMX_LAUNCH((divergence_rows_kernel<double>), dim3(rows_grid), dim3(64), 0, stream, a, clips);
    SMX_LAUNCH((divergence_end_kernel<double>), dim3(end_grid), dim3(64), 0, stream, a, clips);
  }
  SMX_HIP_CHECK(hipGetLastError());
}

void divergence_call(bool device, int elem_bytes, const void *V, int64_t vs, int64_t vp, const void *W, int64_t ws, const void *H, int64_t hs, int64_t clips,
                     int64_t F, int64_t T, int64_t K, int beta, void *out, hipStream_t stream) {
  const char *fn = "nmf_divergence";
  check_shape(fn, F, T, K);
  check_beta(fn, beta);
  check_clips(fn, clips);
  check_stride(fn, "V's row pitch", vp, T);
  check_stride(fn, "V's clip stride", vs, (F - 1) * vp + T);
  check_stride(fn, "W's clip stride", ws, F * K, true);
  check_stride(fn, "H's clip stride", hs, K * T);
  if (clips == 0) return;
  if (!V || !W || !H || !out) throw Failure(format("%s: null pointer", fn));
  const Shape s{F, T, K};
  if (device) {
    divergence_dev(fn, s, elem_bytes, beta, V, vs, vp, W, ws, H, hs, clips, out, stream);
    return;
  }
  const size_t eb = (size_t)elem_bytes;
  host_call(fn, {{V, (size_t)(F * T) * eb}, {W, (size_t)(F * K) * eb}, {H, (size_t)(K * T) * eb}}, out, eb, clips, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t nc, hipStream_t st) {
              divergence_dev(fn, s, elem_bytes, beta, d_in[0], F * T, T, d_in[1], F * K, d_in[2], K * T, nc, d_out, st);
            });
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Decompose -------------------------------------------------------------------------------------------------------------------
int smx_nmf_tile_cap(int64_t *tile_k, int64_t *max_k) {
  return guarded([&] {
    if (tile_k) *tile_k = kTileK;
    if (max_k) *max_k = kMaxK;
  });
}
int smx_nmf_f32(const float *V, const float *W0, const float *H0, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta, float *W, float *H) {
  return guarded([&] { nmf_call("nmf", false, true, 4, V, F * T, T, W0, F * K, H0, K * T, clips, F, T, K, n_iter, beta, W, F * K, H, K * T, nullptr); });
}
int smx_nmf_f64(const double *V, const double *W0, const double *H0, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta, double *W,
                double *H) {
  return guarded([&] { nmf_call("nmf", false, true, 8, V, F * T, T, W0, F * K, H0, K * T, clips, F, T, K, n_iter, beta, W, F * K, H, K * T, nullptr); });
}
int smx_nmf_vram_f32(const float *d_V, int64_t v_stride, int64_t v_pitch, const float *d_W0, int64_t w0_stride, const float *d_H0, int64_t h0_stride,
                     int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta, float *d_W, int64_t w_stride, float *d_H, int64_t h_stride,
                     void *stream) {
  return guarded([&] {
    nmf_call("nmf", true, true, 4, d_V, v_stride, v_pitch, d_W0, w0_stride, d_H0, h0_stride, clips, F, T, K, n_iter, beta, d_W, w_stride, d_H, h_stride,
             (hipStream_t)stream);
  });
}
int smx_nmf_activations_f32(const float *V, const float *W, const float *H0, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta,
                            float *H) {
  return guarded(
      [&] { nmf_call("nmf_activations", false, false, 4, V, F * T, T, W, F * K, H0, K * T, clips, F, T, K, n_iter, beta, nullptr, 0, H, K * T, nullptr); });
}
int smx_nmf_activations_f64(const double *V, const double *W, const double *H0, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta,
                            double *H) {
  return guarded(
      [&] { nmf_call("nmf_activations", false, false, 8, V, F * T, T, W, F * K, H0, K * T, clips, F, T, K, n_iter, beta, nullptr, 0, H, K * T, nullptr); });
}
int smx_nmf_activations_vram_f32(const float *d_V, int64_t v_stride, int64_t v_pitch, const float *d_W, int64_t w_stride, const float *d_H0,
                                 int64_t h0_stride, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta, float *d_H, int64_t h_stride,
                                 void *stream) {
  return guarded([&] {
    nmf_call("nmf_activations", true, false, 4, d_V, v_stride, v_pitch, d_W, w_stride, d_H0, h0_stride, clips, F, T, K, n_iter, beta, nullptr, 0, d_H,
             h_stride, (hipStream_t)stream);
  });
}
int smx_nmf_reconstruct_f32(const float *W, const float *H, int64_t clips, int64_t F, int64_t T, int64_t K, const int64_t *components, int64_t n_components,
                            int as_mask, float *out) {
  return guarded([&] { reconstruct_call(false, 4, W, F * K, H, K * T, clips, F, T, K, components, n_components, as_mask, out, F * T, T, nullptr); });
}
int smx_nmf_reconstruct_f64(const double *W, const double *H, int64_t clips, int64_t F, int64_t T, int64_t K, const int64_t *components,
                            int64_t n_components, int as_mask, double *out) {
  return guarded([&] { reconstruct_call(false, 8, W, F * K, H, K * T, clips, F, T, K, components, n_components, as_mask, out, F * T, T, nullptr); });
}
int smx_nmf_reconstruct_vram_f32(const float *d_W, int64_t w_stride, const float *d_H, int64_t h_stride, int64_t clips, int64_t F, int64_t T, int64_t K,
                                 const int64_t *components, int64_t n_components, int as_mask, float *d_out, int64_t out_stride, int64_t out_pitch, void *stream) {
  return guarded([&] {
    reconstruct_call(true, 4, d_W, w_stride, d_H, h_stride, clips, F, T, K, components, n_components, as_mask, d_out, out_stride, out_pitch, (hipStream_t)stream);
  });
}
int smx_nmf_divergence_f32(const float *V, const float *W, const float *H, int64_t clips, int64_t F, int64_t T, int64_t K, int beta, float *out) {
  return guarded([&] { divergence_call(false, 4, V, F * T, T, W, F * K, H, K * T, clips, F, T, K, beta, out, nullptr); });
}
int smx_nmf_divergence_f64(const double *V, const double *W, const double *H, int64_t clips, int64_t F, int64_t T, int64_t K, int beta, double *out) {
  return guarded([&] { divergence_call(false, 8, V, F * T, T, W, F * K, H, K * T, clips, F, T, K, beta, out, nullptr); });
}
int smx_nmf_divergence_vram_f32(const float *d_V, int64_t v_stride, int64_t v_pitch, const float *d_W, int64_t w_stride, const float *d_H, int64_t h_stride,
                                int64_t clips, int64_t F, int64_t T, int64_t K, int beta, float *d_out, void *stream) {
  return guarded(
      [&] { divergence_call(true, 4, d_V, v_stride, v_pitch, d_W, w_stride, d_H, h_stride, clips, F, T, K, beta, d_out, (hipStream_t)stream); });
}

}  // extern "C"
