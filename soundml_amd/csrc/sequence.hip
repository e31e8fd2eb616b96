// Sequence: the pairwise cost matrix of two feature sequences and dynamic time warping (Sakoe & Chiba 1978; Mueller 2007 ch. 4)
// over device-resident features X [pairs; d; n] and Y [pairs; d; m] (frames fastest).  include/soundml_amd.h words the definition
// and DESIGN.md 4.8h the orders; everything is float64 inside.
//
// Cost: every metric is ONE ascending chain over the feature index k from 0.0, each operation rounded as written (the file is built
// with -ffp-contract=off and no kernel here says fma: a difference of float32 values is not always exact in float64).  Recursion:
// cand_s = (D[prev_s] + weights_mul[s] C) + weights_add[s] for s = 0 (i-1, j-1), 1 (i, j-1), 2 (i-1, j); the first present
// candidate, then each later one only if cand < best.  Only + and < on the same operands: no order of visiting the cells can
// change a bit, so both recursion kernels and every tiling agree.
//
// Ordering between tiles is the launch order on the one stream, inside a workgroup __syncthreads(), and nothing else: no flag in
// memory is polled, no wave waits on another workgroup, every loop's trip count is fixed by the shapes.
//
//   cost_kernel          256 threads per 64 x 64 block of cells; the block's columns of X and of Y are staged in LDS as float64 in
//                        aligned 16-byte loads (an unaligned or strided row is handled at the fetch); a thread owns one index of the
//                        lane dimension and 16 of the other.  Natural form: rounded into [pairs; n; m] (cost_matrix).  Skewed form:
//                        float64 into the scratch of the tiles of ONE tile anti-diagonal, laid out [step][row of the lane][lane]
//                        as the recursion's lanes read it
//   cost_general_kernel  a thread per cell straight from memory, the same chains (SMX_DISABLE_FAST=1)
//   dtw_tile_kernel      one wave per kTileRows x kTileCols tile, one launch per tile anti-diagonal of all pairs; a lane owns kR
//                        consecutive rows and sweeps the columns skewed by its lane index (lane l is at column t - l at step t); the
//                        upper neighbour's last value arrives by one cross-lane move per step, the lane's previous column stays in
//                        registers, the costs of the next kAhead steps are in flight while this block of steps runs.  A tile reads
//                        its top row, left column and corner from the float64 edge scratches and leaves its bottom row and right
//                        column there.  STORE = false (dtw_distance): neither D nor the step codes are written
//   dtw_general_kernel   a workgroup per pair walks the anti-diagonals, a thread per cell and a barrier per diagonal, straight from
//                        memory, three float64 diagonals in scratch: any dtype (float64 always; SMX_DISABLE_FAST=1)
//   dtw_end_kernel       one wave per pair: the subsequence end (strict less, the lower index on ties), the distance, and the walk
//                        back over 64 x 64 blocks of step codes staged in LDS by the whole wave; the path goes reversed into
//                        scratch, then ascending into the output with its -1.0 tail
#include <cstring>

#include "smx_internal.hpp"

namespace smx {
namespace {

#ifndef SMX_SEQUENCE_LANE_ROWS
#define SMX_SEQUENCE_LANE_ROWS 4
#endif
#ifndef SMX_SEQUENCE_TILE_COLS
#define SMX_SEQUENCE_TILE_COLS 256
#endif
constexpr int kR = SMX_SEQUENCE_LANE_ROWS;        // consecutive rows of a lane
constexpr int kTileRows = 64 * kR;
constexpr int kTileCols = SMX_SEQUENCE_TILE_COLS;
constexpr int kTileSteps = kTileCols + 63;        // steps of a full tile: the last lane starts 63 steps late
constexpr int64_t kTileScratch = (int64_t)kTileSteps * kR * 64;   // doubles of one tile's costs, [step][row of the lane][lane]
constexpr int kAhead = 4;                         // steps whose costs are fetched as one block
constexpr int kBlock = 64;                        // the cost kernel's block edge, and the edge of a staged block of step codes
constexpr int kFeatures = 32;                     // features staged at once
constexpr int64_t kScratchBytes = 512ll << 20;    // scratch of one launch group; larger batches go pair range by pair range
constexpr int64_t kMaxCells = 1ll << 29;          // dtw: the step codes of ONE pair, a byte a cell, are the launch group's scratch
constexpr int64_t kMaxIndex = 1ll << 24;          // dtw: the path holds indices in the dtype of the input, exact in float32
static_assert(kBlock % kR == 0 && kTileRows % kBlock == 0 && kTileCols % kBlock == 0, "the cost blocks tile a tile");

struct Weights {
  double add[3], mul[3];
};

// ---- the cost ----------------------------------------------------------------------------------------------------------------------
struct Chain {                                     // the chains of one cell
  double a, xx, yy;
};

__device__ __forceinline__ void chain_step(int metric, double x, double y, Chain &c) {
  if (metric == SMX_METRIC_COSINE) {
    c.a = c.a + x * y;
    c.xx = c.xx + x * x;
    c.yy = c.yy + y * y;
  } else {
    const double diff = x - y;
    c.a = metric == SMX_METRIC_CITYBLOCK ? c.a + fabs(diff) : c.a + diff * diff;
  }
}

__device__ __forceinline__ double chain_end(int metric, const Chain &c) {
  if (metric == SMX_METRIC_COSINE) return 1.0 - c.a / (sqrt(c.xx) * sqrt(c.yy));
  return metric == SMX_METRIC_EUCLIDEAN ? sqrt(c.a) : c.a;
}

// straight from memory: column i of X against column j of Y
template <typename T>
__device__ __forceinline__ double cell_cost(const T *X, int64_t xs, const T *Y, int64_t ys, int64_t d, int64_t i, int64_t j, int metric) {
  Chain c{0.0, 0.0, 0.0};
  for (int64_t k = 0; k < d; ++k) chain_step(metric, (double)X[k * xs + i], (double)Y[k * ys + j], c);
  return chain_end(metric, c);
}

struct CostArgs {
  const void *x, *y;              // [pairs; d; n] rows xs apart, [pairs; d; m] rows ys apart
  void *out;                      // natural: [pairs; n; m] in the dtype of the input
  double *scratch;                // skewed: [pair][slot][kTileScratch]
  int64_t d, n, m, xs, ys;
  int64_t bi, bj;                 // natural: blocks along i and along j
  int metric;
  int g, q0, nq, slots;           // skewed: the tile diagonal, the first tile of this launch on it (counted from tr_lo), how many, slots per pair
  int tr_lo;
};

// count values of `row` from its element `start` on into dst, as float64: whole aligned 16-byte loads; what a load holds before
// the start or behind the end of the span lies in the same 16 bytes as a value of the span and is dropped
template <typename T>
__device__ __forceinline__ void stage_rows(const T *src, int64_t stride, int kc, int count, double *dst) {
  constexpr int E = 16 / (int)sizeof(T), G = kBlock / E + 1;
  for (int idx = threadIdx.x; idx < kc * G; idx += blockDim.x) {
    const int k = idx / G, g = idx - k * G;
    const T *row = src + (int64_t)k * stride;
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) % E);
    const int first = g * E - mis;
    if (first >= count) continue;
    const uint4 raw = *reinterpret_cast<const uint4 *>(row + first);
    T v[E];
    memcpy(v, &raw, 16);
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (first + e >= 0 && first + e < count) dst[k * kBlock + first + e] = (double)v[e];
  }
}

// SKEW: the lane dimension is the rows (in the order the recursion's lanes own them), the 16 others are columns; else the lane
// dimension is the columns, so that the rounded rows leave in whole runs
template <typename T, bool SKEW>
__global__ void __launch_bounds__(256) cost_kernel(CostArgs a) {
  __shared__ __align__(16) double xs_[kFeatures * kBlock];
  __shared__ __align__(16) double ys_[kFeatures * kBlock];
  int64_t pair, i0, j0, ti0 = 0, tj0 = 0;
  int slot = 0;
  if (SKEW) {
    constexpr int per_tile = (kTileRows / kBlock) * (kTileCols / kBlock);
    const int sub = blockIdx.x % per_tile;
    const int64_t rest = blockIdx.x / per_tile;
    const int q = (int)(rest % a.nq);
    pair = rest / a.nq;
    slot = q;
    const int tr = a.tr_lo + a.q0 + q, tc = a.g - tr;
    ti0 = (int64_t)tr * kTileRows, tj0 = (int64_t)tc * kTileCols;
    i0 = ti0 + (sub / (kTileCols / kBlock)) * kBlock;
    j0 = tj0 + (sub % (kTileCols / kBlock)) * kBlock;
  } else {
    const int64_t per_pair = a.bi * a.bj;
    pair = blockIdx.x / per_pair;
    const int64_t b = blockIdx.x % per_pair;
    i0 = (b / a.bj) * kBlock, j0 = (b % a.bj) * kBlock;
  }
  if (i0 >= a.n || j0 >= a.m) return;             // a short tile's empty blocks: the whole workgroup leaves, before any barrier
  const int ni = (int)(a.n - i0 < kBlock ? a.n - i0 : kBlock), nj = (int)(a.m - j0 < kBlock ? a.m - j0 : kBlock);
  const T *X = reinterpret_cast<const T *>(a.x) + pair * a.d * a.xs + i0;
  const T *Y = reinterpret_cast<const T *>(a.y) + pair * a.d * a.ys + j0;

  const int lane = threadIdx.x % kBlock, b = threadIdx.x / kBlock;      // b = 0 .. 3: the others are b + 4 q
  // the own index: a row in the recursion's order (16 / kR lanes' rows side by side), or a column
  const int own = SKEW ? (lane % (kBlock / kR)) * kR + lane / (kBlock / kR) : lane;
  constexpr int kOthers = kBlock / 4;
  Chain c[kOthers];
#pragma unroll
  for (int q = 0; q < kOthers; ++q) c[q] = Chain{0.0, 0.0, 0.0};
  const double *mine = SKEW ? xs_ : ys_, *theirs = SKEW ? ys_ : xs_;
  for (int64_t k0 = 0; k0 < a.d; k0 += kFeatures) {
    const int kc = (int)(a.d - k0 < kFeatures ? a.d - k0 : kFeatures);
    __syncthreads();                              // the previous features have been read
    stage_rows<T>(X + k0 * a.xs, a.xs, kc, ni, xs_);
    stage_rows<T>(Y + k0 * a.ys, a.ys, kc, nj, ys_);
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const double vo = mine[k * kBlock + own];
#pragma unroll
      for (int q = 0; q < kOthers; ++q) {
        const double vq = theirs[k * kBlock + b + 4 * q];
        chain_step(a.metric, SKEW ? vo : vq, SKEW ? vq : vo, c[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kOthers; ++q) {
    const int li = SKEW ? own : b + 4 * q, lj = SKEW ? b + 4 * q : own;
    if (li >= ni || lj >= nj) continue;
    const double v = chain_end(a.metric, c[q]);
    const int64_t i = i0 + li, j = j0 + lj;
    if (SKEW) {
      const int ri = (int)(i - ti0), rj = (int)(j - tj0);               // the cell in its tile
      const int l = ri / kR, r = ri % kR;
      a.scratch[(pair * a.slots + slot) * kTileScratch + ((int64_t)(rj + l) * kR + r) * 64 + l] = v;
    } else {
      reinterpret_cast<T *>(a.out)[(pair * a.n + i) * a.m + j] = (T)v;
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) cost_general_kernel(CostArgs a) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t pair = blockIdx.y;
  if (cell >= a.n * a.m) return;
  const int64_t i = cell / a.m, j = cell % a.m;
  const T *X = reinterpret_cast<const T *>(a.x) + pair * a.d * a.xs, *Y = reinterpret_cast<const T *>(a.y) + pair * a.d * a.ys;
  reinterpret_cast<T *>(a.out)[(pair * a.n + i) * a.m + j] = (T)cell_cost<T>(X, a.xs, Y, a.ys, a.d, i, j, a.metric);
}

// ---- the recursion -----------------------------------------------------------------------------------------------------------------
// one cell: the predecessors that exist, in the order of the steps; `<` and never fmin: a tie keeps the earlier step, a NaN never
// replaces anything, a NaN that came first stays
__device__ __forceinline__ double cell(const Weights &w, bool subseq, bool has_i, bool has_j, double diag, double left, double up, double c, int &code) {
  const double c0 = (diag + w.mul[0] * c) + w.add[0], c1 = (left + w.mul[1] * c) + w.add[1], c2 = (up + w.mul[2] * c) + w.add[2];
  bool have = has_i && has_j;
  double best = c0;
  code = 0;
  if (has_j && (!have || c1 < best)) best = c1, code = 1, have = true;
  if (has_i && (!have || c2 < best)) best = c2, code = 2, have = true;
  if (!has_i && (!has_j || subseq)) best = c, code = 1;        // (0, 0), and all of row 0 of a subsequence alignment
  return best;
}

struct TileArgs {
  const double *cost;             // [pair][slot][kTileScratch]
  double *hrow;                   // [pair][tile row][m]: the bottom row of every tile row
  double *vcol;                   // [pair][tile col][n]: the right column of every tile column
  void *D;                        // float32 [pair][n][m] (STORE)
  unsigned char *steps;           // [pair][n][m] (STORE)
  int64_t n, m;
  int tile_rows, tile_cols, g, tr_lo, q0, nq, slots, subseq;
  Weights w;
};

template <bool STORE>
__global__ void __launch_bounds__(64) dtw_tile_kernel(TileArgs a) {
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x / a.nq;
  const int q = (int)(blockIdx.x % a.nq);
  const int tr = a.tr_lo + a.q0 + q, tc = a.g - tr;
  const int64_t i0 = (int64_t)tr * kTileRows, j0 = (int64_t)tc * kTileCols;
  const int rows = (int)(a.n - i0 < kTileRows ? a.n - i0 : kTileRows), cols = (int)(a.m - j0 < kTileCols ? a.m - j0 : kTileCols);
  const double *cost = a.cost + (pair * a.slots + q) * kTileScratch;
  const double *top = tr ? a.hrow + (pair * a.tile_rows + (tr - 1)) * a.m + j0 : nullptr;
  double *bottom = a.hrow + (pair * a.tile_rows + tr) * a.m + j0;
  const double *ledge = tc ? a.vcol + (pair * a.tile_cols + (tc - 1)) * a.n + i0 : nullptr;
  double *redge = a.vcol + (pair * a.tile_cols + tc) * a.n + i0;
  const bool subseq = a.subseq != 0;
  const Weights w = a.w;
  const int li0 = lane * kR;

  double left[kR];                                // the lane's rows at its previous column
#pragma unroll
  for (int r = 0; r < kR; ++r) left[r] = (ledge && li0 + r < rows) ? ledge[li0 + r] : 0.0;
  double diag = 0.0;                              // the row above the lane's first, at the previous column
  if (ledge) {
    if (lane) diag = li0 - 1 < rows ? ledge[li0 - 1] : 0.0;
    else if (top) diag = top[-1];                 // the corner: the tile row above left it, two launches ago
  }
  double last = 0.0;                              // the lane's last row at its current column: the lane below takes it
  double topc = (top && lane < cols) ? top[lane] : 0.0, topn = 0.0;   // 64 values of the top row, and the next 64 in flight
  const int lanes = (rows + kR - 1) / kR, nsteps = cols + lanes - 1;

  double cur[kAhead][kR], nxt[kAhead][kR];
  auto fetch = [&](double (&into)[kAhead][kR], int t0) {
#pragma unroll
    for (int s = 0; s < kAhead; ++s)
#pragma unroll
      for (int r = 0; r < kR; ++r) into[s][r] = t0 + s < kTileSteps ? cost[((int64_t)(t0 + s) * kR + r) * 64 + lane] : 0.0;
  };
  fetch(cur, 0);
  for (int tb = 0; tb < nsteps; tb += kAhead) {
    fetch(nxt, tb + kAhead);
#pragma unroll
    for (int s = 0; s < kAhead; ++s) {
      const int t = tb + s;
      if (t >= nsteps) break;                     // the same for every lane
      if ((t & 63) == 0) {
        if (t) topc = topn;
        topn = (top && t + 64 + lane < cols) ? top[t + 64 + lane] : 0.0;
      }
      double up = __shfl_up(last, 1);
      const double t0 = __shfl(topc, t & 63);
      if (lane == 0) up = t0;
      const int c = t - lane;
      const bool on = c >= 0 && c < cols;
      const int64_t j = j0 + c;
      double dg = diag, u = up;
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const int li = li0 + r;
        const int64_t i = i0 + li;
        const double old = left[r];
        int code;
        const double best = cell(w, subseq, i > 0, j > 0, dg, old, u, cur[s][r], code);
        if (on && li < rows) {
          left[r] = best;
          if (STORE) {
            reinterpret_cast<float *>(a.D)[(pair * a.n + i) * a.m + j] = (float)best;
            a.steps[(pair * a.n + i) * a.m + j] = (unsigned char)code;
          }
          if (li == rows - 1) bottom[c] = best;
        }
        dg = old, u = best;
      }
      if (on) diag = up;
      last = left[kR - 1];
    }
#pragma unroll
    for (int s = 0; s < kAhead; ++s)
#pragma unroll
      for (int r = 0; r < kR; ++r) cur[s][r] = nxt[s][r];
  }
#pragma unroll
  for (int r = 0; r < kR; ++r)
    if (li0 + r < rows) redge[li0 + r] = left[r];
}

struct GeneralArgs {
  const void *x, *y;
  double *diags;                  // [pair][3][n]
  double *lastrow;                // [pair][m]: row n - 1 in float64
  void *D;                        // [pair][n][m] in the dtype of the input, or null
  unsigned char *steps;           // [pair][n][m], or null
  int64_t d, n, m, xs, ys;
  int metric, subseq;
  Weights w;
};

template <typename T, bool STORE>
__global__ void __launch_bounds__(1024) dtw_general_kernel(GeneralArgs a) {
  const int64_t pair = blockIdx.x;
  const T *X = reinterpret_cast<const T *>(a.x) + pair * a.d * a.xs, *Y = reinterpret_cast<const T *>(a.y) + pair * a.d * a.ys;
  double *buf = a.diags + pair * 3 * a.n, *lastrow = a.lastrow + pair * a.m;
  const Weights w = a.w;
  for (int64_t g = 0; g < a.n + a.m - 1; ++g) {
    const int64_t ilo = g - (a.m - 1) > 0 ? g - (a.m - 1) : 0, ihi = g < a.n - 1 ? g : a.n - 1;
    double *now = buf + (g % 3) * a.n;
    const double *p1 = buf + ((g + 2) % 3) * a.n, *p2 = buf + ((g + 1) % 3) * a.n;   // the diagonals g - 1 and g - 2, by row
    for (int64_t i = ilo + threadIdx.x; i <= ihi; i += 1024) {
      const int64_t j = g - i;
      const double c = cell_cost<T>(X, a.xs, Y, a.ys, a.d, i, j, a.metric);
      const bool hi = i > 0, hj = j > 0;
      int code;
      const double best = cell(w, a.subseq != 0, hi, hj, hi && hj ? p2[i - 1] : 0.0, hj ? p1[i] : 0.0, hi ? p1[i - 1] : 0.0, c, code);
      now[i] = best;
      if (STORE) {
        reinterpret_cast<T *>(a.D)[(pair * a.n + i) * a.m + j] = (T)best;
        a.steps[(pair * a.n + i) * a.m + j] = (unsigned char)code;
      }
      if (i == a.n - 1) lastrow[j] = best;
    }
    __syncthreads();
  }
}

// ---- the end and the way back --------------------------------------------------------------------------------------------------
struct EndArgs {
  const double *lastrow;          // row n - 1 of every pair in float64, pairs lr_stride apart
  int64_t lr_stride;
  const unsigned char *steps;     // [pair][n][m], or null: the distance alone
  int *rev;                       // scratch [pair][2 (n + m - 1)]: the path from its end, (i, j) by (i, j)
  void *path;                     // [pair][2][n + m - 1] in the dtype of the call
  void *dist;                     // [pair] in the dtype of the call, or null
  int64_t n, m;
  int subseq;
};

template <typename T>
__global__ void __launch_bounds__(64) dtw_end_kernel(EndArgs a) {
  __shared__ unsigned char blk[kBlock][kBlock];
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x, n = a.n, m = a.m;
  const double *row = a.lastrow + pair * a.lr_stride;
  int64_t jend = m - 1;
  if (a.subseq) {
    // the sequential rule (start at 0, replace only if strictly smaller) by lanes: a NaN at 0 stays; otherwise the least value
    // that is a number, at its lowest index
    double bv = 0.0;
    int64_t bj = -1;
    for (int64_t j = lane; j < m; j += 64) {
      const double v = row[j];
      if (v == v && (bj < 0 || v < bv)) bv = v, bj = j;
    }
    for (int o = 32; o; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int64_t oj = __shfl_xor(bj, o);
      if (oj >= 0 && (bj < 0 || ov < bv || (ov == bv && oj < bj))) bv = ov, bj = oj;
    }
    const double first = row[0];
    jend = (first != first || bj < 0) ? 0 : bj;
  }
  if (a.dist && lane == 0) reinterpret_cast<T *>(a.dist)[pair] = (T)row[jend];
  if (!a.steps) return;

  const unsigned char *steps = a.steps + pair * n * m;
  const int64_t L = n + m - 1;
  int *rev = a.rev + pair * 2 * L;
  int64_t i = n - 1, j = jend, count = 0;
  bool done = false;
  // a block has the current cell in its last row and column: the walk stays inside for at least kBlock cells, or ends there
  const int64_t blocks = L / kBlock + 2;
  for (int64_t round = 0; round < blocks && !done; ++round) {
    const int64_t bi0 = i - (kBlock - 1) > 0 ? i - (kBlock - 1) : 0, bj0 = j - (kBlock - 1) > 0 ? j - (kBlock - 1) : 0;
    const int nr = (int)(i - bi0 + 1), nc = (int)(j - bj0 + 1);
    __syncthreads();
    if (lane < nc)
      for (int r = 0; r < nr; ++r) blk[r][lane] = steps[(bi0 + r) * m + bj0 + lane];
    __syncthreads();
    for (int s = 0; s < 2 * kBlock; ++s) {        // every lane walks the same way: one LDS byte per cell, read by all
      if (i < bi0 || j < bj0) break;
      if (lane == 0) rev[2 * count] = (int)i, rev[2 * count + 1] = (int)j;
      ++count;
      if (i == 0 && (j == 0 || a.subseq)) {
        done = true;
        break;
      }
      int code = blk[i - bi0][j - bj0];
      if (i == 0) code = 1;                       // whatever the byte says, the walk stays inside the matrix and i + j falls
      else if (j == 0) code = 2;
      if (code == 1) --j;
      else if (code == 2) --i;
      else --i, --j;
    }
  }
  __syncthreads();                                // lane 0's reversed path is visible to the wave
  T *out = reinterpret_cast<T *>(a.path) + pair * 2 * L;
  for (int64_t q = lane; q < L; q += 64) {
    const bool in = q < count;
    out[q] = in ? (T)rev[2 * (count - 1 - q)] : (T)-1;
    out[L + q] = in ? (T)rev[2 * (count - 1 - q) + 1] : (T)-1;
  }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
struct Plan {
  int64_t d, n, m;
  int metric;
  Weights w;
  bool subseq;
};

// the metric, then d, n, m, then the weights (dtw), then the caps of the path (dtw with its path)
void check_plan(const char *fn, int64_t d, int64_t n, int64_t m, int metric, const double *add, const double *mul, bool recursion, bool path, int elem_bytes) {
  if (metric < SMX_METRIC_EUCLIDEAN || metric > SMX_METRIC_COSINE)
    throw InvalidArgument(format("%s: unknown metric %d (euclidean 0, sqeuclidean 1, cityblock 2, cosine 3)", fn, metric));
  if (d < 1) throw InvalidArgument(format("%s: cannot compare frames of %lld features (X is [%lld; %lld])", fn, (long long)d, (long long)d, (long long)n));
  if (n < 1 || m < 1)
    throw InvalidArgument(format("%s: cannot align sequences of %lld and %lld frames (both must have at least 1)", fn, (long long)n, (long long)m));
  if (!recursion) return;
  if (!add || !mul) throw Failure(format("%s: null weights", fn));
  for (int s = 0; s < 3; ++s)
    if (!std::isfinite(add[s]) || !std::isfinite(mul[s]))
      throw InvalidArgument(format("%s: cannot weigh step %d by %g and %g (weights_mul and weights_add must be finite)", fn, s, mul[s], add[s]));
  if (!path) return;
  if (n > kMaxCells / m)
    throw InvalidArgument(format("%s: the step codes of %lld x %lld cells exceed the scratch of one launch group (n m must not exceed %lld; dtw_distance has no such cap)",
                                 fn, (long long)n, (long long)m, (long long)kMaxCells));
  if (elem_bytes == 4 && (n > kMaxIndex || m > kMaxIndex))
    throw InvalidArgument(format("%s: a float32 path cannot hold the indices of %lld and %lld frames exactly (at most %lld each)", fn, (long long)n,
                                 (long long)m, (long long)kMaxIndex));
}

void check_extents(const char *fn, int64_t pairs, const Plan &p, int64_t xs, int64_t ys) {
  if (pairs < 0) throw Failure(format("%s: negative extent (pairs %lld)", fn, (long long)pairs));
  if (xs < p.n) throw Failure(format("%s: x_stride is smaller than the frame count", fn));
  if (ys < p.m) throw Failure(format("%s: y_stride is smaller than the frame count", fn));
}

Plan make_plan(int64_t d, int64_t n, int64_t m, int metric, const double *add, const double *mul, int subseq) {
  Plan p{d, n, m, metric, {}, subseq != 0};
  for (int s = 0; s < 3; ++s) p.w.add[s] = add ? add[s] : 0.0, p.w.mul[s] = mul ? mul[s] : 1.0;
  return p;
}

CostArgs cost_args(const Plan &p, const void *d_x, int64_t xs, const void *d_y, int64_t ys) {
  CostArgs a{};
  a.x = d_x, a.y = d_y;
  a.d = p.d, a.n = p.n, a.m = p.m, a.xs = xs, a.ys = ys;
  a.metric = p.metric;
  return a;
}

void cost_dev(const char *fn, const Plan &p, int elem_bytes, const void *d_x, int64_t xs, const void *d_y, int64_t ys, int64_t pairs, void *d_out,
              hipStream_t stream) {
  if (pairs == 0) return;
  CostArgs a = cost_args(p, d_x, xs, d_y, ys);
  a.out = d_out;
  if (fast_path_disabled()) {
    const unsigned blocks = grid_x(fn, "cells", (p.n * p.m + 255) / 256, 256);
    for (int64_t p0 = 0; p0 < pairs; p0 += kMaxGridYZ) {                   // the grid's second axis holds 65535 pairs
      const int64_t np = std::min<int64_t>(kMaxGridYZ, pairs - p0);
      CostArgs b = a;
      b.x = (const char *)d_x + p0 * p.d * xs * elem_bytes, b.y = (const char *)d_y + p0 * p.d * ys * elem_bytes;
      b.out = (char *)d_out + p0 * p.n * p.m * elem_bytes;
      if (elem_bytes == 8) SMX_LAUNCH((cost_general_kernel<double>), dim3(blocks, (unsigned)np), dim3(256), 0, stream, b);
      else SMX_LAUNCH((cost_general_kernel<float>), dim3(blocks, (unsigned)np), dim3(256), 0, stream, b);
      SMX_HIP_CHECK(hipGetLastError());
    }
    return;
  }
  a.bi = (p.n + kBlock - 1) / kBlock, a.bj = (p.m + kBlock - 1) / kBlock;
  if (a.bi > kMaxGridBlocks / a.bj) throw Failure(format("%s: too many cells for one launch", fn));   // one pair's blocks, before the product
  const int64_t per_launch = std::max<int64_t>(1, clips_per_launch(a.bi * a.bj, 256));   // pair range by pair range (DESIGN.md "Launch extents")
  for (int64_t p0 = 0; p0 < pairs; p0 += per_launch) {
    const int64_t np = std::min(per_launch, pairs - p0);
    a.x = (const char *)d_x + p0 * p.d * xs * elem_bytes, a.y = (const char *)d_y + p0 * p.d * ys * elem_bytes;
    a.out = (char *)d_out + p0 * p.n * p.m * elem_bytes;
    const unsigned blocks = grid_x(fn, "cells", np * a.bi * a.bj, 256);
    if (elem_bytes == 8) SMX_LAUNCH((cost_kernel<double, false>), dim3(blocks), dim3(256), 0, stream, a);
    else SMX_LAUNCH((cost_kernel<float, false>), dim3(blocks), dim3(256), 0, stream, a);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

// The route table: float32 pairs of at least kTileMinCells cells take the tile kernel, everything else the general one.  Measured
// (profiles/sequence/NOTES.md): in a batch of 256 pairs the general kernel wins at 8 x 8 and 16 x 16, they meet at 32 x 32, and the tile
// kernel wins from there on; a single pair that small is within 0.04 ms either way
constexpr int64_t kTileMinCells = 32 * 32;
bool takes_tiles(const Plan &p, int elem_bytes) { return elem_bytes == 4 && !fast_path_disabled() && p.n * p.m >= kTileMinCells; }

int64_t align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// d_D and d_path (dtw), or d_dist (dtw_distance)
void dtw_dev(const char *fn, const Plan &p, int elem_bytes, const void *d_x, int64_t xs, const void *d_y, int64_t ys, int64_t pairs, void *d_D, void *d_path,
             void *d_dist, hipStream_t stream) {
  if (pairs == 0) return;
  const bool store = d_D != nullptr;
  const int64_t n = p.n, m = p.m, L = n + m - 1;
  const bool tiles = takes_tiles(p, elem_bytes);
  const int64_t tile_rows = (n + kTileRows - 1) / kTileRows, tile_cols = (m + kTileCols - 1) / kTileCols;
  const int64_t maxdiag = std::min(tile_rows, tile_cols);
  // per pair: the step codes and the reversed path (dtw), then the route's own float64
  const int64_t steps_bytes = store ? align16(n * m) : 0, rev_bytes = store ? align16(2 * L * 4) : 0;
  const int64_t edge_bytes = tiles ? (tile_rows * m + tile_cols * n) * 8 : (3 * n + m) * 8;
  int64_t slots = 0;
  if (tiles) {
    const int64_t room = std::max<int64_t>(kScratchBytes - steps_bytes - rev_bytes - edge_bytes, kTileScratch * 8);
    slots = std::max<int64_t>(1, std::min<int64_t>(maxdiag, room / (kTileScratch * 8)));   // a long diagonal goes in several launches
  }
  const int64_t per_pair = steps_bytes + rev_bytes + edge_bytes + slots * kTileScratch * 8;
  // a pair range fits the scratch AND every launch of its route (DESIGN.md "Launch extents"): the end kernel's wave per pair, the
  // general kernel's 1024 threads per pair, or a diagonal's cost blocks of 256 and tile waves
  constexpr int per_tile = (kTileRows / kBlock) * (kTileCols / kBlock);
  const int64_t fit = tiles ? std::min(clips_per_launch(slots * per_tile, 256), clips_per_launch(slots, 64)) : clips_per_launch(1, 1024);
  const int64_t step = std::max<int64_t>(1, std::min({pairs, kScratchBytes / per_pair, fit, clips_per_launch(1, 64)}));
  init_device_pool();
  DeviceScratch scratch;
  scratch.pool((size_t)(step * per_pair), stream);
  char *base = scratch.as<char>();
  double *wide = reinterpret_cast<double *>(base);                                    // the route's float64, every pair's
  double *costs = wide + step * (edge_bytes / 8);
  unsigned char *steps = reinterpret_cast<unsigned char *>(costs + step * slots * kTileScratch);
  int *rev = reinterpret_cast<int *>(steps + step * steps_bytes);

  for (int64_t p0 = 0; p0 < pairs; p0 += step) {
    const int64_t np = std::min(step, pairs - p0);
    const void *x = (const char *)d_x + p0 * p.d * xs * elem_bytes, *y = (const char *)d_y + p0 * p.d * ys * elem_bytes;
    void *D = store ? (char *)d_D + p0 * n * m * elem_bytes : nullptr;
    EndArgs e{};
    if (tiles) {
      double *hrow = wide, *vcol = wide + step * tile_rows * m;
      for (int64_t g = 0; g < tile_rows + tile_cols - 1; ++g) {
        const int64_t tr_lo = std::max<int64_t>(0, g - (tile_cols - 1)), tr_hi = std::min(tile_rows - 1, g);
        for (int64_t q0 = 0; q0 <= tr_hi - tr_lo; q0 += slots) {
          const int64_t nq = std::min(slots, tr_hi - tr_lo + 1 - q0);
          CostArgs c = cost_args(p, x, xs, y, ys);
          c.scratch = costs;
          c.g = (int)g, c.tr_lo = (int)tr_lo, c.q0 = (int)q0, c.nq = (int)nq, c.slots = (int)slots;
          SMX_LAUNCH((cost_kernel<float, true>), dim3(grid_x(fn, "tiles", np * nq * per_tile, 256)), dim3(256), 0, stream, c);
          SMX_HIP_CHECK(hipGetLastError());
          TileArgs t{};
          t.cost = costs, t.hrow = hrow, t.vcol = vcol, t.D = D, t.steps = steps;
          t.n = n, t.m = m;
          t.tile_rows = (int)tile_rows, t.tile_cols = (int)tile_cols, t.g = (int)g, t.tr_lo = (int)tr_lo, t.q0 = (int)q0, t.nq = (int)nq, t.slots = (int)slots;
          t.subseq = p.subseq ? 1 : 0;
          t.w = p.w;
          const unsigned waves = grid_x(fn, "tiles", np * nq, 64);
          if (store) SMX_LAUNCH((dtw_tile_kernel<true>), dim3(waves), dim3(64), 0, stream, t);
          else SMX_LAUNCH((dtw_tile_kernel<false>), dim3(waves), dim3(64), 0, stream, t);
          SMX_HIP_CHECK(hipGetLastError());
        }
      }
      e.lastrow = hrow + (tile_rows - 1) * m, e.lr_stride = tile_rows * m;
    } else {
      const dim3 grid(grid_x(fn, "pairs", np, 1024));
      GeneralArgs a{};
      a.x = x, a.y = y, a.diags = wide, a.lastrow = wide + step * 3 * n, a.D = D, a.steps = steps;
      a.d = p.d, a.n = n, a.m = m, a.xs = xs, a.ys = ys;
      a.metric = p.metric, a.subseq = p.subseq ? 1 : 0;
      a.w = p.w;
      if (elem_bytes == 8) {
        if (store) SMX_LAUNCH((dtw_general_kernel<double, true>), grid, dim3(1024), 0, stream, a);
        else SMX_LAUNCH((dtw_general_kernel<double, false>), grid, dim3(1024), 0, stream, a);
      } else {
        if (store) SMX_LAUNCH((dtw_general_kernel<float, true>), grid, dim3(1024), 0, stream, a);
        else SMX_LAUNCH((dtw_general_kernel<float, false>), grid, dim3(1024), 0, stream, a);
      }
      SMX_HIP_CHECK(hipGetLastError());
      e.lastrow = a.lastrow, e.lr_stride = m;
    }
    e.steps = store ? steps : nullptr, e.rev = rev;
    e.path = store ? (char *)d_path + p0 * 2 * L * elem_bytes : nullptr;
    e.dist = d_dist ? (char *)d_dist + p0 * elem_bytes : nullptr;
    e.n = n, e.m = m, e.subseq = p.subseq ? 1 : 0;
    const dim3 ends(grid_x(fn, "pairs", np, 64));
    if (elem_bytes == 8) SMX_LAUNCH((dtw_end_kernel<double>), ends, dim3(64), 0, stream, e);
    else SMX_LAUNCH((dtw_end_kernel<float>), ends, dim3(64), 0, stream, e);
    SMX_HIP_CHECK(hipGetLastError());
  }
}

// ---- the faces ---------------------------------------------------------------------------------------------------------------------
void cost_call(bool device, const void *x, const void *y, int elem_bytes, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t xs, int64_t ys, int metric,
               void *out, hipStream_t stream) {
  const char *fn = "cost_matrix";
  check_plan(fn, d, n, m, metric, nullptr, nullptr, false, false, elem_bytes);
  const Plan p = make_plan(d, n, m, metric, nullptr, nullptr, 0);
  check_extents(fn, pairs, p, xs, ys);
  if (pairs == 0) return;
  if (!x || !y || !out) throw Failure(format("%s: null pointer", fn));
  if (device) {
    cost_dev(fn, p, elem_bytes, x, xs, y, ys, pairs, out, stream);
    return;
  }
  const size_t eb = (size_t)elem_bytes;
  host_call(fn, {{x, (size_t)(d * n) * eb}, {y, (size_t)(d * m) * eb}}, out, (size_t)(n * m) * eb, pairs, false, nullptr,
            [&](const void *const *d_in, void *d_out, int64_t np, hipStream_t st) { cost_dev(fn, p, elem_bytes, d_in[0], n, d_in[1], m, np, d_out, st); });
}

// with_path: D and path; otherwise dist
void dtw_call(const char *fn, bool device, bool with_path, const void *x, const void *y, int elem_bytes, int64_t pairs, int64_t d, int64_t n, int64_t m,
              int64_t xs, int64_t ys, int metric, const double *add, const double *mul, int subseq, void *D, void *path, void *dist, hipStream_t stream) {
  check_plan(fn, d, n, m, metric, add, mul, true, with_path, elem_bytes);
  const Plan p = make_plan(d, n, m, metric, add, mul, subseq);
  check_extents(fn, pairs, p, xs, ys);
  if (pairs == 0) return;
  if (!x || !y || (with_path ? !D || !path : !dist)) throw Failure(format("%s: null pointer", fn));
  if (device) {
    dtw_dev(fn, p, elem_bytes, x, xs, y, ys, pairs, with_path ? D : nullptr, with_path ? path : nullptr, with_path ? nullptr : dist, stream);
    return;
  }
  const size_t eb = (size_t)elem_bytes;
  const std::vector<HostIn> in{{x, (size_t)(d * n) * eb}, {y, (size_t)(d * m) * eb}};
  if (with_path) {
    host_call(fn, in, {HostOut{D, (size_t)(n * m) * eb}, HostOut{path, (size_t)(2 * (n + m - 1)) * eb}}, pairs, false, nullptr,
              [&](const void *const *d_in, void *const *d_out, int64_t np, hipStream_t st) {
                dtw_dev(fn, p, elem_bytes, d_in[0], n, d_in[1], m, np, d_out[0], d_out[1], nullptr, st);
              });
  } else {
    host_call(fn, in, dist, eb, pairs, false, nullptr, [&](const void *const *d_in, void *d_out, int64_t np, hipStream_t st) {
      dtw_dev(fn, p, elem_bytes, d_in[0], n, d_in[1], m, np, nullptr, nullptr, d_out, st);
    });
  }
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

// ---- Sequence --------------------------------------------------------------------------------------------------------------------
int smx_sequence_tile(int64_t *rows, int64_t *cols) {
  return guarded([&] {
    if (rows) *rows = kTileRows;
    if (cols) *cols = kTileCols;
  });
}
int smx_cost_matrix_f32(const float *x, const float *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, float *out) {
  return guarded([&] { cost_call(false, x, y, 4, pairs, d, n, m, n, m, metric, out, nullptr); });
}
int smx_cost_matrix_f64(const double *x, const double *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, double *out) {
  return guarded([&] { cost_call(false, x, y, 8, pairs, d, n, m, n, m, metric, out, nullptr); });
}
int smx_cost_matrix_hbm_f32(const float *d_x, const float *d_y, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t x_stride, int64_t y_stride, int metric,
                            float *d_out, void *stream) {
  return guarded([&] { cost_call(true, d_x, d_y, 4, pairs, d, n, m, x_stride, y_stride, metric, d_out, (hipStream_t)stream); });
}
int smx_dtw_f32(const float *x, const float *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, const double *weights_add,
                const double *weights_mul, int subseq, float *D, float *path) {
  return guarded([&] { dtw_call("dtw", false, true, x, y, 4, pairs, d, n, m, n, m, metric, weights_add, weights_mul, subseq, D, path, nullptr, nullptr); });
}
int smx_dtw_f64(const double *x, const double *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, const double *weights_add,
                const double *weights_mul, int subseq, double *D, double *path) {
  return guarded([&] { dtw_call("dtw", false, true, x, y, 8, pairs, d, n, m, n, m, metric, weights_add, weights_mul, subseq, D, path, nullptr, nullptr); });
}
int smx_dtw_hbm_f32(const float *d_x, const float *d_y, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t x_stride, int64_t y_stride, int metric,
                    const double *weights_add, const double *weights_mul, int subseq, float *d_D, float *d_path, void *stream) {
  return guarded([&] {
    dtw_call("dtw", true, true, d_x, d_y, 4, pairs, d, n, m, x_stride, y_stride, metric, weights_add, weights_mul, subseq, d_D, d_path, nullptr,
             (hipStream_t)stream);
  });
}
int smx_dtw_distance_f32(const float *x, const float *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, const double *weights_add,
                         const double *weights_mul, int subseq, float *out) {
  return guarded(
      [&] { dtw_call("dtw_distance", false, false, x, y, 4, pairs, d, n, m, n, m, metric, weights_add, weights_mul, subseq, nullptr, nullptr, out, nullptr); });
}
int smx_dtw_distance_f64(const double *x, const double *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, const double *weights_add,
                         const double *weights_mul, int subseq, double *out) {
  return guarded(
      [&] { dtw_call("dtw_distance", false, false, x, y, 8, pairs, d, n, m, n, m, metric, weights_add, weights_mul, subseq, nullptr, nullptr, out, nullptr); });
}
int smx_dtw_distance_hbm_f32(const float *d_x, const float *d_y, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t x_stride, int64_t y_stride, int metric,
                             const double *weights_add, const double *weights_mul, int subseq, float *d_out, void *stream) {
  return guarded([&] {
    dtw_call("dtw_distance", true, false, d_x, d_y, 4, pairs, d, n, m, x_stride, y_stride, metric, weights_add, weights_mul, subseq, nullptr, nullptr, d_out,
             (hipStream_t)stream);
  });
}

}  // extern "C"
