// Probe: LDS cost of the access patterns of the 32-lane frame pipeline (stft_fast_p32.hpp), per wave-instruction and CU,
// with 8 and 16 waves per CU all issuing the same pattern back to back (throughput) and with one wave (latency-ish).
//   T0 transposition write   lane l (of 32; two frames per wave in columns 2w, 2w+1): cell l + 33 j      ds_write_b32
//   T1 transposition read    cell i + 33 l                                                             ds_read_b32
//   T2 result write          row l + 32 s                                                              ds_write_b32
//   T3 flush read            rows {0-3,16-19} + 4 h, 4 floats per lane                                  ds_read_b32 x4 (or read2)
//   T4 table read            lane-contiguous float2                                                    ds_read_b64
//   T5 plain                 lane-contiguous float                                                     ds_read_b32 / T6 ds_write_b32
// Wave-contiguous regions (a wave owns 2116 contiguous dwords of a tile buffer instead of two columns of pitch 17), bursts as
// the kernel issues them (no wait inside a burst), figures per VALUE (a dword per lane) so that the forms compare:
//   T11 lane-indexed store    register j of all 64 lanes -> 66 j + lane                    ds_write_addtid_b32 (M0 = region)
//   T12 row read              lane (h, k1): row k1 of pitch 66, dwords 32 h + 2 m, + 1       ds_read_b64
//   T13 T11 + T12             one plane of the transposition in the new layout (T8 is today's)
//   T14 exchange read, pitch 64   lane l: dword (32 - l) & 31 + 32 h of row 15 - s (lane 0: row 16 - s)   ds_read_b32
//   T15 exchange read today   cell 33 (32 - l) + 15 - s of the column (lane 0: cell 16 - s), 2-way between lanes 0 and 31
//   T16 result write          64 s + lane by ds_write_addtid_b32 and 64 (31 - s) + 32 h + 32 - l by ds_write_b32 (T2 twice is today's)
// Build: hipcc -O3 --offload-arch=gfx950 -o lds_pattern_probe lds_pattern_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
constexpr int kStride = 17, kRows = 1056;
constexpr int kRegion = 2116;   // dwords a wave owns in a tile buffer (2116 = 4 mod 32: the eight regions start on different banks)
// eight lane-indexed stores, dword offsets O0 + PITCH i from the LDS byte address `base` (wave-uniform): one statement, M0 set inside
template <int O0, int PITCH>
__device__ __forceinline__ void addtid8(unsigned base, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
  unsigned keep;   // M0 belongs to the compiler: the statement puts back what it found
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "ds_write_addtid_b32 %2 offset:%10\n\tds_write_addtid_b32 %3 offset:%11\n\tds_write_addtid_b32 %4 offset:%12\n\tds_write_addtid_b32 %5 offset:%13\n\t"
               "ds_write_addtid_b32 %6 offset:%14\n\tds_write_addtid_b32 %7 offset:%15\n\tds_write_addtid_b32 %8 offset:%16\n\tds_write_addtid_b32 %9 offset:%17\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(base), "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7),
               "n"(4 * O0), "n"(4 * (O0 + PITCH)), "n"(4 * (O0 + 2 * PITCH)), "n"(4 * (O0 + 3 * PITCH)), "n"(4 * (O0 + 4 * PITCH)),
               "n"(4 * (O0 + 5 * PITCH)), "n"(4 * (O0 + 6 * PITCH)), "n"(4 * (O0 + 7 * PITCH)) : "memory");
}
template <int PITCH>
__device__ __forceinline__ void addtid32(unsigned base, const float (&a)[32]) {
  addtid8<0, PITCH>(base, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
  addtid8<8 * PITCH, PITCH>(base, a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]);
  addtid8<16 * PITCH, PITCH>(base, a[16], a[17], a[18], a[19], a[20], a[21], a[22], a[23]);
  addtid8<24 * PITCH, PITCH>(base, a[24], a[25], a[26], a[27], a[28], a[29], a[30], a[31]);
}
// sixteen 8-byte reads of consecutive pairs from the LDS byte address `at` (per lane), then one wait
__device__ __forceinline__ void read_row_b64(unsigned at, float (&a)[32]) {
  float2 t[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(t[m]) : "v"(at), "n"(8 * m) : "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]), "+v"(t[8]), "+v"(t[9]),
               "+v"(t[10]), "+v"(t[11]), "+v"(t[12]), "+v"(t[13]), "+v"(t[14]), "+v"(t[15])::"memory");
#pragma unroll
  for (int m = 0; m < 16; ++m) { a[2 * m] += t[m].x; a[2 * m + 1] += t[m].y; }
}
template <int T>
__global__ void __launch_bounds__(1024) k(unsigned long long *cyc, int reps, float *sink) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 31, h = lane >> 5;
  const int w8 = wave & 7, g = wave >> 3;
  float *tile = lds + g * kRows * kStride;
  const int col = 2 * w8 + h;
  for (int i = threadIdx.x; i < 2 * kRows * kStride; i += blockDim.x) lds[i] = (float)i;
  __syncthreads();
  float acc[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) acc[i] = (float)(lane + i);
  const int own = l * kStride + col, rd = 33 * l * kStride + col;
  const int fr = (128 * w8 + ((l >> 2) & 3) + 16 * (l >> 4) + 4 * h) * kStride + 4 * (lane & 3);
  float2 *tab = reinterpret_cast<float2 *>(lds + 2 * kRows * kStride);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < reps; ++r) {
    if constexpr (T == 0) {
#pragma unroll
      for (int j = 0; j < 32; ++j) tile[own + 33 * kStride * j] = acc[j];
    }
    if constexpr (T == 1) {
#pragma unroll
      for (int i = 0; i < 32; ++i) acc[i] += tile[rd + kStride * i];
    }
    if constexpr (T == 2) {
#pragma unroll
      for (int s = 0; s < 32; ++s) tile[own + 32 * kStride * s] = acc[s];
    }
    if constexpr (T == 3) {
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const float *src = tile + fr + (32 * (p >> 1) + 8 * (p & 1)) * kStride;
        acc[4 * p] += src[0]; acc[4 * p + 1] += src[1]; acc[4 * p + 2] += src[2]; acc[4 * p + 3] += src[3];
      }
    }
    if constexpr (T == 4) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { const float2 w = tab[l + 32 * i]; acc[2 * i] += w.x; acc[2 * i + 1] += w.y; }
    }
    if constexpr (T == 5) {
#pragma unroll
      for (int i = 0; i < 32; ++i) acc[i] += lds[lane + 64 * i + 64 * 32 * (wave & 3)];
    }
    if constexpr (T == 6) {
#pragma unroll
      for (int i = 0; i < 32; ++i) lds[lane + 64 * i + 64 * 32 * (wave & 3)] = acc[i];
    }
    if constexpr (T == 7) {   // transposition as in the kernel: 32 writes, 32 reads, 32 writes, 32 reads (in place)
#pragma unroll
      for (int j = 0; j < 32; ++j) tile[own + 33 * kStride * j] = acc[j];
#pragma unroll
      for (int i = 0; i < 32; ++i) acc[i] = tile[rd + kStride * i];
    }
    if constexpr (T == 8) {   // round 5: the transposition with the strides swapped -- lane l writes register j to cell 33 l + j (a PAIR
      // of registers per ds_write2_b32: cells 68 bytes apart), lane k1 reads register l' from cell 33 l' + k1.  Both sides conflict free.
      const unsigned wb = (unsigned)((33 * l * kStride + col + g * kRows * kStride) * 4);
#pragma unroll
      for (int j = 0; j < 32; j += 2)
        asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(wb + (unsigned)(j >= 14 ? 14 * kStride * 4 : 0) + (unsigned)(j >= 28 ? 14 * kStride * 4 : 0)), "v"(acc[j]), "v"(acc[j + 1]),
                     "n"((j % 14) * kStride), "n"((j % 14 + 1) * kStride) : "memory");
#pragma unroll
      for (int i = 0; i < 32; ++i) acc[i] = tile[own + 33 * kStride * i];
    }
    if constexpr (T == 9) {   // the write half of T8 alone
      const unsigned wb = (unsigned)((33 * l * kStride + col + g * kRows * kStride) * 4);
#pragma unroll
      for (int j = 0; j < 32; j += 2)
        asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(wb + (unsigned)(j >= 14 ? 14 * kStride * 4 : 0) + (unsigned)(j >= 28 ? 14 * kStride * 4 : 0)), "v"(acc[j]), "v"(acc[j + 1]),
                     "n"((j % 14) * kStride), "n"((j % 14 + 1) * kStride) : "memory");
    }
    if constexpr (T == 10) {   // T7 with the reads as ds_read2_b32 (half the instructions, same LDS-array cycles)
#pragma unroll
      for (int j = 0; j < 32; ++j) tile[own + 33 * kStride * j] = acc[j];
      const unsigned rb = (unsigned)((rd + g * kRows * kStride) * 4);
      float2 t[16];
#pragma unroll
      for (int i = 0; i < 32; i += 2)
        asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(t[i / 2]) : "v"(rb + (unsigned)(i >= 14 ? 14 * kStride * 4 : 0) + (unsigned)(i >= 28 ? 14 * kStride * 4 : 0)),
                     "n"((i % 14) * kStride), "n"((i % 14 + 1) * kStride) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]), "+v"(t[8]), "+v"(t[9]),
                   "+v"(t[10]), "+v"(t[11]), "+v"(t[12]), "+v"(t[13]), "+v"(t[14]), "+v"(t[15])::"memory");
#pragma unroll
      for (int i = 0; i < 16; ++i) { acc[2 * i] = t[i].x; acc[2 * i + 1] = t[i].y; }
    }
    if constexpr (T >= 11) {
      const unsigned region = (unsigned)__builtin_amdgcn_readfirstlane(wave * kRegion * 4);   // LDS byte address of the wave's region (the dynamic LDS starts at 0)
      const unsigned row = region + (unsigned)((66 * l + 32 * h) * 4);
      if constexpr (T == 11) addtid32<66>(region, acc);
      if constexpr (T == 12) read_row_b64(row, acc);
      if constexpr (T == 13) { addtid32<66>(region, acc); read_row_b64(row, acc); }
      if constexpr (T == 14) {
        const float *xr = lds + wave * kRegion + 32 * h + ((32 - l) & 31) + (l < 1 ? 64 : 0);
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] += xr[64 * (15 - s)];
      }
      if constexpr (T == 16) {
        addtid8<0, 64>(region, acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], acc[6], acc[7]);
        addtid8<512, 64>(region, acc[8], acc[9], acc[10], acc[11], acc[12], acc[13], acc[14], acc[15]);
        float *rm = lds + wave * kRegion + 64 * 16 + 32 * h + 32 - l;   // l = 0: element 0 of the next row group
#pragma unroll
        for (int s = 0; s < 16; ++s) rm[64 * (15 - s)] = acc[16 + s];
      }
    }
    if constexpr (T == 15) {
      const float *xr = tile + (l < 1 ? 1 : 33 * (32 - l)) * kStride + col;
#pragma unroll
      for (int s = 0; s < 16; ++s) acc[s] += xr[kStride * (15 - s)];
    }
    asm volatile("" ::: "memory");
  }
  __syncthreads();
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float a = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) a += acc[i];
  sink[blockIdx.x * blockDim.x + threadIdx.x] = a;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}
// How far a lane-indexed store reaches: the ISA text gives M0[15:0] + a 16-bit offset, the LDS here has 160 KB.  Each case stores
// lane + 1 with (M0, offset) into zeroed LDS (all of it allocated, so every candidate address exists) and reports where it landed.
__global__ void __launch_bounds__(64) reach(const unsigned *m0s, int cases, int *where) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  constexpr int kDwords = 160 * 1024 / 4;
  for (int c = 0; c < cases; ++c) {
    for (int i = lane; i < kDwords; i += 64) lds[i] = 0.f;
    __syncthreads();
    unsigned keep;
    const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)m0s[c]);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tds_write_addtid_b32 %2 offset:1024\n\ts_mov_b32 m0, %0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(keep) : "s"(base), "v"((float)(lane + 1)) : "memory");
    __syncthreads();
    int found = -1;
    for (int i = 0; i < kDwords; ++i) if (lds[i] == 1.f) { found = 4 * i; break; }   // lane 0's value
    if (lane == 0) where[c] = found;
    __syncthreads();
  }
}
void run_reach() {
  const std::vector<unsigned> m0s = {0u, 4096u, 65532u, 65536u, 67712u, 100000u, 131072u, 150000u, 0x10000u + 160u * 1024u};
  unsigned *d;
  int *w;
  (void)hipMalloc(&d, m0s.size() * 4);
  (void)hipMalloc(&w, m0s.size() * 4);
  (void)hipMemcpy(d, m0s.data(), m0s.size() * 4, hipMemcpyHostToDevice);
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(reach), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(reach, dim3(1), dim3(64), 160 * 1024, 0, d, (int)m0s.size(), w);
  (void)hipDeviceSynchronize();
  std::vector<int> h(m0s.size());
  (void)hipMemcpy(h.data(), w, m0s.size() * 4, hipMemcpyDeviceToHost);
  for (size_t c = 0; c < m0s.size(); ++c) printf("lane-indexed store, M0 = %u, offset 1024: lane 0's value at LDS byte %d (M0 + 1024 = %u)\n", m0s[c], h[c], m0s[c] + 1024u);
}
template <int T>
void run(const char *name, int ops_per_rep, const char *unit = "wave-instr") {
  unsigned long long *cyc;
  float *sink;
  (void)hipMalloc(&cyc, 256 * 8);
  (void)hipMalloc(&sink, 256 * 1024 * 4);
  const int reps = 400;
  const int ldsb = 2 * kRows * kStride * 4 + 16384;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k<T>), hipFuncAttributeMaxDynamicSharedMemorySize, ldsb);
  printf("%-34s", name);
  for (int threads : {64, 256, 512, 1024}) {
    hipLaunchKernelGGL(k<T>, dim3(256), dim3(threads), ldsb, 0, cyc, reps, sink);
    hipLaunchKernelGGL(k<T>, dim3(256), dim3(threads), ldsb, 0, cyc, reps, sink);
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> h(256);
    (void)hipMemcpy(h.data(), cyc, 256 * 8, hipMemcpyDeviceToHost);
    double mean = 0;
    for (auto c : h) mean += c;
    mean /= 256;
    const int waves = threads / 64;
    printf("  %2dw: %6.2f cyc per %s per CU (%.0f per wave)", waves, mean / ((double)reps * ops_per_rep * waves), unit, mean / ((double)reps * ops_per_rep));
  }
  printf("\n");
}
int main(int argc, char **argv) {
  if (argc > 1 && argv[1][0] == 'r') { run_reach(); return 0; }
  run<0>("transposition write (b32)", 32);
  run<1>("transposition read (b32)", 32);
  run<2>("result write (b32)", 32);
  run<3>("flush read (4 floats per lane)", 32);
  run<4>("table read (b64, lane-contiguous)", 16);
  run<5>("plain read b32", 32);
  run<6>("plain write b32", 32);
  run<7>("transposition write + read", 64);
  run<8>("  strides swapped, ds_write2_b32", 64);
  run<9>("  its write half alone (write2)", 32);
  run<10>("  T7 with ds_read2_b32 reads", 64);
  // wave-contiguous regions, per value (T0-T2, T6 and T9 above are per value as they stand: one value per instruction; T9 has 16 instructions for its 32 values)
  run<9>("write2 half of T8, per value", 32, "value");
  run<11>("lane-indexed store (addtid), pitch 66", 32, "value");
  run<1>("transposition read (b32), per value", 32, "value");
  run<12>("row read (b64), pitch 66", 32, "value");
  run<8>("transposition today (T8), per value", 64, "value");
  run<13>("transposition, regions: addtid + b64", 64, "value");
  run<15>("exchange read today", 16, "value");
  run<14>("exchange read, pitch 64", 16, "value");
  run<2>("result write today (b32)", 32, "value");
  run<16>("result write, regions: addtid + b32", 32, "value");
  run_reach();
  return 0;
}
