// Probe: the whole device's rate of bare float64 multiply-adds on the vector unit: the arithmetic floor of the YIN correlation
// (profiles/pitch/NOTES.md).  Every lane runs `reps` rounds of 16 independent v_fma_f64 from registers, nothing else in the loop;
// HIP events around one launch, the best of 5.  Prints multiply-adds per second at 4, 8 and 16 waves per compute unit.
//   hipcc -O3 --offload-arch=gfx950 tools/probes/f64_fma_rate_probe.hip -o tools/probes/f64_fma_rate_probe
#include <hip/hip_runtime.h>
#include <cstdio>

__global__ void __launch_bounds__(256) fma_loop(double *out, int reps, double s) {
  double v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = threadIdx.x * 0.001 + i;
  for (int r = 0; r < reps; ++r) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_fma_f64 %0, %0, %1, %0" : "+v"(v[i]) : "v"(s));
  }
  double acc = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc += v[i];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

int main() {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
  const int cus = prop.multiProcessorCount, reps = 4000;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  for (int per_cu : {1, 2, 4}) {
    const int blocks = cus * per_cu;
    double *out;
    if (hipMalloc(&out, (size_t)blocks * 256 * 8) != hipSuccess) return 1;
    float best = 1e30f;
    for (int t = 0; t < 6; ++t) {
      (void)hipEventRecord(e0, 0);
      hipLaunchKernelGGL(fma_loop, dim3(blocks), dim3(256), 0, 0, out, reps, 1.0000001);
      (void)hipEventRecord(e1, 0);
      if (hipEventSynchronize(e1) != hipSuccess) return 1;
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (t > 0 && ms < best) best = ms;
    }
    const double fmas = (double)blocks * 256 * reps * 64;
    printf("{\"probe\": \"f64_fma_rate\", \"compute_units\": %d, \"waves_per_cu\": %d, \"ms\": %.4f, \"fma_per_s\": %.4g}\n", cus, per_cu * 4, best,
           fmas / (best * 1e-3));
    (void)hipFree(out);
  }
  return 0;
}
