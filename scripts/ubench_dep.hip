// micro-benchmark: how often ONE wavefront can issue v_fma_f64 when its instructions form NCH independent dependency chains
// (NCH = 1: every instruction waits for the previous result), alone on its SIMD and next to a second wavefront doing the same.
// Answers: is a single wavefront of the spectrum kernels issue-bound or latency-bound, and what does a second wavefront add?
#include <hip/hip_runtime.h>
#include <cstdio>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <int NCH, int OP>
__global__ __launch_bounds__(512) void k(double* out, int iters, double seed) {
  double a[NCH];
  for (int i = 0; i < NCH; ++i) a[i] = seed + 0.001 * (threadIdx.x + i);
  __syncthreads();
  long long t0 = clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 16 / NCH; ++r)
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        if (OP == 0) asm volatile("v_fma_f64 %0, %0, %0, %0" : "+v"(a[i]));
        if (OP == 1) asm volatile("v_mul_f64 %0, %0, %0" : "+v"(a[i]));
        if (OP == 2) asm volatile("v_add_f64 %0, %0, %0" : "+v"(a[i]));
        if (OP == 3) asm volatile("v_rcp_f64 %0, %0" : "+v"(a[i]));
        if (OP == 4) asm volatile("v_fma_f32 %0, %0, %0, %0" : "+v"(*(float*)&a[i]));
        if (OP == 5) asm volatile("v_floor_f64 %0, %0" : "+v"(a[i]));
        if (OP == 6) asm volatile("v_fract_f64 %0, %0" : "+v"(a[i]));
      }
  }
  long long t1 = clock64();
  double s = 0;
  for (int i = 0; i < NCH; ++i) s += a[i];
  out[threadIdx.x] = s;
  if ((threadIdx.x & 63) == 0) out[1024 + (threadIdx.x >> 6)] = (double)(t1 - t0) / (16.0 * iters);
}

// LDS issue-to-use latency (r13_sweep_sched): a chain of dependent reads -- every read's address is the previous address plus
// the low word of the value just loaded (always 0, which the compiler cannot know), so a link is one ds_read, the wait for it and one
// v_add_u32: cycles per link = issue-to-use latency of the read plus that one dependent instruction.  OP 0: ds_read_b64, 1: ds_read_b128.
// Lane l reads at byte offset l * stride_bytes: consecutive elements (no bank conflict beyond the instruction's own passes) or every
// second element (each bank asked twice as often: the two-pass pattern of scripts/ubench_lds.hip's even strides).
template <int OP>
__global__ __launch_bounds__(512) void kl(double* out, int iters, int stride_bytes) {
  __shared__ __align__(16) double lds[8192];
  for (int i = threadIdx.x; i < 8192; i += blockDim.x) lds[i] = 0.0;
  __syncthreads();
  unsigned addr = (unsigned)(size_t)lds + (threadIdx.x & 63) * stride_bytes;
  long long t0 = clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (OP == 0) { double v; asm volatile("ds_read_b64 %0, %1\n s_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr)); addr += (unsigned)__double2loint(v); }
      if (OP == 1) { double2 v; asm volatile("ds_read_b128 %0, %1\n s_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr)); addr += (unsigned)__double2loint(v.x); }
    }
  }
  long long t1 = clock64();
  out[threadIdx.x] = (double)addr;
  if ((threadIdx.x & 63) == 0) out[1024 + (threadIdx.x >> 6)] = (double)(t1 - t0) / (16.0 * iters);
}

int main() {
  double* d;
  CHECK(hipMalloc(&d, 2048 * sizeof(double)));
  double h[2048];
  const char* ops[] = {"v_fma_f64", "v_mul_f64", "v_add_f64", "v_rcp_f64", "v_fma_f32", "v_floor_f64", "v_fract_f64"};
#define RUN(NCH, OP, THREADS) hipLaunchKernelGGL((k<NCH, OP>), dim3(1), dim3(THREADS), 0, 0, d, 2000, 1.37); CHECK(hipDeviceSynchronize()); \
  CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost)); \
  printf("%-10s chains %2d, %d wavefront(s) per SIMD: %.2f cycles per instruction of one wavefront -> SIMD issues one every %.2f cycles\n", ops[OP], NCH, THREADS / 256, h[1024], h[1024] / (THREADS / 256));
#define ALL(OP) RUN(1, OP, 256) RUN(2, OP, 256) RUN(4, OP, 256) RUN(8, OP, 256) RUN(1, OP, 512) RUN(2, OP, 512) RUN(4, OP, 512) RUN(8, OP, 512)
  ALL(0) ALL(1) ALL(2) ALL(3) ALL(4) ALL(5) ALL(6)
  // dependent LDS reads: cycles per link, one and two wavefronts per SIMD, conflict-free and two-pass lane addresses
  const char* lops[] = {"ds_read_b64", "ds_read_b128"};
  double model = 0.0;
#define RUNL(OP, THREADS, STRIDE, WHAT) hipLaunchKernelGGL((kl<OP>), dim3(1), dim3(THREADS), 0, 0, d, 2000, STRIDE); CHECK(hipDeviceSynchronize()); \
  CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost)); \
  printf("%-12s dependent chain, %-13s lane addresses (%2d bytes apart), %d wavefront(s) per SIMD: %.2f cycles per link (read, wait, one v_add_u32)\n", \
         lops[OP], WHAT, STRIDE, THREADS / 256, h[1024]); \
  if (OP == 1 && THREADS == 512 && STRIDE == 32) model = h[1024];
#define ALLL(OP, S1, S2) RUNL(OP, 256, S1, "conflict-free") RUNL(OP, 256, S2, "two-pass") RUNL(OP, 512, S1, "conflict-free") RUNL(OP, 512, S2, "two-pass")
  ALLL(0, 8, 16) ALLL(1, 16, 32)
  // what scripts/issue_model.py takes for a table read of the angle loops: a Hermite cell (ds_read_b128) at scattered lane addresses
  // with a second wavefront on the SIMD
  printf("model latency: %.1f  (ds_read_b128, two-pass lane addresses, 2 wavefronts per SIMD)\n", model);
  return 0;
}
