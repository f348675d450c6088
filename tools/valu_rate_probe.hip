// Issue-rate probe for the pre-split's bit gathers (presplit_bits.h): cycles per wave64
// instruction of v_mul_lo_u32, v_mul_u32_u24, v_dot4_u32_u8 and v_and_b32, from chains of
// independent instructions (8 accumulators, so latency does not limit the rate), at 1, 2 and 4
// waves per SIMD on one CU.  Not part of the library.
//   hipcc --offload-arch=gfx950 -O2 -o tools/valu_rate_probe tools/valu_rate_probe.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

constexpr int kAcc = 8, kUnroll = 32, kIters = 256;  // kAcc * kUnroll * kIters instructions per wave

enum Op { kMulLo, kMul24, kDot4, kAnd };

template <Op op>
__device__ __forceinline__ unsigned step(unsigned x, unsigned k) {
  unsigned r;
  if (op == kMulLo) asm volatile("v_mul_lo_u32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(k));
  else if (op == kMul24) asm volatile("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(x), "v"(k));
  else if (op == kDot4) asm volatile("v_dot4_u32_u8 %0, %1, %2, %1" : "=v"(r) : "v"(x), "v"(k));
  else asm volatile("v_and_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(k));
  return r;
}

// out[wave]: cycles (s_memtime) of the wave's chain; sink keeps the results alive
template <Op op>
__global__ void __launch_bounds__(1024) k_chain(unsigned long long* out, unsigned* sink, unsigned seed) {
  unsigned a[kAcc];
  for (int i = 0; i < kAcc; ++i) a[i] = seed + threadIdx.x * 2654435761u + i;
  const unsigned k = seed | 0x01010101u;
  __syncthreads();
  const unsigned long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < kIters; ++it) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int i = 0; i < kAcc; ++i) a[i] = step<op>(a[i], k);
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  unsigned s = 0;
  for (int i = 0; i < kAcc; ++i) s ^= a[i];
  if (s == 0x12345678u) sink[0] = s;  // (never true in practice: the chains stay live)
  if ((threadIdx.x & 63) == 0) out[threadIdx.x >> 6] = t1 - t0;
}

template <Op op>
static void run(const char* name, unsigned long long* d_out, unsigned* d_sink) {
  for (int waves_per_simd : {1, 2, 4}) {
    const int waves = 4 * waves_per_simd;  // one block on one CU: 4 SIMDs
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
      hipLaunchKernelGGL(k_chain<op>, dim3(1), dim3(64 * waves), 0, 0, d_out, d_sink, 12345u + rep);
      CK(hipDeviceSynchronize());
      unsigned long long h[16];
      CK(hipMemcpy(h, d_out, sizeof(unsigned long long) * waves, hipMemcpyDeviceToHost));
      unsigned long long mx = 0;
      for (int w = 0; w < waves; ++w) mx = h[w] > mx ? h[w] : mx;
      // per SIMD: waves_per_simd chains share the issue port
      const double per = (double)mx / ((double)kAcc * kUnroll * kIters * waves_per_simd);
      best = per < best ? per : best;
    }
    std::printf("%-14s %d waves/SIMD: %.2f counter ticks per wave instruction\n", name, waves_per_simd, best);
  }
}

int main() {
  unsigned long long* d_out;
  unsigned* d_sink;
  CK(hipMalloc(&d_out, sizeof(unsigned long long) * 16));
  CK(hipMalloc(&d_sink, sizeof(unsigned)));
  // (ticks are those of __builtin_readcyclecounter; v_and_b32 is the full-rate yardstick, so the
  // ratios to it are what counts)
  run<kAnd>("v_and_b32", d_out, d_sink);
  run<kMulLo>("v_mul_lo_u32", d_out, d_sink);
  run<kMul24>("v_mul_u32_u24", d_out, d_sink);
  run<kDot4>("v_dot4_u32_u8", d_out, d_sink);
  std::printf("done\n");
  return 0;
}
