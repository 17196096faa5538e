// One wave per SIMD (256 threads, one workgroup per CU): what a lane-guarded LDS store costs a wave
// that runs alone, in shader cycles per region (s_memtime around a loop of 16 regions, each between
// 8 independent v_fma_f32 as the step kernel's stream would have; the 8 v_fma alone are the baseline
// that is subtracted). The guard is a hoisted lane predicate (lane 0 of each 16-lane team) in an
// SGPR pair, the layout the step kernel's: a slice per team, stride = 16 (mod 32) words.
//   a  s_and_saveexec + s_cbranch_execz + K stores + s_or exec   (what the compiler emits today)
//   b  the same without the branch
//   c  K unconditional stores, each address ok ? addr : sink + lane (one v_cndmask per store,
//      a one-word sink slot per lane)
//   c' one v_cndmask of the base address, K stores at offsets (a K-word sink slot per lane, its words
//      16 apart: a lane's words side by side put lanes 0, 4, 8, 12 on one bank)
//   d  K unconditional stores to the lane's own words (16 apart) of v_cndmask(old, value)
//   e  K unconditional stores of a team-uniform value: the 16 lanes of a team write the same word
//   a128 / e128  one ds_write_b128 under the guard (form a) / by every lane of the team (form e)
// for K = 1, 3, 5.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/exec_region_probe tools/exec_region_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>

#define REP16(X) X X X X X X X X X X X X X X X X
constexpr int STRIDE = 528, SINK = 256, WORDS = 16 * STRIDE;  // words; 528 = 16 (mod 32)

#define FMA8                                                                                          \
  asm volatile("v_fma_f32 %0, %0, %8, %9\n\tv_fma_f32 %1, %1, %8, %9\n\tv_fma_f32 %2, %2, %8, %9\n\t" \
               "v_fma_f32 %3, %3, %8, %9\n\tv_fma_f32 %4, %4, %8, %9\n\tv_fma_f32 %5, %5, %8, %9\n\t" \
               "v_fma_f32 %6, %6, %8, %9\n\tv_fma_f32 %7, %7, %8, %9"                                 \
               : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]), "+v"(s[4]), "+v"(s[5]), "+v"(s[6]), "+v"(s[7]) \
               : "v"(sb), "v"(sc));

#define ST(k) "ds_write_b32 %[a], %[v] offset:" #k "\n\t"
#define ST1 ST(0)
#define ST3 ST(0) ST(4) ST(8)
#define ST5 ST(0) ST(4) ST(8) ST(12) ST(16)
#define CST(k) "v_cndmask_b32_e64 %[t], %[snk], %[a], %[m]\n\tds_write_b32 %[t], %[v] offset:" #k "\n\t"
#define CST1 CST(0)
#define CST3 CST(0) CST(4) CST(8)
#define CST5 CST(0) CST(4) CST(8) CST(12) CST(16)
#define DST(k) "v_cndmask_b32_e64 %[t], %[old], %[v], %[m]\n\tds_write_b32 %[own], %[t] offset:" #k "\n\t"
#define DST1 DST(0)
#define DST3 DST(0) DST(64) DST(128)
#define DST5 DST(0) DST(64) DST(128) DST(192) DST(256)
#define WST1 ST(0)
#define WST3 ST(0) ST(64) ST(128)
#define WST5 ST(0) ST(64) ST(128) ST(192) ST(256)

// FORM: 0 baseline, 1 a, 2 b, 3 c, 4 c', 5 d, 6 e, 7 a128, 8 e128; K stores per region
template <int FORM, int K>
__global__ void __launch_bounds__(256) probe(float* out, long long* cyc, int iters) {
  __shared__ float lds[WORDS];
  for (int i = threadIdx.x; i < WORDS; i += 256) lds[i] = 0.0f;
  __syncthreads();
  const int lane = threadIdx.x & 15, team = threadIdx.x >> 4;
  const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;
  const unsigned a = base + 4u * (team * STRIDE);                    // the guarded words (team-uniform address)
  const unsigned snk = base + 4u * (team * STRIDE + SINK + lane);    // one sink word per lane
  const unsigned snkw = base + 4u * (team * STRIDE + SINK + 16 + lane);  // a 5-word sink slot per lane, word k at + 16 k
  const unsigned own = base + 4u * (team * STRIDE + 64 + lane);  // the lane's own words, word k at + 16 k
  const unsigned long long m = __builtin_amdgcn_ballot_w64(lane == 0);
  float s[8], sb = 1.0001f, sc = 1e-7f, v = (float)team, old = 0.0f;
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 v4 = {v, v, v, v};
  for (int i = 0; i < 8; i++) s[i] = (float)threadIdx.x + i;
  unsigned long long sv;
  unsigned t;
  const long long t0 = clock64();
  for (int it = 0; it < iters; it++) {
#define REGION(STK, CSTK, DSTK, WSTK)                                                                                      \
  if constexpr (FORM == 1)                                                                                           \
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\ts_cbranch_execz 1f\n\t" STK "1:\n\ts_or_b64 exec, exec, %[sv]"   \
                 : [sv] "=&s"(sv) : [m] "s"(m), [a] "v"(a), [v] "v"(v) : "memory", "scc");                           \
  else if constexpr (FORM == 2)                                                                                      \
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\t" STK "s_or_b64 exec, exec, %[sv]"                               \
                 : [sv] "=&s"(sv) : [m] "s"(m), [a] "v"(a), [v] "v"(v) : "memory", "scc");                           \
  else if constexpr (FORM == 3)                                                                                      \
    asm volatile(CSTK : [t] "=&v"(t) : [m] "s"(m), [a] "v"(a), [snk] "v"(snk), [v] "v"(v) : "memory");               \
  else if constexpr (FORM == 4)                                                                                      \
    asm volatile("v_cndmask_b32_e64 %[a], %[snk], %[a0], %[m]\n\t" WSTK                                              \
                 : [a] "=&v"(t) : [m] "s"(m), [a0] "v"(a), [snk] "v"(snkw), [v] "v"(v) : "memory");                  \
  else if constexpr (FORM == 5)                                                                                      \
    asm volatile(DSTK : [t] "=&v"(t) : [m] "s"(m), [own] "v"(own), [old] "v"(old), [v] "v"(v) : "memory");           \
  else if constexpr (FORM == 6)                                                                                      \
    asm volatile(STK : : [a] "v"(a), [v] "v"(v) : "memory");                                                         \
  else if constexpr (FORM == 7)                                                                                      \
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\ts_cbranch_execz 1f\n\tds_write_b128 %[a], %[v]\n\t"              \
                 "1:\n\ts_or_b64 exec, exec, %[sv]" : [sv] "=&s"(sv) : [m] "s"(m), [a] "v"(a), [v] "v"(v4) : "memory", "scc"); \
  else if constexpr (FORM == 8)                                                                                      \
    asm volatile("ds_write_b128 %[a], %[v]" : : [a] "v"(a), [v] "v"(v4) : "memory");
#define BODY(STK, CSTK, DSTK, WSTK) REP16(FMA8 REGION(STK, CSTK, DSTK, WSTK))
    if constexpr (K == 1) { BODY(ST1, CST1, DST1, WST1) }
    else if constexpr (K == 3) { BODY(ST3, CST3, DST3, WST3) }
    else { BODY(ST5, CST5, DST5, WST5) }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const long long t1 = clock64();
  __syncthreads();
  float acc = lds[threadIdx.x];
  for (int i = 0; i < 8; i++) acc += s[i];
  out[blockIdx.x * 256 + threadIdx.x] = acc;
  if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

template <int FORM, int K>
static double run(float* out, long long* cyc_d, long long* cyc_h, int nb, int iters) {
  hipLaunchKernelGGL((probe<FORM, K>), dim3(nb), dim3(256), 0, 0, out, cyc_d, iters);
  hipLaunchKernelGGL((probe<FORM, K>), dim3(nb), dim3(256), 0, 0, out, cyc_d, iters);
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(cyc_h, cyc_d, sizeof(long long) * nb * 4, hipMemcpyDeviceToHost);
  double s = 0;
  for (int i = 0; i < nb * 4; i++) s += (double)cyc_h[i];
  return s / (nb * 4) / (iters * 16.0);  // cycles per (8 v_fma + region)
}

template <int K>
static void row(float* out, long long* cyc_d, long long* cyc_h, int nb, int iters, double base) {
  const double a = run<1, K>(out, cyc_d, cyc_h, nb, iters), b = run<2, K>(out, cyc_d, cyc_h, nb, iters),
               c = run<3, K>(out, cyc_d, cyc_h, nb, iters), c2 = run<4, K>(out, cyc_d, cyc_h, nb, iters),
               d = run<5, K>(out, cyc_d, cyc_h, nb, iters), e = run<6, K>(out, cyc_d, cyc_h, nb, iters);
  printf("  K=%d  a %6.1f  b %6.1f  c %6.1f  c' %6.1f  d %6.1f  e %6.1f\n", K, a - base, b - base, c - base, c2 - base,
         d - base, e - base);
}

int main() {
  const int nb = 256, iters = 1000;
  float* out;
  long long *cyc_d, cyc_h[nb * 4];
  (void)hipMalloc(&out, sizeof(float) * nb * 256);
  (void)hipMalloc(&cyc_d, sizeof(long long) * nb * 4);
  const double base = run<0, 1>(out, cyc_d, cyc_h, nb, iters);
  printf("one wave per SIMD, %d workgroups x 256 threads, s_memtime cycles per region (8 v_fma_f32 between regions: "
         "%.1f cycles, subtracted):\n", nb, base);
  row<1>(out, cyc_d, cyc_h, nb, iters, base);
  row<3>(out, cyc_d, cyc_h, nb, iters, base);
  row<5>(out, cyc_d, cyc_h, nb, iters, base);
  const double a128 = run<7, 1>(out, cyc_d, cyc_h, nb, iters), e128 = run<8, 1>(out, cyc_d, cyc_h, nb, iters);
  printf("  one ds_write_b128: a %6.1f  e %6.1f\n", a128 - base, e128 - base);
  hipError_t e = hipGetLastError();
  printf("status: %s\n", hipGetErrorString(e));
  return e == hipSuccess ? 0 : 1;
}
