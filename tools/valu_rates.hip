// valu_rates.hip — measure per-instruction VALU throughput on gfx950 (design input for the
// render kernel: integer multiplies for the RNG, packed fp32, transcendentals, div/sqrt sequences).
// Each kernel runs 8 independent chains of N_ITER x UNROLL inline-asm instructions per lane.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

#define N_ITER 4096
#define OP8(S) S S S S S S S S

template <int K>
__global__ void __launch_bounds__(256) k_rate(uint32_t* out, uint32_t seed) {
  uint32_t a0 = threadIdx.x ^ seed, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5,
           a6 = a0 + 6, a7 = a0 + 7;
  const uint32_t b = seed | 1;
  // a wave-uniform lane mask for the forms that read one from an SGPR pair, and where the SGPR pairs
  // a compare writes end up (so the compares stay)
  const uint64_t sm = 0x5555555555555555ull * (seed | 1);
  uint64_t sink = 0;
  for (int i = 0; i < N_ITER; ++i) {
#define DO(INS) asm volatile(INS " %0, %0, %1" : "+v"(a0) : "v"(b)); asm volatile(INS " %0, %0, %1" : "+v"(a1) : "v"(b)); \
  asm volatile(INS " %0, %0, %1" : "+v"(a2) : "v"(b)); asm volatile(INS " %0, %0, %1" : "+v"(a3) : "v"(b)); \
  asm volatile(INS " %0, %0, %1" : "+v"(a4) : "v"(b)); asm volatile(INS " %0, %0, %1" : "+v"(a5) : "v"(b)); \
  asm volatile(INS " %0, %0, %1" : "+v"(a6) : "v"(b)); asm volatile(INS " %0, %0, %1" : "+v"(a7) : "v"(b));
#define DO1(INS) asm volatile(INS " %0, %0" : "+v"(a0)); asm volatile(INS " %0, %0" : "+v"(a1)); \
  asm volatile(INS " %0, %0" : "+v"(a2)); asm volatile(INS " %0, %0" : "+v"(a3)); \
  asm volatile(INS " %0, %0" : "+v"(a4)); asm volatile(INS " %0, %0" : "+v"(a5)); \
  asm volatile(INS " %0, %0" : "+v"(a6)); asm volatile(INS " %0, %0" : "+v"(a7));
#define DO3(INS) asm volatile(INS " %0, %0, %1, %0" : "+v"(a0) : "v"(b)); asm volatile(INS " %0, %0, %1, %0" : "+v"(a1) : "v"(b)); \
  asm volatile(INS " %0, %0, %1, %0" : "+v"(a2) : "v"(b)); asm volatile(INS " %0, %0, %1, %0" : "+v"(a3) : "v"(b)); \
  asm volatile(INS " %0, %0, %1, %0" : "+v"(a4) : "v"(b)); asm volatile(INS " %0, %0, %1, %0" : "+v"(a5) : "v"(b)); \
  asm volatile(INS " %0, %0, %1, %0" : "+v"(a6) : "v"(b)); asm volatile(INS " %0, %0, %1, %0" : "+v"(a7) : "v"(b));
    if constexpr (K == 0) { DO("v_add_u32") }
    if constexpr (K == 1) { DO("v_mul_lo_u32") }
    if constexpr (K == 2) { DO("v_mul_hi_u32") }
    if constexpr (K == 3) { DO("v_mul_u32_u24") }
    if constexpr (K == 4) { DO("v_mul_f32") }
    if constexpr (K == 5) { DO3("v_fma_f32") }
    if constexpr (K == 6) { DO1("v_sqrt_f32") }
    if constexpr (K == 7) { DO1("v_rcp_f32") }
    if constexpr (K == 8) { DO1("v_sin_f32") }
    if constexpr (K == 9) { DO("v_xor_b32") }
    if constexpr (K == 10) { DO3("v_or3_b32") }
    if constexpr (K == 11) { DO("v_mul_hi_u32_u24") }
    if constexpr (K == 12) { DO1("v_rsq_f32") }
    if constexpr (K == 13) { DO3("v_med3_f32") }
#define DOB(INS) asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a0) : "v"(b)); asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a1) : "v"(b)); \
  asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a2) : "v"(b)); asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a3) : "v"(b)); \
  asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a4) : "v"(b)); asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a5) : "v"(b)); \
  asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a6) : "v"(b)); asm volatile(INS " %0, %0, %1, %0 bitop3:0x96" : "+v"(a7) : "v"(b));
    if constexpr (K == 14) { DOB("v_bitop3_b32") }
    if constexpr (K == 15) { DO1("v_cvt_f32_u32") }
    if constexpr (K == 16) { DO3("v_add3_u32") }
    if constexpr (K == 17) { DO3("v_xad_u32") }
    if constexpr (K == 18) { DO3("v_perm_b32") }
    if constexpr (K == 19) { DO3("v_lshl_add_u32") }
    if constexpr (K == 20) { DO1("v_cvt_f32_ubyte0") }
    if constexpr (K == 21) { DO1("v_cvt_f32_ubyte1") }
    if constexpr (K == 22) { DO3("v_bfi_b32") }
    if constexpr (K == 23) { DO3("v_and_or_b32") }
    if constexpr (K == 24) { DO3("v_lshl_or_b32") }
    if constexpr (K == 25) { DO1("v_cvt_f32_i32") }
    if constexpr (K == 26) { DO3("v_bfe_u32") }
    if constexpr (K == 27) { DO("v_lshrrev_b32") }
    if constexpr (K == 28) { DO("v_mul_u32_u24") }
    // what the render loop's hot blocks are full of (tools/isa_blocks.py charged these one slot
    // unmeasured): three-operand min / max, selects in both encodings, compares into an SGPR pair,
    // fma with a literal, the carry add, mbcnt
    if constexpr (K == 29) { DO3("v_min3_u32") }
    if constexpr (K == 30) { DO3("v_min3_i32") }
    if constexpr (K == 31) { DO3("v_max3_i32") }
#define EACH(M) M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
    if constexpr (K == 42) { DO("v_min_i32") }
    if constexpr (K == 43) { DO("v_max_i32") }
    if constexpr (K == 44) { DO("v_min_f32") }
    if constexpr (K == 45) { DO("v_max_u32") }
    if constexpr (K == 32) {  // VOP2: the mask is vcc (whatever it holds)
#define M(X) asm volatile("v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(X) : "v"(b));
      EACH(M)
#undef M
    }
    if constexpr (K == 33) {  // VOP3: the mask is an SGPR pair
#define M(X) asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(X) : "v"(b), "s"(sm));
      EACH(M)
#undef M
    }
    if constexpr (K == 34) {  // a compare that writes an SGPR pair (eight independent ones)
#define M(X) { uint64_t m_; asm volatile("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(m_) : "v"(X), "v"(b)); sink ^= m_; }
      EACH(M)
#undef M
    }
    if constexpr (K == 35) {
#define M(X) asm volatile("v_fmaak_f32 %0, %0, %1, 0x3fc00000" : "+v"(X) : "v"(b));
      EACH(M)
#undef M
    }
    if constexpr (K == 36) {
#define M(X) asm volatile("v_fmamk_f32 %0, %0, 0x3fc00000, %1" : "+v"(X) : "v"(b));
      EACH(M)
#undef M
    }
    if constexpr (K == 37) {  // the carry add with an SGPR pair as carry-in (the per-lane event count)
#define M(X) asm volatile("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(X) : "s"(sm) : "vcc");
      EACH(M)
#undef M
    }
    if constexpr (K == 38) { DO("v_min_u32") }
    if constexpr (K == 39) {
#define M(X) asm volatile("v_mbcnt_lo_u32_b32 %0, %1, %0" : "+v"(X) : "v"(b));
      EACH(M)
#undef M
    }
    if constexpr (K == 40) {
#define M(X) asm volatile("v_mbcnt_hi_u32_b32 %0, %1, %0" : "+v"(X) : "v"(b));
      EACH(M)
#undef M
    }
    if constexpr (K == 41) {  // the VOPC form of the same compare (writes vcc)
#define M(X) asm volatile("v_cmp_lt_u32_e32 vcc, %0, %1" : : "v"(X), "v"(b) : "vcc");
      EACH(M)
#undef M
    }
    // round 22: what selects restated as bit operations are made of, and the VOP2 select again
    if constexpr (K == 46) { DO("v_ashrrev_i32") }
    if constexpr (K == 47) { DO("v_and_b32") }
    if constexpr (K == 48) {  // the bit operation with one source in an SGPR (xor3k's form)
#define M(X) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(X) : "v"(b), "s"(seed));
      EACH(M)
#undef M
    }
    if constexpr (K == 49) { DO("v_sub_u32") }
    if constexpr (K == 50) {  // the subtract LLVM picks when it folds a compare into it (borrow to vcc)
#define M(X) asm volatile("v_subrev_co_u32_e64 %0, vcc, %0, %1" : "+v"(X) : "v"(b) : "vcc");
      EACH(M)
#undef M
    }
    if constexpr (K == 51) {  // ... with the borrow in an SGPR pair
#define M(X) { uint64_t m_; asm volatile("v_subrev_co_u32_e64 %0, %1, %0, %2" : "+v"(X), "=s"(m_) : "v"(b)); }
      EACH(M)
#undef M
    }
    if constexpr (K == 52) {  // the VOP2 select right behind the compare that writes its vcc: 8 pairs
#define M(X) asm volatile("v_cmp_lt_u32_e32 vcc, %0, %1\n v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(X) : "v"(b) : "vcc");
      EACH(M)
#undef M
    }
    if constexpr (K == 53) {  // one compare into vcc, then 8 VOP2 selects on it: 9 instructions
      asm volatile("v_cmp_lt_u32_e32 vcc, %0, %8\n v_cndmask_b32_e32 %0, %0, %8, vcc\n"
                   "v_cndmask_b32_e32 %1, %1, %8, vcc\n v_cndmask_b32_e32 %2, %2, %8, vcc\n"
                   "v_cndmask_b32_e32 %3, %3, %8, vcc\n v_cndmask_b32_e32 %4, %4, %8, vcc\n"
                   "v_cndmask_b32_e32 %5, %5, %8, vcc\n v_cndmask_b32_e32 %6, %6, %8, vcc\n"
                   "v_cndmask_b32_e32 %7, %7, %8, vcc"
                   : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                   : "v"(b) : "vcc");
    }
    if constexpr (K == 54) {  // the bit select of a VGPR mask (S2 ? S0 : S1)
#define M(X) asm volatile("v_bitop3_b32 %0, %0, %1, %0 bitop3:0xe4" : "+v"(X) : "v"(b));
      EACH(M)
#undef M
    }
    // round 30: the funnel shift that is a shift-or pair (a random word's unit-interval float), all
    // sources in VGPRs and in the render loop's form (the high word an SGPR, the shift an inline
    // constant), and the signed one-bit field extract that spreads a key bit over a word (a lane mask)
    if constexpr (K == 55) { DO3("v_alignbit_b32") }
    if constexpr (K == 56) {
#define M(X) asm volatile("v_alignbit_b32 %0, %1, %0, 9" : "+v"(X) : "s"(seed));
      EACH(M)
#undef M
    }
    if constexpr (K == 57) { DO3("v_bfe_i32") }
    if constexpr (K == 58) {
#define M(X) asm volatile("v_bfe_i32 %0, %0, 4, 1" : "+v"(X));
      EACH(M)
#undef M
    }
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7 ^ (uint32_t)sink;
}

// 64-bit / packed forms need register pairs
template <int K>
__global__ void __launch_bounds__(256) k_rate64(uint64_t* out, uint32_t seed) {
  uint64_t a0 = threadIdx.x ^ seed, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5,
           a6 = a0 + 6, a7 = a0 + 7;
  const uint64_t b = seed | 1;
  for (int i = 0; i < N_ITER; ++i) {
#define P(INS, X) asm volatile(INS : "+v"(X) : "v"(b));
    if constexpr (K == 0) {
#define M(X) asm volatile("v_pk_fma_f32 %0, %0, %1, %0" : "+v"(X) : "v"(b));
      M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
#undef M
    }
    if constexpr (K == 1) {
#define M(X) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(X) : "v"(b));
      M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
#undef M
    }
    if constexpr (K == 2) {
#define M(X) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(X) : "v"(b));
      M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
#undef M
    }
    if constexpr (K == 3) {
#define M(X) { uint32_t lo = (uint32_t)X; asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(X) : "v"(lo), "v"((uint32_t)b)); }
      M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
#undef M
    }
    if constexpr (K == 4) {
#define M(X) asm volatile("v_fma_f64 %0, %0, %1, %0" : "+v"(X) : "v"(b));
      M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
#undef M
    }
    if constexpr (K == 5) {  // the 64-bit accumulator add of the path end
#define M(X) asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(X) : "v"(b));
      M(a0) M(a1) M(a2) M(a3) M(a4) M(a5) M(a6) M(a7)
#undef M
    }
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}

template <typename F>
double time_it(F f) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  f();
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0);
  for (int r = 0; r < 5; ++r) f();
  (void)hipEventRecord(e1);
  (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1);
  return ms / 5;
}

int main() {
  hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
  const int ncu = p.multiProcessorCount;
  const int blocks = ncu * 8;  // 8 blocks x 4 waves = 32 waves/CU
  uint64_t* buf; (void)hipMalloc(&buf, sizeof(uint64_t) * blocks * 256);
  const double insts = (double)blocks * 4 * N_ITER * 8;  // wave-instructions
  auto report = [&](const char* name, double ms) {
    // cycles per wave-instruction per SIMD at 2.4 GHz nominal
    const double per_simd = insts / (ncu * 4);
    printf("%-22s %8.3f ms  %6.2f cyc/wave-instr/SIMD (@2.4GHz)  %7.2f T lane-ops/s\n", name, ms,
           ms * 1e-3 * 2.4e9 / per_simd, insts * 64 / (ms * 1e-3) / 1e12);
  };
#define R32(K, NAME) report(NAME, time_it([&] { hipLaunchKernelGGL(k_rate<K>, dim3(blocks), dim3(256), 0, 0, (uint32_t*)buf, 7u); }));
#define R64(K, NAME) report(NAME, time_it([&] { hipLaunchKernelGGL(k_rate64<K>, dim3(blocks), dim3(256), 0, 0, buf, 7u); }));
  R32(0, "v_add_u32") R32(1, "v_mul_lo_u32") R32(2, "v_mul_hi_u32") R32(3, "v_mul_u32_u24")
  R32(11, "v_mul_hi_u32_u24") R32(4, "v_mul_f32") R32(5, "v_fma_f32") R32(6, "v_sqrt_f32")
  R32(7, "v_rcp_f32") R32(12, "v_rsq_f32") R32(8, "v_sin_f32") R32(9, "v_xor_b32")
  R32(10, "v_or3_b32") R32(13, "v_med3_f32") R32(14, "v_bitop3_b32") R32(15, "v_cvt_f32_u32")
  R32(16, "v_add3_u32") R32(17, "v_xad_u32") R32(18, "v_perm_b32") R32(19, "v_lshl_add_u32")
  R32(20, "v_cvt_f32_ubyte0") R32(21, "v_cvt_f32_ubyte1") R32(22, "v_bfi_b32") R32(23, "v_and_or_b32")
  R32(24, "v_lshl_or_b32") R32(25, "v_cvt_f32_i32") R32(26, "v_bfe_u32") R32(27, "v_lshrrev_b32")
  R64(0, "v_pk_fma_f32") R64(1, "v_pk_mul_f32") R64(2, "v_pk_add_f32") R64(3, "v_mad_u64_u32")
  R64(4, "v_fma_f64") R64(5, "v_lshl_add_u64")
  R32(29, "v_min3_u32") R32(30, "v_min3_i32") R32(31, "v_max3_i32") R32(38, "v_min_u32")
  R32(42, "v_min_i32") R32(43, "v_max_i32") R32(45, "v_max_u32") R32(44, "v_min_f32")
  R32(32, "v_cndmask_b32_e32") R32(33, "v_cndmask_b32_e64") R32(34, "v_cmp_lt_u32_e64 sgpr")
  R32(41, "v_cmp_lt_u32_e32 vcc") R32(35, "v_fmaak_f32") R32(36, "v_fmamk_f32")
  R32(37, "v_addc_co_u32_e64") R32(39, "v_mbcnt_lo_u32_b32") R32(40, "v_mbcnt_hi_u32_b32")
  R32(46, "v_ashrrev_i32") R32(47, "v_and_b32") R32(48, "v_bitop3_b32 sgpr") R32(54, "v_bitop3_b32 0xe4")
  R32(49, "v_sub_u32") R32(50, "v_subrev_co_u32 vcc") R32(51, "v_subrev_co_u32 sgpr")
  R32(55, "v_alignbit_b32") R32(56, "v_alignbit_b32 s,v,9") R32(57, "v_bfe_i32") R32(58, "v_bfe_i32 v,4,1")
  // per compare + select pair, and per instruction of one compare and eight selects (9 per 8 counted)
  R32(52, "v_cmp vcc + cndmask_e32")
  report("cmp vcc, 8 cndmask_e32",
         8.0 / 9.0 * time_it([&] { hipLaunchKernelGGL(k_rate<53>, dim3(blocks), dim3(256), 0, 0, (uint32_t*)buf, 7u); }));
  printf("CUs %d clock %d kHz\n", ncu, p.clockRate);
  return 0;
}
