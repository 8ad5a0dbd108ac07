// bogp_mfma.h -- the one home of the library's FP64 matrix-core idiom: v_mfma_f64_16x16x4_f64 as inline asm, and the wait states that
// inline asm makes the author's job.  Every kernel that issues the instruction includes this file; the rules are stated here once.
//
// Lanes: A = 16 k + i, B = 16 k + j, D[i][j] in lane 16 (i % 4) + j, component i / 4 (tools/probes/probe_mfma_layout.hip).
//
// 1. Why inline asm.  The accumulator must sit in ARCHITECTURAL VGPRs, tied in place ("+v"): the instruction then issues every 64 cycles
//    = the FP64 matrix peak.  The builtin lets the compiler put the accumulator in AGPRs, and the same instruction then takes ~130 cycles
//    (tools/probes/ubench_mfma16.hip, profiles/r01_ubench_mfma16.txt).  One A and one B register feed 2048 flop.
// 2. Why the drain.  The price: the compiler's hazard recogniser does not see an MFMA inside an asm string.  To the compiler the result
//    is ready at once, while the hardware needs 16 passes before anything but the next MFMA of the chain may read the accumulator.  So
//    between the last MFMA of a chain and the first other read of its accumulator there are six `s_nop 15`, placed by hand.  A missing
//    one has produced wrong factors (r03); tests/test_isa_lint.py checks the product's assembly for it.
// 3. Two forms of the drain.  mfma16_drain(c...) names the accumulators as in/out operands: no read of them can be scheduled above it.
//    mfma16_drain() has no operands (a "memory" clobber only) where there are too many accumulators to name: it orders nothing that
//    lives in registers, and the scheduler HAS hoisted an accumulator read above it (kernels_small.hip, rows 60-63 of every workgroup
//    wrong at N = 100).  So every accumulator gets an mfma16_fence() behind the operand-less drain.  The two forms compile differently:
//    a site keeps the one it has.
// 4. Operands written by the VALU (selects, moves that zero or build an accumulator, a cos) must have retired before the MFMA reads
//    them: two wait states.  Compiler-generated code in front of an asm MFMA does not get them inserted; the sites that need them carry
//    their own `s_nop` naming the operands (mma_64, k_gemm64, kernels_elim.hip: SrcC after v_mov; kernels_thompson.hip: all three).
//
// Sites that keep a text of their own, because the header cannot express them without changing their code: the drains over sixteen
// accumulators of kernels_elim.hip (BOGP_ES_ALL_ACC), and the shorter `s_nop 15; s_nop 3` drains of corr_mfma_body.inc (FP64, a chain
// of KS k-steps followed by loads) and kernels_bound32.hip (v_mfma_f32_16x16x4_f32).
#pragma once
#include <hip/hip_runtime.h>

namespace bogp {

typedef double d4 __attribute__((ext_vector_type(4)));

// c += A B; the compiler may move it among its neighbours as data flow allows
__device__ __forceinline__ void mfma16(double a, double b, d4& c) {
  asm("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// the same, volatile: stays in program order relative to the other volatile asm around it
__device__ __forceinline__ void mfma16_pinned(double a, double b, d4& c) {
  asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}

#define BOGP_MFMA16_NOPS "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15"
// the drain without operands: every accumulator needs an mfma16_fence() behind it (3. above)
__device__ __forceinline__ void mfma16_drain() { asm volatile(BOGP_MFMA16_NOPS ::: "memory"); }
__device__ __forceinline__ void mfma16_fence(d4& c) { asm volatile("" : "+v"(c)); }
// the drain that names its accumulators
__device__ __forceinline__ void mfma16_drain(d4& c) { asm volatile(BOGP_MFMA16_NOPS : "+v"(c)); }
__device__ __forceinline__ void mfma16_drain(d4& c0, d4& c1, d4& c2, d4& c3) {
  asm volatile(BOGP_MFMA16_NOPS : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
}

}  // namespace bogp
