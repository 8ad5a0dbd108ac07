// bogp_thompson_phases.h -- the two matrix phases of a sample-path kernel, shared by k_thompson (kernels_thompson.hip) and
// k_thompson_constrained (kernels_thompson_constrained.hip): one wave, 16 rows x 16 columns in ONE v_mfma_f64_16x16x4_f64 accumulator
// acc[row][column]: D row = (lane >> 4) + 4 reg, D column = lane & 15.  What a column means (a path of one target, a member's path of
// target t) is the caller's; the order of every sum here depends on N, d and L alone.
//   thompson_feature_term, per tile of 16 features f0 ..: the phase tile TRANSPOSED, P[feature][row] = Omega_tile X^T, ceil(d / 4) k-steps
//     with A = Omega[f0 + (l & 15)][4 s + (l >> 4)], B = X[c0 + (l & 15)][4 s + (l >> 4)] (zero past d).  Register reg of lane l then holds
//     feature f0 + 4 reg + (l >> 4) of row l & 15: after + phase and cos it IS the A operand A[row = l & 15][k = l >> 4] of the k-step
//     over the features f0 + 4 reg .. + 3, whose B is W[f0 + 4 reg + (l >> 4)][column l & 15] -- four steps into acc, no lane movement,
//     no LDS;
//   thompson_conditioning_term: acc += rT_tile C, A = rT[(n0 + (l >> 4)) ld + c0 + (l & 15)], B = C[n0 + (l >> 4)][l & 15], n ascending
//     in steps of 4 (the four waves read one 512-byte run per n row); rows n >= N are masked to zero, C arrives zero padded to a
//     multiple of 4 rows.
// Neither drains acc: the caller does, in front of its epilogue.
#pragma once
#include "bogp_mfma.h"

namespace bogp {

// Operands built by VALU code (selects, cos, the zeroed accumulator) must have retired (bogp_mfma.h, 4.): the nop pins all three in
// registers two wait states ahead of the instruction.
__device__ __forceinline__ void mfma16t(double a, double b, d4& c) {
  asm volatile("s_nop 1" : "+v"(a), "+v"(b), "+v"(c));
  mfma16(a, b, c);
}

// xp: row c0 + (lane & 15) of X, dereferenced under xrow only.  W: [L][16].
__device__ __forceinline__ void thompson_feature_term(const double* omega, const double* phase, const double* W, int L, int d,
                                                      const double* xp, bool xrow, int li, int lk, d4& acc) {
  for (int f0 = 0; f0 < L; f0 += 16) {
    d4 ph = (d4){0.0, 0.0, 0.0, 0.0};
    const double* op = omega + (size_t)(f0 + li) * d;
    for (int k0 = 0; k0 < d; k0 += 4) {
      const int k = k0 + lk;
      const double ov = k < d ? op[k] : 0.0;
      const double xv = (k < d && xrow) ? xp[k] : 0.0;
      mfma16t(ov, xv, ph);
    }
    double wv[4], pv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wv[r] = W[(size_t)(f0 + 4 * r + lk) * 16 + li];
      pv[r] = phase[f0 + 4 * r + lk];
    }
    mfma16_drain(ph);
#pragma unroll
    for (int r = 0; r < 4; ++r) pv[r] = cos(ph[r] + pv[r]);
#pragma unroll
    for (int r = 0; r < 4; ++r) mfma16t(pv[r], wv[r], acc);
  }
}

// rp: rT + c0 + (lane & 15).  coef: [ceil(N / 4) * 4][16].
__device__ __forceinline__ void thompson_conditioning_term(const double* rp, int64_t ld, const double* coef, int N, int li, int lk,
                                                           d4& acc) {
  const int nfull = N & ~3, N4 = (N + 3) & ~3;
  int n0 = 0;
  for (; n0 + 16 <= nfull; n0 += 16) {
    double rv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rv[u] = rp[(size_t)(n0 + 4 * u + lk) * ld];
      gv[u] = coef[(size_t)(n0 + 4 * u + lk) * 16 + li];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) mfma16t(rv[u], gv[u], acc);
  }
  for (; n0 < N4; n0 += 4) {
    const int n = n0 + lk;
    const double rv = n < N ? rp[(size_t)n * ld] : 0.0;
    const double gv = coef[(size_t)n * 16 + li];
    mfma16t(rv, gv, acc);
  }
}

}  // namespace bogp
