// corr_mfma_body.inc -- the body of kernel A' (kernels_posterior.hip), included once per kernel: k_corr_mfma with BOGP_CORR_STORE 1,
// k_corr_mfma_sums with BOGP_CORR_STORE 0.  Plain text inclusion, not a shared device function, so that the storing kernel compiles from
// the very tokens it always had (an inlined body reschedules its prologue).  Without the store nothing is written to rT -- the kernel
// has no such parameter -- while every other operation, hence every bit of mu_part / w_part, stays.
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int d = a.d;
  const int KS = (d + 3) >> 2;       // k-steps of 4 dimensions; rows d .. 4 KS - 1 of the tile are zero
  double* xs = smem;                 // [4 KS][64] theta-scaled candidate tile, k-major
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t mc0 = (int64_t)blockIdx.x * 64;
  const int64_t mg0 = a.m0 + mc0;
  for (int idx = tid; idx < 64 * d; idx += 256) {
    const int row = idx / d, k = idx - row * d;
    const int64_t gm = mg0 + row;
    const double v = gm < a.M ? Xs[gm * d + k] : 0.0;
    xs[k * 64 + row] = v * sqrt_theta[k];
  }
  for (int idx = tid + 64 * d; idx < 64 * 4 * KS; idx += 256) xs[idx] = 0.0;
  __syncthreads();
  const double pexp = kernel_exponent<KERNEL>(sqrt_theta, d);
  const int li = lane & 15, lk = lane >> 4;
  double na[4];  // |a_m|^2 of this lane's four candidates m = 16 t + li, summed in dimension order (as k_scale_transpose sums |b_n|^2)
#pragma unroll
  for (int t = 0; t < 4; ++t) na[t] = 0.0;
  for (int k = 0; k < d; ++k) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double v = xs[k * 64 + 16 * t + li];
      na[t] = __builtin_fma(v, v, na[t]);
    }
  }
  const int nb0 = blockIdx.y * a.nblk_per_split * 32;
  const int nb1 = min(a.Np, nb0 + a.nblk_per_split * 32);
  double mu[4] = {0.0, 0.0, 0.0, 0.0}, wd[4] = {0.0, 0.0, 0.0, 0.0};
  // (r06, from k_contract16d: every global address of the loop is a wave-uniform base + a lane-constant 32-bit offset, kept opaque inside the loop so that
  // hipcc selects the `v_offset, s[base]` form -- hoisted, each access cost a v_lshl_add_u64 on the FP64 pipe that the MFMAs and the profile's arithmetic share)
  unsigned offA = (unsigned)(((size_t)lk * a.Np + li) * sizeof(double));   // XthT: row lk of a k-step, training point li of the block
  unsigned offN = (unsigned)(lk * sizeof(double));                          // xnorm / gamma / w: training point 4 c + lk
#if BOGP_CORR_STORE
  unsigned offR = (unsigned)(((size_t)lk * a.Mc + li) * sizeof(double));   // rT: row 4 c + lk of the block, candidate 16 t + li
#endif
  const char* const xthB = reinterpret_cast<const char*>(XthT);
  const char* const xnB = reinterpret_cast<const char*>(xnorm);
  const char* const gaB = reinterpret_cast<const char*>(gamma);
  const char* const wvB = reinterpret_cast<const char*>(wvec);
#if BOGP_CORR_STORE
  char* const rtB = reinterpret_cast<char*>(rT + mc0);
#endif
  for (int n0 = nb0 + 16 * g; n0 < nb1; n0 += 64) {
#define BOGP_OPQ(o_) asm("" : "+v"(o_))  /* (beside EVERY access: the zero-extension must sit in the access's own basic block to be matched) */
    d4 acc[4];
    // a_m . b_n over the dimensions, four at a time
    {
      const char* __restrict__ apb = xthB + (size_t)n0 * sizeof(double);
      const double* bp = xs + lk * 64 + li;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
      constexpr int KB = 8;  // A fragments (128-byte runs of XthT: L2 round trips) requested together: 5.5 -> 5.1 ms at C3, 17.5 -> 14.3 ms at C5
      for (int ks0 = 0; ks0 < KS; ks0 += KB) {
        double av[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u)
        {
          BOGP_OPQ(offA);
          av[u] = (4 * (ks0 + u) + lk) < d ? *reinterpret_cast<const double*>(apb + (size_t)4 * (ks0 + u) * a.Np * sizeof(double) + offA) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          if (ks0 + u < KS) {
            const int ks = ks0 + u;
            const double b0 = bp[ks * 256], b1 = bp[ks * 256 + 16], b2 = bp[ks * 256 + 32], b3 = bp[ks * 256 + 48];
            mfma16_pinned(av[u], b0, acc[0]);
            mfma16_pinned(av[u], b1, acc[1]);
            mfma16_pinned(av[u], b2, acc[2]);
            mfma16_pinned(av[u], b3, acc[3]);
          }
        }
      }
    }
    // this lane's four training rows n0 + 4 c + lk: norm, gamma, w (the loads fly while the matrix pipe drains)
    double nbv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      BOGP_OPQ(offN);
      nbv[c] = *reinterpret_cast<const double*>(xnB + (size_t)(n0 + 4 * c) * sizeof(double) + offN);
    }
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");  // (shorter than mfma16_drain(): bogp_mfma.h, the sites with their own text)
#pragma unroll
    for (int t = 0; t < 4; ++t) mfma16_fence(acc[t]);
    double s2[4][4];
    bool near = false;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double nab = na[t] + nbv[c];
        const double v = __builtin_fma(-2.0, acc[t][c], nab);
        s2[t][c] = v;
        near |= v * 64.0 < nab;
      }
    if (__builtin_expect(__ballot(near) != 0ull, 0)) {
      // difference form, kernel A's operations in kernel A's order, for all 16 values of the lane in ONE loop over the dimensions (compact code:
      // sixteen unrolled per-value loops cost 40 VGPRs and an occupancy step); only the FLAGGED values take it, so that r(x*_m, x_n) never
      // depends on which other pairs share the wave
      const double* __restrict__ xr = XthT + n0 + lk;
#pragma unroll
      for (int th = 0; th < 4; th += 2) {  // two candidate tiles at a time: eight accumulators
        double e[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int c = 0; c < 4; ++c) e[t][c] = 0.0;
        const double* xc = xs + 16 * th + li;
#pragma unroll 1
        for (int k = 0; k < d; ++k) {
          double xcv[2], xrv[4];
#pragma unroll
          for (int t = 0; t < 2; ++t) xcv[t] = xc[k * 64 + 16 * t];
#pragma unroll
          for (int c = 0; c < 4; ++c) xrv[c] = xr[(size_t)k * a.Np + 4 * c];
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const double df = xcv[t] - xrv[c];
              e[t][c] = __builtin_fma(df, df, e[t][c]);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (s2[th + t][c] * 64.0 < na[th + t] + nbv[c]) s2[th + t][c] = e[t][c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#if BOGP_CORR_STORE
      char* __restrict__ rrow = rtB + (size_t)(n0 + 4 * c) * a.Mc * sizeof(double);
#endif
      BOGP_OPQ(offN);
      const double gv = *reinterpret_cast<const double*>(gaB + (size_t)(n0 + 4 * c) * sizeof(double) + offN);
      const double wv = *reinterpret_cast<const double*>(wvB + (size_t)(n0 + 4 * c) * sizeof(double) + offN);
#if BOGP_CORR_STORE
      BOGP_OPQ(offR);
#endif
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double r = corr_profile<KERNEL>(s2[t][c], pexp);
#if BOGP_CORR_STORE
        *reinterpret_cast<double*>(rrow + 16 * t * sizeof(double) + offR) = r;
#endif
        mu[t] = __builtin_fma(r, gv, mu[t]);
        wd[t] = __builtin_fma(r, wv, wd[t]);
      }
    }
  }
  // reduce over the 4 waves x 4 row groups of a lane (fixed order) -> partial sums of this slice
  __syncthreads();
  double* red = smem;  // [2][16][64]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    red[(4 * g + lk) * 64 + 16 * t + li] = mu[t];
    red[1024 + (4 * g + lk) * 64 + 16 * t + li] = wd[t];
  }
  __syncthreads();
  if (tid < 64) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      s0 += red[j * 64 + tid];
      s1 += red[1024 + j * 64 + tid];
    }
    mu_part[(size_t)blockIdx.y * a.Mc + mc0 + tid] = s0;
    w_part[(size_t)blockIdx.y * a.Mc + mc0 + tid] = s1;
  }
