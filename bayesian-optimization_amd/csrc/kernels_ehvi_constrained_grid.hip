// kernels_ehvi_constrained_grid.hip -- feasibility-weighted expected hypervolume improvement of an (m + c)-target model over one
// correlation chunk, the EHVI factor FACTORED over the grid that the cells of the feasible front form, and formed for the LIVE rows
// only (gfx950; FP64 VALU + LDS: as in k_ehvi_grid nothing here has the shape of a matrix product, so no matrix instruction is used).
//
// k_ehvi_constrained (kernels_ehvi_constrained.hip) states the criterion: value = E P, and +0.0 where P == 0.0, with P the product of
// the constraints' probabilities of feasibility and E the EHVI of the objectives.  It walks the C cells with a lane per row, so a
// wavefront leaves the walk only when all its 64 rows have P == 0: dead rows scattered among live ones save nothing.  Here E is
// k_ehvi_grid's factored sum (kernels_ehvi_grid.hip: E_tab = sum n_k + V values of G per row, not 2 m C), a group of lanes takes one row
// at a time, and so a dead row is simply never taken.
//
// Work split.  A workgroup owns 256 consecutive rows (one block record, as k_ehvi_constrained).
//   1   a lane per row: k_ehvi_constrained's expressions in its order -- multi_target_moments<MT, 8>, store_moments, P from 1.0 in
//       constraint order, pof_out -- so mu_out, mse_out and pof_out hold its bytes.  mu_k and sd_k = sqrt(max(MSE_k, 1e-9)) of the MO
//       objectives go to LDS (the constraints' moments never do).  live = the row exists && !(P == 0.0): a NaN P is live.
//   1b  compaction: the live rows' slots go, in row order, into ONE list in LDS -- a ballot and a popcount prefix inside the wave, the
//       waves' offsets through four words of LDS (as k_thompson_ehvi_constrained lists its feasible pairs).  L entries.
//   2   a group of GS lanes per list entry, NG = 256 / GS entries in flight, ceil(L / NG) rounds -- uniform over the workgroup, so every
//       barrier is reached by every lane; L == 0 runs none.  The groups past the list's end in the last round run on slot 256
//       (mu = 0, sd = 1) and are dropped.  Per entry: ehvi_grid_row (bogp_ehvi_grid_row.h), k_ehvi_grid's steps A, B, C and butterfly.
//   3   a lane per row: value = live ? E P : +0.0, val_out, the block's np.argmax record (first maximum, NaN maximal).
// LDS: 2 MO 257 + 256 doubles, the tables (3072 doubles where TABLED), 256 slots of the list: 55.8 KB at MO = 7, tabled.
//
// ORDER.  E of a row is k_ehvi_grid's sum in k_ehvi_grid's order: it depends on (MO, n_0 .. n_{MO-2}, V) alone -- through GS and TABLED,
// which the host derives from the table's size -- and never on M, the chunk, the row's place in the list or how many of its neighbours
// are live: an entry's group and round change which lanes and which table hold it, not one operand of one operation.
#include "bogp_device.h"
#include "bogp_ehvi_grid_row.h"
#include "bogp_internal.h"

namespace bogp {

template <int MO, int MT, int GS, bool TABLED>
__global__ __launch_bounds__(256) void k_ehvi_constrained_grid(ConstrainedEhviGridArgs a) {
  static_assert(MO >= 2 && MO < MT && MT <= 8, "objectives 2 .. MT - 1, at least one constraint");
  constexpr int NG = 256 / GS;                // entries in flight
  constexpr int TCAP = EHVI_GRID_TABLE / NG;  // doubles per table
  constexpr int LD = 257;                     // slots per target: the workgroup's rows, and slot 256 for a group without an entry
  __shared__ double s_mu[MO * LD], s_sd[MO * LD], s_val[256];
  __shared__ double s_tab[TABLED ? EHVI_GRID_TABLE : 1];
  __shared__ unsigned short s_list[256];
  __shared__ int s_wcount[4];
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;  // row inside the chunk
  const bool valid = i < a.mcount;
  const int64_t g = a.m0 + i;
  // ---- 1. moments and feasibility, a lane per row (k_ehvi_constrained's calls)
  double P = 1.0;
  if (valid) {
    double mu[MT], mse[MT];
    multi_target_moments<MT, 8>(a.rT, a.gamma, a.ld_gamma, a.N, a.ss_part, a.nJ, a.w_part, a.S, a.Mc, i, a.beta, a.G, a.estimate_trend, a.sigma2, mu, mse);
    store_moments<MT>(a.mu_out, a.mse_out, g, mu, mse);
#pragma unroll
    for (int k = 0; k < MO; ++k) {
      s_mu[k * LD + tid] = mu[k];
      s_sd[k * LD + tid] = sqrt(fmax(mse[k], 1e-9));
    }
#pragma unroll
    for (int k = MO; k < MT; ++k) P *= feasibility(mu[k], mse[k], a.sigma2[k], a.lo[k - MO], a.hi[k - MO]);
    if (a.pof_out) a.pof_out[g] = P;
  }
  if (tid < MO) {
    s_mu[tid * LD + 256] = 0.0;
    s_sd[tid * LD + 256] = 1.0;
  }
  const bool live = valid && !(P == 0.0);
  // ---- 1b. the list of the workgroup's live rows, in row order
  const int w = tid >> 6, lane = tid & 63;
  const unsigned long long mask = __ballot(live);
  if (lane == 0) s_wcount[w] = __popcll(mask);
  __syncthreads();
  int base = 0, L = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ck = s_wcount[k];
    if (k < w) base += ck;
    L += ck;
  }
  L = __builtin_amdgcn_readfirstlane(L);
  if (live) s_list[base + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)tid;
  // ---- 2. the criterion, a group of GS lanes per list entry
  const int grp = tid / GS, l = tid % GS;
  double* const tab = s_tab + (TABLED ? grp * TCAP : 0);
  int d0[MO - 1];
  grid_first_digits<MO>(a, l, d0);
  __syncthreads();
  for (int e0 = 0; e0 < L; e0 += NG) {
    const int ent = e0 + grp;
    const int slot = ent < L ? (int)s_list[ent] : 256;
    const double acc = ehvi_grid_row<MO, GS, TABLED, LD>(a, tab, s_mu + slot, s_sd + slot, l, d0);
    if (l == 0 && ent < L) s_val[slot] = acc;
  }
  __syncthreads();
  // ---- 3. values and the block's record, a lane per row
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    v = live ? s_val[tid] * P : 0.0;
    idx = g;
    a.val_out[g] = v;
  }
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (tid == 0) {
    a.blk_val[a.blk_offset + blockIdx.x] = best.v;
    a.blk_idx[a.blk_offset + blockIdx.x] = best.i;
  }
}

template <int MO, int MT>
static void launch_one(const ConstrainedEhviGridArgs& a, unsigned nblk, hipStream_t st) {
  if (!a.tabled) hipLaunchKernelGGL((k_ehvi_constrained_grid<MO, MT, 64, false>), dim3(nblk), 256, 0, st, a);
  else if (a.group == 16) hipLaunchKernelGGL((k_ehvi_constrained_grid<MO, MT, 16, true>), dim3(nblk), 256, 0, st, a);
  else hipLaunchKernelGGL((k_ehvi_constrained_grid<MO, MT, 64, true>), dim3(nblk), 256, 0, st, a);
}

// the 21 pairs 2 <= MO < MT <= BOGP_MAX_TARGETS, as launch_ehvi_constrained dispatches them
template <int MT>
static bool launch_objectives(const ConstrainedEhviGridArgs& a, unsigned nblk, hipStream_t st) {
  switch (a.m_obj) {
    case 2: if constexpr (MT > 2) { launch_one<2, MT>(a, nblk, st); return true; } break;
    case 3: if constexpr (MT > 3) { launch_one<3, MT>(a, nblk, st); return true; } break;
    case 4: if constexpr (MT > 4) { launch_one<4, MT>(a, nblk, st); return true; } break;
    case 5: if constexpr (MT > 5) { launch_one<5, MT>(a, nblk, st); return true; } break;
    case 6: if constexpr (MT > 6) { launch_one<6, MT>(a, nblk, st); return true; } break;
    case 7: if constexpr (MT > 7) { launch_one<7, MT>(a, nblk, st); return true; } break;
    default: break;
  }
  return false;
}

hipError_t launch_ehvi_constrained_grid(const ConstrainedEhviGridArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.mcount + 255) / 256);
  if (a.C < 1 || (a.group != 16 && a.group != 64) || (a.tabled && a.E > 12 * a.group)) return hipErrorInvalidValue;  // (a table the LDS does not hold)
  bool ok = false;
  switch (a.m) {
    case 3: ok = launch_objectives<3>(a, nblk, st); break;
    case 4: ok = launch_objectives<4>(a, nblk, st); break;
    case 5: ok = launch_objectives<5>(a, nblk, st); break;
    case 6: ok = launch_objectives<6>(a, nblk, st); break;
    case 7: ok = launch_objectives<7>(a, nblk, st); break;
    case 8: ok = launch_objectives<8>(a, nblk, st); break;
    default: break;
  }
  if (!ok) return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace bogp
