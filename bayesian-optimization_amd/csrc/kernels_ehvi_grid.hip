// kernels_ehvi_grid.hip -- expected hypervolume improvement of an m-target model over one correlation chunk, FACTORED over the grid
// that the cells of a front form (gfx950; FP64 VALU + LDS: the criterion is sums of products of a few transcendental values per
// row, nothing in it has the shape of a matrix product, so no matrix instruction is used).
//
// k_ehvi (kernels_ehvi.hip) walks the C cells per row and forms 2 m values of G per cell.  The cells of pareto.hypercell_bounds are
// a grid: axis k < m - 1 has n_k intervals [e_k[i], e_k[i + 1]) (e_k[n_k] = +inf), the columns are their products, row-major with
// axis 0 slowest, and column c is the cell [column] x [last_val[last_idx[c]], +inf).  Per candidate row, with the moments and
// sd_k = sqrt(max(MSE_k, 1e-9)) exactly as k_ehvi forms them (multi_target_moments, a lane per row: the same bytes in mu_out / mse_out),
//   g_k[i]    = G((e_k[i] - mu_k) / sd_k),  G(z) = phi(z) - z Phi(-z) (ehvi_G),  g_k[n_k] = 0 exactly        k < m - 1
//   t_k[i]    = sd_k (g_k[i] - g_k[i + 1])                                                                   i < n_k
//   t_last[v] = sd_{m-1} G((last_val[v] - mu_{m-1}) / sd_{m-1})                                              v < V
//   EHVI      = sum_c (((t_0[i_0(c)] t_1[i_1(c)]) ... t_{m-2}[i_{m-2}(c)]) t_last[last_idx[c]])
// -- the factors ehvi_cells multiplies per cell, each formed once: E = sum n_k + V values of G per row instead of 2 m C.
//
// Work split.  A workgroup owns 256 consecutive rows (one block record, as k_ehvi).  Phase 1, a lane per row: moments, stores, mu_k
// and sd_k to LDS.  Phase 2: a GROUP of GS lanes (16 where E <= 192, else 64) takes one row at a time, 256 / GS rows in flight,
// GS rounds; the rows of a workgroup's last, partial block that do not exist run on mu = 0, sd = 1 and are dropped, so that every
// barrier is reached by every lane.  Per row:
//   A. the group's lanes are dealt over the E table entries (entry e to lane e mod GS): g, or t_last, into the row's table in LDS;
//   B. the same deal over the entries of the axes: t_k[i] = sd_k (g[e] - g[e + 1]) in place (a round reads before it writes, and
//      later rounds lie above it), 0 for g behind an axis' last interval;
//   C. the lanes are dealt over the columns (column c to lane c mod GS).  A lane keeps its column's digits (i_0 .. i_{m-2}) and adds
//      GS to them in the grid's mixed radix per round (args.step: one add, compare and subtract per axis, no division); per column
//      m LDS reads, one coalesced read of last_idx (the same for every row: L2 / vL1D resident) and m multiplications.
// Each table is 12 GS doubles (EHVI_GRID_TABLE = 3072 per workgroup).  A grid with E > 768 -- two objectives and a front past 383
// points, or a lopsided hand-made grid -- has no table: phase C forms its column's m factors from G directly (TABLED = false),
// lanes over columns as above, which is k_ehvi's work spread over 64 lanes.
//
// ORDER.  It depends on (m, n_0 .. n_{m-2}, V) alone -- through GS and TABLED, which the host derives from E -- never on M, the chunk,
// the row or its neighbours.  Product of a column: axes 0, 1, .. m - 2 from the left, then t_last.  Sum of a row: lane l of the group
// adds its columns l, l + GS, l + 2 GS, .. in that order from 0.0; the GS partials are folded by a butterfly over lane distances
// GS / 2, GS / 4, .. 1 (p_l + p_{l xor d}: every lane holds the same bits after each stage).
// np.argmax order over the rows (first maximum, NaN maximal) into the per-block records, as k_ehvi.
#include "bogp_device.h"
#include "bogp_ehvi_grid_row.h"
#include "bogp_internal.h"

namespace bogp {

template <int MT, int GS, bool TABLED>
__global__ __launch_bounds__(256) void k_ehvi_grid(EhviGridArgs a) {
  constexpr int NG = 256 / GS;              // rows in flight
  constexpr int TCAP = EHVI_GRID_TABLE / NG;  // doubles per table
  __shared__ double s_mu[MT * 256], s_sd[MT * 256], s_val[256];
  __shared__ double s_tab[TABLED ? EHVI_GRID_TABLE : 1];
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;  // row inside the chunk
  const bool valid = i < a.mcount;
  const int64_t g = a.m0 + i;
  // ---- 1. moments, a lane per row (k_ehvi's calls)
  if (valid) {
    double mu[MT], mse[MT];
    multi_target_moments<MT>(a, i, mu, mse);
    store_moments<MT>(a.mu_out, a.mse_out, g, mu, mse);
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      s_mu[k * 256 + tid] = mu[k];
      s_sd[k * 256 + tid] = sqrt(fmax(mse[k], 1e-9));
    }
  } else {
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      s_mu[k * 256 + tid] = 0.0;
      s_sd[k * 256 + tid] = 1.0;
    }
  }
  // ---- 2. the criterion, a group of GS lanes per row
  const int grp = tid / GS, l = tid % GS;
  double* const tab = s_tab + (TABLED ? grp * TCAP : 0);
  int d0[MT - 1];
  grid_first_digits<MT>(a, l, d0);
  __syncthreads();
  for (int it = 0; it < GS; ++it) {  // steps A, B, C and the butterfly: bogp_ehvi_grid_row.h
    const int row = it * NG + grp;
    const double acc = ehvi_grid_row<MT, GS, TABLED, 256>(a, tab, s_mu + row, s_sd + row, l, d0);
    if (l == 0) s_val[row] = acc;
  }
  __syncthreads();
  // ---- 3. values and the block's record, a lane per row
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    v = s_val[tid];
    idx = g;
    a.ehvi_out[g] = v;
  }
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (tid == 0) {
    a.blk_val[a.blk_offset + blockIdx.x] = best.v;
    a.blk_idx[a.blk_offset + blockIdx.x] = best.i;
  }
}

template <int MT>
static void launch_ehvi_grid_m(const EhviGridArgs& a, unsigned nblk, hipStream_t st) {
  if (!a.tabled) hipLaunchKernelGGL((k_ehvi_grid<MT, 64, false>), dim3(nblk), 256, 0, st, a);
  else if (a.group == 16) hipLaunchKernelGGL((k_ehvi_grid<MT, 16, true>), dim3(nblk), 256, 0, st, a);
  else hipLaunchKernelGGL((k_ehvi_grid<MT, 64, true>), dim3(nblk), 256, 0, st, a);
}

hipError_t launch_ehvi_grid(const EhviGridArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.mcount + 255) / 256);
  if ((a.group != 16 && a.group != 64) || (a.tabled && a.E > 12 * a.group)) return hipErrorInvalidValue;  // (a table the LDS does not hold)
  switch (a.m) {
    case 2: launch_ehvi_grid_m<2>(a, nblk, st); break;
    case 3: launch_ehvi_grid_m<3>(a, nblk, st); break;
    case 4: launch_ehvi_grid_m<4>(a, nblk, st); break;
    case 5: launch_ehvi_grid_m<5>(a, nblk, st); break;
    case 6: launch_ehvi_grid_m<6>(a, nblk, st); break;
    case 7: launch_ehvi_grid_m<7>(a, nblk, st); break;
    case 8: launch_ehvi_grid_m<8>(a, nblk, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bogp
