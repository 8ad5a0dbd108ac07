// bogp_ehvi_grid_row.h -- one candidate row's EHVI over the grid of a front's cells, evaluated by a group of GS lanes: the steps A, B, C
// and the butterfly of kernels_ehvi_grid.hip (which states the sum, the tables and the ORDER), as device functions that k_ehvi_grid and
// k_ehvi_constrained_grid (kernels_ehvi_constrained_grid.hip) both call.  `A` is the kernel's argument block: any struct with
// EhviGridArgs' grid fields (pts, last_idx, n, off, step, E, C) -- the functions read nothing else of it, so each kernel keeps the field
// order its own loop over the training points wants (bogp_internal.h).  MT counts the grid's axes: the targets of k_ehvi_grid, the
// objectives of k_ehvi_constrained_grid.
#pragma once
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

// axis of table entry e: the number of off[1 .. MT - 1] that are <= e (MT - 1: the last axis' values); *end: where its axis' entries end
template <int MT, class A>
__device__ __forceinline__ int grid_axis_of(const A& a, int e, int* end) {
  int k = 0;
  *end = a.E;
#pragma unroll
  for (int j = MT - 1; j >= 1; --j) {
    k += e >= a.off[j] ? 1 : 0;
    if (e < a.off[j]) *end = a.off[j];
  }
  return k;
}

// the digits (i_0 .. i_{MT-2}) of column l: a lane's first column, the same for every row
template <int MT, class A>
__device__ __forceinline__ void grid_first_digits(const A& a, int l, int (&d0)[MT - 1]) {
  int rem = l;
#pragma unroll
  for (int k = MT - 2; k >= 0; --k) {
    d0[k] = rem % a.n[k];
    rem /= a.n[k];
  }
}

// The row's sum, the same bits in every lane of its group.  mu / sd: the row's moments, target k at [k * LD]; tab: the group's table
// (TABLED; 12 GS doubles); l: the lane inside the group; d0: grid_first_digits of l.  Every lane of the workgroup calls it together: a
// tabled row holds three barriers (behind A, behind B, and behind C, where the next row's entries overwrite this table).
template <int MT, int GS, bool TABLED, int LD, class A>
__device__ __forceinline__ double ehvi_grid_row(const A& a, double* tab, const double* mu_r, const double* sd_r, int l, const int (&d0)[MT - 1]) {
  const int E = a.E, C = a.C, off_last = a.off[MT - 1];
  if constexpr (TABLED) {
    for (int e = l; e < E; e += GS) {  // A
      int end;
      const int k = grid_axis_of<MT>(a, e, &end);
      const double sd = sd_r[k * LD];
      const double gv = ehvi_G((a.pts[e] - mu_r[k * LD]) / sd);
      tab[e] = e >= off_last ? sd * gv : gv;
    }
    __syncthreads();
    for (int e = l; e < off_last; e += GS) {  // B
      int end;
      const int k = grid_axis_of<MT>(a, e, &end);
      const double g0 = tab[e];
      const double g1 = e + 1 < end ? tab[e + 1] : 0.0;
      const double t = sd_r[k * LD] * (g0 - g1);
      tab[e] = t;
    }
    __syncthreads();
  }
  double acc = 0.0;
  int dg[MT - 1];
#pragma unroll
  for (int k = 0; k < MT - 1; ++k) dg[k] = d0[k];
  for (int c = l; c < C; c += GS) {  // C
    double p = 1.0;
    double tl;
    if constexpr (TABLED) {
#pragma unroll
      for (int k = 0; k < MT - 1; ++k) p *= tab[a.off[k] + dg[k]];
      tl = tab[off_last + a.last_idx[c]];
    } else {
#pragma unroll
      for (int k = 0; k < MT - 1; ++k) {
        const int e = a.off[k] + dg[k];
        const double mu = mu_r[k * LD], sd = sd_r[k * LD];
        const double g0 = ehvi_G((a.pts[e] - mu) / sd);
        const double g1 = dg[k] + 1 < a.n[k] ? ehvi_G((a.pts[e + 1] - mu) / sd) : 0.0;
        p *= sd * (g0 - g1);
      }
      const double mu = mu_r[(MT - 1) * LD], sd = sd_r[(MT - 1) * LD];
      tl = sd * ehvi_G((a.pts[off_last + a.last_idx[c]] - mu) / sd);
    }
    acc += p * tl;
    int carry = 0;  // the digits of column c + GS
#pragma unroll
    for (int k = MT - 2; k >= 0; --k) {
      int v = dg[k] + a.step[k] + carry;
      carry = v >= a.n[k] ? 1 : 0;
      dg[k] = v - (carry ? a.n[k] : 0);
    }
  }
#pragma unroll
  for (int dist = GS / 2; dist >= 1; dist >>= 1) acc += shfl_xor_f64(acc, dist);
  if constexpr (TABLED) __syncthreads();  // the next row's entries overwrite this table
  return acc;
}

}  // namespace bogp
