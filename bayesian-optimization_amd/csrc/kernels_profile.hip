// kernels_profile.hip -- bogp_selftest_profile: the radial profile of a correlation function (or one of its building blocks) evaluated on the
// device for an array of arguments, so that tests can hold the special functions of bogp_device.h (K_nu, 1 / Gamma) to committed
// tables one argument at a time instead of through a posterior; bogp_selftest_criteria: the same for the scalar criterion functions
// (ndtr, acq_value, feasibility, the two upper bounds, prune_below); bogp_selftest_feasibility_grad: feasibility_grad, three results a row.
// See include/bogp.h.
#include "bogp_device.h"
#include "bogp_handle.h"

using namespace bogp;

namespace {

template <int KERNEL>
__global__ void k_profile(const double* __restrict__ in, double* __restrict__ out, int64_t n, double pexp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = corr_profile<KERNEL>(in[i], pexp);
}
__global__ void k_special(const double* __restrict__ in, double* __restrict__ out, int64_t n, double pexp, int what) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double rg;
  switch (what) {
    case BOGP_SELFTEST_BESSEL_K: out[i] = bessel_k_nu(pexp, in[i]); break;
    case BOGP_SELFTEST_BESSEL_K_PAIRS: out[i] = bessel_k_nu(in[2 * i], in[2 * i + 1]); break;
    case BOGP_SELFTEST_MATERN_NU_PAIRS: out[i] = corr_profile<BOGP_KERNEL_MATERN_NU>(in[2 * i + 1], in[2 * i]); break;
    default: bessel_k_nu(in[i], 1.0, &rg); out[i] = rg; break;
  }
}

// one row of BOGP_CRITERIA_COLUMNS doubles per thread; the functions of bogp_device.h themselves, no expression of theirs restated
__global__ void k_criteria(const double* __restrict__ rows, double* __restrict__ out, int64_t n, int what) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* r = rows + i * BOGP_CRITERIA_COLUMNS;
  switch (what) {
    case BOGP_CRITERIA_NDTR: out[i] = ndtr(r[0]); break;
    case BOGP_CRITERIA_NORM_PDF: out[i] = norm_pdf(r[0]); break;
    case BOGP_CRITERIA_EHVI_G: out[i] = ehvi_G(r[0]); break;
    case BOGP_CRITERIA_ACQ_VALUE: out[i] = acq_value((int)r[0], r[1], r[2], r[3], r[4], r[5]); break;
    case BOGP_CRITERIA_FEASIBILITY: out[i] = feasibility(r[0], r[1], r[2], r[3], r[4]); break;
    case BOGP_CRITERIA_ACQ_UPPER_BOUND: out[i] = acq_upper_bound((int)r[0], r[1], r[2], r[3], r[4], r[5]); break;
    case BOGP_CRITERIA_ACQ_UPPER_BOUND_INTERVAL: out[i] = acq_upper_bound_interval((int)r[0], r[1], r[2], r[3], r[4], r[5], r[6]); break;
    default: out[i] = prune_below(r[0], r[1]) ? 1.0 : 0.0; break;
  }
}

// feasibility_grad itself on rows of (mu, mse, sigma2, lo, hi): F, dF/dmu, dF/dsd
__global__ void k_feasibility_grad(const double* __restrict__ rows, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* r = rows + i * 5;
  double F, dm, ds;
  feasibility_grad(r[0], r[1], r[2], r[3], r[4], &F, &dm, &ds);
  out[3 * i] = F;
  out[3 * i + 1] = dm;
  out[3 * i + 2] = ds;
}

}  // namespace

extern "C" int bogp_selftest_feasibility_grad(bogp_handle* h, const double* rows, int64_t n, double* out) {
  if (!h) return BOGP_ERR_INVALID;
  if (!rows || !out || n <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_feasibility_grad: null pointer or empty array");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  double *din = nullptr, *dout = nullptr;
  if (hipMalloc((void**)&din, n * 5 * sizeof(double)) != hipSuccess || hipMalloc((void**)&dout, n * 3 * sizeof(double)) != hipSuccess) {
    dfree(din); dfree(dout);
    FAIL(h, BOGP_ERR_HIP, "bogp_selftest_feasibility_grad: hipMalloc failed");
  }
  hipError_t e = hipMemcpyAsync(din, rows, n * 5 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_feasibility_grad, dim3((unsigned)((n + 255) / 256)), 256, 0, st, din, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  dfree(din); dfree(dout);
  if (e != hipSuccess) FAIL(h, BOGP_ERR_HIP, "bogp_selftest_feasibility_grad: %s", hipGetErrorString(e));
  return BOGP_OK;
}

extern "C" int bogp_selftest_criteria(bogp_handle* h, int what, const double* rows, int64_t n, double* out) {
  if (!h) return BOGP_ERR_INVALID;
  if (!rows || !out || n <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_criteria: null pointer or empty array");
  if (what < BOGP_CRITERIA_NDTR || what > BOGP_CRITERIA_PRUNE_BELOW) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_criteria: unknown selector %d", what);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  double *din = nullptr, *dout = nullptr;
  if (hipMalloc((void**)&din, n * BOGP_CRITERIA_COLUMNS * sizeof(double)) != hipSuccess || hipMalloc((void**)&dout, n * sizeof(double)) != hipSuccess) {
    dfree(din); dfree(dout);
    FAIL(h, BOGP_ERR_HIP, "bogp_selftest_criteria: hipMalloc failed");
  }
  hipError_t e = hipMemcpyAsync(din, rows, n * BOGP_CRITERIA_COLUMNS * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_criteria, dim3((unsigned)((n + 255) / 256)), 256, 0, st, din, dout, n, what);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  dfree(din); dfree(dout);
  if (e != hipSuccess) FAIL(h, BOGP_ERR_HIP, "bogp_selftest_criteria: %s", hipGetErrorString(e));
  return BOGP_OK;
}

extern "C" int bogp_selftest_profile(bogp_handle* h, int what, int kernel, double pexp, const double* arg, int64_t n, double* out) {
  if (!h) return BOGP_ERR_INVALID;
  if (!arg || !out || n <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_profile: null pointer or empty array");
  if (what < BOGP_SELFTEST_PROFILE || what > BOGP_SELFTEST_MATERN_NU_PAIRS) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_profile: unknown selector %d", what);
  if (what == BOGP_SELFTEST_PROFILE && (kernel < 0 || kernel > BOGP_KERNEL_MATERN_NU)) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_profile: unknown kernel id %d", kernel);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  double *din = nullptr, *dout = nullptr;
  const int64_t nin = what >= BOGP_SELFTEST_BESSEL_K_PAIRS ? 2 * n : n;  // the *_PAIRS selectors read (order, argument) pairs
  if (hipMalloc((void**)&din, nin * sizeof(double)) != hipSuccess || hipMalloc((void**)&dout, n * sizeof(double)) != hipSuccess) {
    dfree(din); dfree(dout);
    FAIL(h, BOGP_ERR_HIP, "bogp_selftest_profile: hipMalloc failed");
  }
  hipError_t e = hipMemcpyAsync(din, arg, nin * sizeof(double), hipMemcpyHostToDevice, st);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (e == hipSuccess) {
    if (what != BOGP_SELFTEST_PROFILE) {
      hipLaunchKernelGGL(k_special, grid, 256, 0, st, din, dout, n, pexp, what);
    } else {
      switch (kernel) {
#define BOGP_CASE(K) case K: hipLaunchKernelGGL(k_profile<K>, grid, 256, 0, st, din, dout, n, pexp); break;
        BOGP_CASE(BOGP_KERNEL_SE) BOGP_CASE(BOGP_KERNEL_MATERN12) BOGP_CASE(BOGP_KERNEL_MATERN32) BOGP_CASE(BOGP_KERNEL_MATERN52)
        BOGP_CASE(BOGP_KERNEL_ABSEXP) BOGP_CASE(BOGP_KERNEL_CUBIC) BOGP_CASE(BOGP_KERNEL_GENEXP) BOGP_CASE(BOGP_KERNEL_MATERN_NU)
#undef BOGP_CASE
      }
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  dfree(din); dfree(dout);
  if (e != hipSuccess) FAIL(h, BOGP_ERR_HIP, "bogp_selftest_profile: %s", hipGetErrorString(e));
  return BOGP_OK;
}
