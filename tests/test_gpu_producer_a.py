"""The VALU correlation producer k_corr_chunk<KERNEL, PV> (kernel A, csrc/kernels_posterior.hip) where it alone serves: since the
matrix-core producer took over SE and Matern 1/2, 3/2, 5/2 without a fused trend, the seam tests of test_gpu_producer.py no
longer reach it.  Two families (tests/producer_cases.py; their preconditions are asserted by tests/test_producer_cases_host.py):
  1. PV == 0 with absolute_exponential, cubic, generalized_exponential, general-nu Matern -- own dist_accumulate (a product starting at
     1 with a clamp; a pow() per pair and dimension), own pre-scaling of the coordinates (theta, theta^(1/p), sqrt(theta)), the exponent
     as entry d of the scaled array: d = 1, 2, 7, 20, 50, N off every tile size, three and four slices, candidates ON, a hair beside
     and far outside the training set, ragged M;
  2. PV == 16 / 32, a polynomial trend of 2 .. 32 columns fused into the producer as MFMA tiles (LDS staging, the hand-written
     accumulator layout of the store to t_part), at p = 4, 8, 16 | 17, 21, 28, 32 | 33 -- the last one already on the trend-rows path --
     and with each of the four kernels of family 1.
Every case: likelihood, posterior, criteria and winners against the oracle at the parity tolerances of test_gpu_parity.py; one chunk
against a dozen (BOGP_CHUNK_MB=1) bit for bit; for a constant trend the small-batch path (M <= 32: k_batch_corr + k_gemm64) too.
Each test prints its worst errors as fractions of their allowance (pytest -s / -rP shows them).

Measured on an MI355X when these tests were written (no case failed; the library was not changed).  p = basis columns, Np = padded
training rows, S = slices of the producer, chunks = launches at BOGP_CHUNK_MB=1 for the 1801-row stack; then the worst error of the
posterior mean, the MSE and the three criteria as a fraction of the allowance (1 = at the tolerance):
    case                          p    Np  S  chunks  mu       mse      criteria
    absexp-N600-d20               1   608  3  10      1.9e-06  2.8e-03  6.2e-03
    absexp-N530-d50               1   544  3  10      1.2e-05  1.9e-03  7.1e-04
    absexp-N1000-d7               1  1024  4  15      3.3e-06  2.8e-03  4.2e-04
    absexp-N777-d1                1   800  4  15      1.7e-06  4.6e-02  4.6e-03
    genexp(1.5)-N600-d20          1   608  3  10      2.3e-06  2.1e-09  1.1e-05
    genexp(1.5)-N530-d50          1   544  3  10      2.6e-06  1.1e-09  3.2e-06
    genexp(1.5)-N1000-d7          1  1024  4  15      2.3e-06  3.0e-08  2.0e-05
    genexp(0.7)-N600-d20          1   608  3  10      4.6e-06  1.9e-02  5.6e-03
    genexp(0.7)-N530-d50          1   544  3  10      5.3e-06  9.4e-03  3.2e-04
    genexp(0.7)-N1000-d7          1  1024  4  15      1.3e-05  4.1e-02  1.2e-03
    genexp(1.5)-N777-d1           1   800  4  15      2.7e-04  7.8e-04  2.9e-03
    cubic-N600-d20                1   608  3  10      1.3e-07  8.9e-04  1.6e-08
    cubic-N1000-d7                1  1024  4  15      6.3e-06  9.4e-08  1.8e-05
    cubic-N530-d50                1   544  3  10      2.0e-07  2.4e-10  6.3e-07
    matern_nu(1.7)-N600-d20       1   608  3  10      1.3e-06  6.8e-09  2.6e-06
    matern_nu(1.7)-N530-d50       1   544  3  10      2.4e-06  1.7e-09  5.4e-06
    matern_nu(1.7)-N1000-d7       1  1024  4  15      7.5e-06  9.5e-08  9.7e-06
    matern_nu(0.8)-N600-d20       1   608  3  10      3.5e-05  7.3e-08  2.5e-04
    matern_nu(0.8)-N530-d50       1   544  3  10      1.6e-05  1.0e-07  1.2e-04
    matern_nu(0.8)-N1000-d7       1  1024  4  15      3.9e-05  4.8e-08  3.2e-05
    cubic-N777-d2                 1   800  4  15      2.7e-06  1.1e-04  7.7e-05
    matern_nu(1.7)-N777-d2        1   800  4  15      6.5e-07  5.6e-04  2.3e-04
    matern_nu(0.8)-N777-d2        1   800  4  15      2.1e-07  4.0e-03  6.1e-05
    m52-lin-N600-d15             16   608  3  10      7.5e-07  2.3e-09  1.5e-06
    se-lin-N600-d16              17   608  3  10      6.5e-07  9.4e-10  5.6e-07
    m32-lin-N777-d31             32   800  4  15      1.8e-06  7.8e-10  2.6e-06
    absexp-quad-N530-d5          21   544  3  10      2.0e-06  3.7e-03  4.5e-04
    cubic-quad-N600-d6           28   608  3  10      4.8e-06  2.5e-07  1.0e-04
    se-lin-N600-d32              33   608  3  15      3.9e-07  5.6e-10  1.6e-06  (trend-rows path: the chunk is 832 rows tall)
    m12-lin-N1000-d3              4  1024  4  15      2.0e-06  2.9e-03  2.6e-04
    genexp(1.5)-lin-N600-d7       8   608  3  10      5.3e-06  2.6e-08  1.1e-05
    matern_nu(1.7)-lin-N600-d7    8   608  3  10      2.8e-06  2.9e-08  2.2e-06
Family 1 at worst: mu 2.7e-4, MSE 4.6e-2, criteria 6.2e-3 of the allowance; family 2: 5.3e-6, 3.7e-3, 4.5e-4."""
import numpy as np
import pytest

import producer_cases as PC
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

from bogp import _lib  # noqa: E402

MU_TOL = dict(rtol=1e-6, atol=1e-9)  # the parity tolerances (tests/test_gpu_parity.py); the MSE's atol is 1e-12 sigma2
ACQ = list(PC.ACQ)


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _used(a, ref, rtol, atol):
    """Worst |a - ref| as a fraction of the allowance rtol |ref| + atol."""
    a, ref = np.ravel(a), np.ravel(ref)
    return float(np.max(np.abs(a - ref) / (rtol * np.abs(ref) + atol))) if a.size else 0.0


def _commit(eng, c):
    b = PC.build(c)
    eng.set_train(b["X"], b["y"])
    return eng.commit(c.kernel, O.MODE_NOISY, b["par"], PC.NOISE, True, 0.0, trend=c.trend)


def _posterior_and_sweep(eng, Xs, pl):
    eng.upload_candidates(Xs)
    mu, mse = eng.predict()
    best, idx, vals = eng.sweep(ACQ, pl, True, return_values=True)
    return mu, mse, best, idx, vals, eng.last_timing()["n_chunks"]


def _check_rows(mu, mse, vals, idx, best, omu, omse, ovals, s2, winners=(0, 1, 2)):
    """Posterior, criteria and winners of one candidate set against the oracle's rows of the same set."""
    np.testing.assert_allclose(mu, omu, **MU_TOL)
    np.testing.assert_allclose(mse, omse, rtol=1e-6, atol=1e-12 * s2)
    assert np.all(mse >= 0.0)
    solid = omse > 1e-9 * s2  # (elsewhere the MSE is rounding noise and the criteria are step functions of it)
    np.testing.assert_allclose(vals[:, solid], ovals[:, solid], rtol=1e-6, atol=1e-300)
    for k in range(len(ACQ)):
        assert idx[k] == int(np.argmax(vals[k])) and best[k] == vals[k][idx[k]]
    for k in winners:  # unconditional: the oracle's winner leads by >= 1e-4 relative (tests/test_producer_cases_host.py)
        assert idx[k] == int(np.argmax(ovals[k])), (k, idx[k], int(np.argmax(ovals[k])))
    return (_used(mu, omu, 1e-6, 1e-9), _used(mse, omse, 1e-6, 1e-12 * s2), _used(vals[:, solid], ovals[:, solid], 1e-6, 1e-300))


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_kernel_a_matches_the_oracle(eng, monkeypatch, case):
    c, b, o = case, PC.build(case), PC.oracle(case)
    s2, pl, p, M = o["sigma2"], b["plugin"], PC.trend_size(case), PC.M_STACK
    monkeypatch.delenv("BOGP_CHUNK_MB", raising=False)
    # 1. the likelihood of the committed state
    llf = _commit(eng, c)
    np.testing.assert_allclose(llf, o["llf"], rtol=1e-9)
    # 2. predict on the stack and the far block
    eng.upload_candidates(b["Xall"])
    mu_all, mse_all = eng.predict()
    np.testing.assert_allclose(mu_all, o["mu"], **MU_TOL)
    np.testing.assert_allclose(mse_all, o["mse"], rtol=1e-6, atol=1e-12 * s2)
    assert np.all(mse_all >= 0.0)
    if c.kernel == O.KERNEL_CUBIC:  # rows with every training point outside the support: r = 0 exactly, the prior (+ the trend's share)
        far = b["Xall"][M:]
        outside = np.all(np.max(np.abs(far[:, None, :] - b["X"][None, :, :]), axis=2) * c.theta >= 1.0, axis=1)
        assert outside.any()
        np.testing.assert_allclose(mse_all[M:][outside], o["mse"][M:][outside], rtol=1e-6, atol=1e-12 * s2)
        assert np.all(mse_all[M:][outside] >= s2 * (1.0 - 1e-6))
    mu_only, none = eng.predict(eval_MSE=False)
    assert none is None
    np.testing.assert_array_equal(mu_only, mu_all)
    # 3. the sweep on the stack, one chunk
    mu, mse, best, idx, vals, n1 = _posterior_and_sweep(eng, b["Xs"], pl)
    assert n1 == 1
    np.testing.assert_array_equal(mu, mu_all[:M])  # (a row's posterior does not depend on the rows behind it)
    np.testing.assert_array_equal(mse, mse_all[:M])
    used = _check_rows(mu, mse, vals, idx, best, o["mu"][:M], o["mse"][:M], o["vals"], s2)
    _, idx_plain = eng.sweep(ACQ, pl, True)  # winners only: the call a BO step makes
    np.testing.assert_array_equal(idx_plain, o["idx"])
    # 4. a dozen chunks, the last one ragged: every bit of the single-chunk run (bogp_api_sweep.hip: the slices of the training set
    # are a function of N only), and the chunk count that belongs to the path the model is meant to take
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")
    mu_c, mse_c, best_c, idx_c, vals_c, nc = _posterior_and_sweep(eng, b["Xs"], pl)
    monkeypatch.delenv("BOGP_CHUNK_MB")
    assert nc == PC.chunks_1mib(c) and nc >= 8
    np.testing.assert_array_equal(mu_c, mu)
    np.testing.assert_array_equal(mse_c, mse)
    np.testing.assert_array_equal(vals_c, vals)
    np.testing.assert_array_equal(idx_c, idx)
    np.testing.assert_array_equal(best_c, best)
    if p == 1:
        # 5. M <= 32 and a constant trend: k_batch_corr + k_gemm64.  Rows ON training points (only UCB has a comparable winner
        # there) and 32 rows of the box
        for rows, winners in ((slice(0, PC.SMALL_M), (2,)), (PC.SMALL_BOX, (0, 1, 2))):
            mu_s, mse_s, best_s, idx_s, vals_s, n0 = _posterior_and_sweep(eng, b["Xs"][rows], pl)
            assert n0 == 0  # (no chunk was launched)
            sub = _check_rows(mu_s, mse_s, vals_s, idx_s, best_s, o["mu"][rows], o["mse"][rows], o["vals"][:, rows], s2, winners)
            used = tuple(max(a, b_) for a, b_ in zip(used, sub))
    else:
        # 6. the path: the full polynomial state is there; up to 32 columns the chunk is Np rows tall -- the producer carries the
        # trend -- while 33 columns extend it by the trend rows: the chunk count asserted above differs between the two for every
        # case (tests/test_producer_cases_host.py), no other public field shows the path
        s = eng.get_state(with_C=False)
        assert s["Ft"].shape == (c.N, p) and s["G"].shape == (p, p) and s["beta"].shape == (p,)
        np.testing.assert_allclose(s["sigma2"], s2, rtol=1e-10)
    print("%s: family %d p=%d Np=%d S=%d chunks=%d | used of the allowance: mu %.3g, mse %.3g, criteria %.3g"
          % (PC.case_id(c), c.family, p, PC.padded_rows(c.N), PC.slices(c.N), nc, *used))  # fmt: skip


@pytest.mark.parametrize("pair", PC.IDENTITIES, ids=lambda pr: PC.case_id(pr[0]) + "=" + PC.case_id(pr[1]))
def test_generalized_exponential_is_se_at_p2_and_absolute_exponential_at_p1(eng, monkeypatch, pair):
    """Kernel A's pow() path against an independently written kernel on the same data: p = 2.0 against the squared exponential
    (k_corr_mfma), p = 1.0 against the absolute exponential (kernel A's fabs path).  The oracle's pairs agree to 0.0
    (tests/test_producer_cases_host.py); the device's at the parity tolerances, with the same winners."""
    monkeypatch.delenv("BOGP_CHUNK_MB", raising=False)
    out = []
    for c in pair:
        b = PC.build(c)
        llf = _commit(eng, c)
        eng.upload_candidates(b["Xall"])
        mu, mse = eng.predict()
        eng.upload_candidates(b["Xs"])
        _, idx = eng.sweep(ACQ, b["plugin"], True)
        out.append((llf, mu, mse, idx))
    (la, ma, va, ia), (lb, mb, vb, ib) = out
    s2 = PC.SIGMA2_PAR
    print("%s against %s: |llf| rel %.3g, mu %.3g and mse %.3g of the allowance (max |d mu| %.3g, max |d mse| / sigma2 %.3g)"
          % (PC.case_id(pair[0]), PC.case_id(pair[1]), abs(la - lb) / abs(lb), _used(ma, mb, 1e-6, 1e-9), _used(va, vb, 1e-6, 1e-12 * s2),
             np.abs(ma - mb).max(), np.abs(va - vb).max() / s2))  # fmt: skip
    # measured on an MI355X (the bounds stay the parity tolerances) -- p = 2 against SE: llf 1.6e-16 relative, max |d mu| 5.6e-15 (1.1e-6
    # of the allowance), max |d mse| 2.7e-15 sigma2 (5.5e-8 of it); p = 1 against absolute_exponential: llf identical, max |d mu|
    # 1.1e-14 (2.2e-6 of the allowance), max |d mse| 2.9e-15 sigma2 (2.9e-3 of it, on the rows ON training points)
    np.testing.assert_allclose(la, lb, rtol=1e-9)
    np.testing.assert_allclose(ma, mb, **MU_TOL)
    np.testing.assert_allclose(va, vb, rtol=1e-6, atol=1e-12 * s2)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(ia, PC.oracle(pair[0])["idx"])
