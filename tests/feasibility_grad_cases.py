"""Shared by tests/test_constrained_grad_host.py, tests/test_gpu_constrained_grad.py and tests/support/make_feasibility_grad_table.py
(not a test module): the arguments at which `feasibility_grad` of csrc/bogp_device.h is held to exact values (ledger T21), the
reference-style expression at them, the exact value by mpmath, and the allowance of each derivative.

The rows are the seeded draw `criteria_cases.draw("feasibility")` (10 000 rows, sigma2 = 1, sd >= 1e-3: the guard stays off), so
out[:, 0] is held by the committed table G46 already; tests/golden/G47_feasibility_grad_truth.npz adds the two derivatives
    dF/dmu = (phi(za) - phi(zb)) / sd,    dF/dsd = (za phi(za) - zb phi(zb)) / sd,     za = (lo - mu) / sd, zb = (hi - mu) / sd
in exact arithmetic AT THE DOUBLE INPUTS (mpmath, 60 digits), an infinite side contributing 0, stored as G46 stores its values: the
nearest double `_true` and the float32 relative residual `_rlo` (exact = true (1 + rlo)).

Allowance, first-order conditioning with eps = 2^-52: a rounding of z is amplified by z^2 in phi, the exponential, the division by
sqrt(2 pi) and the division by sd add one rounding each, and the two terms enter by magnitude --
    dF/dmu   eps ((2 + za^2) phi(za) + (2 + zb^2) phi(zb)) / sd
    dF/dsd   eps ((2 + za^2) |za| phi(za) + (2 + zb^2) |zb| phi(zb)) / sd
with the term of an infinite side 0 (it contributes exactly 0 to the value).  A row is compared where |exact| >= 1e-290 (ledger T11);
elsewhere the result must be finite and at most 1e-289 in magnitude."""
import numpy as np

import criteria_cases as CC

NAMES = ("dmu", "dsd")
EPS, TINY, INF = CC.EPS, CC.TINY, CC.INF

# The reference-style expressions (numpy's exp on the double z) against the exact values, worst |value - exact| / allowance over the full
# draw (tests/support/make_feasibility_grad_table.py prints them; the host test asserts each as an upper limit), rounded up in the third
# digit; the allowed factor of the library, host and device, is F = ceil(4 x that) (ledger T18 / T20's rule: the margin is for another
# libm).  F comes from the reference expression, never from the library.
# Measured with numpy on glibc over all 10 000 rows: 1.105 and 1.104, both at row 1878 (za = 32.2, hi = +inf: a lower tail bound far
# above the mean); every fifth row alone gives 0.882 and 0.881.
REFERENCE_RATIO = {"dmu": 1.11, "dsd": 1.11}
F = {n: int(np.ceil(4.0 * r)) for n, r in REFERENCE_RATIO.items()}  # 5, 5


def draw():
    return CC.draw("feasibility")


def _phi(z):
    with np.errstate(all="ignore"):
        return np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def _sides(c):
    """phi and z of each side with an infinite side's term removed: (pa, pb, za, zb) with z = 0 where the side is infinite"""
    sd = np.sqrt(c["mse"])
    fa, fb = np.isfinite(c["lo"]), np.isfinite(c["hi"])
    with np.errstate(all="ignore"):
        za = np.where(fa, (c["lo"] - c["mu"]) / sd, 0.0)
        zb = np.where(fb, (c["hi"] - c["mu"]) / sd, 0.0)
    return np.where(fa, _phi(za), 0.0), np.where(fb, _phi(zb), 0.0), za, zb, sd


def reference(name, c):
    pa, pb, za, zb, sd = _sides(c)
    return (pa - pb) / sd if name == "dmu" else (za * pa - zb * pb) / sd


def allowance(name, c):
    pa, pb, za, zb, sd = _sides(c)
    if name == "dmu":
        return EPS * ((2.0 + za * za) * pa + (2.0 + zb * zb) * pb) / sd
    return EPS * ((2.0 + za * za) * np.abs(za) * pa + (2.0 + zb * zb) * np.abs(zb) * pb) / sd


def exact(c, rows=None):
    """{name: (true, rlo)} by mpmath at 60 digits; `rows`: indices to evaluate (all by default)."""
    import mpmath as mp

    mp.mp.dps = 60
    rows = np.arange(len(c["mu"])) if rows is None else np.asarray(rows)
    pdf = lambda x: mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)  # noqa: E731
    out = {n: (np.empty(len(rows)), np.empty(len(rows), dtype=np.float32)) for n in NAMES}
    for j, i in enumerate(rows):
        mu, sd = mp.mpf(float(c["mu"][i])), mp.sqrt(mp.mpf(float(c["mse"][i])))
        lo, hi = float(c["lo"][i]), float(c["hi"][i])
        dm = ds = mp.mpf(0)
        if np.isfinite(lo):
            za = (mp.mpf(lo) - mu) / sd
            dm, ds = dm + pdf(za), ds + za * pdf(za)
        if np.isfinite(hi):
            zb = (mp.mpf(hi) - mu) / sd
            dm, ds = dm - pdf(zb), ds - zb * pdf(zb)
        for n, v in (("dmu", dm / sd), ("dsd", ds / sd)):
            t = float(v)
            out[n][0][j] = t
            out[n][1][j] = float((v - mp.mpf(t)) / mp.mpf(t)) if t != 0.0 else 0.0
    return out


def ratios(value, true, rlo, allow):
    """|value - exact| / allowance on the rows that are compared (|exact| >= TINY), and the mask of those rows"""
    return CC.ratios(value, true, rlo, allow)


def tiny_rows_ok(value, cmp):
    v = value[~cmp]
    return bool(np.all(np.isfinite(v) & (np.abs(v) <= 1e-289)))
