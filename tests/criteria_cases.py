"""Shared by tests/test_criteria_host.py, tests/test_gpu_criteria.py and oracle/make_criteria_table.py (not a test module): the
arguments at which the scalar criterion functions of csrc/bogp_device.h are held to exact values (ledger T20), the reference's value
at them, the exact value by mpmath, and the allowance of each criterion.

Draws are seeded and regenerated, never stored.  The tails are populated by drawing z, not y_hat:
    z       half uniform on [-37, 8], half N(0, 2^2)
    sd      sqrt(mse) with mse = (10^U(-4, 1.5))^2        (MGFI: 10^U(-3, 0.5)) -- so that the reference, which takes (mu, mse),
                                                           and the device, which takes sd, see the same double
    plugin  N(0, 1) 10^U(-2, 1)
    y_hat   plugin - z sd                                  (EpsilonPI: divided by coef, so that z stays the argument of Phi)
`z` of a row is what the draw conditions count; it is the argument of Phi / phi in the row as drawn: a for ndtr, x for norm_pdf, -g
for ehvi_G(g) (G(g) = EI(z = -g) / sd: its cancelling tail is g -> +inf), (plugin - coef y_hat) / sd for EI and EpsilonPI, beta' for
MGFI, and for feasibility minus the distance from the mean to the interval in standard deviations (0 inside it).

The exact value is the expression of bogp_device.h in exact arithmetic AT THE DOUBLE INPUTS (mpmath, 60 digits).  The allowance is the
criterion's first-order conditioning with eps = 2^-52: a rounding of z is amplified by z^2 in Phi and phi (d log Phi / d log z ~ z^2
in the tail), and terms that cancel enter by magnitude --
    ndtr, norm_pdf   eps (1 + z^2) |value|
    EI, ehvi_G       eps (1 + z^2) (|A| + |B|)                      A, B the two terms of the sum
    EpsilonPI        phi(z) eps ((|plugin| + |coef y_hat|) / sd + |z|) + eps Phi(z)
    UCB              eps (|y_hat| + |par sd|)
    MGFI             value (eps + (phi / Phi)(beta') eps ((|plugin| + |y_hat| + t sd^2) / sd + |beta'|)
                            + eps (|t plugin| + |t y_hat| + t + t^2 sd^2 / 2 + |exponent|))
    feasibility      eps ((1 + za^2) A + (1 + zb^2) B)               ledger T18's, A and B the two cdf values of the branch taken
A value is compared where |exact| >= 1e-290 (ledger T11: below, the device library's erfc / exp leave the normal range at their own
points); elsewhere it must be finite, >= 0 and <= 1e-289.

Rows per criterion: the committed table stores 12 bytes a row and a committed file stays under 1 MiB, so the six criteria with tails
take 10 000 rows each, norm_pdf 6000 and UCB (a sum and a product: no tail, no switch) 2000."""
import numpy as np
from scipy.special import ndtr

from oracle import gp_oracle as O
from support import constrained_ref as R

EPS = 2.0**-52
TINY = 1e-290
INF = float("inf")
NAMES = ("ndtr", "norm_pdf", "ehvi_G", "EI", "PI", "UCB", "MGFI", "feasibility")
ROWS = {"ndtr": 10_000, "norm_pdf": 6000, "ehvi_G": 10_000, "EI": 10_000, "PI": 10_000, "UCB": 2000, "MGFI": 10_000, "feasibility": 10_000}
SEED = {n: 4600 + i for i, n in enumerate(NAMES)}
ACQ_ID = {"EI": O.ACQ_EI, "PI": O.ACQ_EPSILON_PI, "UCB": O.ACQ_UCB, "MGFI": O.ACQ_MGFI}
PARS = {"EI": (0.0,), "PI": (1e-10, 0.05), "UCB": (0.5, 50.0, -3.0), "MGFI": (0.5, 2.0, 22.36, 30.0)}
T_MAX = 22.36

# The reference's expressions (numpy + scipy.special.ndtr) against the exact values, worst |value - exact| / allowance over the draw
# (tests/test_criteria_host.py asserts each as an upper limit); the allowed factor of the library, host and device, is
# F = 4 x that, rounded up (ledger T18's rule: the margin is for another libm).  F comes from the reference, never from the device.
# Measured with scipy 1.15.3 / numpy on glibc (oracle/make_criteria_table.py prints them), rounded up in the third digit.
REFERENCE_RATIO = {"ndtr": 1.77, "norm_pdf": 1.02, "ehvi_G": 1.10, "EI": 1.43, "PI": 1.05, "UCB": 0.82, "MGFI": 0.77, "feasibility": 1.74}
F = {n: int(np.ceil(4.0 * r)) for n, r in REFERENCE_RATIO.items()}  # 8, 5, 5, 6, 5, 4, 4, 7


def _z(rng, n):
    z = np.where(np.arange(n) % 2 == 0, rng.uniform(-37.0, 8.0, n), rng.normal(0.0, 2.0, n))
    return np.clip(z, -37.0, 37.0)


def _sd(rng, n, lo, hi):
    mse = (10.0 ** rng.uniform(lo, hi, n)) ** 2
    return np.sqrt(mse), mse


def draw(name):
    """-> dict of float64 columns of ROWS[name] entries; always `z` (see the module docstring), the rest by criterion."""
    rng = np.random.default_rng(SEED[name])
    n = ROWS[name]
    z = _z(rng, n)
    if name in ("ndtr", "norm_pdf"):
        return dict(z=z, a=z)
    if name == "ehvi_G":
        return dict(z=z, g=-z)
    if name == "feasibility":
        sd, mse = _sd(rng, n, -3.0, 1.0)
        mu = rng.normal(size=n) * 10.0 ** rng.uniform(-2.0, 1.2, n)
        kind = rng.integers(4, size=n)  # (-inf, hi], [lo, +inf), an interval of width w sd below / above its near end
        w = 10.0 ** rng.uniform(-4.0, 1.0, n)
        za = np.select([kind == 0, kind == 1, kind == 2], [-INF, -z, z - w], -z)
        zb = np.select([kind == 0, kind == 1, kind == 2], [z, INF, z], -z + w)
        with np.errstate(invalid="ignore"):
            lo = np.where(np.isinf(za), za, mu + za * sd)
            hi = np.where(np.isinf(zb), zb, mu + zb * sd)
        hi = np.maximum(hi, lo)
        with np.errstate(divide="ignore"):
            za, zb = (lo - mu) / sd, (hi - mu) / sd  # as the double inputs give them
        dist = np.where(za > 0, za, np.where(zb < 0, -zb, 0.0))
        return dict(z=-dist, mu=mu, mse=mse, sigma2=np.ones(n), lo=lo, hi=hi, za=za, zb=zb)
    sd, mse = _sd(rng, n, *((-3.0, 0.5) if name == "MGFI" else (-4.0, 1.5)))
    plugin = rng.normal(size=n) * 10.0 ** rng.uniform(-2.0, 1.0, n)
    par = np.asarray(PARS[name])[rng.integers(len(PARS[name]), size=n)]
    y_hat = plugin - z * sd
    if name == "PI":
        y_hat = y_hat / np.where(y_hat > 0, 1 - par, 1 + par)
        coef = np.where(y_hat > 0, 1 - par, 1 + par)
        z = (plugin - coef * y_hat) / sd
    elif name == "MGFI":
        t = np.minimum(par, T_MAX)
        z = (plugin - (y_hat - t * sd * sd)) / sd  # beta'
    elif name == "EI":
        z = (plugin - y_hat) / sd
    return dict(z=z, par=par, y_hat=y_hat, sd=sd, mse=mse, plugin=plugin, sigma2=np.ones(n))


def checksum(c):
    return float(sum(np.sum(v[np.isfinite(v)]) for k, v in sorted(c.items())))


def device_columns(name, c):
    """(attribute of bogp._lib naming the selector, the argument columns of bogp_selftest_criteria)"""
    if name == "ndtr":
        return "CRITERIA_NDTR", (c["a"],)
    if name == "norm_pdf":
        return "CRITERIA_NORM_PDF", (c["a"],)
    if name == "ehvi_G":
        return "CRITERIA_EHVI_G", (c["g"],)
    if name == "feasibility":
        return "CRITERIA_FEASIBILITY", (c["mu"], c["mse"], c["sigma2"], c["lo"], c["hi"])
    return "CRITERIA_ACQ_VALUE", (np.full(len(c["z"]), float(ACQ_ID[name])), c["par"], c["y_hat"], c["sd"], c["plugin"], c["sigma2"])


def reference(name, c):
    """The reference's expression (acquisition_fun.py as oracle.gp_oracle.acquisition restates it; analytic.py:223-274 for G) in numpy."""
    with np.errstate(all="ignore"):
        if name == "ndtr":
            return ndtr(c["a"])
        if name == "norm_pdf":
            return O._pdf(c["a"])
        if name == "ehvi_G":
            return O._pdf(c["g"]) - c["g"] * ndtr(-c["g"])
        if name == "feasibility":
            return R.feasibility(c["mu"], c["mse"], 1.0, c["lo"], c["hi"])
        out = np.empty(len(c["z"]))
        for par in PARS[name]:
            m = c["par"] == par
            out[m] = O.acquisition(ACQ_ID[name], par, c["y_hat"][m], c["mse"][m], c["plugin"][m], 1.0, True)
        return out


def _pdf(z):
    with np.errstate(all="ignore"):
        return np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def allowance(name, c, true):
    """The allowance of every row, in double from the inputs and the exact value `true` (scipy's ndtr where a cdf enters: a relative
    1e-16 of an allowance)."""
    with np.errstate(all="ignore"):
        z = c["z"]
        if name in ("ndtr", "norm_pdf"):
            return EPS * (1.0 + z * z) * np.abs(true)
        if name == "ehvi_G":
            g = c["g"]
            return EPS * (1.0 + g * g) * (_pdf(g) + np.abs(g) * ndtr(-g))
        if name == "EI":
            return EPS * (1.0 + z * z) * (np.abs(c["plugin"] - c["y_hat"]) * ndtr(z) + c["sd"] * _pdf(z))
        if name == "PI":
            coef = np.where(c["y_hat"] > 0, 1 - c["par"], 1 + c["par"])
            return _pdf(z) * EPS * ((np.abs(c["plugin"]) + np.abs(coef * c["y_hat"])) / c["sd"] + np.abs(z)) + EPS * ndtr(z)
        if name == "UCB":
            return EPS * (np.abs(c["y_hat"]) + np.abs(c["par"] * c["sd"]))
        if name == "MGFI":
            t, sd, pl, y = np.minimum(c["par"], T_MAX), c["sd"], c["plugin"], c["y_hat"]
            ex = t * (pl - y - 1.0) + t * t * sd * sd / 2.0
            return np.abs(true) * (EPS + _pdf(z) / ndtr(z) * EPS * ((np.abs(pl) + np.abs(y) + t * sd * sd) / sd + np.abs(z))
                                   + EPS * (np.abs(t * pl) + np.abs(t * y) + t + t * t * sd * sd / 2.0 + np.abs(ex)))  # fmt: skip
        za, zb = c["za"], c["zb"]
        up = za > 0
        A, B = np.where(up, ndtr(-za), ndtr(za)), np.where(up, ndtr(-zb), ndtr(zb))
        za2, zb2 = np.where(np.isfinite(za), za * za, 0.0), np.where(np.isfinite(zb), zb * zb, 0.0)
        return EPS * ((1.0 + za2) * A + (1.0 + zb2) * B)


def bound_allowance(a_id, par, y_hat, sd_ub, plugin, value):
    """The allowance of acq_upper_bound's finite, non-constant results (arrays; `value` the bound itself): the criterion's own at sd_ub
    -- EI is acq_value; EpsilonPI with a negative numerator ndtr(num / sd_ub); UCB y_hat + par sd_ub; MGFI with y_hat >= plugin the
    criterion -- and for MGFI with y_hat < plugin, where Phi is replaced by 1, the criterion's without the Phi term."""
    name = {v: k for k, v in ACQ_ID.items()}[int(a_id)]
    par, y_hat, sd_ub, plugin, value = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(par, y_hat, sd_ub, plugin, value))
    c = dict(par=par, y_hat=y_hat, sd=sd_ub, plugin=plugin)
    with np.errstate(all="ignore"):
        if name == "EI":
            c["z"] = (plugin - y_hat) / sd_ub
        elif name == "PI":
            c["z"] = (plugin - np.where(y_hat > 0, 1 - par, 1 + par) * y_hat) / sd_ub
        elif name == "MGFI":
            t = np.minimum(par, T_MAX)
            c["z"] = np.where(y_hat >= plugin, (plugin - (y_hat - t * sd_ub * sd_ub)) / sd_ub, 40.0)  # (phi / Phi)(40) = 0: no Phi term
        else:
            c["z"] = np.zeros_like(y_hat)
        return allowance(name, c, value)


def exact(name, c, rows=None):
    """(true, rlo): the expression of bogp_device.h in exact arithmetic at the double inputs, as a double and the float32 relative
    residual (exact = true (1 + rlo)); mpmath at 60 digits.  `rows`: indices to evaluate (all by default)."""
    import mpmath as mp

    mp.mp.dps = 60
    rows = np.arange(len(c["z"])) if rows is None else np.asarray(rows)
    f = lambda k, i: mp.mpf(float(c[k][i]))  # noqa: E731
    pdf = lambda x: mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)  # noqa: E731
    dbl_max = mp.mpf(np.finfo(float).max)
    true, rlo = np.empty(len(rows)), np.empty(len(rows), dtype=np.float32)
    for j, i in enumerate(rows):
        if name == "ndtr":
            v = mp.ncdf(f("a", i))
        elif name == "norm_pdf":
            v = pdf(f("a", i))
        elif name == "ehvi_G":
            g = f("g", i)
            v = pdf(g) - g * mp.ncdf(-g)
        elif name == "feasibility":
            mu, sd = f("mu", i), mp.sqrt(f("mse", i))
            lo, hi = float(c["lo"][i]), float(c["hi"][i])
            za = -mp.inf if lo == -INF else (mp.mpf(lo) - mu) / sd
            zb = mp.inf if hi == INF else (mp.mpf(hi) - mu) / sd
            v = mp.ncdf(-za) - mp.ncdf(-zb) if za > 0 else mp.ncdf(zb) - mp.ncdf(za)
        else:
            par, y, sd, pl = f("par", i), f("y_hat", i), f("sd", i), f("plugin", i)
            if name == "EI":
                x = (pl - y) / sd
                v = (pl - y) * mp.ncdf(x) + sd * pdf(x)
            elif name == "PI":
                coef = 1 - par if y > 0 else 1 + par
                v = mp.ncdf((pl - coef * y) / sd)
            elif name == "UCB":
                v = y + par * sd
            else:
                t = min(par, mp.mpf(T_MAX))
                e = mp.exp(t * (pl - y - 1) + t * t * sd * sd / 2)
                v = mp.ncdf((pl - (y - t * sd * sd)) / sd) * e
                if e > dbl_max or v > dbl_max:  # the overflow select of acq_value
                    v = mp.mpf(0)
        true[j] = float(v)
        rlo[j] = float((v - mp.mpf(true[j])) / mp.mpf(true[j])) if true[j] != 0.0 else 0.0
    return true, rlo


def ratios(value, true, rlo, allow):
    """|value - exact| / allowance on the rows that are compared (|exact| >= TINY), and the mask of those rows"""
    cmp = np.abs(true) >= TINY
    with np.errstate(all="ignore"):
        err = np.abs((value[cmp] - true[cmp]) / true[cmp] - rlo[cmp].astype(np.float64)) * np.abs(true[cmp])
        return err / allow[cmp], cmp


def tiny_rows_ok(value, cmp):
    v = value[~cmp]
    return bool(np.all(np.isfinite(v) & (v >= 0.0) & (v <= 1e-289)))


def draw_conditions(name, c, cmp):
    """Conditions on the draw (not tolerances): -> list of (description, count, required)"""
    z = c["z"]
    out = [("compared rows", int(cmp.sum()), int(np.ceil(0.95 * len(z))))]
    if name != "UCB":  # (a sum and a product: no z enters)
        out += [("z < -20", int(np.sum(z < -20)), 500), ("|z| < 1", int(np.sum(np.abs(z) < 1)), 500)]
    if name == "PI":
        for par in PARS["PI"]:
            m = c["par"] == par
            out += [("par %g, y_hat > 0" % par, int(np.sum(m & (c["y_hat"] > 0))), 200), ("par %g, y_hat <= 0" % par, int(np.sum(m & (c["y_hat"] <= 0))), 200)]
    if name == "feasibility":
        out += [("za > 0", int(np.sum(c["za"] > 0)), 200), ("za <= 0", int(np.sum(c["za"] <= 0)), 200)]
    if name == "MGFI":  # the switch of the MGFI bound
        out += [("y_hat >= plugin", int(np.sum(c["y_hat"] >= c["plugin"])), 200), ("y_hat < plugin", int(np.sum(c["y_hat"] < c["plugin"])), 200)]
    return out
