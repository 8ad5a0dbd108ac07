"""First measurements of the constrained EHVI sweep (bogp_sweep_ehvi_constrained, k_ehvi_constrained) at the C3 model size (d = 20,
Matern-5/2, 1e6 candidates generated on the device), N = 2048 and N = 512, (m, c) = (2, 1), (2, 3), (3, 1) with the fronts of
tools/time_ehvi.py (32 points: 33 cells at m = 2, about 1 000 at m = 3).  Per case, medians over `--reps` repetitions (after one warm-up
call) of the whole call and of its acquisition_ms (device events around the criterion kernel, bogp_last_timing):
  constrained-ehvi   the new sweep on the (m + c)-target model, and the same call without cells (C = 0: the kernel is then the read of
                     the chunk alone; its achieved bytes/s = 8 N rows / kernel time)
  ehvi               bogp_sweep_ehvi on the model of the m objective columns alone, same cells and parameters (k_ehvi: one load in flight)
  constrained        bogp_sweep_constrained (EI x PoF) on the same (m + c)-target model (k_constrained)
The (3, 1) case at N = 2048 runs three more times for the skipped cell loop: bounds that leave no row at P == 0, about half of them
(the share printed; once in the generated order, once with the P == 0 rows moved to the front so that whole wavefronts skip), and
all of them (lo == hi).  Writes the lines to `--out` (default profiles/constrained_ehvi_sweep.txt) as well."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto  # noqa: E402

d, M, P = 20, 1_000_000, 32
INF = float("inf")


def front(m, rng):
    """P mutually non-dominated points above the origin: on the positive part of the unit sphere (tools/time_ehvi.py)."""
    Z = np.abs(rng.normal(size=(P, m)))
    return Z / np.linalg.norm(Z, axis=1, keepdims=True)


def med(fn, reps, stamp):
    fn()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        ks.append(stamp()["acquisition_ms"])
    return 1e3 * float(np.median(ts)), float(np.median(ks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_ehvi_sweep.txt"))
    a = ap.parse_args()
    assert a.reps >= 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/time_constrained_ehvi_sweep.py: 1e6 candidates, d = 20, Matern-5/2; medians of %d after one warm-up; ms" % a.reps)
    rng = np.random.default_rng(0)
    eng = _lib.Engine(0)
    par = np.r_[np.full(d, 0.01), 0.9]
    for N in (2048, 512):
        X = rng.uniform(-5, 5, size=(N, d))
        for m, c in ((2, 1), (2, 3), (3, 1)):
            Y = np.column_stack([np.sin(X @ rng.normal(size=d) / 4) for _ in range(m + c)])
            lower, upper = pareto.hypercell_bounds(front(m, rng), np.full(m, -0.1))
            lo, hi = np.full(c, -INF), np.zeros(c)
            none = np.zeros((0, m))
            eng.set_train(X, Y[:, :m])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, par, 1e-6, False, 0.0)
            eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), M, 7)
            t_e, k_e = med(lambda: eng.sweep_ehvi(lower, upper), a.reps, eng.last_timing)
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, par, 1e-6, False, 0.0)
            eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), M, 7)
            clo, chi = np.r_[np.full(m - 1, -INF), lo], np.r_[np.full(m - 1, INF), hi]
            t_c, k_c = med(lambda: eng.sweep_constrained([(_lib.ACQ_EI, 0.0)], float(Y[:, 0].min()), True, clo, chi), a.reps, eng.last_timing)
            t_n, k_n = med(lambda: eng.sweep_ehvi_constrained(lower, upper, lo, hi), a.reps, eng.last_timing)
            t_0, k_0 = med(lambda: eng.sweep_ehvi_constrained(none, none, lo, hi), a.reps, eng.last_timing)
            say("N=%d m=%d c=%d cells=%d  constrained-ehvi %.2f (k_ehvi_constrained %.3f)  | C=0: %.2f (kernel %.3f, %.0f GB/s)  | ehvi on the "
                "objectives %.2f (k_ehvi %.3f)  | constrained EI %.2f (k_constrained %.3f)"
                % (N, m, c, len(lower), t_n, k_n, t_0, k_0, 8.0 * N * M / (k_0 * 1e-3) / 1e9, t_e, k_e, t_c, k_c))  # fmt: skip
            if (N, m, c) != (2048, 3, 1):
                continue
            # the skipped cell loop: P == 0 exactly where (lo - mu) / sd exceeds about 38.5 (Phi underflows)
            _, _, _, mu, mse = eng.sweep_ehvi_constrained(none, none, lo, hi, return_pof=True, return_moments=True)
            reach = mu[:, m] + 38.6 * np.sqrt(mse[:, m])
            runs = [("no row", [-INF], [INF]), ("about half", [float(np.median(reach))], [INF]), ("every row (lo == hi)", [0.25], [0.25])]
            for name, slo, shi in runs:
                t_s, k_s = med(lambda: eng.sweep_ehvi_constrained(lower, upper, slo, shi), a.reps, eng.last_timing)
                pof = eng.sweep_ehvi_constrained(lower, upper, slo, shi, return_pof=True)[2]
                share = float(np.mean(pof == 0.0))
                say("  skip, %s at P == 0 (share %.3f, generated order): %.2f (k_ehvi_constrained %.3f)" % (name, share, t_s, k_s))
                if 0.0 < share < 1.0:  # the same rows with the P == 0 ones first: whole wavefronts skip the cell loop
                    Xs = eng.read_candidates(np.arange(M))
                    eng.upload_candidates(Xs[np.argsort(pof != 0.0, kind="stable")])
                    t_s, k_s = med(lambda: eng.sweep_ehvi_constrained(lower, upper, slo, shi), a.reps, eng.last_timing)
                    say("  skip, %s at P == 0 (share %.3f, P == 0 rows first): %.2f (k_ehvi_constrained %.3f)" % (name, share, t_s, k_s))
                    eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), M, 7)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
