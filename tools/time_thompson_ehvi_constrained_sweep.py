"""Thompson batches for constrained multi-objective runs (bogp_sweep_thompson_ehvi_constrained, k = 8 ranks) beside its two siblings in
the same process: C3's shape (N = 2048, d = 20, Matern-5/2, 1e6 candidates generated on the device) and N = 512, noiseless.  Per shape,
(m_obj, n_con, q) = (2, 1, 5) over 30 cells and (3, 1, 4) over 1024 cells, L = 256 / 1024 / 4096, and constraint bounds at which about
0.05, 0.5 and all of the (row, member) pairs are feasible by the draw (the bound is the share quantile of the constraint's path values
over the first 20000 candidates; the realised share there is printed).  Medians over `--reps` runs after a warm-up, with the
run-to-run spread (max - min) of each kernel time:
  ehvi-constrained   wall, producer, draw at X + solves, k_thompson_ehvi_constrained, per share
  constrained        the same columns through bogp_sweep_thompson_constrained (no cell loop at all): k_thompson_constrained
  ehvi               k_thompson_ehvi on the objective-only model of the same m_obj, q and cells, and the same call over ONE cell: the
                     difference is that kernel's cell loop, every pair running it
The claim under test: (k_thompson_ehvi_constrained - k_thompson_constrained) falls with the feasible share at C = 1024, and at share 1
stays within run-to-run spread of k_thompson_ehvi's loop cost.  For scale, per shape: one constrained-EHVI sweep
(bogp_sweep_ehvi_constrained) and q Kriging-believer proposals (bogp_sweep_believer_ehvi_constrained)."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bogp import _lib, pareto, thompson  # noqa: E402
from time_thompson_ehvi_sweep import front_of, series, timed  # noqa: E402

D, M, K, M_PROBE = 20, 1_000_000, 8, 20_000
SHARES = (0.05, 0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--features", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    box = np.full(D, -5.0), np.full(D, 5.0)
    for N in args.sizes:
        rng = np.random.default_rng(N)
        X = rng.uniform(-5, 5, size=(N, D))
        Y = np.column_stack([np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N) for _ in range(4)])
        theta = np.full(D, 0.01)
        st = SimpleNamespace(X=X, kernel=_lib.KERNEL_MATERN52, theta=theta, nu=None)  # what thompson.draw reads of a model
        print("N=%d d=%d M=%d k=%d reps=%d" % (N, D, M, K, args.reps))
        for mo, q in ((2, 5), (3, 4)):
            m = mo + 1
            ref = np.quantile(Y[:, :mo], 0.3, axis=0)
            F = front_of(mo, ref, Y[:, :mo].max(axis=0))
            lower, upper = pareto.hypercell_bounds(F, ref)
            draws = {L: thompson.draw(st, q * m, L, seed=L) for L in args.features}
            objs = {L: thompson.draw(st, q * mo, L, seed=L) for L in args.features}
            # ---- the objective-only model: k_thompson_ehvi over the same cells, and over one cell
            eng.set_train(X, Y[:, :mo])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, False, 0.0)
            eng.generate_candidates(*box, M, 7)
            loop = {}
            for L in args.features:
                e = series(args.reps, lambda: eng.sweep_thompson_ehvi(objs[L], q, lower, upper, k=K), eng.thompson_ehvi_last)
                e1 = series(args.reps, lambda: eng.sweep_thompson_ehvi(objs[L], q, lower[:1], upper[:1], k=K), eng.thompson_ehvi_last)
                loop[L] = (e["paths"] - e1["paths"], e["spread"] + e1["spread"])
                print("  ehvi m=%d q=%d C=%-4d             L = %-4d  wall %8.3f ms   k_thompson_ehvi %7.3f ms (spread %.3f)   one cell %7.3f ms (spread %.3f): "
                      "cell loop %7.3f ms" % (mo, q, len(lower), L, e["wall"], e["paths"], e["spread"], e1["paths"], e1["spread"], loop[L][0]), flush=True)  # fmt: skip
            # ---- the model with the constraint column
            eng.set_train(X, Y[:, :m])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, False, 0.0)
            for L in args.features:
                dr = draws[L]
                eng.generate_candidates(*box, M_PROBE, 7)  # (a probe set from the same generator and seed)
                free = np.array([-np.inf]), np.array([np.inf])
                probe = eng.sweep_thompson_ehvi_constrained(dr, q, lower, upper, *free, k=1, return_values=True)["paths"][:, mo]
                eng.generate_candidates(*box, M, 7)
                c = series(args.reps, lambda: eng.sweep_thompson_constrained(dr, q, np.full(m - 1, -np.inf), np.full(m - 1, np.inf), k=K), eng.thompson_constrained_last)
                print("  constrained m=%d q=%d               L = %-4d  wall %8.3f ms   k_thompson_constrained %7.3f ms (spread %.3f)"
                      % (m, q, L, c["wall"], c["paths"], c["spread"]), flush=True)  # fmt: skip
                for share in SHARES:
                    hi = np.array([np.inf if share == 1.0 else np.quantile(probe, share)])
                    e = series(args.reps, lambda: eng.sweep_thompson_ehvi_constrained(dr, q, lower, upper, free[0], hi, k=K), eng.thompson_ehvi_constrained_last)
                    print("  ehvi-constrained m_obj=%d q=%d C=%-4d L = %-4d  share %.2f (probe %.3f)  wall %8.3f ms   producer %7.3f ms  draw at X + solves %7.3f ms  "
                          "k_thompson_ehvi_constrained %7.3f ms (spread %.3f, %d chunks)   over constrained %+7.3f ms   ehvi's cell loop %7.3f ms (spread %.3f)"
                          % (mo, q, len(lower), L, share, float(np.mean(probe <= hi[0])), e["wall"], e["corr"], e["solve"], e["paths"], e["spread"], e["chunks"],
                             e["paths"] - c["paths"], loop[L][0], loop[L][1]), flush=True)  # fmt: skip
            lo, hi = np.array([-np.inf]), np.median(Y[:, mo:m], axis=0)
            wall = [timed(lambda: eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=K))[0] for _ in range(args.reps + 1)][1:]
            print("  bogp_sweep_ehvi_constrained, C = %d, k = %d              wall %8.3f ms (spread %.3f)" % (len(lower), K, np.median(wall), max(wall) - min(wall)))
            wall = [timed(lambda: eng.sweep_believer_ehvi_constrained(F, ref, q, lo, hi))[0] for _ in range(args.reps + 1)][1:]
            print("  bogp_sweep_believer_ehvi_constrained, q = %d              wall %8.3f ms (spread %.3f)" % (q, np.median(wall), max(wall) - min(wall)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
