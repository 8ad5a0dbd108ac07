"""The polish of multi-objective Thompson batches (bogp_point_eval_path_hvi / bogp_polish_path_hvi, kernels_point_path_hvi.hip) on one
MI355X: d = 20, Matern-5/2, noiseless, (m, q) = (2, 8) over 30 cells and (3, 5) over 1024 cells, n_starts = 8 (B = 8 q starts), per N
and L medians over `--reps` runs after a warm-up, in one process:
  eval        one bogp_point_eval_path_hvi at B = 1 and at B = 8 q, wall (upload of the operands, ONE launch, read-back)
  iteration   the time of a polish iteration: (polish of 41 evaluations - polish of 1 evaluation) / 40, pgtol = factr = 0 so no start stops
  polish      bogp_polish_path_hvi with the library's defaults (50 evaluations at most)
  single      the same three figures of bogp_point_eval_path / bogp_polish_path (ONE path a point) on the first objective's model, same X,
              theta, L and B: what one of the m paths costs alone
  best HVI    per member the best row of a 1e4-row sweep, that sweep + polish of its 8 best improving rows, and the same at 1e5 rows: the
              mean over the members of the hypervolume the member's draw adds (0 where it improves nowhere) -- higher is better
Nothing here was tuned."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto, thompson  # noqa: E402

D, STARTS, BETA = 20, 8, 0.0
M52 = _lib.KERNEL_MATERN52


def median_ms(fn, reps):
    ts = []
    for _ in range(reps + 1):  # run 0 warms up
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:]))


def front_cells(Y):
    """m = 2: 29 points on an arc (30 cells); m = 3: 31 mutually non-dominated points on a stair (32 x 32 = 1024 cells)."""
    m = Y.shape[1]
    ref, top = np.quantile(Y, 0.3, axis=0), Y.max(axis=0)
    if m == 2:
        a = np.linspace(0.05, 0.95, 29) * np.pi / 2
        P = ref + 0.6 * (top - ref) * np.column_stack([np.cos(a), np.sin(a)])
    else:
        s = np.linspace(0.1, 0.8, 31)
        P = ref + (top - ref) * np.column_stack([s, s[::-1], 0.3 + 0.4 * np.abs(s - 0.45)])
    return pareto.hypercell_bounds(P, ref)


def three(eval1, evalB, polish, reps):
    """(eval B = 1, eval B, iteration in us, whole polish) of one family; polish(**kw) runs its polish entry."""
    stay = dict(pgtol=0.0, factr=0.0)
    p1, p41 = median_ms(lambda: polish(max_evals=1, **stay), reps), median_ms(lambda: polish(max_evals=41, **stay), reps)
    return median_ms(eval1, reps), median_ms(evalB, reps), 1e3 * (p41 - p1) / 40, median_ms(polish, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--features", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    lo, hi = np.full(D, -5.0), np.full(D, 5.0)
    for N in args.sizes:
        for m, q in ((2, 8), (3, 5)):
            rng = np.random.default_rng(N)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.column_stack([np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N) for _ in range(m)])
            theta, Bq = np.full(D, 0.01), q * STARTS
            lower, upper = front_cells(Y)
            members = np.repeat(np.arange(q), STARTS)
            for L in args.features:
                # ---- one path a point: the first objective's own model, the same number of points
                eng.set_train(X, Y[:, 0])
                eng.commit(M52, _lib.MODE_NOISELESS, theta, 0.0, False, BETA)
                dr1 = thompson.draw(SimpleNamespace(X=X, kernel=M52, theta=theta, nu=None), q, L, seed=L)
                eng.generate_candidates(lo, hi, 10_000, 7)
                o1 = eng.sweep_thompson(dr1, minimize=False, k=STARTS)
                s1 = o1["best_x"].reshape(Bq, D)
                single = three(lambda: eng.point_eval_path(s1[:1], dr1, o1["coef"], members[:1], minimize=False),
                               lambda: eng.point_eval_path(s1, dr1, o1["coef"], members, minimize=False),
                               lambda **kw: eng.polish_path(s1, lo, hi, dr1, o1["coef"], members, minimize=False, **kw), args.reps)
                # ---- the joint paths
                eng.set_train(X, Y)
                eng.commit(M52, _lib.MODE_NOISELESS, theta, 0.0, False, BETA)
                dr = thompson.draw_multi(SimpleNamespace(X=X, y=Y, kernel=M52, theta=theta, nu=None, multi=True), q, L, seed=L)
                best = {}
                for M in (10_000, 100_000):
                    eng.generate_candidates(lo, hi, M, 7)
                    out = eng.sweep_thompson_ehvi(dr, q, lower, upper, k=STARTS)
                    starts = out["best_x"][:, 0].reshape(Bq, D)
                    ok = (out["best_idx"][:, 0] >= 0) & (out["best_val"][:, 0] > -np.inf)  # improving rows; the others start from the box's centre, HVI as it is
                    starts = np.where(ok.reshape(Bq, 1), starts, 0.0)
                    _, fp, ne = eng.polish_path_hvi(starts, lo, hi, dr, out["coef"], members, lower, upper)
                    best[M] = (float(np.mean(np.fmax(out["best_val"][:, 0, 0], 0.0))), float(np.mean(fp.reshape(q, STARTS).max(axis=1))), float(ne.mean()))
                    if M == 10_000:
                        coef, s10 = out["coef"], starts
                joint = three(lambda: eng.point_eval_path_hvi(s10[:1], dr, coef, members[:1], lower, upper),
                              lambda: eng.point_eval_path_hvi(s10, dr, coef, members, lower, upper),
                              lambda **kw: eng.polish_path_hvi(s10, lo, hi, dr, coef, members, lower, upper, **kw), args.reps)
                print("N=%d m=%d q=%d C=%d L=%d B=%d" % (N, m, q, len(lower), L, Bq))
                for name, f in (("joint  (m paths + HVI)", joint), ("single (one path)     ", single)):
                    print("    %s: eval B=1 %.3f ms, B=%d %.3f ms; iteration %.1f us; polish %.3f ms" % (name, f[0], Bq, f[1], f[2], f[3]))
                print("    joint / single: iteration %.2f (m = %d); mean %.1f evaluations a start" % (joint[2] / single[2], m, best[10_000][2]))
                print("    mean best HVI: 1e4-row sweep %.5f, + polish %.5f; 1e5-row sweep %.5f, + polish %.5f"
                      % (best[10_000][0], best[10_000][1], best[100_000][0], best[100_000][1]), flush=True)  # fmt: skip
    eng.close()


if __name__ == "__main__":
    main()
