"""The polish of Thompson batches under modelled constraints (bogp_point_eval_path_feasible / bogp_polish_path_feasible,
kernels_point_path_feasible.hip) on one MI355X: d = 20, Matern-5/2, noiseless, L = 1024, (m_obj, n_con, q) = (1, 2, 5) and (2, 1, 5) over 30
cells, every constraint feasible below the 0.4 quantile of its observations, n_starts = 8 (B = 8 q starts: each member's first rows of
`merge_ranks`, whatever their tier), per N medians over `--reps` runs after a warm-up, in one process:
  eval        one bogp_point_eval_path_feasible at B = 1 and at B = 8 q, wall (upload of the operands, ONE launch, read-back)
  iteration   the time of a polish iteration: (polish of 41 evaluations - polish of 1 evaluation) / 40, pgtol = factr = 0 so no start stops
  polish      bogp_polish_path_feasible with the library's defaults (50 evaluations at most), rho = 100, tau = 0.05
  best        per member its best listed row of a 1e4-row sweep and its best point behind the polish's acceptance rule, by the sweep's own
              ranking on the TRUE bounds: the members whose best is of tier A, and the mean tier-A score over the members that had one
              before (m_obj = 1: the drawn objective, minimised -- lower is better; m_obj = 2: the hypervolume added -- higher is better)
  table       rho x tau: the share of the polished points that are feasible under the TRUE bounds, and the share accepted (ranking
              strictly above their start)
Nothing here was tuned."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bogp import _lib, thompson  # noqa: E402
from time_thompson_ehvi_polish import front_cells, three  # noqa: E402

D, STARTS, BETA, L = 20, 8, 0.0, 1024
M52 = _lib.KERNEL_MATERN52


def ranked(y, mo, lower, upper, lo, hi, sigma2):
    """(tier, score) of every row of y (B, m) by the sweep's rule on the true bounds."""
    paths = np.ascontiguousarray(y.T)[None]
    sel = (thompson.select_numpy(paths, lo, hi, sigma2, True, 1) if mo == 1 else
           thompson.hvi_constrained_select_numpy(paths, mo, lower, upper, lo, hi, sigma2, 1))  # fmt: skip
    scores = np.stack([sel[n][0] for n in ("AB" if mo == 1 else "ABV")])
    tier = np.argmax(scores > -np.inf, axis=0)
    return tier, scores[tier, np.arange(len(tier))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    blo, bhi = np.full(D, -5.0), np.full(D, 5.0)
    for N in args.sizes:
        for mo, nc, q in ((1, 2, 5), (2, 1, 5)):
            m, Bq = mo + nc, q * STARTS
            rng = np.random.default_rng(N)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.column_stack([np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N) for _ in range(m)])
            theta, members = np.full(D, 0.01), np.repeat(np.arange(q), STARTS)
            lo, hi = np.full(nc, -np.inf), np.quantile(Y[:, mo:], 0.4, axis=0)
            lower, upper = front_cells(Y[:, :mo]) if mo == 2 else (None, None)
            eng.set_train(X, Y)
            eng.commit(M52, _lib.MODE_NOISELESS, theta, 0.0, False, BETA)
            sigma2 = np.ravel(eng.get_state(with_C=False)["sigma2"])
            dr = thompson.draw_multi(SimpleNamespace(X=X, y=Y, kernel=M52, theta=theta, nu=None, multi=True), q, L, seed=N)
            eng.generate_candidates(blo, bhi, 10_000, 7)
            out = (eng.sweep_thompson_constrained(dr, q, lo, hi, minimize=True, k=STARTS) if mo == 1 else
                   eng.sweep_thompson_ehvi_constrained(dr, q, lower, upper, lo, hi, k=STARTS))  # fmt: skip
            lists = [thompson.merge_ranks(out["best_val"][c], out["best_idx"][c], STARTS) for c in range(q)]
            assert all(len(li) == STARTS for li in lists)
            starts = np.array([out["best_x"][c, w, r] for c in range(q) for _, w, r in lists[c]])
            t0 = np.array([w for c in range(q) for _, w, _ in lists[c]])
            s0 = np.array([out["best_val"][c, w, r] for c in range(q) for _, w, r in lists[c]])
            ops = (dr, out["coef"], members, lower, upper)

            def run(rho, tau):
                plo, phi = thompson.tighten(lo, hi, np.sqrt(sigma2[mo:]), tau)
                xp, _, ne = eng.polish_path_feasible(starts, blo, bhi, *ops, plo, phi, minimize=True, rho=rho)
                yp = eng.point_eval_path_feasible(xp, *ops, plo, phi, minimize=True, rho=rho, jacobian=False)[2]
                tier, score = ranked(yp, mo, lower, upper, lo, hi, sigma2)
                feas = np.all((lo <= yp[:, mo:]) & (yp[:, mo:] <= hi), axis=1)
                return tier, score, feas, (tier < t0) | ((tier == t0) & (score > s0)), ne

            plo, phi = thompson.tighten(lo, hi, np.sqrt(sigma2[mo:]), 0.05)
            f = three(lambda: eng.point_eval_path_feasible(starts[:1], dr, out["coef"], members[:1], lower, upper, plo, phi, rho=100.0),
                      lambda: eng.point_eval_path_feasible(starts, *ops, plo, phi, rho=100.0),
                      lambda **kw: eng.polish_path_feasible(starts, blo, bhi, *ops, plo, phi, rho=100.0, **kw), args.reps)
            print("N=%d m_obj=%d n_con=%d q=%d C=%d L=%d B=%d" % (N, mo, nc, q, 0 if lower is None else len(lower), L, Bq))
            print("    eval B=1 %.3f ms, B=%d %.3f ms; iteration %.1f us; polish %.3f ms" % (f[0], Bq, f[1], f[2], f[3]))
            tier, score, feas, acc, ne = run(100.0, 0.05)
            t1, s1 = np.where(acc, tier, t0).reshape(q, STARTS), np.where(acc, score, s0).reshape(q, STARTS)
            bt0, bt1 = t0.reshape(q, STARTS)[:, 0], t1.min(axis=1)  # a member's list is in rank order: its first row is its best
            bs1 = np.array([s1[c][t1[c] == bt1[c]].max() for c in range(q)])
            both = (bt0 == 0) & (bt1 == 0)
            sign = -1.0 if mo == 1 else 1.0  # (A of a minimised objective is -path)
            print("    members whose best is of tier A: %d -> %d of %d; mean tier-A score over those before: %.5f -> %.5f; mean %.1f evaluations a start"
                  % ((bt0 == 0).sum(), (bt1 == 0).sum(), q, sign * s0.reshape(q, STARTS)[both, 0].mean() if both.any() else np.nan,
                     sign * bs1[both].mean() if both.any() else np.nan, ne.mean()))  # fmt: skip
            for rho in (10.0, 100.0, 1000.0):
                cells = ["tau %.2f: feasible %.2f accepted %.2f" % ((tau,) + tuple(float(np.mean(v)) for v in run(rho, tau)[2:4])) for tau in (0.0, 0.05, 0.2)]
                print("    rho %6.0f | %s" % (rho, " | ".join(cells)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
