"""Times the lifted sweep (bogp_lift_sweep_topk) against the plain bogp_sweep_topk over the SAME M reduced-space rows -- what a user
would otherwise have to run before penalising on the host -- for the D = 20 / r = 3 state of the golden G41 (its lift, reduced box
and hyper-parameters) with the training set scaled to N points: rows drawn in the reduced box, y the weighted sphere of the lifted
points, standardised.  One process, warm-up, the two calls alternating, median of `--repeat` wall times around the (synchronous)
calls; the candidates are drawn on the device once per M.  Writes `--out` (default profiles/lift_sweep.txt) and exits 1 unless the
lifted sweep takes under half the plain sweep's time at N = 2048, M = 1e6.

    python tools/time_lift_sweep.py [--sizes 512,2048] [--candidates 1000000,10000000] [--repeat 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bogp  # noqa: E402
from bogp import _lib  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X (HBM3E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048")
    ap.add_argument("--candidates", default="1000000,10000000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_sweep.txt"))
    a = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "G41_pcabo.npz"))
    lift = bogp.Lift(g["d20_A"], g["d20_mean"], g["d20_center"], g["d20_bounds"][:, 0], g["d20_bounds"][:, 1])
    rb = np.array(lift.reduced_bounds())
    r, D = lift.r, lift.D
    w = np.arange(1, D + 1)
    eng = _lib.Engine(0)
    acq = [(_lib.ACQ_EI, 0.0)]
    lines = ["lifted sweep vs plain sweep_topk over the same M rows; D = %d, r = %d, EI, k = 1; median of %d, ms" % (D, r, a.repeat),
             "%6s %9s %10s %10s %10s %10s %10s %10s %7s %10s %8s" % ("N", "M", "n_feasible", "filter", "sweep", "merge", "total", "plain", "ratio",
                                                                  "filter GB/s", "of HBM")]  # fmt: skip
    ok = None
    for N in (int(v) for v in a.sizes.split(",")):
        rng = np.random.default_rng(N)
        X = rng.uniform(rb[:, 0], rb[:, 1], size=(N, r))
        y = np.sum((w * lift.to_original(X)) ** 2, axis=1)
        y = ((y - y.mean()) / y.std()).reshape(-1, 1)
        eng.set_train(X, y)
        par = np.array(g["d20_par"], dtype=float)
        for attempt in range(8):  # the golden's length scales were fitted on 46 points: shorten them until R factorises at N points
            try:
                eng.commit(int(g["d20_kernel"]), int(g["d20_mode"]), par, float(g["d20_noise_var"]), True, 0.0)
                break
            except _lib.NotPositiveDefinite:
                par[:r] *= 4.0
        else:
            raise SystemExit("no positive definite correlation matrix at N = %d" % N)
        plugin = float(y.min())
        for M in (int(float(v)) for v in a.candidates.split(",")):
            eng.generate_candidates(rb[:, 0], rb[:, 1], M, seed=20 + N)
            eng.set_lift(lift.A, lift.mean, lift.center, lift.lo, lift.hi)
            t_lift, t_plain, parts = [], [], []
            for it in range(a.repeat + 1):  # (iteration 0 is the warm-up: buffers are sized there)
                t0 = time.perf_counter()
                lb, li, nf = eng.lift_sweep_topk(acq, plugin, True, 1)
                t1 = time.perf_counter()
                tm = eng.last_timing()
                info = eng.lift_last()
                t2 = time.perf_counter()
                pb, pi = eng.sweep_topk(acq, plugin, True, 1)
                t3 = time.perf_counter()
                if it:
                    t_lift.append((t1 - t0) * 1e3)
                    t_plain.append((t3 - t2) * 1e3)
                    parts.append((info["filter_ms"], tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"], info["merge_ms"]))
            eng.clear_lift()
            # a feasible row beats every penalty (EI >= 0), so both calls name the same winner unless the plain winner is infeasible
            note = "" if li[0, 0] == pi[0, 0] else "  (plain argmax %d is infeasible; lifted %d)" % (pi[0, 0], li[0, 0])
            tl, tp = statistics.median(t_lift), statistics.median(t_plain)
            f, s, m = (statistics.median(p[i] for p in parts) for i in range(3))
            nbytes = M * r * 8 + M * 8 + nf * (r + 1) * 8
            bw = nbytes / (f * 1e-3)
            lines.append("%6d %9d %10d %10.3f %10.3f %10.3f %10.3f %10.3f %7.3f %10.1f %7.1f%%%s" % (N, M, nf, f, s, m, tl, tp, tl / tp, bw / 1e9,
                                                                                                  100 * bw / HBM_PEAK, note))  # fmt: skip
            print(lines[-1], flush=True)
            if N == 2048 and M == 1000000:
                ok = tl < 0.5 * tp
    lines.append("filter = penalty + scan + the read-back of n_feasible + compaction (event time, the host round trip included); sweep = the "
                 "posterior pass over the survivors (bogp_last_timing); merge = scatter + argmax; total / plain = wall time of the call")
    if ok is not None:
        lines.append("target (total under half of plain at N = 2048, M = 1e6): %s" % ("met" if ok else "MISSED"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))
    eng.close()
    if ok is False:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
