"""First measurements of the constrained sweep (bogp_sweep_constrained, k_constrained) at the C3 model size (d = 20, Matern-5/2, 1e6
candidates generated on the device), N = 2048 and N = 512, m = 2 and 4 targets.  Per case, medians over `--reps` repetitions of
  constrained   the whole call (EI x PoF, q = 1, k = 1) and its acquisition_ms (= k_constrained, bogp_last_timing)
  sweep         bogp_sweep (one EI on target 0) with pruning off: the unpruned single-target sweep the constrained one is built on
  ehvi1         bogp_sweep_ehvi with one cell at the same m: the nearest existing m-target tail
`--lib PATH` loads another build of libbogp.so (e.g. the parent commit's, to alternate the two: `--only baseline` then skips the
constrained call, which an older library does not have).  Prints one line per case and repetition block."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib  # noqa: E402

d, M = 20, 1_000_000


def med(fn, reps, stamp=None):
    fn()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if stamp is not None:
            ks.append(stamp()["acquisition_ms"])
    return 1e3 * float(np.median(ts)), (float(np.median(ks)) if ks else float("nan"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another libbogp.so to load")
    ap.add_argument("--only", choices=["all", "baseline"], default="all")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="build")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    if a.only == "baseline":  # an older library: bind only what it exports
        for name in ("bogp_feasibility", "bogp_sweep_constrained"):
            _lib.SIGNATURES.pop(name, None)
    rng = np.random.default_rng(0)
    eng = _lib.Engine(0)
    for N in (2048, 512):
        X = rng.uniform(-5, 5, size=(N, d))
        for m in (2, 4):
            Y = np.column_stack([np.sin(X @ rng.normal(size=d) / 4) for _ in range(m)])
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(d, 0.01), 0.9], 1e-6, False, 0.0)
            eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), M, 7)
            plugin = float(Y[:, 0].min())
            eng.set_prune(False)
            t_sw, k_sw = med(lambda: eng.sweep([(_lib.ACQ_EI, 0.0)], plugin, True), a.reps, eng.last_timing)
            eng.set_prune(True)
            one_lo, one_hi = np.full((1, m), -1.0), np.full((1, m), np.inf)
            t_eh, k_eh = med(lambda: eng.sweep_ehvi(one_lo, one_hi), a.reps, eng.last_timing)
            line = "%s N=%d m=%d  sweep(EI, unpruned) %.2f ms (k_acquisition %.3f)  sweep_ehvi(1 cell) %.2f ms (k_ehvi %.3f)" % (a.tag, N, m, t_sw, k_sw, t_eh, k_eh)
            if a.only == "all":
                lo, hi = np.full(m - 1, -np.inf), np.zeros(m - 1)
                t_c, k_c = med(lambda: eng.sweep_constrained([(_lib.ACQ_EI, 0.0)], plugin, True, lo, hi), a.reps, eng.last_timing)
                tm = eng.last_timing()
                line += "  sweep_constrained %.2f ms (k_constrained %.3f; corr %.2f contract %.2f, %d chunks)  constrained / sweep %.3f" % (
                    t_c, k_c, tm["corr_ms"], tm["contract_ms"], tm["n_chunks"], t_c / t_sw)
            print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
