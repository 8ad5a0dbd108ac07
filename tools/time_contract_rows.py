"""The direct contraction against the rows of a launch, at 64, 32 and 16 candidates a workgroup (k_contract16d / k_contract16n,
csrc/kernels_posterior.hip; DESIGN.md section 5.2''') and with the automatic choice (bogp_contract_tile_rows): the table the crossover
constants of csrc/bogp_internal.h were read from (profiles/contract_rows.txt, section B).
Two models: the benchmark's C3 (N = 2048, d = 20, Matern-5/2: eight column groups) and a small one (N = 600, d = 10: three).  Per row
count one predict() per tile setting, the four settings interleaved, `--reps` times; the figure is contract_ms of bogp_last_timing (the
HIP-event time of the one contraction launch), as the median.  The whole table runs `--passes` times: the spread between two passes of
a cell is what a difference between two tiles has to exceed.  The MSE bytes of the four settings are compared on the way.
usage: python tools/time_contract_rows.py [--reps 25] [--passes 2] [--rows 64,256,...]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bogp import _lib

ROWS = (64, 256, 832, 2048, 4096, 8192, 16384)
TILES = (64, 32, 16, 0)
MODELS = (("C3", 2048, 20, 0.01), ("small", 600, 10, 0.02))


def engine(N, d, theta):
    rng = np.random.default_rng(0)
    X = rng.uniform(-5, 5, size=(N, d))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    eng = _lib.Engine(0)
    eng.set_train(X, y)
    eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(d, theta), 0.9], 1e-6, False, 0.0)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    args = ap.parse_args()
    rows = [int(r) for r in args.rows.split(",")]
    for name, N, d, theta in MODELS:
        eng = engine(N, d, theta)
        nJ = -(-N // 256)
        print("== %s: N = %d, d = %d, %d column groups; contract_ms, median of %d (min .. max); passes side by side" % (name, N, d, nJ, args.reps))
        print("%7s %6s | %s | auto takes" % ("rows", "wg64", " | ".join("%-38s" % ("tile %s" % (t or "auto")) for t in TILES)))
        table = {}
        for p in range(args.passes):
            for M in rows:
                eng.upload_candidates(np.random.default_rng(M).uniform(-5, 5, size=(M, d)))
                ms = {t: [] for t in TILES}
                bits = {}
                for r in range(args.reps + 3):
                    for t in TILES:
                        eng.set_contract_tile(t)
                        mu, mse = eng.predict()
                        if r >= 3:
                            ms[t].append(eng.last_timing()["contract_ms"])
                        bits[t] = mse.tobytes()
                        if t == 0:
                            table[(M, "auto")] = eng.last_contract_tile()
                assert len(set(bits.values())) == 1, "the MSE bytes differ between tiles at %d rows" % M
                for t in TILES:
                    table.setdefault((M, t), []).append((np.median(ms[t]), min(ms[t]), max(ms[t])))
        for M in rows:
            cells = []
            for t in TILES:
                cells.append("  ".join("%.4f (%.4f .. %.4f)" % c for c in table[(M, t)]))
            t64 = (M + 63) // 64
            print("%7d %6d | %s | %d" % (M, t64 * nJ, " | ".join(cells), table[(M, "auto")]))
        eng.close()


if __name__ == "__main__":
    main()
